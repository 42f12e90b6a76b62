// The general forward convolution behind the Inception-v3 pool3 extractor of the FID (metrics/inception.py: every BasicConv2d of
// torchvision's inception_v3 with the FID patches, i.e. conv without bias + BatchNorm(eps 0.001, eval) + ReLU, the batch norm folded
// into weight and bias by the caller), and the small layers around it:
//
//     te_conv2d_f32          : any kh x kw <= 7 x 7, stride 1 or 2, zero padding below the kernel size, fused bias and ReLU, written into
//                              a channel slice of a concatenated output (the torch.cat of a Mixed block never happens)
//     te_pool3_f32           : the 3 x 3 pools of the network (max stride 2; max stride 1 pad 1; average stride 1 pad 1 that does not
//                              count the padding), into a channel slice as well
//     te_resize_bilinear_f32 : F.interpolate(size, mode='bilinear', align_corners=False), the resize to 299 x 299 in front of the network
//
// te_conv2d_f32 is an implicit GEMM on v_mfma_f32_32x32x2_f32 (an fp32 fma chain in a fixed order of k: exact fp32):
//     M = Co (rows: the weight [Co, K] in torch layout IS the row-major A operand), N = the B * Ho * Wo output pixels flattened across
//     the batch (a tile may span images), K = Ci * kh * kw in the weight's own order k = (c * kh + ky) * kw + kx.
// A workgroup owns 64 output channels x BN pixels (BN = 128, or 64 where 128 would leave the chip idle).  Per 32-deep step the 64 x 32
// weight panel and the BN x 32 patch panel go through registers into LDS (pitch 36 floats: 16-byte aligned stores, conflict-free
// ds_read_b128); the next step's loads are in flight behind the MFMAs.  The patch is gathered on the fly: a thread owns ONE pixel for
// the whole K loop (its image base and top-left tap are decoded once; lanes run along ox, so a wave's loads are contiguous at stride 1)
// and a wave owns one run of consecutive k per step, so the (c, ky, kx) decode is wave-uniform: two divisions per step, then carries.
// Taps outside the image, pixels >= P, channels >= Co and k >= K are zeros.  No im2col tensor, no workspace, no split of K, no atomics.
// An output element is one chain over k ascending in the permutation of gemm_nt_f32.h (lane half h feeds k = 8q + 4h + u of every step
// to MFMA (q, u)), which depends on nothing but K: an image's outputs are bitwise the same whatever batch and whatever tile it is in.
// The kernel itself is the template conv2d_kernel<BN, AL, Gather, Epilogue> of conv2d_body.h, which the other networks instantiate with
// other gathers and epilogues through the same launch(); te_conv2d_f32 is <GatherPlain, EpiBiasAct>.
#include "te_common.h"

#ifdef CONV2D_PROF   // experimental builds: per-wave cycle counts of the three phases of the K loop, read back with te_debug_conv2d_prof
#define TE_PROF
#endif
#include "te_prof.h"

PROF_BUFFER(conv2d, 1024 * 4 * 4)

#include "conv2d_body.h"         // the kernel template (shared with resnet.hip); its profiling lines write the buffer above

namespace {

using namespace te::conv2d;

// mode 0: max, stride 2, no padding (floor); 1: max, stride 1, pad 1 (padding never wins); 2: average, stride 1, pad 1, over the taps
// inside the image.  One thread per output element, lanes along ox.  Max: a greater value or a NaN replaces (te_maxpool2_fwd_f32).
__global__ __launch_bounds__(256) void pool3_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t total, int C, int H, int W,
                                                    int Ho, int Wo, int mode, int Ctot, int c0) {
#pragma clang fp contract(off)
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int ox = (int)(o % Wo), oy = (int)(o / Wo % Ho);
    const int64_t plane = o / Wo / Ho;
    const int64_t b = plane / C;
    const int ch = (int)(plane - b * C);
    const int s = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
    const float* src = x + plane * H * W;
    float v = 0.f;
    int taps = 0;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * s - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * s - pad + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const float t = src[(int64_t)iy * W + ix];
            if (taps == 0) v = t;
            else if (mode == 2) v = v + t;
            else if (t > v || t != t) v = t;
            ++taps;
        }
    }
    if (mode == 2) v = v / (float)taps;                      // (taps >= 1: the centre tap of a pad-1 window is inside the image)
    out[((b * Ctot + c0 + ch) * Ho + oy) * Wo + ox] = v;
}

// upsample_bilinear2d's tap: src = (in / out) * (dst + 0.5) - 0.5 clamped at 0, first tap floor(src), second tap the next sample inside
// the image, l1 = src - floor(src).  src = (in * (2 dst + 1) - out) / (2 out) is evaluated in integers: evaluated in fp32 the
// coordinate carries an error of about in * 2^-23 (1e-4 of a sample at 1024 px), which reaches the output multiplied by the
// difference of the two taps.  Here floor and remainder are exact and l1 is rounded once.  Equal sizes: l1 = 0, a copy.
__device__ __forceinline__ void resize_tap(int dst, int in_size, int out_size, int& i0, int& i1, float& l0, float& l1) {
    int64_t num = (int64_t)in_size * (2 * dst + 1) - out_size;
    const int64_t den = 2 * (int64_t)out_size;
    if (num < 0) num = 0;
    i0 = (int)(num / den);
    const int64_t rem = num - (int64_t)i0 * den;
    if (i0 > in_size - 1) i0 = in_size - 1;                  // (cannot happen: src <= in - 0.5 - in / (2 out) < in)
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = (float)rem / (float)den;
    l0 = 1.f - l1;
}

__global__ __launch_bounds__(256) void resize_kernel(float* __restrict__ out, const float* __restrict__ x, int H, int W, int OH, int OW) {
#pragma clang fp contract(off)
    const int64_t plane = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)OH * OW) return;
    const int oy = (int)(i / OW), ox = (int)(i % OW);
    int ya, yb, xa, xb;
    float ly0, ly1, lx0, lx1;
    resize_tap(oy, H, OH, ya, yb, ly0, ly1);
    resize_tap(ox, W, OW, xa, xb, lx0, lx1);
    const float* src = x + plane * H * W;
    const float* ra = src + (int64_t)ya * W;
    const float* rb = src + (int64_t)yb * W;
    out[plane * OH * OW + i] = ly0 * (lx0 * ra[xa] + lx1 * ra[xb]) + ly1 * (lx0 * rb[xa] + lx1 * rb[xb]);
}

}  // namespace

extern "C" int te_conv2d_f32(float* out, const float* x, const float* w, const float* bias, int B, int Ci, int Co, int H, int W, int kh,
                             int kw, int s, int py, int px, int Ctot, int c0, int act, te_stream_t stream) {
    TE_REQUIRE(out && x && w && bias, TE_ERR_NULL, "te_conv2d_f32: NULL pointer");
    ConvArgs a;
    a.out = out; a.x = x; a.w = w; a.bias = bias;
    if (const int rc = fill_args(a, "te_conv2d_f32", B, Ci, Co, H, W, kh, kw, s, py, px, Ctot, c0, act)) return rc;
    launch<GatherPlain, EpiBiasAct>(a, (hipStream_t)stream);
    return te::launch_status("te_conv2d_f32");
}

extern "C" int te_pool3_f32(float* out, const float* x, int B, int C, int H, int W, int mode, int Ctot, int c0, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_pool3_f32: NULL pointer");
    TE_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE, "te_pool3_f32: B, C, H, W must be positive (got %d, %d, %d, %d)", B, C, H, W);
    TE_REQUIRE(mode >= 0 && mode <= 2, TE_ERR_UNSUPPORTED,
               "te_pool3_f32: mode 0 (max, stride 2), 1 (max, stride 1, pad 1) or 2 (average, stride 1, pad 1), got %d", mode);
    TE_REQUIRE(mode != 0 || (H >= 3 && W >= 3), TE_ERR_SHAPE, "te_pool3_f32: an unpadded 3 x 3 window does not fit a %d x %d plane", H, W);
    TE_REQUIRE(c0 >= 0 && Ctot >= 1 && (int64_t)c0 + C <= Ctot, TE_ERR_SHAPE,
               "te_pool3_f32: the slice [%d, %d + %d) is outside the %d output channels", c0, c0, C, Ctot);
    const int Ho = mode == 0 ? (H - 3) / 2 + 1 : H, Wo = mode == 0 ? (W - 3) / 2 + 1 : W;
    const int64_t total = (int64_t)B * C * Ho * Wo;
    TE_REQUIRE(te::cdiv(total, 256) <= 0x7fffffff, TE_ERR_SHAPE, "te_pool3_f32: too many outputs (%lld)", (long long)total);
    pool3_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(out, x, total, C, H, W, Ho, Wo, mode, Ctot, c0);
    return te::launch_status("te_pool3_f32");
}

extern "C" int te_resize_bilinear_f32(float* out, const float* x, int64_t planes, int H, int W, int OH, int OW, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_resize_bilinear_f32: NULL pointer");
    TE_REQUIRE(planes >= 1 && planes <= 65535 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, TE_ERR_SHAPE,
               "te_resize_bilinear_f32: 1 <= planes <= 65535 and positive H, W, OH, OW (got %lld, %d, %d, %d, %d)", (long long)planes, H, W,
               OH, OW);
    TE_REQUIRE(H <= (1 << 22) && W <= (1 << 22) && OH <= (1 << 22) && OW <= (1 << 22), TE_ERR_SHAPE,
               "te_resize_bilinear_f32: sizes above 2^22 are not supported");
    resize_kernel<<<dim3((unsigned)te::cdiv((int64_t)OH * OW, 256), (unsigned)planes), 256, 0, (hipStream_t)stream>>>(out, x, H, W, OH, OW);
    return te::launch_status("te_resize_bilinear_f32");
}

PROF_READBACK(conv2d)
