// The backward pass of the ArcFace IR-SE50 identity network (irse.hip) with respect to its INPUT: the network is frozen, so there is no
// weight gradient and no training-mode batch norm.  What pSp/criteria/id_loss.py:23-45 IDLoss.forward needs from torch autograd:
//
//     te_conv2d_dgrad_f32    : the data gradient of te_conv2d_f32 / te_conv2d_prelu_f32, with the PReLU' or the affine + add epilogue
//     te_se_bwd_f32          : SEModule and the gated product backwards: gout, r, gate, pooled -> the gradient of r
//     te_id_stem_bwd_f32     : PReLU', the stem convolution, AdaptiveAvgPool2d and the crop backwards, to the image
//     te_rows_unit_bwd_f32   : l2_norm backwards
//
// The adjoint of a convolution is a convolution: te_conv2d_dgrad_f32 and the stem run the main loop of conv2d_body.h (the k order of the
// forward family) over the incoming gradient, on a weight the host transposed and flipped once, phase by phase (dgrad_body.h, which the
// grouped data gradient of psp_heads_bwd.hip shares).
// No atomics; every reduction is a fixed-order chain or a fixed-shape tree; an image's gradient is bitwise independent of its batch.
#include "te_common.h"
#include "dgrad_body.h"
#include "irse_common.h"

namespace {

using namespace te::dgrad;
using namespace te::irse;

// ------------------------------------------------------------------------------------------------------ squeeze-and-excitation
using te::wave_sum;

// ggate[plane] = sum_hw gout * r: one wave per plane, lane l takes i = l, l + 64, ... as one fma chain, the lanes meet in a butterfly
__global__ __launch_bounds__(256) void se_ggate_kernel(float* __restrict__ ggate, const float* __restrict__ gout, const float* __restrict__ r,
                                                       int64_t planes, int HW) {
    const int lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const float* g = gout + plane * HW;
    const float* q = r + plane * HW;
    float acc = 0.f;
    for (int i = lane; i < HW; i += 64) acc = fmaf(g[i], q[i], acc);
    acc = wave_sum(acc);
    if (lane == 0) ggate[plane] = acc;
}

// One workgroup of four waves per image, as se_excite_kernel.  Step 1: the hidden units again, by se_excite_kernel's own se_unit (they
// are not kept), before the ReLU.  Step 2: a live hidden unit's gradient is one wave's dot product over the channels of w2[:, r] with
// gz[c] = ggate[c] * gate[c] * (1 - gate[c]); a dead one (hidden <= 0 or NaN: torch's threshold rule) gets 0.  Step 3: a thread per
// channel, one fma chain over r ascending, divided by the plane: what every pixel of r[b,c] receives through the mean.
__global__ __launch_bounds__(kSeThreads) void se_bwd_kernel(float* __restrict__ gmean, const float* __restrict__ ggate,
                                                            const float* __restrict__ gate, const float* __restrict__ pooled,
                                                            const float* __restrict__ w1, const float* __restrict__ w2, int C, int R, float hw) {
    __shared__ float hidden[kSeMaxR];
    __shared__ float gh[kSeMaxR];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float* p = pooled + (int64_t)blockIdx.x * C;
    const float* gg = ggate + (int64_t)blockIdx.x * C;
    const float* gt = gate + (int64_t)blockIdx.x * C;
    for (int r = wid; r < R; r += kSeThreads / 64) {
        const float acc = se_unit(p, w1, C, r, lane);
        if (lane == 0) hidden[r] = acc;
    }
    __syncthreads();
    for (int r = wid; r < R; r += kSeThreads / 64) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float s = gt[c];
            acc = fmaf(w2[(int64_t)c * R + r], gg[c] * (s * (1.f - s)), acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) gh[r] = hidden[r] > 0.f ? acc : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kSeThreads) {
        float z = 0.f;
        for (int r = 0; r < R; ++r) z = fmaf(w1[(int64_t)r * C + c], gh[r], z);
        gmean[(int64_t)blockIdx.x * C + c] = __fdiv_rn(z, hw);
    }
}

// gr = gout * gate[plane] + gmean[plane], one fma; four consecutive elements of a plane per thread (HW % 4 == 0) or one
template <bool VEC>
__global__ __launch_bounds__(256) void se_gr_kernel(float* __restrict__ gr, const float* __restrict__ gout, const float* __restrict__ gate,
                                                    const float* __restrict__ gmean, int64_t items, int per_plane) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const int64_t plane = t / per_plane;
    const float s = gate[plane], m = gmean[plane];
    if (VEC) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(gout + 4 * t);
        f32x4 o;
        o.x = fmaf(g.x, s, m); o.y = fmaf(g.y, s, m); o.z = fmaf(g.z, s, m); o.w = fmaf(g.w, s, m);
        *reinterpret_cast<f32x4*>(gr + 4 * t) = o;
    } else {
        gr[t] = fmaf(gout[t], s, m);
    }
}

// ------------------------------------------------------------------------------------------------------ the stem
struct StemBwdArgs : DgradArgs {
    const float* spre;           // the stem's kept pre-activation, in the layout of g
    const float* sslope;         // [Co]
};

// a tap of g * PReLU'(pre): the product with the slope is one rounding; c is wave-uniform
struct GatherPreluGrad {
    static __device__ __forceinline__ const float* image(const StemBwdArgs& a, int64_t b) { return a.x + b * a.Ci * a.H * a.W; }
    static __device__ __forceinline__ int plane(const StemBwdArgs& a) { return a.H * a.W; }
    static __device__ __forceinline__ float tap(const float* img, const StemBwdArgs& a, int HW, int c, int iy, int ix) {
        const int at = c * HW + iy * a.W + ix;
        const float g = img[at];
        return a.spre[(img - a.x) + at] > 0.f ? g : __fmul_rn(g, a.sslope[c]);
    }
};

// AdaptiveAvgPool2d and the crop backwards as a GATHER: an image pixel sums the pooled windows [floor(i L / Pn), ceil((i + 1) L / Pn))
// that contain it (at most 2 x 2 of them where L >= Pn), each divided by its count, rows then columns ascending; 0 outside the box
__global__ __launch_bounds__(256) void stem_unpool_kernel(float* __restrict__ gimg, const float* __restrict__ gp, int64_t total, int H, int W,
                                                          int y0, int x0, int Lh, int Lw, int Pn) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int x = (int)(o % W) - x0, y = (int)(o / W % H) - y0;
    const int64_t plane = o / W / H;
    float s = 0.f;
    if ((unsigned)y < (unsigned)Lh && (unsigned)x < (unsigned)Lw) {
        const int ia = y * Pn / Lh, ib = ((y + 1) * Pn - 1) / Lh;              // the windows' inverse (Pn, L <= 32768: the products fit)
        const int ja = x * Pn / Lw, jb = ((x + 1) * Pn - 1) / Lw;
        const float* src = gp + plane * Pn * Pn;
        for (int i = ia; i <= ib; ++i) {                     // (its own copy of te::adaptive_window's bounds: the call changes the instruction stream)
            const int rows = ((i + 1) * Lh + Pn - 1) / Pn - i * Lh / Pn;
            for (int j = ja; j <= jb; ++j) {
                const int cols = ((j + 1) * Lw + Pn - 1) / Pn - j * Lw / Pn;
                s = __fadd_rn(s, __fdiv_rn(src[i * Pn + j], (float)(rows * cols)));
            }
        }
    }
    gimg[o] = s;
}

// ------------------------------------------------------------------------------------------------------ the rows
// Row i = blockIdx.x, one wave, rows_dot_kernel's shape: <e, ge> and the norm's square are fp64 chains per lane and fp64 butterflies
__global__ __launch_bounds__(64) void rows_unit_bwd_kernel(float* __restrict__ ga, const float* __restrict__ ge, const float* __restrict__ e,
                                                           const float* __restrict__ a, int D) {
    const int lane = threadIdx.x;
    const int64_t at = (int64_t)blockIdx.x * D;
    double dot = 0.0, sq = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = a[at + d];
        dot = fma((double)e[at + d], (double)ge[at + d], dot);
        sq = fma(v, v, sq);
    }
    const float dt = (float)wave_sum(dot);
    const float norm = (float)sqrt(wave_sum(sq));
    for (int d = lane; d < D; d += 64) ga[at + d] = __fdiv_rn(fmaf(-e[at + d], dt, ge[at + d]), norm);
}

}  // namespace

extern "C" int te_conv2d_dgrad_f32(float* gx, const float* g, const float* wt, const float* pre, const float* slope, const float* in_scale,
                                   const float* add, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px, int add_s,
                                   te_stream_t stream) {
    TE_REQUIRE(gx && g && wt, TE_ERR_NULL, "te_conv2d_dgrad_f32: NULL pointer");
    TE_REQUIRE((pre == nullptr) == (slope == nullptr), TE_ERR_NULL, "te_conv2d_dgrad_f32: pre and slope must both be given or both be NULL");
    TE_REQUIRE(!pre || (!in_scale && !add), TE_ERR_UNSUPPORTED, "te_conv2d_dgrad_f32: the PReLU' epilogue (pre) takes neither in_scale nor add");
    TE_REQUIRE(!add || add_s == 1 || add_s == 2, TE_ERR_UNSUPPORTED, "te_conv2d_dgrad_f32: add_s must be 1 or 2 (got %d)", add_s);
    int Ho, Wo;
    if (const int rc = check_dgrad("te_conv2d_dgrad_f32", B, Ci, Co, H, W, kh, kw, s, py, px, Ho, Wo)) return rc;
    DgradArgs a;
    a.out = gx; a.x = g; a.pre = pre; a.slope = slope; a.in_scale = in_scale; a.add = add;
    a.as = add ? add_s : 1; a.AH = (H - 1) / a.as + 1; a.AW = (W - 1) / a.as + 1;
    launch_dgrad<GatherPlain>(a, wt, B, Ci, Co, H, W, kh, kw, s, py, px, Ho, Wo, (hipStream_t)stream);
    return te::launch_status("te_conv2d_dgrad_f32");
}

extern "C" int te_se_bwd_f32(float* gr, float* ws, const float* gout, const float* r, const float* gate, const float* pooled, const float* w1,
                             const float* w2, int B, int C, int R, int Ho, int Wo, te_stream_t stream) {
    TE_REQUIRE(gr && ws && gout && r && gate && pooled && w1 && w2, TE_ERR_NULL, "te_se_bwd_f32: NULL pointer");
    TE_REQUIRE(B >= 1 && C >= 1 && R >= 1 && R <= kSeMaxR && (int64_t)C * R <= 0x7fffffff && Ho >= 1 && Wo >= 1 && (int64_t)Ho * Wo <= 0x7fffffff,
               TE_ERR_SHAPE, "te_se_bwd_f32: B, C, Ho, Wo >= 1, 1 <= R <= %d, C * R and Ho * Wo below 2^31 (got %d, %d, %d, %d, %d)", kSeMaxR, B, C,
               R, Ho, Wo);
    const int64_t planes = (int64_t)B * C;
    const int HW = Ho * Wo;
    TE_REQUIRE(planes <= ((int64_t)1 << 40) / HW && te::cdiv(planes, 4) <= 0x7fffffff, TE_ERR_SHAPE,
               "te_se_bwd_f32: at most 2^40 elements (got %lld planes of %d x %d)", (long long)planes, Ho, Wo);
    hipStream_t st = (hipStream_t)stream;
    float* ggate = ws;
    float* gmean = ws + planes;
    se_ggate_kernel<<<(unsigned)te::cdiv(planes, 4), 256, 0, st>>>(ggate, gout, r, planes, HW);
    se_bwd_kernel<<<(unsigned)B, kSeThreads, 0, st>>>(gmean, ggate, gate, pooled, w1, w2, C, R, (float)HW);
    if (HW % 4 == 0 && te::aligned16(gr) && te::aligned16(gout)) {
        const int64_t items = planes * HW / 4;
        se_gr_kernel<true><<<(unsigned)te::cdiv(items, 256), 256, 0, st>>>(gr, gout, gate, gmean, items, HW / 4);
    } else {
        const int64_t items = planes * HW;
        se_gr_kernel<false><<<(unsigned)te::cdiv(items, 256), 256, 0, st>>>(gr, gout, gate, gmean, items, HW);
    }
    return te::launch_status("te_se_bwd_f32");
}

extern "C" int te_id_stem_bwd_f32(float* gimg, float* ws, const float* g, const float* wt, const float* pre, const float* slope, int N, int H,
                                  int W, int y0, int y1, int x0, int x1, int Pn, int Co, te_stream_t stream) {
    TE_REQUIRE(gimg && ws && g && wt && pre && slope, TE_ERR_NULL, "te_id_stem_bwd_f32: NULL pointer");
    if (const int rc = check_id_window("te_id_stem_bwd_f32", N, H, W, y0, y1, x0, x1, Pn, Co)) return rc;
    TE_REQUIRE(te::cdiv((int64_t)N * 3 * H * W, 256) <= 0x7fffffff, TE_ERR_SHAPE,
               "te_id_stem_bwd_f32: one image (3 * H * W) must fit 31 bits and the batch 2^39 elements");
    int Ho, Wo;
    if (const int rc = check_dgrad("te_id_stem_bwd_f32", N, 3, Co, Pn, Pn, 3, 3, 1, 1, 1, Ho, Wo)) return rc;
    hipStream_t st = (hipStream_t)stream;
    StemBwdArgs a;
    a.out = ws; a.x = g; a.pre = nullptr; a.slope = nullptr; a.in_scale = nullptr; a.add = nullptr; a.as = 1; a.AH = Pn; a.AW = Pn;
    a.spre = pre; a.sslope = slope;
    launch_dgrad<GatherPreluGrad>(a, wt, N, 3, Co, Pn, Pn, 3, 3, 1, 1, 1, Ho, Wo, st);
    const int64_t total = (int64_t)N * 3 * H * W;
    stem_unpool_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, st>>>(gimg, ws, total, H, W, y0, x0, y1 - y0, x1 - x0, Pn);
    return te::launch_status("te_id_stem_bwd_f32");
}

extern "C" int te_rows_unit_bwd_f32(float* ga, const float* ge, const float* e, const float* a, int64_t I, int D, te_stream_t stream) {
    TE_REQUIRE(ga && ge && e && a, TE_ERR_NULL, "te_rows_unit_bwd_f32: NULL pointer");
    TE_REQUIRE(I >= 1 && I <= 0x7fffffff && D >= 1, TE_ERR_SHAPE, "te_rows_unit_bwd_f32: 1 <= I < 2^31 and D >= 1 (got %lld, %d)", (long long)I, D);
    rows_unit_bwd_kernel<<<(unsigned)I, 64, 0, (hipStream_t)stream>>>(ga, ge, e, a, D);
    return te::launch_status("te_rows_unit_bwd_f32");
}
