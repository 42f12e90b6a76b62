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
#include "te_common.h"

#ifdef CONV2D_PROF   // experimental builds: per-wave cycle counts of the three phases of the K loop, read back with te_debug_conv2d_prof
#define TE_PROF
#endif
#include "te_prof.h"

namespace {

constexpr int BM = 64;           // output channels per workgroup
constexpr int BK = 32;
constexpr int LD = 36;           // LDS row pitch in floats (csrc/gemm_nt_f32.h)
constexpr int NT = 256;
constexpr int kMaxKernel = 7;
constexpr int kWideGridMin = 512;    // BN = 128 only where it still gives two workgroups per CU

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

PROF_BUFFER(conv2d, 1024 * 4 * 4)

struct ConvArgs {
    float* out;
    const float* x;
    const float* w;
    const float* bias;
    int64_t P;                   // B * Ho * Wo
    int Ci, Co, H, W, kh, kw, s, py, px, Ho, Wo, Ctot, c0, act, K;
};

// 64 rows x 32 k of the weight [Co, K] -> two 4-float groups per thread; rows >= Co and k >= K are zeros
template <bool AL>
__device__ __forceinline__ void load_weights(f32x4 (&r)[2], const float* __restrict__ w, int m0, int Co, int K, int k0) {
    const int t = threadIdx.x;
    const int k = k0 + (t & 7) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + (t >> 3) + 32 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < Co) {
            const float* p = w + (int64_t)row * K + k;
            if (AL) {
                if (k < K) v = *reinterpret_cast<const f32x4*>(p);       // K % 4 == 0: the four are inside the row or all past it
            } else {
                if (k < K) v.x = p[0];
                if (k + 1 < K) v.y = p[1];
                if (k + 2 < K) v.z = p[2];
                if (k + 3 < K) v.w = p[3];
            }
        }
        r[i] = v;
    }
}

// the thread's pixel, decoded once
struct Pixel {
    const float* img;            // x + b * Ci * H * W
    int iy0, ix0;                // the input row / column of tap (0, 0); may be negative
    bool live;
};

// NPT consecutive k (from k0, wave-uniform) of the thread's pixel: x[b, c, iy0 + ky, ix0 + kx] or 0
template <int NPT>
__device__ __forceinline__ void gather(float (&r)[NPT], const Pixel& px, const ConvArgs& a, int k0) {
    const int khw = a.kh * a.kw;
    int c = k0 / khw;
    const int rem = k0 - c * khw;
    int ky = rem / a.kw, kx = rem - ky * a.kw;
    const int HW = a.H * a.W;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int iy = px.iy0 + ky, ix = px.ix0 + kx;
        const bool in = px.live && c < a.Ci && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        r[j] = in ? px.img[c * HW + iy * a.W + ix] : 0.f;
        if (++kx == a.kw) {
            kx = 0;
            if (++ky == a.kh) { ky = 0; ++c; }
        }
    }
}

template <int BN, bool AL>
__global__ __launch_bounds__(NT) void conv2d_kernel(const ConvArgs a) {
    constexpr int NACC = BN / 64;                // 32 x 32 tiles per wave along the pixels
    constexpr int NPT = BN * BK / NT;            // patch elements per thread and step: 8 or 16 consecutive k
    constexpr int KG = BK / NPT;                 // k runs per step; a wave has one
    __shared__ __attribute__((aligned(16))) float Ws[BM * LD];
    __shared__ __attribute__((aligned(16))) float Xs[BN * LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * BM;
    const int64_t p0 = (int64_t)blockIdx.x * BN;
    const int HoWo = a.Ho * a.Wo;

    // gather role: pixel n of the tile, k run kg (threadIdx.x / BN is the same for a whole wave: BN is a multiple of 64)
    const int n = threadIdx.x % BN;
    const int kg = __builtin_amdgcn_readfirstlane(threadIdx.x / BN);
    static_assert(KG * BN == NT, "one k run per group of BN threads");
    Pixel px;
    {
        const int64_t p = p0 + n;
        px.live = p < a.P;
        const int64_t b = px.live ? p / HoWo : 0;
        const int r = px.live ? (int)(p - b * HoWo) : 0;
        const int oy = r / a.Wo, ox = r - oy * a.Wo;
        px.img = a.x + b * a.Ci * a.H * a.W;
        px.iy0 = oy * a.s - a.py;
        px.ix0 = ox * a.s - a.px;
    }

    f32x16 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    f32x4 rw[2];
    float rx[NPT];
    load_weights<AL>(rw, a.w, m0, a.Co, a.K, 0);
    gather<NPT>(rx, px, a, kg * NPT);
    const float* wp = Ws + (wm * 32 + c) * LD + 4 * h;
    const float* xp = Xs + (wn * (BN / 2) + c) * LD + 4 * h;
    PROF_ONLY(unsigned long long pc[3] = {0, 0, 0}; unsigned long long tlast = __builtin_readcyclecounter();)
    for (int kk = 0; kk < a.K; kk += BK) {
        __syncthreads();                                     // the previous step's LDS reads are done
        {
            const int t = threadIdx.x;
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(Ws + ((t >> 3) + 32 * i) * LD + (t & 7) * 4) = rw[i];
#pragma unroll
            for (int j = 0; j < NPT; j += 4) {
                const f32x4 v = {rx[j], rx[j + 1], rx[j + 2], rx[j + 3]};
                *reinterpret_cast<f32x4*>(Xs + n * LD + kg * NPT + j) = v;
            }
        }
        __syncthreads();
        PROF_LAP(pc[0]);
        if (kk + BK < a.K) {                                 // in flight behind the MFMAs below
            load_weights<AL>(rw, a.w, m0, a.Co, a.K, kk + BK);
            gather<NPT>(rx, px, a, kk + BK + kg * NPT);
        }
        PROF_LAP(pc[1]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(wp + 8 * q);
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xp + i * 32 * LD + 8 * q);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(u.x, v.x, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(u.y, v.y, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(u.z, v.z, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(u.w, v.w, acc[i], 0, 0, 0);
            }
        }
        PROF_LAP(pc[2]);
    }
    PROF_ONLY(if (lane == 0 && blockIdx.y == 0 && blockIdx.x < 1024) {
        for (int i = 0; i < 3; ++i) te_conv2d_prof_buf[(blockIdx.x * 4 + wid) * 4 + i] = pc[i];
    })
    // accumulator register e of lane (c, h): channel (e & 3) + 8 (e >> 2) + 4 h of the wave's 32, pixel c of tile i
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int64_t p = p0 + wn * (BN / 2) + i * 32 + c;
        if (p >= a.P) continue;
        const int64_t b = p / HoWo;
        const int r = (int)(p - b * HoWo);
        float* dst = a.out + (b * a.Ctot + a.c0) * HoWo + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (m < a.Co) {
                float v = acc[i][e] + a.bias[m];
                if (a.act == 1) v = te::relu_nan(v);
                dst[(int64_t)m * HoWo] = v;
            }
        }
    }
}

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

template <int BN>
void launch_conv(const ConvArgs& a, bool al, hipStream_t st) {
    const dim3 grid((unsigned)te::cdiv(a.P, BN), (unsigned)te::cdiv(a.Co, BM));
    if (al) conv2d_kernel<BN, true><<<grid, NT, 0, st>>>(a);
    else conv2d_kernel<BN, false><<<grid, NT, 0, st>>>(a);
}

}  // namespace

extern "C" int te_conv2d_f32(float* out, const float* x, const float* w, const float* bias, int B, int Ci, int Co, int H, int W, int kh,
                             int kw, int s, int py, int px, int Ctot, int c0, int act, te_stream_t stream) {
    TE_REQUIRE(out && x && w && bias, TE_ERR_NULL, "te_conv2d_f32: NULL pointer");
    TE_REQUIRE(B >= 1 && Ci >= 1 && Co >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE,
               "te_conv2d_f32: B, Ci, Co, H, W must be positive (got %d, %d, %d, %d, %d)", B, Ci, Co, H, W);
    TE_REQUIRE(kh >= 1 && kh <= kMaxKernel && kw >= 1 && kw <= kMaxKernel, TE_ERR_UNSUPPORTED,
               "te_conv2d_f32: 1 <= kh, kw <= %d (got %d x %d)", kMaxKernel, kh, kw);
    TE_REQUIRE(s == 1 || s == 2, TE_ERR_UNSUPPORTED, "te_conv2d_f32: the stride must be 1 or 2 (got %d)", s);
    TE_REQUIRE(py >= 0 && py < kh && px >= 0 && px < kw, TE_ERR_SHAPE,
               "te_conv2d_f32: 0 <= py < kh and 0 <= px < kw (got padding %d, %d for a %d x %d kernel)", py, px, kh, kw);
    TE_REQUIRE(act == 0 || act == 1, TE_ERR_UNSUPPORTED, "te_conv2d_f32: act must be 0 (none) or 1 (ReLU), got %d", act);
    TE_REQUIRE(H + 2 * py >= kh && W + 2 * px >= kw, TE_ERR_SHAPE,
               "te_conv2d_f32: a %d x %d kernel with padding %d, %d does not fit a %d x %d image (Ho, Wo >= 1)", kh, kw, py, px, H, W);
    TE_REQUIRE(c0 >= 0 && Ctot >= 1 && (int64_t)c0 + Co <= Ctot, TE_ERR_SHAPE,
               "te_conv2d_f32: the slice [%d, %d + %d) is outside the %d output channels", c0, c0, Co, Ctot);
    const int Ho = (H + 2 * py - kh) / s + 1, Wo = (W + 2 * px - kw) / s + 1;
    TE_REQUIRE((int64_t)Ci * H * W <= 0x7fffffff && (int64_t)Ci * kh * kw <= 0x7fffffff - BK && (int64_t)Ho * Wo <= 0x7fffffff, TE_ERR_SHAPE,
               "te_conv2d_f32: one image (Ci * H * W), Ci * kh * kw and Ho * Wo must fit 31 bits");
    ConvArgs a;
    a.out = out; a.x = x; a.w = w; a.bias = bias;
    a.P = (int64_t)B * Ho * Wo;
    a.Ci = Ci; a.Co = Co; a.H = H; a.W = W; a.kh = kh; a.kw = kw; a.s = s; a.py = py; a.px = px;
    a.Ho = Ho; a.Wo = Wo; a.Ctot = Ctot; a.c0 = c0; a.act = act; a.K = Ci * kh * kw;
    TE_REQUIRE(te::cdiv(a.P, 64) <= 0x7fffffff && te::cdiv(Co, BM) <= 65535, TE_ERR_SHAPE,
               "te_conv2d_f32: too many outputs (%lld pixels, %d channels)", (long long)a.P, Co);
    const bool al = a.K % 4 == 0 && te::aligned16(w);
    hipStream_t st = (hipStream_t)stream;
    if (te::cdiv(a.P, 128) * te::cdiv(Co, BM) >= kWideGridMin) launch_conv<128>(a, al, st);
    else launch_conv<64>(a, al, st);
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
