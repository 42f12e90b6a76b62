// LPIPS-VGG perceptual distance (utils/lpips/networks_basic.py:21-87, pretrained_networks.py:98-136): the kernels whose shapes the
// convolution family does not cover.  conv1_2 ... conv5_3 run on the plain 3x3 convolution (op/modconv.py planner); here:
//
//     stem   : ScalingLayer -> conv1_1 (3 -> 64, pad 1) -> bias -> ReLU (vgg_stem_kernel of vgg_stem.h with the rule StemScaled; with
//              StemIdentity it is torchvision's vgg16.features[0:2], te_vgg_stem_fwd_f32) and its data gradient (64 -> 3, relu1_1
//              mask, 1/scale)
//     pool   : 2x2 / stride 2 max-pool forward and backward (torch's rule: first maximum in row-major order, NaN propagates)
//     head   : normalize_tensor, squared difference, lin weights, spatial mean (per-block partials + a fixed-order sum) and the
//              gradient with respect to the pred features
//     pair   : the same head for an interleaved batch of pairs, both sides normalised in the kernel, the channel loop split over
//              the block (the PPL metric, transeditor_amd/metrics.py)
//     crop   : window + integer-factor bilinear resize to the LPIPS input
//
// One thread per output pixel everywhere except the paired head; every reduction is a fixed-order loop or a fixed-shape tree (no atomics).
#include "te_common.h"
#include "vgg_stem.h"

namespace {

// ScalingLayer (networks_basic.py:89-96): (x - shift) / scale
__constant__ float kShift[3] = {-.030f, -.088f, -.188f};
__constant__ float kScale[3] = {.458f, .448f, .450f};
constexpr float kEps = 1e-10f;   // normalize_tensor eps (utils/lpips/__init__.py:43-45)

// the stem's input rules (vgg_stem.h).  StemIdentity: torchvision's vgg16.features[0] on the raw input.  StemScaled: the scaling
// happens BEFORE nn.Conv2d's zero padding
struct StemIdentity {
    static constexpr bool kWindow = false;
    static __device__ __forceinline__ int channel(int c) { return c; }
    static __device__ __forceinline__ float value(float v, int) { return v; }
};

struct StemScaled {
    static constexpr bool kWindow = false;
    static __device__ __forceinline__ int channel(int c) { return c; }
    static __device__ __forceinline__ float value(float v, int c) { return (v - kShift[c]) / kScale[c]; }
};

// gx[n,c,y,x] = (1/scale[c]) * sum_{o,ky,kx} w[o,c,ky,kx] * g[n,o,y+1-ky,x+1-kx] * (y1[n,o,...] > 0)
__global__ __launch_bounds__(256) void stem_dgrad_kernel(float* __restrict__ gx, const float* __restrict__ g,
                                                         const float* __restrict__ y1, const float* __restrict__ w, int H, int W) {
    __shared__ float ws[64 * 27];
    for (int i = threadIdx.x; i < 64 * 27; i += 256) ws[i] = w[i];
    __syncthreads();
    const int n = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int yy = (int)(p / W), xx = (int)(p % W);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const float* gn = g + (int64_t)n * 64 * HW;
    const float* yn = y1 + (int64_t)n * 64 * HW;
    for (int o = 0; o < 64; ++o) {
        const float* go = gn + (int64_t)o * HW;
        const float* yo = yn + (int64_t)o * HW;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int oy = yy + 1 - ky;
            if (oy < 0 || oy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ox = xx + 1 - kx;
                if (ox < 0 || ox >= W) continue;
                const int64_t q = (int64_t)oy * W + ox;
                const float gv = yo[q] > 0.f ? go[q] : 0.f;
                const int t = ky * 3 + kx;
                a0 = fmaf(ws[o * 27 + t], gv, a0);
                a1 = fmaf(ws[o * 27 + 9 + t], gv, a1);
                a2 = fmaf(ws[o * 27 + 18 + t], gv, a2);
            }
        }
    }
    float* gxn = gx + (int64_t)n * 3 * HW + p;
    gxn[0] = a0 / kScale[0];
    gxn[HW] = a1 / kScale[1];
    gxn[2 * HW] = a2 / kScale[2];
}

// index (0..3, row-major) of the window's maximum under torch's rule (max_pool2d: `val > max || isnan(val)` updates)
__device__ __forceinline__ int pool_argmax(const float* __restrict__ x, int64_t q, int W, float& m) {
    const float v[4] = {x[q], x[q + 1], x[q + W], x[q + W + 1]};
    int idx = 0;
    m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k] > m || v[k] != v[k]) { m = v[k]; idx = k; }
    return idx;
}

__global__ __launch_bounds__(256) void pool_fwd_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t total, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t plane = i / ((int64_t)Ho * Wo);
    const int r = (int)(i - plane * Ho * Wo);
    const int oy = r / Wo, ox = r % Wo;
    float m;
    pool_argmax(x, plane * H * W + (int64_t)(2 * oy) * W + 2 * ox, W, m);
    out[i] = m;
}

// every input pixel belongs to exactly one window: all four are written (no zero fill)
__global__ __launch_bounds__(256) void pool_bwd_kernel(float* __restrict__ gx, const float* __restrict__ g, const float* __restrict__ x,
                                                       int64_t total, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t plane = i / ((int64_t)Ho * Wo);
    const int r = (int)(i - plane * Ho * Wo);
    const int oy = r / Wo, ox = r % Wo;
    const int64_t q = plane * H * W + (int64_t)(2 * oy) * W + 2 * ox;
    float m;
    const int idx = pool_argmax(x, q, W, m);
    const float gv = g[i];
    gx[q] = idx == 0 ? gv : 0.f;
    gx[q + 1] = idx == 1 ? gv : 0.f;
    gx[q + W] = idx == 2 ? gv : 0.f;
    gx[q + W + 1] = idx == 3 ? gv : 0.f;
}

__device__ __forceinline__ float block_sum256(float v, float* part) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wid] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// 1 / (sqrt(sum_c x^2) + eps), correctly rounded in every kernel that uses it: the normalise-only mode (cached target) and the
// head's own normalisation of the pred features agree bit for bit, so d(x, x) == 0 exactly
__device__ __forceinline__ float norm_inv(float s) { return __fdiv_rn(1.f, __fadd_rn(__fsqrt_rn(s), kEps)); }

// the paired head's form: the same quantity from an fp64 sum of squares, rounded to fp32 once.  At PPL's scale the two sides of a pair
// differ by 1e-4 of their size, so an error of 1e-7 in a side's norm is 1e-3 of every difference at that pixel, all with one sign
__device__ __forceinline__ float norm_inv_f64(double s) { return (float)(1.0 / (sqrt(s) + (double)kEps)); }

// normalize_tensor: out = x / (sqrt(sum_c x^2) + eps)
__global__ __launch_bounds__(256) void normalize_kernel(float* __restrict__ out, const float* __restrict__ x, int C, int64_t HW) {
    const int n = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float* xn = x + (int64_t)n * C * HW + p;
    float s = 0.f;
    for (int c = 0; c < C; ++c) { const float v = xn[(int64_t)c * HW]; s = fmaf(v, v, s); }
    const float inv = norm_inv(s);
    float* on = out + (int64_t)n * C * HW + p;
    for (int c = 0; c < C; ++c) on[(int64_t)c * HW] = __fmul_rn(xn[(int64_t)c * HW], inv);
}

// partial[n, blockIdx.x] = sum over the block's pixels of sum_c w[c] * (f[n,c,p] / (|f[n,:,p]| + eps) - t[nt,c,p])^2
__global__ __launch_bounds__(256) void head_fwd_kernel(float* __restrict__ partial, const float* __restrict__ f,
                                                       const float* __restrict__ t, const float* __restrict__ w, int Nt, int C,
                                                       int64_t HW) {
#pragma clang fp contract(off)   // (f * inv) rounded before the subtraction, as the normalise-only mode stores it: d(x, x) == 0
    __shared__ float part[4];
    const int n = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    if (p < HW) {
        const float* fn = f + (int64_t)n * C * HW + p;
        const float* tn = t + (int64_t)(Nt == 1 ? 0 : n) * C * HW + p;
        float s = 0.f;
        for (int c = 0; c < C; ++c) { const float a = fn[(int64_t)c * HW]; s = fmaf(a, a, s); }
        const float inv = norm_inv(s);
        for (int c = 0; c < C; ++c) {
            const float d = fn[(int64_t)c * HW] * inv - tn[(int64_t)c * HW];
            v = fmaf(w[c] * d, d, v);      // (explicit fma: kept)
        }
    }
    const float s = block_sum256(v, part);
    if (threadIdx.x == 0) partial[(int64_t)n * gridDim.x + blockIdx.x] = s;
}

// d/df of the head at one pixel (see te_hip.h): u_c = 2 w_c (fhat_c - t_c) gd[n] / HW,
//     g = u / (r + eps) - f (f . u) / (r (r + eps)^2)      (second term 0 at r = 0)
// then gf = (gin + g) * (relu_mask ? (f > 0) : 1)
__global__ __launch_bounds__(256) void head_bwd_kernel(float* __restrict__ gf, const float* __restrict__ gin, const float* __restrict__ gd,
                                                       const float* __restrict__ f, const float* __restrict__ t, const float* __restrict__ w,
                                                       int Nt, int C, int64_t HW, int relu_mask) {
    const int n = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int64_t base = (int64_t)n * C * HW + p;
    const float* fn = f + base;
    const float* tn = t + (int64_t)(Nt == 1 ? 0 : n) * C * HW + p;
    const float sc = 2.f * gd[n] / (float)HW;
    float s = 0.f;
    for (int c = 0; c < C; ++c) { const float a = fn[(int64_t)c * HW]; s = fmaf(a, a, s); }
    const float r = __fsqrt_rn(s), re = r + kEps, inv = norm_inv(s);
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
        const float a = fn[(int64_t)c * HW];
        const float u = sc * w[c] * (__fmul_rn(a, inv) - tn[(int64_t)c * HW]);
        dot = fmaf(a, u, dot);
    }
    const float k = r > 0.f ? dot / (r * re * re) : 0.f;
    float* gn = gf + base;
    const float* gi = gin ? gin + base : nullptr;
    for (int c = 0; c < C; ++c) {
        const float a = fn[(int64_t)c * HW];
        const float u = sc * w[c] * (__fmul_rn(a, inv) - tn[(int64_t)c * HW]);
        float gv = u * inv - a * k;
        if (gi) gv += gi[(int64_t)c * HW];
        if (relu_mask && !(a > 0.f)) gv = 0.f;
        gn[(int64_t)c * HW] = gv;
    }
}

// Paired head (PPL, metrics/evaluate_query.py:234 through networks_basic.py:65-73): images 2n and 2n+1 of an interleaved batch are a
// pair; both sides are normalised here, nothing normalised is stored.  A block is 16 waves over a tile of PT = min(256, HW rounded up
// to 64) pixels: PT / 64 waves side by side along the pixels (consecutive lanes read consecutive pixels of one channel plane), the
// other factor CG = 1024 / PT (4 at PT = 256, 16 at PT = 64; whole part) splits the channel loop.  Pass 1: each thread's sum of squares over its channel slice for
// both sides, in fp64 -> LDS -> every thread adds the CG slices of its pixel in slice order, so all CG threads of a pixel hold the
// same norm; 1 / (norm + eps) is rounded to fp32 once (norm_inv_f64).
// Pass 2: the slice's terms, (a * inv_a) and (b * inv_b) each rounded, then the difference, then the square (never a^2 + b^2 - 2ab).
// Reduction: wave shuffle tree, 16 wave sums in LDS, added in wave order by thread 0 (no atomics).
constexpr int kPairThreads = 1024;

__global__ __launch_bounds__(kPairThreads) void pair_head_kernel(float* __restrict__ partial, const float* __restrict__ f,
                                                                 const float* __restrict__ w, int C, int64_t HW, int PT) {
#pragma clang fp contract(off)   // as head_fwd_kernel: both products rounded before the subtraction, d(x, x) == 0
    __shared__ double ssa[kPairThreads], ssb[kPairThreads];
    __shared__ float part[kPairThreads / 64];
    const int n = blockIdx.y;
    const int CG = kPairThreads / PT;
    const int pix = threadIdx.x % PT, cg = threadIdx.x / PT;      // PT is a multiple of 64: a wave has one cg, 64 consecutive pixels
    const int64_t p = (int64_t)blockIdx.x * PT + pix;
    const int cpg = (C + CG - 1) / CG;
    const int c0 = cg * cpg, c1 = min(C, c0 + cpg);
    const bool live = p < HW;
    const float* fa = f + (int64_t)(2 * n) * C * HW + p;
    const float* fb = fa + (int64_t)C * HW;
    double sa = 0.0, sb = 0.0;
    if (live) {
        // squares are exact in fp64 and the sums of up to a few hundred of them round far below fp32: the norm carries no
        // accumulation error.  Two chains per side keep loads in flight.
        double qa[2] = {0.0, 0.0}, qb[2] = {0.0, 0.0};
        int c = c0;
        for (; c + 2 <= c1; c += 2) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double a = fa[(int64_t)(c + k) * HW], b = fb[(int64_t)(c + k) * HW];
                qa[k] = fma(a, a, qa[k]);
                qb[k] = fma(b, b, qb[k]);
            }
        }
        if (c < c1) {
            const double a = fa[(int64_t)c * HW], b = fb[(int64_t)c * HW];
            qa[0] = fma(a, a, qa[0]);
            qb[0] = fma(b, b, qb[0]);
        }
        sa = qa[0] + qa[1];
        sb = qb[0] + qb[1];
    }
    ssa[threadIdx.x] = sa;
    ssb[threadIdx.x] = sb;
    __syncthreads();
    float v = 0.f;
    if (live) {
        sa = ssa[pix];
        sb = ssb[pix];
        for (int g = 1; g < CG; ++g) { sa += ssa[g * PT + pix]; sb += ssb[g * PT + pix]; }
        const float ia = norm_inv_f64(sa), ib = norm_inv_f64(sb);
        for (int c = c0; c < c1; ++c) {
            const float d = fa[(int64_t)c * HW] * ia - fb[(int64_t)c * HW] * ib;
            v = fmaf(w[c] * d, d, v);      // (explicit fma: kept)
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = part[0];
        for (int k = 1; k < kPairThreads / 64; ++k) s += part[k];
        partial[(int64_t)n * gridDim.x + blockIdx.x] = s;
    }
}

// Window [y0, y0+hc) x [x0, x0+wc) of img [B,3,H,W] resampled by the integer factor fy = hc / h, fx = wc / w with the arithmetic of
// F.interpolate(mode='bilinear', align_corners=False) applied to the window alone (upsample_bilinear2d: src = scale * (dst + 0.5) - 0.5
// clamped at 0, second tap i0 + 1 unless i0 is the window's last row / column, weights l1 = src - i0, l0 = 1 - l1; rows first mixed
// along x, then along y).  Factor 1: src = dst, l1 = 0, a windowed copy.  One thread per output pixel, lanes along x.
__device__ __forceinline__ void bilinear_tap(int dst, int factor, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float src = (float)factor * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

__global__ __launch_bounds__(256) void crop_resize_kernel(float* __restrict__ out, const float* __restrict__ img, int H, int W, int y0,
                                                          int x0, int hc, int wc, int h, int w) {
#pragma clang fp contract(off)
    const int64_t plane = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)h * w) return;
    const int oy = (int)(i / w), ox = (int)(i % w);
    int ya, yb, xa, xb;
    float ly0, ly1, lx0, lx1;
    bilinear_tap(oy, hc / h, hc, ya, yb, ly0, ly1);
    bilinear_tap(ox, wc / w, wc, xa, xb, lx0, lx1);
    const float* src = img + plane * H * W + (int64_t)y0 * W + x0;
    const float* ra = src + (int64_t)ya * W;
    const float* rb = src + (int64_t)yb * W;
    out[plane * h * w + i] = ly0 * (lx0 * ra[xa] + lx1 * ra[xb]) + ly1 * (lx0 * rb[xa] + lx1 * rb[xb]);
}

struct DistArgs {
    const float* partial[8];
    int nblk[8];
    int64_t hw[8];
};

// d[n] = sum_l (sum_b partial_l[n, b]) / HW_l, layers in order 0..L-1 (networks_basic.py:80-82: val = res[0]; val += res[l])
__global__ __launch_bounds__(64) void dist_kernel(float* __restrict__ d, DistArgs a, int L, int N) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float val = 0.f;
    for (int l = 0; l < L; ++l) {
        const float* pl = a.partial[l] + (int64_t)n * a.nblk[l];
        float s = 0.f;
        for (int b = 0; b < a.nblk[l]; ++b) s += pl[b];
        const float m = s / (float)a.hw[l];
        val = l == 0 ? m : val + m;
    }
    d[n] = val;
}

}  // namespace

extern "C" int te_lpips_stem_fwd_f32(float* out, const float* x, const float* w, const float* b, int N, int H, int W, te_stream_t stream) {
    TE_REQUIRE(out && x && w && b, TE_ERR_NULL, "te_lpips_stem_fwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && H > 0 && W > 0 && N < 65536, TE_ERR_SHAPE, "te_lpips_stem_fwd_f32: bad dims");
    te::launch_vgg_stem<StemScaled>(out, x, w, b, N, H, W, H, W, 0, 0, stream);
    return te::launch_status("te_lpips_stem_fwd_f32");
}

extern "C" int te_vgg_stem_fwd_f32(float* out, const float* x, const float* w, const float* b, int N, int H, int W, te_stream_t stream) {
    TE_REQUIRE(out && x && w && b, TE_ERR_NULL, "te_vgg_stem_fwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && H > 0 && W > 0 && N < 65536, TE_ERR_SHAPE, "te_vgg_stem_fwd_f32: bad dims");
    te::launch_vgg_stem<StemIdentity>(out, x, w, b, N, H, W, H, W, 0, 0, stream);
    return te::launch_status("te_vgg_stem_fwd_f32");
}

extern "C" int te_lpips_stem_dgrad_f32(float* gx, const float* g, const float* y1, const float* w, int N, int H, int W,
                                       te_stream_t stream) {
    TE_REQUIRE(gx && g && y1 && w, TE_ERR_NULL, "te_lpips_stem_dgrad_f32: NULL pointer");
    TE_REQUIRE(N > 0 && H > 0 && W > 0 && N < 65536, TE_ERR_SHAPE, "te_lpips_stem_dgrad_f32: bad dims");
    const int64_t HW = (int64_t)H * W;
    stem_dgrad_kernel<<<dim3((unsigned)te::cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(gx, g, y1, w, H, W);
    return te::launch_status("te_lpips_stem_dgrad_f32");
}

extern "C" int te_maxpool2_fwd_f32(float* out, const float* x, int64_t planes, int H, int W, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_maxpool2_fwd_f32: NULL pointer");
    TE_REQUIRE(planes > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, TE_ERR_SHAPE, "te_maxpool2_fwd_f32: H, W must be even");
    const int64_t total = planes * (H / 2) * (W / 2);
    pool_fwd_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(out, x, total, H, W);
    return te::launch_status("te_maxpool2_fwd_f32");
}

extern "C" int te_maxpool2_bwd_f32(float* gx, const float* g, const float* x, int64_t planes, int H, int W, te_stream_t stream) {
    TE_REQUIRE(gx && g && x, TE_ERR_NULL, "te_maxpool2_bwd_f32: NULL pointer");
    TE_REQUIRE(planes > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, TE_ERR_SHAPE, "te_maxpool2_bwd_f32: H, W must be even");
    const int64_t total = planes * (H / 2) * (W / 2);
    pool_bwd_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(gx, g, x, total, H, W);
    return te::launch_status("te_maxpool2_bwd_f32");
}

extern "C" int te_lpips_normalize_f32(float* out, const float* x, int N, int C, int64_t HW, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_lpips_normalize_f32: NULL pointer");
    TE_REQUIRE(N > 0 && C > 0 && HW > 0 && N < 65536, TE_ERR_SHAPE, "te_lpips_normalize_f32: bad dims");
    normalize_kernel<<<dim3((unsigned)te::cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(out, x, C, HW);
    return te::launch_status("te_lpips_normalize_f32");
}

extern "C" int te_lpips_head_blocks(int64_t HW) { return HW > 0 ? (int)te::cdiv(HW, 256) : TE_ERR_SHAPE; }

extern "C" int te_lpips_head_fwd_f32(float* partial, const float* f, const float* t, const float* w, int N, int Nt, int C, int64_t HW,
                                     te_stream_t stream) {
    TE_REQUIRE(partial && f && t && w, TE_ERR_NULL, "te_lpips_head_fwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && C > 0 && HW > 0 && N < 65536 && (Nt == 1 || Nt == N), TE_ERR_SHAPE, "te_lpips_head_fwd_f32: bad dims");
    head_fwd_kernel<<<dim3((unsigned)te::cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(partial, f, t, w, Nt, C, HW);
    return te::launch_status("te_lpips_head_fwd_f32");
}

extern "C" int te_lpips_head_bwd_f32(float* gf, const float* gin, const float* gd, const float* f, const float* t, const float* w, int N,
                                     int Nt, int C, int64_t HW, int relu_mask, te_stream_t stream) {
    TE_REQUIRE(gf && gd && f && t && w, TE_ERR_NULL, "te_lpips_head_bwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && C > 0 && HW > 0 && N < 65536 && (Nt == 1 || Nt == N), TE_ERR_SHAPE, "te_lpips_head_bwd_f32: bad dims");
    head_bwd_kernel<<<dim3((unsigned)te::cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(gf, gin, gd, f, t, w, Nt, C, HW, relu_mask);
    return te::launch_status("te_lpips_head_bwd_f32");
}

extern "C" int te_lpips_dist_f32(float* d, const float* const* partial, const int64_t* hw, int L, int N, te_stream_t stream) {
    TE_REQUIRE(d && partial && hw, TE_ERR_NULL, "te_lpips_dist_f32: NULL pointer");
    TE_REQUIRE(L >= 1 && L <= 8 && N > 0, TE_ERR_SHAPE, "te_lpips_dist_f32: 1 <= L <= 8 layers");
    DistArgs a{};
    for (int l = 0; l < L; ++l) {
        TE_REQUIRE(partial[l] && hw[l] > 0, TE_ERR_NULL, "te_lpips_dist_f32: layer %d", l);
        a.partial[l] = partial[l];
        a.hw[l] = hw[l];
        a.nblk[l] = (int)te::cdiv(hw[l], 256);
    }
    dist_kernel<<<(unsigned)te::cdiv(N, 64), 64, 0, (hipStream_t)stream>>>(d, a, L, N);
    return te::launch_status("te_lpips_dist_f32");
}

static int pair_tile(int64_t HW) { return HW >= 256 ? 256 : (int)(te::cdiv(HW, 64) * 64); }

extern "C" int te_lpips_pair_head_fwd_f32(float* partial, const float* f, const float* w, int N, int C, int64_t HW, te_stream_t stream) {
    TE_REQUIRE(partial && f && w, TE_ERR_NULL, "te_lpips_pair_head_fwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && C > 0 && HW > 0 && N < 65536, TE_ERR_SHAPE, "te_lpips_pair_head_fwd_f32: bad dims");
    const int PT = pair_tile(HW);
    // one partial per 256 pixels: the split of te_lpips_head_blocks, so te_lpips_dist_f32 adds them as it adds the unpaired head's
    pair_head_kernel<<<dim3((unsigned)te::cdiv(HW, 256), N), kPairThreads, 0, (hipStream_t)stream>>>(partial, f, w, C, HW, PT);
    return te::launch_status("te_lpips_pair_head_fwd_f32");
}

extern "C" int te_crop_resize_bilinear_f32(float* out, const float* img, int B, int H, int W, int y0, int x0, int hc, int wc, int h,
                                           int w, te_stream_t stream) {
    TE_REQUIRE(out && img, TE_ERR_NULL, "te_crop_resize_bilinear_f32: NULL pointer");
    TE_REQUIRE(B > 0 && B < 21845 && H > 0 && W > 0 && h > 0 && w > 0, TE_ERR_SHAPE, "te_crop_resize_bilinear_f32: bad dims");
    TE_REQUIRE(y0 >= 0 && x0 >= 0 && hc > 0 && wc > 0 && (int64_t)y0 + hc <= H && (int64_t)x0 + wc <= W, TE_ERR_SHAPE,
               "te_crop_resize_bilinear_f32: window [%d:%d+%d, %d:%d+%d] outside %dx%d", y0, y0, hc, x0, x0, wc, H, W);
    TE_REQUIRE(hc % h == 0 && wc % w == 0, TE_ERR_SHAPE, "te_crop_resize_bilinear_f32: the window must be an integer multiple of the output");
    crop_resize_kernel<<<dim3((unsigned)te::cdiv((int64_t)h * w, 256), 3 * B), 256, 0, (hipStream_t)stream>>>(out, img, H, W, y0, x0, hc,
                                                                                                             wc, h, w);
    return te::launch_status("te_crop_resize_bilinear_f32");
}
