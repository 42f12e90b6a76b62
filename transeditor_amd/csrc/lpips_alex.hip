// The AlexNet LPIPS of the diversity score (metrics/lpips.py:49-82 as metrics/evaluate_query.py:82-133 calls it): the three pieces that
// te_conv2d_f32 and te_pool3_f32 do not cover.  conv2 ... conv5 of torchvision's alexnet().features run on te_conv2d_f32 (act 1), the
// two max pools in front of conv2 and conv3 on te_pool3_f32 mode 0; here:
//
//     te_alex_stem_fwd_f32      : (x - mu) / sigma, Conv2d(3, Co, 11, stride 4, padding 2), bias and ReLU in one pass over the image: the
//                                 main loop of conv2d_body.h with a gather that scales a tap on the way into LDS
//     te_lpips_unit_f32         : f * rsqrt(sum_c f^2 + 1e-10), the normalisation of metrics/lpips.py:16-17 (eps INSIDE the root)
//     te_lpips_allpairs_fwd_f32 : one layer's head for every pair of a group at once,
//     te_lpips_allpairs_dist_f32  and the sum of the layers' spatial means into D [N,N]
//
// The reference scores a group of 40 images as 780 calls that run the network on both images again; here the network runs once over
// the group and the pairs are a property of the head.  Forward only, NCHW fp32, no atomics, every reduction a fixed-order loop or a
// fixed-shape tree: results are bit-reproducible from run to run.
#include "te_common.h"
#include "conv2d_body.h"

namespace {

using namespace te::conv2d;

constexpr float kEps = 1e-10f;   // metrics/lpips.py:16

// ------------------------------------------------------------------------------------------------------------------ the stem
// a tap of the scaled image: (x[c] - mu[c]) / sigma[c], two correctly rounded fp32 steps (what torch's (x - mu) / sigma stores).  The
// loop's own gather gives 0 for a tap outside the image, so the zero padding is that of the SCALED image.  c is wave-uniform.
struct GatherScaled {
    static __device__ __forceinline__ const float* image(const ConvArgs& a, int64_t b) { return a.x + b * 3 * a.H * a.W; }
    static __device__ __forceinline__ int plane(const ConvArgs& a) { return a.H * a.W; }
    static __device__ __forceinline__ float tap(const float* img, const ConvArgs& a, int HW, int c, int iy, int ix) {
        const float mu = c == 0 ? -0.03f : c == 1 ? -0.088f : -0.188f;
        const float sigma = c == 0 ? 0.458f : c == 1 ? 0.448f : 0.450f;
        return __fdiv_rn(__fsub_rn(img[c * HW + iy * a.W + ix], mu), sigma);
    }
};

// ------------------------------------------------------------------------------------------------ the unit normalisation
// A block is 16 waves over a tile of PT = min(256, HW rounded up to 64) pixels, as pair_head_kernel (lpips.hip): PT / 64 waves side
// by side along the pixels, the other factor CG = 1024 / PT splits the channel loop.  Pass 1: each thread's sum of squares over its
// channel slice in fp64 (the squares are exact, the sum of a few hundred rounds far below fp32) -> LDS -> every thread adds the CG
// slices of its pixel in slice order; rsqrt(sum + eps) is evaluated in fp64 and rounded to fp32 once.  Pass 2: the slice's f * inv,
// one rounding.  A pixel that is zero on every channel: inv = 1e5, 0 * 1e5 = 0 exactly.  out may be f: a thread's pass-2 elements are
// its own pass-1 elements, and every pass-1 read of the block precedes the barrier.
constexpr int kUnitThreads = 1024;

__global__ __launch_bounds__(kUnitThreads) void unit_kernel(float* out, const float* f, int C, int64_t HW, int PT) {
    __shared__ double ss[kUnitThreads];
    const int n = blockIdx.y;
    const int CG = kUnitThreads / PT;
    const int pix = threadIdx.x % PT, cg = threadIdx.x / PT;      // PT is a multiple of 64: a wave has one cg, 64 consecutive pixels
    const int64_t p = (int64_t)blockIdx.x * PT + pix;
    const int cpg = (C + CG - 1) / CG;
    const int c0 = min(C, cg * cpg), c1 = min(C, c0 + cpg);
    const bool live = p < HW;
    const float* fn = f + (int64_t)n * C * HW + p;
    double s = 0.0;
    if (live) {
        double q[2] = {0.0, 0.0};                                 // two chains keep loads in flight
        int c = c0;
        for (; c + 2 <= c1; c += 2) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double a = fn[(int64_t)(c + k) * HW];
                q[k] = fma(a, a, q[k]);
            }
        }
        if (c < c1) {
            const double a = fn[(int64_t)c * HW];
            q[0] = fma(a, a, q[0]);
        }
        s = q[0] + q[1];
    }
    ss[threadIdx.x] = s;
    __syncthreads();
    if (!live) return;
    s = ss[pix];
    for (int g = 1; g < CG; ++g) s += ss[g * PT + pix];
    const float inv = (float)(1.0 / sqrt(s + (double)kEps));
    float* on = out + (int64_t)n * C * HW + p;
    for (int c = c0; c < c1; ++c) on[(int64_t)c * HW] = __fmul_rn(fn[(int64_t)c * HW], inv);
}

int unit_tile(int64_t HW) { return HW >= 256 ? 256 : (int)(te::cdiv(HW, 64) * 64); }

// ---------------------------------------------------------------------------------------------------- the all-pairs head
// A workgroup of 256 threads takes a block of 256 pixels (a thread owns one pixel: consecutive lanes read consecutive pixels of one
// channel plane), a slice of kCC channels and a tile of kT x kT images (ta <= tb: images 8 ta ... 8 ta + 7 against 8 tb ... 8 tb + 7).
// Per channel a thread loads its pixel of the 16 images (the next channel's loads are issued before this channel's arithmetic) and
// adds the 64 pairs' terms w[c] (a - b)^2 to 64 accumulators: the difference is formed before the square, w * d is rounded, then one
// fma.  A pair's accumulator is therefore a chain over the slice's channels in ascending order that sees the pair's own two values
// and nothing else; the block's 256 chains are added by a fixed tree (shuffle butterfly inside a wave, the four wave sums as
// (0 + 1) + (2 + 3)).  The partial of (pair, pixel block, channel slice) depends on nothing but the two images, C and HW: not on N,
// not on the tile, not on the other images.  (a - b) and (b - a) give the same term bit for bit, an image against itself gives 0 in
// every term.  Image slots past N read nothing and hold zeros; their partials are written and never read.
// The channel slices are there for the grid: at N = 40 the tiles are 15 and the three 15 x 15 planes of AlexNet one pixel block each,
// and a workgroup's arithmetic is 192 instructions per channel on each of four waves.
constexpr int kT = 8;
constexpr int kPB = 256;
constexpr int kCC = 32;

__host__ __device__ inline int64_t tile_pairs(int64_t T) { return T * (T + 1) / 2; }
// the index of tile (ta, tb), ta <= tb, among the upper-triangle tiles in row-major order
__host__ __device__ inline int64_t tile_index(int64_t ta, int64_t tb, int64_t T) { return ta * T - ta * (ta - 1) / 2 + (tb - ta); }

__global__ __launch_bounds__(kPB) void allpairs_kernel(float* __restrict__ partial, const float* __restrict__ fh, const float* __restrict__ w,
                                                       int N, int C, int64_t HW, int T) {
#pragma clang fp contract(off)   // w * d rounded before the fma, as pair_head_kernel
    __shared__ float part[4][kT * kT];
    const int ta = blockIdx.x / T, tb = blockIdx.x - ta * T;
    if (ta > tb) return;                                          // (the whole block: no barrier has been passed)
    const int64_t p = (int64_t)blockIdx.y * kPB + threadIdx.x;
    const bool live = p < HW;
    const int64_t CHW = (int64_t)C * HW;
    const float* pa[kT];
    const float* pb[kT];
    bool la[kT], lb[kT];
#pragma unroll
    for (int k = 0; k < kT; ++k) {
        const int i = ta * kT + k, j = tb * kT + k;
        la[k] = live && i < N;
        lb[k] = live && j < N;
        pa[k] = fh + (la[k] ? (int64_t)i * CHW + p : 0);
        pb[k] = fh + (lb[k] ? (int64_t)j * CHW + p : 0);
    }
    float acc[kT][kT];
#pragma unroll
    for (int i = 0; i < kT; ++i)
#pragma unroll
        for (int j = 0; j < kT; ++j) acc[i][j] = 0.f;
    const int c0 = blockIdx.z * kCC, c1 = min(C, c0 + kCC);
    float a[kT], b[kT], an[kT], bn[kT];
#pragma unroll
    for (int k = 0; k < kT; ++k) {
        an[k] = la[k] ? pa[k][(int64_t)c0 * HW] : 0.f;
        bn[k] = lb[k] ? pb[k][(int64_t)c0 * HW] : 0.f;
    }
    for (int c = c0; c < c1; ++c) {
        const float wc = w[c];
#pragma unroll
        for (int k = 0; k < kT; ++k) {
            a[k] = an[k];
            b[k] = bn[k];
        }
        if (c + 1 < c1) {                                         // in flight behind the 192 instructions below
            const int64_t o = (int64_t)(c + 1) * HW;
#pragma unroll
            for (int k = 0; k < kT; ++k) {
                an[k] = la[k] ? pa[k][o] : 0.f;
                bn[k] = lb[k] ? pb[k][o] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < kT; ++i)
#pragma unroll
            for (int j = 0; j < kT; ++j) {
                const float d = a[i] - b[j];
                acc[i][j] = fmaf(wc * d, d, acc[i][j]);           // (explicit fma: kept)
            }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kT; ++i)
#pragma unroll
        for (int j = 0; j < kT; ++j) {
            float v = acc[i][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) part[wid][i * kT + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < kT * kT) {
        const int t = threadIdx.x;
        const float s = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
        partial[((tile_index(ta, tb, T) * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z) * (kT * kT) + t] = s;
    }
}

struct PairDistArgs {
    const float* partial[8];
    int nblk[8];                 // pixel blocks x channel slices: a pair's partials of one layer, in the order they are added
    int64_t hw[8];
};

// D[i,j] = sum_l (sum_b partial_l[pair (min, max), b]) / HW_l, the partials (pixel blocks, and a block's channel slices inside it)
// and the layers in ascending order (metrics/lpips.py:77-81: lpips_value = 0; lpips_value += mean).  (i, j) and (j, i) read the same
// partials: D is symmetric bit for bit.
__global__ __launch_bounds__(256) void allpairs_dist_kernel(float* __restrict__ D, PairDistArgs a, int L, int N, int T) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (int64_t)N * N) return;
    const int i = (int)(o / N), j = (int)(o - (int64_t)i * N);
    const int lo = min(i, j), hi = max(i, j);
    const int64_t t = tile_index(lo / kT, hi / kT, T);
    const int local = (lo % kT) * kT + hi % kT;
    float val = 0.f;
    for (int l = 0; l < L; ++l) {
        const float* pl = a.partial[l] + t * a.nblk[l] * (kT * kT) + local;
        float s = 0.f;
#pragma unroll 8                 // (eight independent loads in flight; the additions stay in order)
        for (int b = 0; b < a.nblk[l]; ++b) s += pl[(int64_t)b * (kT * kT)];
        const float m = s / (float)a.hw[l];
        val = l == 0 ? m : val + m;
    }
    D[o] = val;
}

// the limits the three head entry points share
int check_head(const char* who, int N, int C, int64_t HW) {
    TE_REQUIRE(N >= 1 && N < 65536 && C >= 1 && HW >= 1, TE_ERR_SHAPE, "%s: 1 <= N < 65536 and positive C, HW (got %d, %d, %lld)", who, N, C,
               (long long)HW);
    TE_REQUIRE(HW <= (int64_t)65535 * kPB && (int64_t)C * HW <= 0x7fffffff && C <= 65535 * kCC, TE_ERR_SHAPE,
               "%s: HW must stay below 65535 * 256, C below 65535 * 32 and one image's tap (C * HW) must fit 31 bits (got %d x %lld)", who, C,
               (long long)HW);
    return 0;
}

}  // namespace

extern "C" int te_alex_stem_fwd_f32(float* out, const float* x, const float* w, const float* b, int N, int H, int W, int Co,
                                    te_stream_t stream) {
    TE_REQUIRE(out && x && w && b, TE_ERR_NULL, "te_alex_stem_fwd_f32: NULL pointer");
    TE_REQUIRE(N >= 1 && N < 65536 && H >= 1 && W >= 1 && Co >= 1, TE_ERR_SHAPE,
               "te_alex_stem_fwd_f32: 1 <= N < 65536 and positive H, W, Co (got %d, %d, %d, %d)", N, H, W, Co);
    TE_REQUIRE(H + 4 >= 11 && W + 4 >= 11, TE_ERR_SHAPE, "te_alex_stem_fwd_f32: an 11 x 11 kernel with padding 2 does not fit a %d x %d image", H,
               W);
    TE_REQUIRE((int64_t)3 * H * W <= 0x7fffffff, TE_ERR_SHAPE, "te_alex_stem_fwd_f32: one image (3 * H * W) must fit 31 bits");
    ConvArgs a;
    a.out = out; a.x = x; a.w = w; a.bias = b;
    if (const int rc = fill_args(a, "te_alex_stem_fwd_f32", N, 3, Co, H, W, 11, 11, 4, 2, 2, Co, 0, 1, 11, true)) return rc;
    launch<GatherScaled, EpiBiasAct, PartWhole, false>(a, (hipStream_t)stream);                  // K = 363: the unaligned weight path
    return te::launch_status("te_alex_stem_fwd_f32");
}

extern "C" int te_lpips_unit_f32(float* out, const float* f, int N, int C, int64_t HW, te_stream_t stream) {
    TE_REQUIRE(out && f, TE_ERR_NULL, "te_lpips_unit_f32: NULL pointer");
    if (const int rc = check_head("te_lpips_unit_f32", N, C, HW)) return rc;
    const int PT = unit_tile(HW);
    unit_kernel<<<dim3((unsigned)te::cdiv(HW, PT), N), kUnitThreads, 0, (hipStream_t)stream>>>(out, f, C, HW, PT);
    return te::launch_status("te_lpips_unit_f32");
}

extern "C" int64_t te_lpips_allpairs_ws_floats(int N, int C, int64_t HW) {
    if (N < 1 || N >= 65536 || C < 1 || C > 65535 * kCC || HW < 1 || HW > (int64_t)65535 * kPB) return TE_ERR_SHAPE;
    return tile_pairs(te::cdiv(N, kT)) * te::cdiv(HW, kPB) * te::cdiv(C, kCC) * (kT * kT);
}

extern "C" int te_lpips_allpairs_fwd_f32(float* partial, const float* fh, const float* w, int N, int C, int64_t HW, te_stream_t stream) {
    TE_REQUIRE(partial && fh && w, TE_ERR_NULL, "te_lpips_allpairs_fwd_f32: NULL pointer");
    if (const int rc = check_head("te_lpips_allpairs_fwd_f32", N, C, HW)) return rc;
    const int T = (int)te::cdiv(N, kT);
    const dim3 grid((unsigned)(T * T), (unsigned)te::cdiv(HW, kPB), (unsigned)te::cdiv(C, kCC));
    allpairs_kernel<<<grid, kPB, 0, (hipStream_t)stream>>>(partial, fh, w, N, C, HW, T);
    return te::launch_status("te_lpips_allpairs_fwd_f32");
}

extern "C" int te_lpips_allpairs_dist_f32(float* D, const float* const* partial, const int* c, const int64_t* hw, int L, int N,
                                          te_stream_t stream) {
    TE_REQUIRE(D && partial && c && hw, TE_ERR_NULL, "te_lpips_allpairs_dist_f32: NULL pointer");
    TE_REQUIRE(L >= 1 && L <= 8 && N >= 1 && N < 65536, TE_ERR_SHAPE, "te_lpips_allpairs_dist_f32: 1 <= L <= 8 layers and 1 <= N < 65536 (got %d, %d)",
               L, N);
    PairDistArgs a{};
    for (int l = 0; l < L; ++l) {
        TE_REQUIRE(partial[l], TE_ERR_NULL, "te_lpips_allpairs_dist_f32: layer %d has no partials", l);
        TE_REQUIRE(hw[l] >= 1 && hw[l] <= (int64_t)65535 * kPB && c[l] >= 1 && c[l] <= 65535 * kCC && (int64_t)c[l] * hw[l] <= 0x7fffffff,
                   TE_ERR_SHAPE, "te_lpips_allpairs_dist_f32: layer %d has C = %d, HW = %lld", l, c[l], (long long)hw[l]);
        a.partial[l] = partial[l];
        a.hw[l] = hw[l];
        a.nblk[l] = (int)(te::cdiv(hw[l], kPB) * te::cdiv(c[l], kCC));             // (below 2^31: C * HW is)
    }
    const int T = (int)te::cdiv(N, kT);
    allpairs_dist_kernel<<<(unsigned)te::cdiv((int64_t)N * N, 256), 256, 0, (hipStream_t)stream>>>(D, a, L, N, T);
    return te::launch_status("te_lpips_allpairs_dist_f32");
}
