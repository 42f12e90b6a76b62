// The two ends of the DEX age / gender scorer (our_interfaceGAN/ffhq_utils/dex/{api,models}.py: a VGG16 with a softmax over 101 ages or
// 2 genders) that the VGG trunk of csrc/lpips.hip and the fc kernel of csrc/vggfc.hip do not cover:
//
//     te_dex_stem_fwd_f32 : the generator's RGB image in [-1, 1] -> BGR in {0, ..., 255} (edit_all_noinversion_ffhq.py:113-116), the
//                           centre crop (api.py:47-52, :62) and conv1_1 + ReLU (models.py:11-12), in one pass over the image
//     te_cls_score_f32    : cls -> softmax (models.py:55-56) -> the expected age sum_c (c + 1) p_c (api.py:42-44, :56-58) or the
//                           first class's probability (api.py:64)
//
// The stem is stem_fwd_kernel of csrc/lpips.hip with another input rule: one thread per output pixel, the weights in LDS, the 27
// inputs in registers.  The head is shaped for latency, not throughput: one workgroup per row, its 16 waves split the classes, the
// lanes of a wave stride K with 16-byte loads.  Every reduction is a fixed-shape tree (no atomics) over the row's own data, so a row's
// result is bitwise independent of the batch it is in.
#include "te_common.h"
#include "byte_level.h"

namespace {

using te::to_byte_level;                           // clamp / +1 / /2 / *255 / round in torch's bits (byte_level.h)

// out[n,o,y,x] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * v[n, 2 - c, y0 + y + ky - 1, x0 + x + kx - 1]), v = to_byte_level(img), for
// (y, x) in the crop x crop window at (y0, x0); a tap outside the WINDOW is zero (the reference crops first, then nn.Conv2d pads).
__global__ __launch_bounds__(256) void dex_stem_kernel(float* __restrict__ out, const float* __restrict__ img, const float* __restrict__ w,
                                                       const float* __restrict__ b, int H, int W, int crop, int y0, int x0) {
    __shared__ float ws[64 * 27];
    __shared__ float bs[64];
    for (int i = threadIdx.x; i < 64 * 27; i += 256) ws[i] = w[i];
    if (threadIdx.x < 64) bs[threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int CC = crop * crop;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= CC) return;
    const int yy = p / crop, xx = p % crop;
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* xc = img + ((int64_t)n * 3 + (2 - c)) * HW;             // BGR: the convolution's channel c is the image's 2 - c
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = yy + ky - 1, ix = xx + kx - 1;
                const bool ok = iy >= 0 && iy < crop && ix >= 0 && ix < crop;
                in[c * 9 + ky * 3 + kx] = ok ? to_byte_level(xc[(int64_t)(y0 + iy) * W + (x0 + ix)]) : 0.f;
            }
        }
    }
    float* o = out + (int64_t)n * 64 * CC + p;
    for (int m = 0; m < 64; ++m) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = fmaf(ws[m * 27 + k], in[k], acc);
        acc += bs[m];
        o[(int64_t)m * CC] = acc > 0.f ? acc : (acc != acc ? acc : 0.f);      // torch's relu: a NaN propagates
    }
}

constexpr int kHeadThreads = 1024;                 // 16 waves; also the most classes (one thread per class in the softmax)
constexpr int kHeadWaves = kHeadThreads / 64;

using f32x4 = __attribute__((ext_vector_type(4))) float;

// all 64 lanes end with the same value: a butterfly whose shape does not depend on the data
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// the 16 wave values in wave order, by every thread alike.  `part` is free again when the call returns.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* part) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = MAX ? wave_max(v) : wave_sum(v);
    if (lane == 0) part[wid] = v;
    __syncthreads();
    float r = part[0];
#pragma unroll
    for (int k = 1; k < kHeadWaves; ++k) r = MAX ? fmaxf(r, part[k]) : r + part[k];
    __syncthreads();
    return r;
}

// Row i = blockIdx.x.  Pass 1: wave `wid` owns the classes wid, wid + 16, ...; lane l takes k = 4 l, 4 l + 256, ... of a[i,:] and
// w[c,:] as 16-byte loads into four fma chains (one per vector component), the lanes' sums meet in a butterfly, the logit goes to LDS.
// Pass 2: thread c owns class c: the row maximum, exp(logit - max), their sum, p = e / sum, the score's weighted sum.
__global__ __launch_bounds__(kHeadThreads) void cls_score_kernel(float* __restrict__ score, float* __restrict__ prob,
                                                                 const float* __restrict__ a, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, int C, int K, int mode) {
    __shared__ float logit[kHeadThreads];
    __shared__ float part[kHeadWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const float* ai = a + i * K;
    for (int c = wid; c < C; c += kHeadWaves) {
        const float* wc = w + (int64_t)c * K;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = 4 * lane; k < K; k += 256) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(ai + k);
            const f32x4 y = *reinterpret_cast<const f32x4*>(wc + k);
            acc.x = fmaf(x.x, y.x, acc.x);
            acc.y = fmaf(x.y, y.y, acc.y);
            acc.z = fmaf(x.z, y.z, acc.z);
            acc.w = fmaf(x.w, y.w, acc.w);
        }
        const float s = wave_sum((acc.x + acc.y) + (acc.z + acc.w));
        if (lane == 0) logit[c] = s + bias[c];
    }
    __syncthreads();
    const int c = threadIdx.x;
    const bool live = c < C;
    const float l = live ? logit[c] : -INFINITY;
    const float m = block_reduce<true>(l, part);          // (fmaxf passes over a NaN; it comes back through exp below, as in torch)
    const float e = live ? expf(l - m) : 0.f;
    const float sum = block_reduce<false>(e, part);
    const float p = e / sum;
    if (prob && live) prob[i * C + c] = p;
    if (mode == 0) {
        const float ex = block_reduce<false>(live ? (float)(c + 1) * p : 0.f, part);
        if (c == 0) score[i] = ex;
    } else if (c == 0) {
        score[i] = p;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int te_dex_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int H, int W, int crop,
                                   te_stream_t stream) {
    TE_REQUIRE(out && img && w && b, TE_ERR_NULL, "te_dex_stem_fwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && H > 0 && W > 0 && N < 65536, TE_ERR_SHAPE, "te_dex_stem_fwd_f32: bad dims");
    TE_REQUIRE(crop >= 1 && crop <= H && crop <= W && crop <= 32768, TE_ERR_SHAPE,
               "te_dex_stem_fwd_f32: the crop (%d) must be positive and fit the %d x %d image", crop, H, W);
    TE_REQUIRE((H - crop) % 2 == 0 && (W - crop) % 2 == 0, TE_ERR_SHAPE,
               "te_dex_stem_fwd_f32: a centre crop of %d needs H - crop and W - crop even (got %d x %d)", crop, H, W);
    const int CC = crop * crop;
    dex_stem_kernel<<<dim3((unsigned)te::cdiv(CC, 256), N), 256, 0, (hipStream_t)stream>>>(out, img, w, b, H, W, crop, (H - crop) / 2,
                                                                                          (W - crop) / 2);
    return te::launch_status("te_dex_stem_fwd_f32");
}

extern "C" int te_cls_score_f32(float* score, float* prob, const float* a, const float* w, const float* bias, int64_t I, int C, int K,
                                int mode, te_stream_t stream) {
    TE_REQUIRE(score && a && w && bias, TE_ERR_NULL, "te_cls_score_f32: NULL pointer");
    TE_REQUIRE(I >= 1 && I <= 0x7fffffff, TE_ERR_SHAPE, "te_cls_score_f32: 1 <= I < 2^31 (got %lld)", (long long)I);
    TE_REQUIRE(C >= 1 && C <= kHeadThreads, TE_ERR_SHAPE, "te_cls_score_f32: 1 <= C <= %d (got %d)", kHeadThreads, C);
    TE_REQUIRE(K >= 4 && K % 4 == 0, TE_ERR_SHAPE, "te_cls_score_f32: K must be a positive multiple of 4 (got %d)", K);
    TE_REQUIRE(aligned16(a) && aligned16(w), TE_ERR_SHAPE, "te_cls_score_f32: a and w must be 16-byte aligned");
    TE_REQUIRE(mode == 0 || mode == 1, TE_ERR_UNSUPPORTED, "te_cls_score_f32: mode must be 0 (expectation) or 1 (p_0), got %d", mode);
    cls_score_kernel<<<(unsigned)I, kHeadThreads, 0, (hipStream_t)stream>>>(score, prob, a, w, bias, C, K, mode);
    return te::launch_status("te_cls_score_f32");
}
