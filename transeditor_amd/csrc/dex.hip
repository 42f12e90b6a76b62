// The two ends of the DEX age / gender scorer (our_interfaceGAN/ffhq_utils/dex/{api,models}.py: a VGG16 with a softmax over 101 ages or
// 2 genders) that the VGG trunk of csrc/lpips.hip and the fc kernel of csrc/vggfc.hip do not cover:
//
//     te_dex_stem_fwd_f32 : the generator's RGB image in [-1, 1] -> BGR in {0, ..., 255} (edit_all_noinversion_ffhq.py:113-116), the
//                           centre crop (api.py:47-52, :62) and conv1_1 + ReLU (models.py:11-12), in one pass over the image
//     te_cls_score_f32    : cls -> softmax (models.py:55-56) -> the expected age sum_c (c + 1) p_c (api.py:42-44, :56-58) or the
//                           first class's probability (api.py:64)
//
// The stem is vgg_stem_kernel (vgg_stem.h) with the rule StemByteBgr on the crop's window: one thread per output pixel, the weights
// in LDS, the 27 inputs in registers.  The head is shaped for latency, not throughput: one workgroup per row, its 16 waves split the classes, the
// lanes of a wave stride K with 16-byte loads.  Every reduction is a fixed-shape tree (no atomics) over the row's own data, so a row's
// result is bitwise independent of the batch it is in.
#include "te_common.h"
#include "byte_level.h"
#include "vgg_stem.h"
#include "wave_dot.h"

namespace {

// the stem's input rule: v = to_byte_level(img[n, 2 - c]), clamp / +1 / /2 / *255 / round in torch's bits (byte_level.h); the reference
// crops first, then nn.Conv2d pads
struct StemByteBgr {
    static constexpr bool kWindow = true;
    static __device__ __forceinline__ int channel(int c) { return 2 - c; }
    static __device__ __forceinline__ float value(float v, int) { return te::to_byte_level(v); }
};

constexpr int kHeadThreads = 1024;                 // 16 waves; also the most classes (one thread per class in the softmax)
constexpr int kHeadWaves = kHeadThreads / 64;

using te::wave_max;
using te::wave_sum;

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
// w[c,:] (te::wave_dot, wave_dot.h), the logit goes to LDS.
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
        const float s = te::wave_dot<4>(ai, w + (int64_t)c * K, K, lane, [](float v) { return v; });
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

}  // namespace

extern "C" int te_dex_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int H, int W, int crop,
                                   te_stream_t stream) {
    TE_REQUIRE(out && img && w && b, TE_ERR_NULL, "te_dex_stem_fwd_f32: NULL pointer");
    if (const int rc = te::check_centre_crop("te_dex_stem_fwd_f32", N, H, W, crop, 64)) return rc;      // (conv1_1 has 64 channels)
    te::launch_vgg_stem<StemByteBgr>(out, img, w, b, N, H, W, crop, crop, (H - crop) / 2, (W - crop) / 2, stream);
    return te::launch_status("te_dex_stem_fwd_f32");
}

extern "C" int te_cls_score_f32(float* score, float* prob, const float* a, const float* w, const float* bias, int64_t I, int C, int K,
                                int mode, te_stream_t stream) {
    TE_REQUIRE(score && a && w && bias, TE_ERR_NULL, "te_cls_score_f32: NULL pointer");
    TE_REQUIRE(I >= 1 && I <= 0x7fffffff, TE_ERR_SHAPE, "te_cls_score_f32: 1 <= I < 2^31 (got %lld)", (long long)I);
    TE_REQUIRE(C >= 1 && C <= kHeadThreads, TE_ERR_SHAPE, "te_cls_score_f32: 1 <= C <= %d (got %d)", kHeadThreads, C);
    TE_REQUIRE(K >= 4 && K % 4 == 0, TE_ERR_SHAPE, "te_cls_score_f32: K must be a positive multiple of 4 (got %d)", K);
    TE_REQUIRE(te::aligned16(a) && te::aligned16(w), TE_ERR_SHAPE, "te_cls_score_f32: a and w must be 16-byte aligned");
    TE_REQUIRE(mode == 0 || mode == 1, TE_ERR_UNSUPPORTED, "te_cls_score_f32: mode must be 0 (expectation) or 1 (p_0), got %d", mode);
    cls_score_kernel<<<(unsigned)I, kHeadThreads, 0, (hipStream_t)stream>>>(score, prob, a, w, bias, C, K, mode);
    return te::launch_status("te_cls_score_f32");
}
