// The parts of the CelebA-HQ attribute classifier (our_interfaceGAN/celebahq_utils/dex/networks/classifiers/attribute_classifier.py: D
// with fixed_size=True, use_mbstd=False, a progressive-GAN discriminator with one logit; attribute_utils.py:8-32) that the 3x3
// convolutions of csrc/conv.hip / csrc/wino6.hip and the fc kernel of csrc/vggfc.hip do not cover:
//
//     te_attr_stem_fwd_f32 : the generator's RGB image in [-1, 1] -> BGR in {0, ..., 255} (edit_all_noinversion_celebahq.py:175-177),
//                            the f x f box mean down to the network's resolution (attribute_utils.py:8-19) and fromrgb_lod0 =
//                            1x1 convolution + bias + leaky ReLU (attribute_classifier.py:62-71), in one pass over the image
//     te_avgpool2_act_f32  : Downscale2d, then the activation (attribute_classifier.py:100-104: conv -> bias -> downscale -> act)
//     te_attr_score_f32    : the activation of dense0, dense1 (attribute_classifier.py:147-148) and softmax([l, -l])[:, 1]
//                            (attribute_utils.py:28-32)
//
// The stem is vgg_stem_kernel's shape (vgg_stem.h): one thread per output pixel, the weights in LDS, the three channel means in registers, the
// stores of one channel coalesced over the pixels.  The pool is memory bound: one thread per two output pixels with two 16-byte
// loads where the rows allow it, one thread per output pixel elsewhere; the grid is NOT capped and no thread loops.  The score head is
// shaped for latency: one wave per row, its lanes stride K with 16-byte loads, the sum is a fixed-shape butterfly (no atomics), so a
// row's result is bitwise independent of the batch it is in.
#include <float.h>
#include "te_common.h"
#include "byte_level.h"
#include "wave_dot.h"

namespace {

constexpr int kStemMaxC0 = 1024;                   // the stem's LDS holds w [C0,3] and b [C0]: 16 KB at the most

using te::f32x4;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// v > 0 ? v : slope * v: a NaN fails the comparison and stays a NaN
__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }

// out[n,o,y,x] = lrelu(b[o] + sum_c w[o,c] * m_c), m_c = the f x f box mean of v[n, c, f y .. f y + f - 1, f x .. f x + f - 1]: summed
// row-major in fp32 from 0, then divided by f * f; v = to_byte_level(img[n, 2 - c]) (RAW) or img[n, c] (!RAW)
template <bool RAW>
__global__ __launch_bounds__(256) void attr_stem_kernel(float* __restrict__ out, const float* __restrict__ img, const float* __restrict__ w,
                                                        const float* __restrict__ b, int S, int R, int f, int C0) {
    __shared__ float ws[kStemMaxC0 * 3];
    __shared__ float bs[kStemMaxC0];
    for (int i = threadIdx.x; i < C0 * 3; i += 256) ws[i] = w[i];
    for (int i = threadIdx.x; i < C0; i += 256) bs[i] = b[i];
    __syncthreads();
    const int n = blockIdx.y;
    const int RR = R * R;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= RR) return;
    const int yy = p / R, xx = p % R;
    const int64_t SS = (int64_t)S * S;
    const float ff = (float)(f * f);
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* xc = img + ((int64_t)n * 3 + (RAW ? 2 - c : c)) * SS + (int64_t)yy * f * S + (int64_t)xx * f;
        float s = 0.f;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) {
                const float t = xc[(int64_t)dy * S + dx];
                s += RAW ? te::to_byte_level(t) : t;
            }
        m[c] = __fdiv_rn(s, ff);
    }
    float* o = out + (int64_t)n * C0 * RR + p;
    for (int k = 0; k < C0; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc = fmaf(ws[k * 3 + c], m[c], acc);
        o[(int64_t)k * RR] = leaky(acc + bs[k], 0.2f);
    }
}

__device__ __forceinline__ float pool4(float x00, float x01, float x10, float x11, float slope) {
    return leaky((((x00 + x01) + x10) + x11) * 0.25f, slope);
}

// thread t2 = (row pair r, column quad j): rows 2 r and 2 r + 1 of the [planes * H, W] matrix (H is even, so a pair never straddles two
// planes), columns 4 j .. 4 j + 3 -> the two outputs (r, 2 j) and (r, 2 j + 1) of the [planes * H / 2, W / 2] matrix
__global__ __launch_bounds__(256) void avgpool2_act_vec_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t items, int W,
                                                               float slope) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const int Wq = W >> 2;
    const int64_t r = t / Wq;
    const int j = (int)(t - r * Wq);
    const float* x0 = x + 2 * r * W + 4 * j;
    const f32x4 a = *reinterpret_cast<const f32x4*>(x0);
    const f32x4 c = *reinterpret_cast<const f32x4*>(x0 + W);
    f32x2 o;
    o.x = pool4(a.x, a.y, c.x, c.y, slope);
    o.y = pool4(a.z, a.w, c.z, c.w, slope);
    *reinterpret_cast<f32x2*>(out + r * (W >> 1) + 2 * j) = o;
}

// one thread per output pixel
__global__ __launch_bounds__(256) void avgpool2_act_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t items, int W,
                                                           float slope) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const int Wh = W >> 1;
    const int64_t r = t / Wh;
    const int j = (int)(t - r * Wh);
    const float* x0 = x + 2 * r * W + 2 * j;
    out[t] = pool4(x0[0], x0[1], x0[W], x0[W + 1], slope);
}

// Row i = blockIdx.x, one wave: te::wave_dot (wave_dot.h) of leaky(a[i,:]) and w.
__global__ __launch_bounds__(64) void attr_score_kernel(float* __restrict__ logit, float* __restrict__ score, const float* __restrict__ a,
                                                        const float* __restrict__ w, const float* __restrict__ bias, int K, float slope) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const float l = te::wave_dot<2>(a + i * K, w, K, lane, [slope](float v) { return leaky(v, slope); }) + bias[0];
    if (lane != 0) return;
    if (logit) logit[i] = l;
    if (score) {
        // softmax([l, -l])[1] = 1 / (1 + exp(2 l)), with the exponential of the NEGATIVE magnitude so that it never overflows; a
        // score below FLT_MIN (l > 43.66) is returned as 0, so no denormal leaves the kernel.  A NaN logit takes the second branch.
        float s;
        if (l >= 0.f) {
            const float e = expf(-2.f * l);
            s = e < FLT_MIN ? 0.f : e / (1.f + e);
        } else {
            s = 1.f / (1.f + expf(2.f * l));
        }
        score[i] = s;
    }
}

}  // namespace

extern "C" int te_attr_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, int N, int S, int R, int C0,
                                    int preprocessed, te_stream_t stream) {
    TE_REQUIRE(out && img && w && b, TE_ERR_NULL, "te_attr_stem_fwd_f32: NULL pointer");
    TE_REQUIRE(N > 0 && N < 65536, TE_ERR_SHAPE, "te_attr_stem_fwd_f32: 1 <= N < 65536 (got %d)", N);
    TE_REQUIRE(R >= 1 && S >= R && S % R == 0 && S <= 32768, TE_ERR_SHAPE,
               "te_attr_stem_fwd_f32: the image size (%d) must be a positive multiple of the resolution (%d), at most 32768", S, R);
    TE_REQUIRE(C0 >= 1 && C0 <= kStemMaxC0, TE_ERR_SHAPE, "te_attr_stem_fwd_f32: 1 <= C0 <= %d (got %d)", kStemMaxC0, C0);
    TE_REQUIRE(preprocessed == 0 || preprocessed == 1, TE_ERR_UNSUPPORTED, "te_attr_stem_fwd_f32: preprocessed must be 0 or 1, got %d",
               preprocessed);
    const dim3 grid((unsigned)te::cdiv((int64_t)R * R, 256), N);
    if (preprocessed)
        attr_stem_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(out, img, w, b, S, R, S / R, C0);
    else
        attr_stem_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(out, img, w, b, S, R, S / R, C0);
    return te::launch_status("te_attr_stem_fwd_f32");
}

extern "C" int te_avgpool2_act_f32(float* out, const float* x, int64_t planes, int H, int W, float slope, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_avgpool2_act_f32: NULL pointer");
    TE_REQUIRE(planes > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, TE_ERR_SHAPE,
               "te_avgpool2_act_f32: planes >= 1 and even H, W >= 2 (got %lld planes of %d x %d)", (long long)planes, H, W);
    const int64_t outputs = planes * (H / 2) * (W / 2);
    TE_REQUIRE(planes <= ((int64_t)1 << 40) / ((int64_t)H * W) && te::cdiv(outputs, 256) <= 0x7fffffff, TE_ERR_SHAPE,
               "te_avgpool2_act_f32: %lld planes of %d x %d are more than one launch covers", (long long)planes, H, W);
    if (W % 4 == 0 && te::aligned16(x) && ((uintptr_t)out & 7) == 0) {
        const int64_t items = outputs / 2;
        avgpool2_act_vec_kernel<<<(unsigned)te::cdiv(items, 256), 256, 0, (hipStream_t)stream>>>(out, x, items, W, slope);
    } else {
        avgpool2_act_kernel<<<(unsigned)te::cdiv(outputs, 256), 256, 0, (hipStream_t)stream>>>(out, x, outputs, W, slope);
    }
    return te::launch_status("te_avgpool2_act_f32");
}

extern "C" int te_attr_score_f32(float* logit, float* score, const float* a, const float* w, const float* bias, int64_t I, int K,
                                 float slope, te_stream_t stream) {
    TE_REQUIRE((logit || score) && a && w && bias, TE_ERR_NULL, "te_attr_score_f32: NULL pointer (one of logit and score may be NULL)");
    TE_REQUIRE(I >= 1 && I <= 0x7fffffff, TE_ERR_SHAPE, "te_attr_score_f32: 1 <= I < 2^31 (got %lld)", (long long)I);
    TE_REQUIRE(K >= 4 && K % 4 == 0, TE_ERR_SHAPE, "te_attr_score_f32: K must be a positive multiple of 4 (got %d)", K);
    TE_REQUIRE(te::aligned16(a) && te::aligned16(w), TE_ERR_SHAPE, "te_attr_score_f32: a and w must be 16-byte aligned");
    attr_score_kernel<<<(unsigned)I, 64, 0, (hipStream_t)stream>>>(logit, score, a, w, bias, K, slope);
    return te::launch_status("te_attr_score_f32");
}
