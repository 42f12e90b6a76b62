// What the ArcFace IR-SE50 identity network (pSp/models/encoders/model_irse.py:10-49 Backbone with helpers.py:16-120, applied by
// pSp/criteria/id_loss.py:8-21) needs beyond te_conv2d_f32, te_adaptive_avgpool_f32 and te_fc_stream_f32:
//
//     te_conv2d_prelu_f32   : the first convolution of a unit: BatchNorm2d in FRONT of a zero-padded 3 x 3 convolution, then PReLU
//     te_id_stem_fwd_f32    : the crop, AdaptiveAvgPool2d((Pn, Pn)) and input_layer (conv 3 x 3 + batch norm + PReLU) in one pass
//     te_se_excite_f32      : the two 1 x 1 convolutions of SEModule on the pooled vector, ReLU and sigmoid
//     te_se_scale_add_f32   : res * gate + shortcut, the shortcut read with the stride of MaxPool2d(1, s)
//     te_rows_unit_f32      : l2_norm
//     te_rows_dot_f32       : the paired dot products of two sets of embeddings
//
// Both convolutions are the main loop of conv2d_body.h with other policies.  The batch norm in front of the padded convolution is a
// GATHER (a tap inside the image is scale[c] * x + shift[c], a tap of the padding is 0: the shift cannot be a bias, the padded taps
// do not carry it), PReLU is an epilogue; the stem's gather averages the tap's window of the full image on the way into LDS.  The
// forward pass; te_conv2d_prelu_keep_f32 and te_id_stem_keep_f32 are the same two kernels with an epilogue that also stores the
// pre-activation, for the backward pass of irse_bwd.hip.  No atomics, no workspace, every reduction a fixed-order chain or a fixed-shape tree.
#include "te_common.h"
#include "conv2d_body.h"
#include "irse_common.h"

namespace {

using namespace te::conv2d;
using namespace te::irse;
using te::wave_sum;

// ------------------------------------------------------------------------------------------------------ the two convolutions
struct PreluArgs : ConvArgs {
    const float* in_scale;       // [Ci] or NULL (then in_shift is NULL too)
    const float* in_shift;
    const float* slope;          // [Co]
    float* pre;                  // the *_keep entry points: where t goes, in the layout of out
};

struct IdStemArgs : PreluArgs {  // H = W = Pn: the convolution sees the pooled plane
    int IH, IW, y0, x0, Lh, Lw;  // the image's size, the window's corner in it and the window's sides
};

// scale[c] * x + shift[c] as ONE fma (a single rounding); c is wave-uniform.  The loop's own gather gives 0 outside the image.
struct GatherAffine {
    static __device__ __forceinline__ const float* image(const PreluArgs& a, int64_t b) { return a.x + b * a.Ci * a.H * a.W; }
    static __device__ __forceinline__ int plane(const PreluArgs& a) { return a.H * a.W; }
    static __device__ __forceinline__ float tap(const float* img, const PreluArgs& a, int HW, int c, int iy, int ix) {
        return fmaf(a.in_scale[c], img[c * HW + iy * a.W + ix], a.in_shift[c]);
    }
};

// tap (c, iy, ix) of the pooled Pn x Pn plane: the mean of window [floor(iy Lh / Pn), ceil((iy + 1) Lh / Pn)) x (likewise in x) of the
// Lh x Lw window of the image, summed row-major in fp32 and divided by the count: adaptive_avgpool_kernel (vggfc.hip) on the crop
struct GatherPooled {
    static __device__ __forceinline__ const float* image(const IdStemArgs& a, int64_t b) {
        return a.x + b * 3 * a.IH * a.IW + a.y0 * a.IW + a.x0;
    }
    static __device__ __forceinline__ int plane(const IdStemArgs& a) { return a.IH * a.IW; }
    static __device__ __forceinline__ float tap(const float* img, const IdStemArgs& a, int HW, int c, int iy, int ix) {
        int ya, yb, xa, xb;
        te::adaptive_window<int>(iy, a.Lh, a.H, ya, yb);                                // (Pn, Lh <= 32768: the products fit)
        te::adaptive_window<int>(ix, a.Lw, a.W, xa, xb);
        const float* src = img + c * HW;
        float s = 0.f;
        bool first = true;
        for (int yy = ya; yy < yb; ++yy)
            for (int xx = xa; xx < xb; ++xx) {
                const float v = src[yy * a.IW + xx];
                s = first ? v : __fadd_rn(s, v);
                first = false;
            }
        return __fdiv_rn(s, (float)((yb - ya) * (xb - xa)));
    }
};

// t = acc + bias (the loop's); out = t > 0 ? t : slope[m] * t.  A NaN fails the comparison and slope * NaN is a NaN.
struct EpiPrelu {
    template <class Args>
    static __device__ __forceinline__ float apply(const Args& a, float v, const float* dst, int m, int HoWo) {
        return v > 0.f ? v : __fmul_rn(a.slope[m], v);
    }
};

// the same, and t itself goes to pre: what the backward pass (irse_bwd.hip) takes the PReLU branch from.  With a negative slope a
// positive output does not tell the branch, so the differentiable forward keeps t; out has the bits EpiPrelu gives
struct EpiPreluKeep {
    template <class Args>
    static __device__ __forceinline__ float apply(const Args& a, float v, const float* dst, int m, int HoWo) {
        a.pre[(dst - a.out) + (int64_t)m * HoWo] = v;
        return v > 0.f ? v : __fmul_rn(a.slope[m], v);
    }
};

// (a.pre set: the keeping epilogue)
template <class Gather, class Args>
void launch_either(const Args& a, hipStream_t st) {
    if (a.pre) launch<Gather, EpiPreluKeep>(a, st);
    else launch<Gather, EpiPrelu>(a, st);
}

// ------------------------------------------------------------------------------------------------------ squeeze-and-excitation
// One workgroup of four waves per image.  Step 1: the waves split the R hidden units; a unit is one wave's dot product over the C
// pooled values (lane l takes k = l, l + 64, ... as one fma chain, the lanes' sums meet in a butterfly), ReLU -> LDS.  Step 2: a
// thread per channel (c = t, t + 256, ...): one fma chain over the R hidden units in ascending order, then the sigmoid with the
// exponential of the NEGATIVE magnitude, so nothing overflows.  Nothing depends on B.  (A unit is se_unit of irse_common.h.)
__global__ __launch_bounds__(kSeThreads) void se_excite_kernel(float* __restrict__ gate, const float* __restrict__ pooled,
                                                               const float* __restrict__ w1, const float* __restrict__ w2, int C, int R) {
    __shared__ float hidden[kSeMaxR];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float* p = pooled + (int64_t)blockIdx.x * C;
    for (int r = wid; r < R; r += kSeThreads / 64) {
        const float acc = se_unit(p, w1, C, r, lane);
        if (lane == 0) hidden[r] = te::relu_nan(acc);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kSeThreads) {
        const float* w = w2 + (int64_t)c * R;
        float z = 0.f;
        for (int r = 0; r < R; ++r) z = fmaf(w[r], hidden[r], z);
        float g;
        if (z >= 0.f) {
            g = 1.f / (1.f + expf(-z));
        } else {                                             // (a NaN logit comes here and stays a NaN)
            const float e = expf(z);
            g = e / (1.f + e);
        }
        gate[(int64_t)blockIdx.x * C + c] = g;
    }
}

// ------------------------------------------------------------------------------------------------------ res * gate + shortcut
// item t = four consecutive outputs of one plane (Ho * Wo is a multiple of 4, s = 1: sc has the layout of res)
template <bool GATE>
__global__ __launch_bounds__(256) void se_scale_add_vec_kernel(float* __restrict__ out, const float* __restrict__ res,
                                                               const float* __restrict__ gate, const float* __restrict__ sc, int64_t items,
                                                               int HoWo4) {
#pragma clang fp contract(off)   // the product is rounded before the sum: no fma
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const f32x4 r = *reinterpret_cast<const f32x4*>(res + 4 * t);
    const f32x4 h = *reinterpret_cast<const f32x4*>(sc + 4 * t);
    const float g = GATE ? gate[t / HoWo4] : 1.f;
    f32x4 o;
    o.x = (GATE ? r.x * g : r.x) + h.x;
    o.y = (GATE ? r.y * g : r.y) + h.y;
    o.z = (GATE ? r.z * g : r.z) + h.z;
    o.w = (GATE ? r.w * g : r.w) + h.w;
    *reinterpret_cast<f32x4*>(out + 4 * t) = o;
}

// one thread per output element
template <bool GATE>
__global__ __launch_bounds__(256) void se_scale_add_kernel(float* __restrict__ out, const float* __restrict__ res,
                                                           const float* __restrict__ gate, const float* __restrict__ sc, int64_t total, int Ho,
                                                           int Wo, int Hs, int Ws, int s) {
#pragma clang fp contract(off)   // the product is rounded before the sum: no fma
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int x = (int)(o % Wo), y = (int)(o / Wo % Ho);
    const int64_t plane = o / Wo / Ho;
    const float h = sc[(plane * Hs + (int64_t)s * y) * Ws + s * x];
    const float r = res[o];
    out[o] = (GATE ? r * gate[plane] : r) + h;
}

// ------------------------------------------------------------------------------------------------------ the rows
// Row i = blockIdx.x, one wave.  Lane l takes d = l, l + 64, ...; the squares (products) of fp32 values are exact in fp64, the
// lane's sum is an fp64 chain, the lanes' sums meet in an fp64 butterfly; the result is rounded to fp32 once.
__global__ __launch_bounds__(64) void rows_unit_kernel(float* __restrict__ out, const float* __restrict__ a, int D) {
    const int lane = threadIdx.x;
    const float* row = a + (int64_t)blockIdx.x * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = row[d];
        s = fma(v, v, s);
    }
    const float norm = (float)sqrt(wave_sum(s));
    float* o = out + (int64_t)blockIdx.x * D;
    for (int d = lane; d < D; d += 64) o[d] = __fdiv_rn(row[d], norm);          // (a zero row: 0 / 0 = NaN, as torch.div gives)
}

__global__ __launch_bounds__(64) void rows_dot_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                                                      int D) {
    const int lane = threadIdx.x;
    const float* ra = a + (int64_t)blockIdx.x * D;
    const float* rb = b + (int64_t)blockIdx.x * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s = fma((double)ra[d], (double)rb[d], s);
    s = wave_sum(s);
    if (lane == 0) out[blockIdx.x] = (float)s;
}

}  // namespace

namespace {

// te_conv2d_prelu_f32 (pre == NULL) and te_conv2d_prelu_keep_f32
int conv2d_prelu(const char* who, float* out, float* pre, const float* x, const float* w, const float* bias, const float* slope,
                 const float* in_scale, const float* in_shift, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px,
                 te_stream_t stream) {
    TE_REQUIRE(out && x && w && bias && slope, TE_ERR_NULL, "%s: NULL pointer", who);
    TE_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), TE_ERR_NULL, "%s: in_scale and in_shift must both be given or both be NULL", who);
    PreluArgs a;
    a.out = out; a.x = x; a.w = w; a.bias = bias; a.slope = slope; a.in_scale = in_scale; a.in_shift = in_shift; a.pre = pre;
    if (const int rc = fill_args(a, who, B, Ci, Co, H, W, kh, kw, s, py, px, Co, 0, 0)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (in_scale) launch_either<GatherAffine>(a, st);
    else launch_either<GatherPlain>(a, st);
    return te::launch_status(who);
}

// te_id_stem_fwd_f32 (pre == NULL) and te_id_stem_keep_f32
int id_stem(const char* who, float* out, float* pre, const float* img, const float* w, const float* b, const float* slope, int N, int H, int W,
            int y0, int y1, int x0, int x1, int Pn, int Co, te_stream_t stream) {
    TE_REQUIRE(out && img && w && b && slope, TE_ERR_NULL, "%s: NULL pointer", who);
    if (const int rc = check_id_window(who, N, H, W, y0, y1, x0, x1, Pn, Co)) return rc;
    IdStemArgs a;
    a.out = out; a.x = img; a.w = w; a.bias = b; a.slope = slope; a.in_scale = nullptr; a.in_shift = nullptr; a.pre = pre;
    if (const int rc = fill_args(a, who, N, 3, Co, Pn, Pn, 3, 3, 1, 1, 1, Co, 0, 0)) return rc;
    a.IH = H; a.IW = W; a.y0 = y0; a.x0 = x0; a.Lh = y1 - y0; a.Lw = x1 - x0;
    launch_either<GatherPooled>(a, (hipStream_t)stream);                         // K = 27 takes the unaligned weight path
    return te::launch_status(who);
}

}  // namespace

extern "C" int te_conv2d_prelu_f32(float* out, const float* x, const float* w, const float* bias, const float* slope, const float* in_scale,
                                   const float* in_shift, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px,
                                   te_stream_t stream) {
    return conv2d_prelu("te_conv2d_prelu_f32", out, nullptr, x, w, bias, slope, in_scale, in_shift, B, Ci, Co, H, W, kh, kw, s, py, px, stream);
}

extern "C" int te_conv2d_prelu_keep_f32(float* out, float* pre, const float* x, const float* w, const float* bias, const float* slope,
                                        const float* in_scale, const float* in_shift, int B, int Ci, int Co, int H, int W, int kh, int kw, int s,
                                        int py, int px, te_stream_t stream) {
    TE_REQUIRE(pre, TE_ERR_NULL, "te_conv2d_prelu_keep_f32: NULL pointer");
    return conv2d_prelu("te_conv2d_prelu_keep_f32", out, pre, x, w, bias, slope, in_scale, in_shift, B, Ci, Co, H, W, kh, kw, s, py, px, stream);
}

extern "C" int te_id_stem_fwd_f32(float* out, const float* img, const float* w, const float* b, const float* slope, int N, int H, int W,
                                  int y0, int y1, int x0, int x1, int Pn, int Co, te_stream_t stream) {
    return id_stem("te_id_stem_fwd_f32", out, nullptr, img, w, b, slope, N, H, W, y0, y1, x0, x1, Pn, Co, stream);
}

extern "C" int te_id_stem_keep_f32(float* out, float* pre, const float* img, const float* w, const float* b, const float* slope, int N, int H,
                                   int W, int y0, int y1, int x0, int x1, int Pn, int Co, te_stream_t stream) {
    TE_REQUIRE(pre, TE_ERR_NULL, "te_id_stem_keep_f32: NULL pointer");
    return id_stem("te_id_stem_keep_f32", out, pre, img, w, b, slope, N, H, W, y0, y1, x0, x1, Pn, Co, stream);
}

extern "C" int te_se_excite_f32(float* gate, const float* pooled, const float* w1, const float* w2, int B, int C, int R, te_stream_t stream) {
    TE_REQUIRE(gate && pooled && w1 && w2, TE_ERR_NULL, "te_se_excite_f32: NULL pointer");
    TE_REQUIRE(B >= 1 && C >= 1 && R >= 1 && R <= kSeMaxR && (int64_t)C * R <= 0x7fffffff, TE_ERR_SHAPE,
               "te_se_excite_f32: B, C >= 1, 1 <= R <= %d and C * R below 2^31 (got %d, %d, %d)", kSeMaxR, B, C, R);
    se_excite_kernel<<<(unsigned)B, kSeThreads, 0, (hipStream_t)stream>>>(gate, pooled, w1, w2, C, R);
    return te::launch_status("te_se_excite_f32");
}

extern "C" int te_se_scale_add_f32(float* out, const float* res, const float* gate, const float* sc, int B, int C, int Ho, int Wo, int Hs,
                                   int Ws, int s, te_stream_t stream) {
    TE_REQUIRE(out && res && sc, TE_ERR_NULL, "te_se_scale_add_f32: NULL pointer (gate alone may be NULL)");
    TE_REQUIRE(s == 1 || s == 2, TE_ERR_UNSUPPORTED, "te_se_scale_add_f32: the shortcut's stride must be 1 or 2 (got %d)", s);
    TE_REQUIRE(B >= 1 && C >= 1 && Ho >= 1 && Wo >= 1 && Hs >= 1 && Ws >= 1, TE_ERR_SHAPE,
               "te_se_scale_add_f32: B, C, Ho, Wo, Hs, Ws must be positive (got %d, %d, %d, %d, %d, %d)", B, C, Ho, Wo, Hs, Ws);
    TE_REQUIRE(Ho == (Hs - 1) / s + 1 && Wo == (Ws - 1) / s + 1, TE_ERR_SHAPE,
               "te_se_scale_add_f32: a %d x %d shortcut read with stride %d is %d x %d, not %d x %d", Hs, Ws, s, (Hs - 1) / s + 1,
               (Ws - 1) / s + 1, Ho, Wo);
    const int64_t planes = (int64_t)B * C;
    TE_REQUIRE((int64_t)Hs * Ws <= 0x7fffffff && planes <= ((int64_t)1 << 40) / ((int64_t)Hs * Ws), TE_ERR_SHAPE,
               "te_se_scale_add_f32: a plane must fit 31 bits and the shortcut 2^40 elements (got %lld planes of %d x %d)", (long long)planes, Hs,
               Ws);
    const int64_t total = planes * Ho * Wo;
    hipStream_t st = (hipStream_t)stream;
    if (s == 1 && Wo % 4 == 0 && te::aligned16(out) && te::aligned16(res) && te::aligned16(sc)) {
        const int64_t items = total / 4;
        const unsigned grid = (unsigned)te::cdiv(items, 256);
        if (gate) se_scale_add_vec_kernel<true><<<grid, 256, 0, st>>>(out, res, gate, sc, items, Ho * Wo / 4);
        else se_scale_add_vec_kernel<false><<<grid, 256, 0, st>>>(out, res, gate, sc, items, Ho * Wo / 4);
    } else {
        const unsigned grid = (unsigned)te::cdiv(total, 256);
        if (gate) se_scale_add_kernel<true><<<grid, 256, 0, st>>>(out, res, gate, sc, total, Ho, Wo, Hs, Ws, s);
        else se_scale_add_kernel<false><<<grid, 256, 0, st>>>(out, res, gate, sc, total, Ho, Wo, Hs, Ws, s);
    }
    return te::launch_status("te_se_scale_add_f32");
}

extern "C" int te_rows_unit_f32(float* out, const float* a, int64_t I, int D, te_stream_t stream) {
    TE_REQUIRE(out && a, TE_ERR_NULL, "te_rows_unit_f32: NULL pointer");
    TE_REQUIRE(I >= 1 && I <= 0x7fffffff && D >= 1, TE_ERR_SHAPE, "te_rows_unit_f32: 1 <= I < 2^31 and D >= 1 (got %lld, %d)", (long long)I, D);
    rows_unit_kernel<<<(unsigned)I, 64, 0, (hipStream_t)stream>>>(out, a, D);
    return te::launch_status("te_rows_unit_f32");
}

extern "C" int te_rows_dot_f32(float* out, const float* a, const float* b, int64_t I, int D, te_stream_t stream) {
    TE_REQUIRE(out && a && b, TE_ERR_NULL, "te_rows_dot_f32: NULL pointer");
    TE_REQUIRE(I >= 1 && I <= 0x7fffffff && D >= 1, TE_ERR_SHAPE, "te_rows_dot_f32: 1 <= I < 2^31 and D >= 1 (got %lld, %d)", (long long)I, D);
    rows_dot_kernel<<<(unsigned)I, 64, 0, (hipStream_t)stream>>>(out, a, b, D);
    return te::launch_status("te_rows_dot_f32");
}
