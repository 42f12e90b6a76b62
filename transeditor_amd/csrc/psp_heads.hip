// What the dual-space pSp encoder (pSp/models/encoders/psp_encoders_new.py:35-140 GradualStyleEncoder(50, 'ir_se'), applied by
// pSp/models/psp_new.py:90-109) needs beyond the IR-SE units of irse.hip and te_conv2d_f32:
//
//     te_conv2d_heads_f32   : G convolutions of one shape in one launch (the 30 GradualStyleBlock heads, level by level), bias and
//                             leaky ReLU fused, on a shared input or on each head's own; 1 x 1 on a 1 x 1 plane is the grouped EqualLinear
//     te_upsample_add_f32   : _upsample_add: bilinear align_corners=True upsampling plus the lateral
//     te_psp_codes_f32      : stack, adjust_style over the head axis, permute and the latent averages
//
// The grouped convolution is the main loop of conv2d_body.h with one more gather (the workgroup's 64-channel block names its head,
// the head names the channel offset of its input), one more epilogue (leaky ReLU) and, for planes of a few pixels, one more part
// policy: the k chain is cut into S ranges that S workgroups run, the partial tiles go to a workspace and a second kernel adds them
// over s ascending.  The k permutation is untouched.  Forward only, no atomics, every sum a fixed-order chain: bit-reproducible, an
// image's outputs independent of the batch it is in.
#include "te_common.h"
#include "conv2d_body.h"
#include "psp_upsample.h"

namespace {

using namespace te::conv2d;
using te::psp::corner_tap;

constexpr int kMaxSplits = 16;
// The split rule, from (K, Ho * Wo) alone (measured: profiles/README.md, 'Encoder inversion'): a plane of at most kSplitPlane pixels
// is one 64-pixel tile per image at the most, so at batch 1 the grid is G * Cg / 64 workgroups (240 for the 30 heads, fewer where a
// level is two launches) that each walk all of K; from kSplitMinK on the chain is cut into kSplitWays ranges.
constexpr int kSplitPlane = 64;
constexpr int kSplitMinK = 2048;
constexpr int kSplitWays = 8;

struct HeadsArgs : ConvArgs {
    int64_t xb;                  // floats between two images of x: Gx * Ci * H * W, Gx = 1 (shared) or G
    int64_t xg;                  // floats between the inputs of two heads: 0 (shared) or Ci * H * W
    int64_t part;                // floats between two partial results of the workspace: B * G * Cg * Ho * Wo
    int Cg, kper;                // channels per head; k per range (a multiple of BK)
    float slope;
};

// head g = the workgroup's channel block / (Cg / 64): Cg % 64 == 0, so a block never straddles two heads
struct GatherHeads {
    static __device__ __forceinline__ const float* image(const HeadsArgs& a, int64_t b) {
        return a.x + b * a.xb + (int64_t)(blockIdx.y * BM / a.Cg) * a.xg;
    }
    static __device__ __forceinline__ int plane(const HeadsArgs& a) { return a.H * a.W; }
    static __device__ __forceinline__ float tap(const float* img, const HeadsArgs& a, int HW, int c, int iy, int ix) {
        return img[c * HW + iy * a.W + ix];
    }
};

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : __fmul_rn(v, slope); }   // a NaN fails v > 0 and stays one

struct EpiLeaky {
    static __device__ __forceinline__ float apply(const HeadsArgs& a, float v, const float* dst, int m, int HoWo) { return leaky(v, a.slope); }
};

struct EpiPartial {
    static __device__ __forceinline__ float apply(const HeadsArgs& a, float v, const float* dst, int m, int HoWo) { return v; }
};

// range blockIdx.z of the k chain; the bare accumulators go to ws[blockIdx.z][B][G * Cg][Ho * Wo] (Ctot = Co, c0 = 0 there)
struct PartSplit : DestDense {
    static __device__ __forceinline__ int k_begin(const HeadsArgs& a) { return blockIdx.z * a.kper; }
    static __device__ __forceinline__ int k_end(const HeadsArgs& a) { return min(a.K, (int)(blockIdx.z + 1) * a.kper); }
    static __device__ __forceinline__ float* out(const HeadsArgs& a) { return a.out + blockIdx.z * a.part; }
    static __device__ __forceinline__ float finish(const HeadsArgs& a, float acc, int m) { return acc; }
};

// out[b, c0 + m, r] = leaky(((ws[0] + ws[1]) + ... + ws[S - 1]) + bias[m]); one thread per output element
__global__ __launch_bounds__(256) void heads_reduce_kernel(float* __restrict__ out, const float* __restrict__ ws, const float* __restrict__ bias,
                                                           int64_t total, int64_t part, int Co, int HoWo, int S, int Ctot, int c0, float slope) {
#pragma clang fp contract(off)
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int r = (int)(o % HoWo);
    const int64_t bm = o / HoWo;
    const int64_t b = bm / Co;
    const int m = (int)(bm - b * Co);
    float v = ws[o];
    for (int s = 1; s < S; ++s) v = v + ws[s * part + o];
    out[(b * Ctot + c0 + m) * HoWo + r] = leaky(v + bias[m], slope);
}

inline int steps_of(int64_t K) { return (int)te::cdiv(K, (int64_t)BK); }

// the rule's S for (K, Ho * Wo)
inline int rule_splits(int64_t K, int64_t HoWo) {
    if (HoWo > kSplitPlane || K < kSplitMinK) return 1;
    const int steps = steps_of(K);
    return (int)te::cdiv(steps, te::cdiv(steps, kSplitWays));
}

inline bool heads_dims_ok(int Ci, int kh, int kw, int Ho, int Wo) {
    return Ci >= 1 && kh >= 1 && kh <= kMaxKernel && kw >= 1 && kw <= kMaxKernel && Ho >= 1 && Wo >= 1 &&
           (int64_t)Ci * kh * kw <= 0x7fffffff - BK && (int64_t)Ho * Wo <= 0x7fffffff;
}

// ------------------------------------------------------------------------------------------------------ upsample and add
// corner_tap (psp_upsample.h): the taps and their weights.  A tap of weight 0 is not read into the mix, so equal sizes give x + y.
__device__ __forceinline__ float mix(float l0, float a, float l1, float b) { return l1 == 0.f ? a : fmaf(l1, b, __fmul_rn(l0, a)); }

__global__ __launch_bounds__(256) void upsample_add_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ y,
                                                           int h, int w, int H, int W) {
#pragma clang fp contract(off)
    const int64_t plane = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int oy = (int)(i / W), ox = (int)(i % W);
    int ya, yb, xa, xb;
    float ly0, ly1, lx0, lx1;
    corner_tap(oy, h, H, ya, yb, ly0, ly1);
    corner_tap(ox, w, W, xa, xb, lx0, lx1);
    const float* src = x + plane * h * w;
    const float* ra = src + (int64_t)ya * w;
    const float* rb = src + (int64_t)yb * w;
    const float top = mix(lx0, ra[xa], lx1, ra[xb]);
    const float v = ly1 == 0.f ? top : mix(ly0, top, ly1, mix(lx0, rb[xa], lx1, rb[xb]));
    out[plane * H * W + i] = v + y[plane * H * W + i];
}

// ------------------------------------------------------------------------------------------------------ the codes
// item i = (b, t, c), c fastest (the reads of lat run along c): t < T is z[b, c, t], t >= T is p[b, c, t - T]
__global__ __launch_bounds__(256) void psp_codes_kernel(float* __restrict__ z, float* __restrict__ p, const float* __restrict__ lat,
                                                        const float* __restrict__ A, const float* __restrict__ bz, const float* __restrict__ z_avg,
                                                        const float* __restrict__ p_avg, int64_t total, int Ns, int Np, int D, int T) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % D);
    const int t = (int)(i / D % (T + Np));
    const int64_t b = i / D / (T + Np);
    const float* row = lat + b * (Ns + Np) * D + c;
    if (t < T) {
        float acc = bz[t];
        for (int j = 0; j < Ns; ++j) acc = fmaf(A[t * Ns + j], row[(int64_t)j * D], acc);
        if (z_avg) acc = acc + z_avg[c * T + t];
        z[(b * D + c) * T + t] = acc;
    } else {
        const int u = t - T;
        float v = row[(int64_t)(Ns + u) * D];
        if (p_avg) v = v + p_avg[c * Np + u];
        p[(b * D + c) * Np + u] = v;
    }
}

}  // namespace

extern "C" int te_conv2d_heads_splits(int Ci, int kh, int kw, int Ho, int Wo) {
    if (!heads_dims_ok(Ci, kh, kw, Ho, Wo)) return TE_ERR_SHAPE;
    return rule_splits((int64_t)Ci * kh * kw, (int64_t)Ho * Wo);
}

extern "C" int64_t te_conv2d_heads_ws_bytes(int64_t B, int G, int Cg, int Ci, int kh, int kw, int Ho, int Wo) {
    if (!heads_dims_ok(Ci, kh, kw, Ho, Wo) || B < 1 || B > 0x7fffffff || G < 1 || Cg < 1 || (int64_t)G * Cg > 65535 * (int64_t)BM)
        return TE_ERR_SHAPE;
    const int S = rule_splits((int64_t)Ci * kh * kw, (int64_t)Ho * Wo);
    const int64_t per = (int64_t)G * Cg * Ho * Wo;
    if (per > ((int64_t)1 << 56) / (4 * kMaxSplits) / B) return TE_ERR_SHAPE;
    return S > 1 ? S * B * per * 4 : 0;
}

extern "C" int te_conv2d_heads_f32(float* out, float* ws, int64_t ws_bytes, const float* x, const float* w, const float* bias, int B, int G,
                                   int Ci, int Cg, int H, int W, int kh, int kw, int s, int py, int px, int Ctot, int c0, int shared,
                                   float slope, int splits, te_stream_t stream) {
    TE_REQUIRE(out && x && w && bias, TE_ERR_NULL, "te_conv2d_heads_f32: NULL pointer");
    TE_REQUIRE(G >= 1 && Cg >= 1 && (int64_t)G * Cg <= 65535 * (int64_t)BM, TE_ERR_SHAPE,
               "te_conv2d_heads_f32: G and Cg must be positive with G * Cg <= %d (got %d, %d)", 65535 * BM, G, Cg);
    TE_REQUIRE(Cg % BM == 0, TE_ERR_UNSUPPORTED, "te_conv2d_heads_f32: Cg must be a multiple of %d (got %d)", BM, Cg);
    TE_REQUIRE(splits >= 0 && splits <= kMaxSplits, TE_ERR_SHAPE, "te_conv2d_heads_f32: 0 <= splits <= %d (got %d)", kMaxSplits, splits);
    HeadsArgs a;
    a.out = out; a.x = x; a.w = w; a.bias = bias;
    if (const int rc = fill_args(a, "te_conv2d_heads_f32", B, Ci, G * Cg, H, W, kh, kw, s, py, px, Ctot, c0, 0)) return rc;
    const int64_t HoWo = (int64_t)a.Ho * a.Wo;
    const int steps = steps_of(a.K);
    const int S = splits ? splits : rule_splits(a.K, HoWo);
    const int per = (int)te::cdiv(steps, S);
    TE_REQUIRE(te::cdiv(steps, per) == S, TE_ERR_SHAPE, "te_conv2d_heads_f32: %d steps of k do not make %d non-empty ranges", steps, S);
    a.xg = shared ? 0 : (int64_t)Ci * H * W;
    a.xb = (shared ? 1 : (int64_t)G) * Ci * H * W;
    a.Cg = Cg; a.kper = per * BK; a.slope = slope;
    a.part = (int64_t)B * a.Co * HoWo;
    TE_REQUIRE(a.part <= ((int64_t)1 << 56) / (4 * kMaxSplits), TE_ERR_SHAPE, "te_conv2d_heads_f32: too many outputs (%lld)", (long long)a.part);
    hipStream_t st = (hipStream_t)stream;
    if (S == 1) {
        launch<GatherHeads, EpiLeaky>(a, st);
        return te::launch_status("te_conv2d_heads_f32");
    }
    TE_REQUIRE(ws && ws_bytes >= S * a.part * 4, TE_ERR_WORKSPACE, "te_conv2d_heads_f32: %d ranges of k need a workspace of %lld bytes (got %lld)", S,
               (long long)(S * a.part * 4), (long long)(ws ? ws_bytes : 0));
    TE_REQUIRE(te::cdiv(a.part, 256) <= 0x7fffffff, TE_ERR_SHAPE, "te_conv2d_heads_f32: too many outputs (%lld)", (long long)a.part);
    HeadsArgs p = a;
    p.out = ws; p.Ctot = a.Co; p.c0 = 0;
    launch<GatherHeads, EpiPartial, PartSplit, true, false>(p, st, S);                            // the rule splits planes of one 64-pixel tile: BN = 64 alone
    heads_reduce_kernel<<<(unsigned)te::cdiv(a.part, 256), 256, 0, st>>>(out, ws, bias, a.part, a.part, a.Co, (int)HoWo, S, Ctot, c0, slope);
    return te::launch_status("te_conv2d_heads_f32");
}

extern "C" int te_upsample_add_f32(float* out, const float* x, const float* y, int64_t planes, int h, int w, int H, int W, te_stream_t stream) {
    TE_REQUIRE(out && x && y, TE_ERR_NULL, "te_upsample_add_f32: NULL pointer");
    TE_REQUIRE(planes >= 1 && planes <= 65535 && h >= 1 && w >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE,
               "te_upsample_add_f32: 1 <= planes <= 65535 and positive h, w, H, W (got %lld, %d, %d, %d, %d)", (long long)planes, h, w, H, W);
    TE_REQUIRE(h <= (1 << 15) && w <= (1 << 15) && H <= (1 << 15) && W <= (1 << 15), TE_ERR_SHAPE,
               "te_upsample_add_f32: sizes above 32768 are not supported");
    upsample_add_kernel<<<dim3((unsigned)te::cdiv((int64_t)H * W, 256), (unsigned)planes), 256, 0, (hipStream_t)stream>>>(out, x, y, h, w, H, W);
    return te::launch_status("te_upsample_add_f32");
}

extern "C" int te_psp_codes_f32(float* z, float* p, const float* lat, const float* A, const float* bz, const float* z_avg, const float* p_avg,
                                int64_t B, int Ns, int Np, int D, int T, te_stream_t stream) {
    TE_REQUIRE(z && p && lat && A && bz, TE_ERR_NULL, "te_psp_codes_f32: NULL pointer (the averages alone may be NULL)");
    TE_REQUIRE(B >= 1 && Ns >= 1 && Np >= 1 && D >= 1 && T >= 1, TE_ERR_SHAPE,
               "te_psp_codes_f32: B, Ns, Np, D, T must be positive (got %lld, %d, %d, %d, %d)", (long long)B, Ns, Np, D, T);
    TE_REQUIRE((int64_t)Ns + Np <= 65536 && T <= 65536 && (int64_t)D * (T + Np) <= 0x7fffffff && (int64_t)D * (Ns + Np) <= 0x7fffffff &&
                   B <= ((int64_t)1 << 40) / ((int64_t)D * (T + Np)),
               TE_ERR_SHAPE, "te_psp_codes_f32: the sizes are outside the limits (B %lld, Ns %d, Np %d, D %d, T %d)", (long long)B, Ns, Np, D, T);
    const int64_t total = B * D * (T + Np);
    psp_codes_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(z, p, lat, A, bz, z_avg, p_avg, total, Ns, Np, D, T);
    return te::launch_status("te_psp_codes_f32");
}
