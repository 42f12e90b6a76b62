// The backward pass of everything that sits on the backbone of the dual-space pSp encoder (psp_heads.hip; the reference leaves it to torch
// autograd in pSp/training/coach_new.py:128-135 over psp_encoders_new.py:11-32 and :84-140): what training the heads needs.
//
//     te_conv2d_heads_dgrad_f32  : the data gradient of te_conv2d_heads_f32 for heads that read their own activations, with the leaky
//                                  ReLU' of the layer the gradient enters as the epilogue
//     te_conv2d_heads_wgrad_f32  : the weight and bias gradient of te_conv2d_heads_f32 and (G = 1) of the lateral te_conv2d_f32
//     te_upsample_add_bwd_f32    : the adjoint of te_upsample_add_f32 with respect to x, a gather
//     te_psp_codes_bwd_f32       : the adjoint of te_psp_codes_f32
//
// The data gradient is launch_dgrad of dgrad_body.h with one more gather: the workgroup's 64-channel block of gx names its head, the
// head names the channel offset into g.  The weight gradient is a GEMM gw[m, n] = sum_r g[m, r] * im2col(x)[n, r] on the fp32-input
// MFMA with the LDS layout and the k permutation of conv2d_body.h (lane half h feeds r = 8q + 4h + u of every 32-deep step to MFMA
// (q, u)); both operands are gathers.  No atomics; every sum is a fixed-order chain or a fixed-shape tree: bit-reproducible.
#include <algorithm>
#include "te_common.h"
#include "dgrad_body.h"
#include "psp_upsample.h"
#include "wave_dot.h"

namespace {

using namespace te::dgrad;
using te::wave_sum;
using te::psp::corner_tap;                // the forward's own taps and weights

// ------------------------------------------------------------------------------------------------------ the grouped data gradient
struct HeadsDgradArgs : DgradArgs {
    int64_t gimg, ghead;         // floats between two images of g (Ctot * Ho * Wo) and between two heads' channels of it (Cg * Ho * Wo)
    int Cih;                     // channels of gx per head (the forward's Ci): a multiple of 64, so a block never straddles two heads
    float lslope;
};

struct GatherHeadGrad {
    static __device__ __forceinline__ const float* image(const HeadsDgradArgs& a, int64_t b) {
        return a.x + b * a.gimg + (int64_t)(blockIdx.y * BM / a.Cih) * a.ghead;
    }
    static __device__ __forceinline__ int plane(const HeadsDgradArgs& a) { return a.H * a.W; }
    static __device__ __forceinline__ float tap(const float* img, const HeadsDgradArgs& a, int HW, int c, int iy, int ix) {
        return img[c * HW + iy * a.W + ix];
    }
};

// gx = act > 0 ? acc : acc * slope (act: the kept OUTPUT of the layer the gradient enters; slope > 0, so its sign is the
// pre-activation's); torch's rule: 0, -0 and NaN take the slope.  EpiDgrad's PReLU' line with a scalar slope
struct EpiLeakyGrad {
    static __device__ __forceinline__ float apply(const HeadsDgradArgs& a, float v, const float* dst, int m, int GHW) {
        if (!a.pre) return v;
        return a.pre[(dst - a.out) + (int64_t)m * GHW] > 0.f ? v : __fmul_rn(v, a.lslope);
    }
};

// ------------------------------------------------------------------------------------------------------ the weight gradient
constexpr int BN = 64;           // columns n = (c, ky, kx) per workgroup
constexpr int kMaxSplits = 16;
// The split rule, from (M = Cg, N = Ci * kh * kw, R = B * Ho * Wo) alone.  What it rests on, none of it timed when it was written
// (measurements: profiles/README.md, 'Encoder head training'): a head's gw is (M / 64) * ceil(N / 64) tiles and a workgroup walks all
// of R for its tile, so a launch with fewer tiles than the chip has compute units (kNumCU) leaves units idle however long R is.  The
// head launches have 576 tiles per head and are never split; the laterals (512 x 256 and 512 x 128, one head) have 32 and 16.  Below
// kNumCU tiles per head R is cut into S ranges of whole 32-deep steps until S * tiles reaches kNumCU, with at most kMaxSplits ranges
// and at least kSplitMinSteps steps per range (a shorter range is mostly the prologue and the epilogue of the loop).
constexpr int kSplitMinSteps = 4;

struct WgradArgs {
    float* out;                  // gw [G*Cg, N], or the workspace [S][G*Cg][N]
    const float* g;              // channel c0 of image 0
    const float* x;
    int64_t gimg;                // floats between two images of g: Ctot * Ho * Wo
    int64_t ximg, xhead;         // floats between two images of x and between two heads' inputs (0: shared)
    int64_t part;                // floats between two partial results: G * Cg * N
    int R, rper;                 // B * Ho * Wo; r per range (a multiple of BK)
    int Cg, H, W, kh, kw, s, py, px, Ho, Wo, N;
};

// four consecutive r (from r0) of row `row` of g: element r = (b, q) is g[b * gimg + row * HoWo + q]; r >= r_end reads 0
__device__ __forceinline__ f32x4 load_g(const WgradArgs& a, int row, int HoWo, int r0, int r_end) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int b = r0 / HoWo, q = r0 - b * HoWo;
    const float* p = a.g + (int64_t)row * HoWo;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (r0 + u < r_end) v[u] = p[b * a.gimg + q];
        if (++q == HoWo) { q = 0; ++b; }
    }
    return f32x4{v[0], v[1], v[2], v[3]};
}

// eight consecutive r (from r0) of im2col column (c, ky, kx): x[b, c, s * oy + ky - py, s * ox + kx - px], 0 outside the plane, past
// r_end and for a column n >= N.  xc: channel c of the head's input in image 0; (dy, dx) = (ky - py, kx - px)
__device__ __forceinline__ void load_x(float (&v)[8], const WgradArgs& a, const float* xc, bool col, int dy, int dx, int HoWo, int r0, int r_end) {
    int b = r0 / HoWo;
    const int q = r0 - b * HoWo;
    int oy = q / a.Wo, ox = q - oy * a.Wo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int iy = oy * a.s + dy, ix = ox * a.s + dx;
        const bool in = col && r0 + j < r_end && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        v[j] = in ? xc[b * a.ximg + iy * a.W + ix] : 0.f;
        if (++ox == a.Wo) {
            ox = 0;
            if (++oy == a.Ho) { oy = 0; ++b; }
        }
    }
}

// One workgroup: 64 channels of one head x 64 columns n, over range blockIdx.z of r.  The accumulators start at +0 and a tap that only
// ever sees padding adds g * 0 to them: exactly +0 for finite g.
__global__ __launch_bounds__(NT) void heads_wgrad_kernel(const WgradArgs a) {
    __shared__ __attribute__((aligned(16))) float Gs[BM * LD];
    __shared__ __attribute__((aligned(16))) float Xs[BN * LD];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int HoWo = a.Ho * a.Wo;
    const int rb = blockIdx.z * a.rper, re = min(a.R, rb + a.rper);

    // the x role: column n0 + lane, r run kg (wave-uniform)
    const int kg = __builtin_amdgcn_readfirstlane(wid);
    const int n = n0 + lane;
    const bool col = n < a.N;
    const int khw = a.kh * a.kw;
    const int ch = col ? n / khw : 0;
    const int rem = col ? n - ch * khw : 0;
    const int ky = rem / a.kw, kx = rem - ky * a.kw;
    const float* xc = a.x + (int64_t)(m0 / a.Cg) * a.xhead + (int64_t)ch * a.H * a.W;
    const int dy = ky - a.py, dx = kx - a.px;
    // the g role: rows (t >> 3) and (t >> 3) + 32 of the block, r run t & 7
    const int grow = m0 + (t >> 3), gk = (t & 7) * 4;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    f32x4 rg[2];
    float rx[8];
    rg[0] = load_g(a, grow, HoWo, rb + gk, re);
    rg[1] = load_g(a, grow + 32, HoWo, rb + gk, re);
    load_x(rx, a, xc, col, dy, dx, HoWo, rb + kg * 8, re);
    const float* gp = Gs + (wm * 32 + c) * LD + 4 * h;
    const float* xp = Xs + (wn * 32 + c) * LD + 4 * h;
    for (int rr = rb; rr < re; rr += BK) {
        __syncthreads();                                     // the previous step's LDS reads are done
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(Gs + ((t >> 3) + 32 * i) * LD + gk) = rg[i];
#pragma unroll
        for (int j = 0; j < 8; j += 4) {
            const f32x4 v = {rx[j], rx[j + 1], rx[j + 2], rx[j + 3]};
            *reinterpret_cast<f32x4*>(Xs + lane * LD + kg * 8 + j) = v;
        }
        __syncthreads();
        if (rr + BK < re) {                                   // in flight behind the MFMAs below
            rg[0] = load_g(a, grow, HoWo, rr + BK + gk, re);
            rg[1] = load_g(a, grow + 32, HoWo, rr + BK + gk, re);
            load_x(rx, a, xc, col, dy, dx, HoWo, rr + BK + kg * 8, re);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(gp + 8 * q);
            const f32x4 v = *reinterpret_cast<const f32x4*>(xp + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u.x, v.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u.y, v.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u.z, v.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u.w, v.w, acc, 0, 0, 0);
        }
    }
    // accumulator register e of lane (c, h): channel (e & 3) + 8 (e >> 2) + 4 h of the wave's 32, column c of the wave's 32
    const int no = n0 + wn * 32 + c;
    if (no >= a.N) return;
    float* dst = a.out + blockIdx.z * a.part + no;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        dst[(int64_t)m * a.N] = acc[e];
    }
}

// gw[o] = ((ws[0] + ws[1]) + ...) + ws[S - 1], the ranges in ascending order of r; one thread per element
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(float* __restrict__ gw, const float* __restrict__ ws, int64_t part, int S) {
#pragma clang fp contract(off)
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= part) return;
    float v = ws[o];
    for (int s = 1; s < S; ++s) v = v + ws[s * part + o];
    gw[o] = v;
}

// gb[ch] = sum_r g[ch, r]: one wave per channel, lane l takes r = l, l + 64, ... as one chain, the lanes meet in a butterfly
__global__ __launch_bounds__(256) void bias_grad_kernel(float* __restrict__ gb, const float* __restrict__ g, int64_t gimg, int Co, int HoWo, int R) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= Co) return;
    const float* p = g + (int64_t)ch * HoWo;
    float acc = 0.f;
    for (int r = lane; r < R; r += 64) {
        const int b = r / HoWo;
        acc = acc + p[b * gimg + (r - b * HoWo)];
    }
    acc = wave_sum(acc);
    if (lane == 0) gb[ch] = acc;
}

inline int steps_of(int64_t R) { return (int)te::cdiv(R, (int64_t)BK); }

// the rule's S for (M, N, R)
inline int rule_splits(int M, int64_t N, int64_t R) {
    const int64_t tiles = (M / BM) * te::cdiv(N, (int64_t)BN);
    if (tiles >= te::kNumCU) return 1;
    const int steps = steps_of(R);
    const int64_t want = std::min<int64_t>(std::min<int64_t>(kMaxSplits, te::cdiv(te::kNumCU, tiles)), steps / kSplitMinSteps);
    if (want <= 1) return 1;
    return (int)te::cdiv(steps, te::cdiv(steps, want));      // whole steps per range, every range non-empty
}

inline bool wgrad_dims_ok(int64_t B, int G, int Cg, int Ci, int kh, int kw, int Ho, int Wo) {
    return B >= 1 && G >= 1 && Cg >= 1 && Cg % BM == 0 && (int64_t)G * Cg <= 65535 * (int64_t)BM && Ci >= 1 && kh >= 1 && kh <= kMaxKernel &&
           kw >= 1 && kw <= kMaxKernel && Ho >= 1 && Wo >= 1 && (int64_t)Ci * kh * kw <= 0x7fffffff - BN &&
           (int64_t)Ho * Wo <= 0x7fffffff && B <= (0x7fffffff - BK) / ((int64_t)Ho * Wo) &&
           (int64_t)G * Cg <= ((int64_t)1 << 56) / (4 * kMaxSplits) / ((int64_t)Ci * kh * kw);
}

// ------------------------------------------------------------------------------------------------------ upsample and add, backwards
// the weight with which output o reads source i: l0 where i is its first tap, l1 where it is its second (0: the tap does not enter)
__device__ __forceinline__ float tap_weight(int o, int i, int in_size, int out_size) {
    int i0, i1;
    float l0, l1;
    corner_tap(o, in_size, out_size, i0, i1, l0, l1);
    if (i == i0) return l0;
    return i == i1 ? l1 : 0.f;
}

// the outputs whose first tap is i - 1 or i: [lo, hi]; every output where a side is 1
__device__ __forceinline__ void reach(int i, int in_size, int out_size, int& lo, int& hi) {
    lo = 0; hi = out_size - 1;
    if (in_size == 1 || out_size == 1) return;
    const int64_t den = in_size - 1, span = out_size - 1;
    if (i > 0) lo = (int)(((int64_t)(i - 1) * span + den - 1) / den);
    hi = min(hi, (int)(((int64_t)(i + 1) * span + den - 1) / den) - 1);
}

// source pixel (i, j) of a plane: the sum over the outputs that read it, rows ascending, then columns ascending, of g * (wy * wx), one
// fma chain that the first term opens; then + add.  A GATHER: no atomics
__global__ __launch_bounds__(256) void upsample_add_bwd_kernel(float* __restrict__ gx, const float* __restrict__ g, const float* __restrict__ add,
                                                               int h, int w, int H, int W) {
#pragma clang fp contract(off)
    const int64_t plane = blockIdx.y;
    const int at = blockIdx.x * 256 + threadIdx.x;
    if (at >= h * w) return;
    const int i = at / w, j = at - i * w;
    int ya, yb, xa, xb;
    reach(i, h, H, ya, yb);
    reach(j, w, W, xa, xb);
    const float* src = g + plane * H * W;
    float acc = 0.f;
    bool open = false;
    for (int oy = ya; oy <= yb; ++oy) {
        const float wy = tap_weight(oy, i, h, H);
        if (wy == 0.f) continue;
        for (int ox = xa; ox <= xb; ++ox) {
            const float wx = tap_weight(ox, j, w, W);
            if (wx == 0.f) continue;
            const float wt = __fmul_rn(wy, wx);
            const float v = src[(int64_t)oy * W + ox];
            acc = open ? fmaf(v, wt, acc) : __fmul_rn(v, wt);
            open = true;
        }
    }
    const int64_t o = plane * h * w + at;
    gx[o] = add ? acc + add[o] : acc;
}

// ------------------------------------------------------------------------------------------------------ the codes, backwards
// item i = (b, j, c), c fastest: glat[b, j, c] = sum_t A[t, j] * gz[b, c, t] (t ascending, in fp64, rounded once) for j < Ns, else
// gp[b, c, j - Ns]
__global__ __launch_bounds__(256) void psp_codes_glat_kernel(float* __restrict__ glat, const float* __restrict__ gz, const float* __restrict__ gp,
                                                             const float* __restrict__ A, int64_t total, int Ns, int Np, int D, int T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % D);
    const int j = (int)(i / D % (Ns + Np));
    const int64_t b = i / D / (Ns + Np);
    if (j < Ns) {
        const float* row = gz + (b * D + c) * T;
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc = fma((double)A[t * Ns + j], (double)row[t], acc);
        glat[i] = (float)acc;
    } else {
        glat[i] = gp[(b * D + c) * Np + (j - Ns)];
    }
}

// block (t, j): j < Ns is gA[t, j] = sum over (b, c) of gz[b, c, t] * lat[b, j, c], j == Ns is gbz[t] = sum over (b, c) of gz[b, c, t].
// One wave: lane l takes the items (b, c) = l, l + 64, ... (b-major) as one fp64 chain, the lanes meet in an fp64 butterfly, one rounding
__global__ __launch_bounds__(64) void psp_codes_gA_kernel(float* __restrict__ gA, float* __restrict__ gbz, const float* __restrict__ gz,
                                                          const float* __restrict__ lat, int64_t BD, int Ns, int Np, int D, int T) {
    const int lane = threadIdx.x;
    const int t = blockIdx.x / (Ns + 1), j = blockIdx.x - t * (Ns + 1);
    double acc = 0.0;
    for (int64_t i = lane; i < BD; i += 64) {
        const double v = gz[i * T + t];
        if (j < Ns) {
            const int64_t b = i / D;
            acc = fma(v, (double)lat[(b * (Ns + Np) + j) * D + (i - b * D)], acc);
        } else {
            acc += v;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        if (j < Ns) gA[t * Ns + j] = (float)acc;
        else gbz[t] = (float)acc;
    }
}

}  // namespace

extern "C" int te_conv2d_heads_dgrad_f32(float* gx, const float* g, const float* wt, const float* act, int B, int G, int Ci, int Cg, int H, int W,
                                         int kh, int kw, int s, int py, int px, int gCtot, int gc0, float slope, te_stream_t stream) {
    const char* who = "te_conv2d_heads_dgrad_f32";
    TE_REQUIRE(gx && g && wt, TE_ERR_NULL, "%s: NULL pointer (act alone may be NULL)", who);
    TE_REQUIRE(G >= 1 && Ci >= 1 && Cg >= 1 && (int64_t)G * Ci <= 65535 * (int64_t)BM && (int64_t)G * Cg <= 0x7fffffff, TE_ERR_SHAPE,
               "%s: G, Ci and Cg must be positive with G * Ci <= %d (got %d, %d, %d)", who, 65535 * BM, G, Ci, Cg);
    TE_REQUIRE(Ci % BM == 0, TE_ERR_UNSUPPORTED, "%s: Ci must be a multiple of %d (got %d)", who, BM, Ci);
    TE_REQUIRE(slope > 0.f, TE_ERR_UNSUPPORTED, "%s: the slope must be positive: the kept output then carries the pre-activation's sign (got %g)",
               who, (double)slope);
    TE_REQUIRE(gc0 >= 0 && (int64_t)gc0 + (int64_t)G * Cg <= gCtot, TE_ERR_SHAPE, "%s: the slice [%d, %d + %d) is outside the %d channels of g", who,
               gc0, gc0, G * Cg, gCtot);
    int Ho, Wo;
    if (const int rc = check_dgrad(who, B, G * Ci, Cg, H, W, kh, kw, s, py, px, Ho, Wo)) return rc;
    HeadsDgradArgs a;
    a.out = gx; a.x = g + (int64_t)gc0 * Ho * Wo; a.pre = act; a.slope = nullptr; a.in_scale = nullptr; a.add = nullptr;
    a.as = 1; a.AH = H; a.AW = W;
    a.gimg = (int64_t)gCtot * Ho * Wo; a.ghead = (int64_t)Cg * Ho * Wo; a.Cih = Ci; a.lslope = slope;
    launch_dgrad<GatherHeadGrad, EpiLeakyGrad>(a, wt, B, G * Ci, Cg, H, W, kh, kw, s, py, px, Ho, Wo, (hipStream_t)stream);
    return te::launch_status(who);
}

extern "C" int te_conv2d_heads_wgrad_splits(int Cg, int Ci, int kh, int kw, int64_t B, int Ho, int Wo) {
    if (!wgrad_dims_ok(B, 1, Cg, Ci, kh, kw, Ho, Wo)) return TE_ERR_SHAPE;
    return rule_splits(Cg, (int64_t)Ci * kh * kw, B * Ho * Wo);
}

extern "C" int64_t te_conv2d_heads_wgrad_ws_bytes(int64_t B, int G, int Cg, int Ci, int kh, int kw, int Ho, int Wo) {
    if (!wgrad_dims_ok(B, G, Cg, Ci, kh, kw, Ho, Wo)) return TE_ERR_SHAPE;
    const int S = rule_splits(Cg, (int64_t)Ci * kh * kw, B * Ho * Wo);
    return S > 1 ? (int64_t)S * G * Cg * Ci * kh * kw * 4 : 0;
}

extern "C" int te_conv2d_heads_wgrad_f32(float* gw, float* gb, float* ws, int64_t ws_bytes, const float* g, const float* x, int B, int G, int Ci,
                                         int Cg, int H, int W, int kh, int kw, int s, int py, int px, int gCtot, int gc0, int shared, int splits,
                                         te_stream_t stream) {
    const char* who = "te_conv2d_heads_wgrad_f32";
    TE_REQUIRE(gw && gb && g && x, TE_ERR_NULL, "%s: NULL pointer", who);
    TE_REQUIRE(G >= 1 && Cg >= 1 && (int64_t)G * Cg <= 65535 * (int64_t)BM, TE_ERR_SHAPE, "%s: G and Cg must be positive with G * Cg <= %d (got %d, %d)",
               who, 65535 * BM, G, Cg);
    TE_REQUIRE(Cg % BM == 0, TE_ERR_UNSUPPORTED, "%s: Cg must be a multiple of %d (got %d)", who, BM, Cg);
    TE_REQUIRE(splits >= 0 && splits <= kMaxSplits, TE_ERR_SHAPE, "%s: 0 <= splits <= %d (got %d)", who, kMaxSplits, splits);
    int Ho, Wo;
    if (const int rc = check_geometry(who, B, Ci, G * Cg, H, W, kh, kw, s, py, px, Ho, Wo)) return rc;
    TE_REQUIRE(gc0 >= 0 && (int64_t)gc0 + (int64_t)G * Cg <= gCtot, TE_ERR_SHAPE, "%s: the slice [%d, %d + %d) is outside the %d channels of g", who,
               gc0, gc0, G * Cg, gCtot);
    const int64_t Gx = shared ? 1 : G;
    TE_REQUIRE(wgrad_dims_ok(B, G, Cg, Ci, kh, kw, Ho, Wo) && Gx * Ci * H * W <= 0x7fffffff, TE_ERR_SHAPE,
               "%s: one image of x (%lld * %d * %d), the columns (%d * %d * %d) and the reduction (%d * %d * %d) must fit 31 bits", who,
               (long long)(Gx * Ci), H, W, Ci, kh, kw, B, Ho, Wo);
    WgradArgs a;
    a.g = g + (int64_t)gc0 * Ho * Wo; a.x = x;
    a.gimg = (int64_t)gCtot * Ho * Wo;
    a.ximg = Gx * Ci * H * W; a.xhead = shared ? 0 : (int64_t)Ci * H * W;
    a.N = Ci * kh * kw; a.R = B * Ho * Wo;
    a.part = (int64_t)G * Cg * a.N;
    a.Cg = Cg; a.H = H; a.W = W; a.kh = kh; a.kw = kw; a.s = s; a.py = py; a.px = px; a.Ho = Ho; a.Wo = Wo;
    const int steps = steps_of(a.R);
    const int S = splits ? splits : rule_splits(Cg, a.N, a.R);
    const int per = (int)te::cdiv(steps, S);
    TE_REQUIRE(te::cdiv(steps, per) == S, TE_ERR_SHAPE, "%s: %d steps of r do not make %d non-empty ranges", who, steps, S);
    a.rper = per * BK;
    TE_REQUIRE(S == 1 || (ws && ws_bytes >= S * a.part * 4), TE_ERR_WORKSPACE, "%s: %d ranges of r need a workspace of %lld bytes (got %lld)", who, S,
               (long long)(S * a.part * 4), (long long)(ws ? ws_bytes : 0));
    TE_REQUIRE(te::cdiv(a.part, 256) <= 0x7fffffff, TE_ERR_SHAPE, "%s: too many weights (%lld)", who, (long long)a.part);
    hipStream_t st = (hipStream_t)stream;
    a.out = S == 1 ? gw : ws;
    const dim3 grid((unsigned)te::cdiv(a.N, BN), (unsigned)(G * Cg / BM), (unsigned)S);
    heads_wgrad_kernel<<<grid, NT, 0, st>>>(a);
    if (S > 1) wgrad_reduce_kernel<<<(unsigned)te::cdiv(a.part, 256), 256, 0, st>>>(gw, ws, a.part, S);
    bias_grad_kernel<<<(unsigned)te::cdiv(G * Cg, 4), 256, 0, st>>>(gb, a.g, a.gimg, G * Cg, Ho * Wo, a.R);
    return te::launch_status(who);
}

extern "C" int te_upsample_add_bwd_f32(float* gx, const float* g, const float* add, int64_t planes, int h, int w, int H, int W, te_stream_t stream) {
    TE_REQUIRE(gx && g, TE_ERR_NULL, "te_upsample_add_bwd_f32: NULL pointer (add alone may be NULL)");
    TE_REQUIRE(planes >= 1 && planes <= 65535 && h >= 1 && w >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE,
               "te_upsample_add_bwd_f32: 1 <= planes <= 65535 and positive h, w, H, W (got %lld, %d, %d, %d, %d)", (long long)planes, h, w, H, W);
    TE_REQUIRE(h <= (1 << 15) && w <= (1 << 15) && H <= (1 << 15) && W <= (1 << 15), TE_ERR_SHAPE,
               "te_upsample_add_bwd_f32: sizes above 32768 are not supported");
    upsample_add_bwd_kernel<<<dim3((unsigned)te::cdiv((int64_t)h * w, 256), (unsigned)planes), 256, 0, (hipStream_t)stream>>>(gx, g, add, h, w, H, W);
    return te::launch_status("te_upsample_add_bwd_f32");
}

extern "C" int te_psp_codes_bwd_f32(float* glat, float* gA, float* gbz, const float* gz, const float* gp, const float* lat, const float* A,
                                    int64_t B, int Ns, int Np, int D, int T, te_stream_t stream) {
    TE_REQUIRE(glat && gA && gbz && gz && gp && lat && A, TE_ERR_NULL, "te_psp_codes_bwd_f32: NULL pointer");
    TE_REQUIRE(B >= 1 && Ns >= 1 && Np >= 1 && D >= 1 && T >= 1, TE_ERR_SHAPE,
               "te_psp_codes_bwd_f32: B, Ns, Np, D, T must be positive (got %lld, %d, %d, %d, %d)", (long long)B, Ns, Np, D, T);
    TE_REQUIRE((int64_t)Ns + Np <= 65536 && T <= 65536 && (int64_t)D * (T + Np) <= 0x7fffffff && (int64_t)D * (Ns + Np) <= 0x7fffffff &&
                   B <= ((int64_t)1 << 40) / ((int64_t)D * (T + Np)) && B <= ((int64_t)1 << 40) / ((int64_t)D * (Ns + Np)) &&
                   (int64_t)T * (Ns + 1) <= 0x7fffffff,
               TE_ERR_SHAPE, "te_psp_codes_bwd_f32: the sizes are outside the limits (B %lld, Ns %d, Np %d, D %d, T %d)", (long long)B, Ns, Np, D, T);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = B * (Ns + Np) * D;
    psp_codes_glat_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, st>>>(glat, gz, gp, A, total, Ns, Np, D, T);
    psp_codes_gA_kernel<<<(unsigned)(T * (Ns + 1)), 64, 0, st>>>(gA, gbz, gz, lat, B * D, Ns, Np, D, T);
    return te::launch_status("te_psp_codes_bwd_f32");
}
