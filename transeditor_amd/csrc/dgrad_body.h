// The data gradient of a convolution on the main loop of conv2d_body.h, written once for its two users:
//     irse_bwd.hip       te_conv2d_dgrad_f32, te_id_stem_bwd_f32 (the frozen identity network, with respect to its input)
//     psp_heads_bwd.hip  te_conv2d_heads_dgrad_f32 (the grouped heads of the pSp encoder)
// The adjoint of a convolution is a convolution over the incoming gradient, on a weight the host transposed and flipped.  A stride-2
// layer is NOT a gather over the zero-inserted plane (three of four taps there are zeros the MFMA would multiply): its four output
// phases (y % 2, x % 2) are four dense stride-1 implicit GEMMs over g with the sub-kernels 1x1, 1x2, 2x1 and 2x2 of the 3x3, each
// stored with a pitch of 2 (PartPhase).  A user adds a gather over g and, where its epilogue is not EpiDgrad's, an epilogue.
#pragma once
#include "te_common.h"
#include "conv2d_body.h"

namespace te {
namespace dgrad {

using namespace te::conv2d;

// The loop's view of one phase: its "input" is g [B,Co,Ho,Wo] (Ci, H, W of ConvArgs), its "output channels" are the forward's input
// channels (Co of ConvArgs), its pixels the Hp x Wp outputs of the phase (Ho, Wo of ConvArgs), stride 1.
struct DgradArgs : ConvArgs {
    const float* pre;            // [B,Cx,GH,GW] or NULL: the PReLU' epilogue
    const float* slope;          // [Cx]
    const float* in_scale;       // [Cx] or NULL
    const float* add;            // [B,Cx,AH,AW] or NULL
    int GH, GW;                  // the plane of gx
    int ds, ry, rx;              // the phase: gx rows ry, ry + ds, ..., columns rx, rx + ds, ...
    int as, AH, AW;              // add is read at (y / as, x / as) where as divides y and x
};

struct PartPhase {
    static __device__ __forceinline__ int k_begin(const DgradArgs& a) { return 0; }
    static __device__ __forceinline__ int k_end(const DgradArgs& a) { return a.K; }
    static __device__ __forceinline__ float* out(const DgradArgs& a) { return a.out; }
    static __device__ __forceinline__ float finish(const DgradArgs& a, float acc, int m) { return acc; }
    static __device__ __forceinline__ float* dest(const DgradArgs& a, float* out, int64_t b, int r, int HoWo) {
        const int oy = r / a.Wo, ox = r - oy * a.Wo;
        return out + b * a.Co * a.GH * a.GW + (oy * a.ds + a.ry) * a.GW + ox * a.ds + a.rx;
    }
    static __device__ __forceinline__ int pitch(const DgradArgs& a, int HoWo) { return a.GH * a.GW; }
};

// pre given : gx = acc * (pre > 0 ? 1 : slope[m])      torch's rule: pre == 0, -0 and NaN take the slope
// else      : gx = in_scale[m] * acc + add             each term optional; one fma where both are there
struct EpiDgrad {
    static __device__ __forceinline__ float apply(const DgradArgs& a, float v, const float* dst, int m, int GHW) {
        const int64_t at = dst - a.out;                      // plane 0 of the image: (b * Cx) * GHW + y * GW + x
        if (a.pre) return a.pre[at + (int64_t)m * GHW] > 0.f ? v : __fmul_rn(v, a.slope[m]);
        float t = 0.f;
        if (a.add) {
            const int64_t plane0 = at / GHW;
            const int rem = (int)(at - plane0 * GHW);
            const int y = rem / a.GW, x = rem - y * a.GW;
            if (a.as == 1) t = a.add[at + (int64_t)m * GHW];
            else if (y % a.as == 0 && x % a.as == 0) t = a.add[((plane0 + m) * a.AH + y / a.as) * a.AW + x / a.as];
        }
        if (a.in_scale) return a.add ? fmaf(a.in_scale[m], v, t) : __fmul_rn(a.in_scale[m], v);
        return a.add ? __fadd_rn(v, t) : v;
    }
};

// the taps ky = k0 + s j (j < n) that reach output rows of parity r, and the padding of the phase's stride-1 convolution over g with
// those taps flipped: row y = s yy + r reads g rows yy - pad + j', j' = n - 1 - j
struct Phase { int k0, n, pad; };
inline Phase phase_of(int r, int k, int s, int p) {
    Phase f;
    f.k0 = (r + p) % s;
    f.n = f.k0 < k ? (k - f.k0 + s - 1) / s : 0;
    f.pad = f.n - 1 - (r + p - f.k0) / s;
    return f;
}

// every phase of a data gradient on the loop, with gather `Gather` over g.  `a` arrives with out, x, pre, slope, in_scale, add, as, AH, AW
// set; the weight holds the phases (ry, rx) = (0, 0), (0, 1), (1, 0), (1, 1) one behind the other, each [Cx, Co * ny * nx]
template <class Gather, class Epi = EpiDgrad, class Args>
void launch_dgrad(Args a, const float* wt, int B, int Cx, int Co, int H, int W, int kh, int kw, int s, int py, int px, int Ho, int Wo,
                  hipStream_t st) {
    a.Co = Cx; a.H = Ho; a.W = Wo; a.s = 1; a.GH = H; a.GW = W; a.ds = s; a.Ctot = Cx; a.c0 = 0; a.act = 0; a.bias = nullptr;
    for (int ry = 0; ry < s; ++ry)
        for (int rx = 0; rx < s; ++rx) {
            const Phase fy = phase_of(ry, kh, s, py), fx = phase_of(rx, kw, s, px);
            const int Hp = (H - ry + s - 1) / s, Wp = (W - rx + s - 1) / s;
            const bool empty = fy.n == 0 || fx.n == 0;       // no tap reaches this phase: the loop runs no step and the epilogue sees 0
            a.w = wt;
            a.Ci = empty ? 0 : Co; a.kh = empty ? 1 : fy.n; a.kw = empty ? 1 : fx.n; a.K = a.Ci * a.kh * a.kw;
            a.py = empty ? 0 : fy.pad; a.px = empty ? 0 : fx.pad;
            a.Ho = Hp; a.Wo = Wp; a.P = (int64_t)B * Hp * Wp; a.ry = ry; a.rx = rx;
            wt += (int64_t)Cx * a.K;
            if (a.P == 0) continue;
            launch<Gather, Epi, PartPhase>(a, st);
        }
}

// the checks of a data gradient on the forward layer's geometry; -> Ho, Wo.  The loop runs the other way round: it gathers
// g [B,Co,Ho,Wo] into the Ci channels of gx; the epilogue indexes one image of gx with an int
inline int check_dgrad(const char* who, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px, int& Ho, int& Wo) {
    if (const int rc = check_geometry(who, B, Ci, Co, H, W, kh, kw, s, py, px, Ho, Wo)) return rc;
    TE_REQUIRE((int64_t)Ci * H * W <= 0x7fffffff, TE_ERR_SHAPE, "%s: one image of gx (%d * %d * %d) must fit 31 bits", who, Ci, H, W);
    return check_limits(who, B, Co, Ci, Ho, Wo, kh, kw, H, W);
}

}  // namespace dgrad
}  // namespace te
