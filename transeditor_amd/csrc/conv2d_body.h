// The implicit-GEMM kernel of the general fp32 convolution as a template, with its launch and its checks, written once for every frozen
// network that runs it:
//     conv2d.hip      te_conv2d_f32 (Inception-v3 and the plain layers of all the others)
//     resnet.hip      te_conv2d_res_f32, te_pose_stem_fwd_f32 (the ResNet-18 pose scorer)
//     lpips_alex.hip  te_alex_stem_fwd_f32
//     irse.hip        te_conv2d_prelu[_keep]_f32, te_id_stem_{fwd,keep}_f32 (ArcFace IR-SE50)
//     irse_bwd.hip    te_conv2d_dgrad_f32, te_id_stem_bwd_f32 (its backward pass: the adjoint is the same loop over the gradient)
//     psp_heads.hip   te_conv2d_heads_f32 (the pSp encoder's grouped heads)
//     psp_heads_bwd.hip  te_conv2d_heads_dgrad_f32 (their data gradient; dgrad_body.h holds what it shares with irse_bwd.hip)
// A new network on this loop adds a gather, an epilogue and an entry point, and no launcher: the entry point checks what is its own,
// fills its Args (ConvArgs or a struct derived from it; fill_args does the shared checks and the shared fields) and calls
// launch<Gather, Epi[, Part]>(a, stream).  Compile-time policies make the variants:
//     the gather   : where a tap of the patch comes from (GatherPlain: x[b, c, iy, ix] of a dense [B,Ci,H,W] tensor), and
//     the epilogue : what happens to acc + bias before the store (EpiBiasAct: the activation),
//     the part     : which range of k the workgroup runs and where the tile goes (PartWhole: all of it, into `out`; psp_heads.hip splits;
//                    irse_bwd.hip stores a phase of a stride-2 data gradient with a pitch of 2: the destination is the part's DestDense or its own).
// Everything else - the tile shapes, the LDS layout, the order of k inside an output's one fp32 fma chain (the permutation of
// gemm_nt_f32.h: lane half h feeds k = 8q + 4h + u of every 32-deep step to MFMA (q, u)) - is the same for all of them, so two variants
// that gather the same values produce the same accumulators bit for bit.  The description of the loop is at the top of conv2d.hip.
#pragma once
#include "te_common.h"
#include "te_prof.h"

namespace te {
namespace conv2d {

constexpr int BM = 64;           // output channels per workgroup
constexpr int BK = 32;
constexpr int LD = 36;           // LDS row pitch in floats (csrc/gemm_nt_f32.h)
constexpr int NT = 256;
constexpr int kMaxKernel = 7;
constexpr int kWideGridMin = 512;    // BN = 128 only where it still gives two workgroups per CU

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

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
    const float* img;            // the image b of the gather's source
    int iy0, ix0;                // the input row / column of tap (0, 0); may be negative
    bool live;
};

// the gather of a dense [B,Ci,H,W] input
struct GatherPlain {
    template <class Args>
    static __device__ __forceinline__ const float* image(const Args& a, int64_t b) { return a.x + b * a.Ci * a.H * a.W; }
    template <class Args>
    static __device__ __forceinline__ int plane(const Args& a) { return a.H * a.W; }
    // tap (c, iy, ix), inside the H x W plane
    template <class Args>
    static __device__ __forceinline__ float tap(const float* img, const Args& a, int HW, int c, int iy, int ix) {
        return img[c * HW + iy * a.W + ix];
    }
};

// out = act(acc + bias)
struct EpiBiasAct {
    template <class Args>
    static __device__ __forceinline__ float apply(const Args& a, float v, const float* dst, int m, int HoWo) {   // the element is dst[m * HoWo]
        if (a.act == 1) v = te::relu_nan(v);
        return v;
    }
};

// where pixel r of image b of the tile goes and the pitch between two of its channels: the slice [c0, c0 + Co) of a dense [B,Ctot,Ho,Wo]
struct DestDense {
    template <class Args>
    static __device__ __forceinline__ float* dest(const Args& a, float* out, int64_t b, int r, int HoWo) { return out + (b * a.Ctot + a.c0) * HoWo + r; }
    template <class Args>
    static __device__ __forceinline__ int pitch(const Args& a, int HoWo) { return HoWo; }
};

// the part of the k chain a workgroup runs and where its tile goes: the whole chain, bias added, into `out`.  A split launch (psp_heads.hip)
// names another range of k and another destination; the order of k inside the range is the same
struct PartWhole : DestDense {
    template <class Args>
    static __device__ __forceinline__ int k_begin(const Args& a) { return 0; }
    template <class Args>
    static __device__ __forceinline__ int k_end(const Args& a) { return a.K; }
    template <class Args>
    static __device__ __forceinline__ float* out(const Args& a) { return a.out; }
    template <class Args>
    static __device__ __forceinline__ float finish(const Args& a, float acc, int m) { return acc + a.bias[m]; }
};

// NPT consecutive k (from k0, wave-uniform) of the thread's pixel: the tap (c, iy0 + ky, ix0 + kx) or 0
template <int NPT, class Gather, class Args>
__device__ __forceinline__ void gather(float (&r)[NPT], const Pixel& px, const Args& a, int k0) {
    const int khw = a.kh * a.kw;
    int c = k0 / khw;
    const int rem = k0 - c * khw;
    int ky = rem / a.kw, kx = rem - ky * a.kw;
    const int HW = Gather::plane(a);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int iy = px.iy0 + ky, ix = px.ix0 + kx;
        const bool in = px.live && c < a.Ci && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        r[j] = in ? Gather::tap(px.img, a, HW, c, iy, ix) : 0.f;
        if (++kx == a.kw) {
            kx = 0;
            if (++ky == a.kh) { ky = 0; ++c; }
        }
    }
}

// The kernel.  `Args` is ConvArgs or a struct derived from it that carries what the policies need.  PROF_ONLY lines exist in
// conv2d.hip's profiling build alone (it owns the buffer they write).
template <int BN, bool AL, class Gather, class Epi, class Part = PartWhole, class Args = ConvArgs>
__global__ __launch_bounds__(NT) void conv2d_kernel(const Args a) {
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
        px.img = Gather::image(a, b);
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
    const int kb = Part::k_begin(a), ke = Part::k_end(a);
    load_weights<AL>(rw, a.w, m0, a.Co, a.K, kb);
    gather<NPT, Gather>(rx, px, a, kb + kg * NPT);
    const float* wp = Ws + (wm * 32 + c) * LD + 4 * h;
    const float* xp = Xs + (wn * (BN / 2) + c) * LD + 4 * h;
    PROF_ONLY(unsigned long long pc[3] = {0, 0, 0}; unsigned long long tlast = __builtin_readcyclecounter();)
    for (int kk = kb; kk < ke; kk += BK) {
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
        if (kk + BK < ke) {                                   // in flight behind the MFMAs below
            load_weights<AL>(rw, a.w, m0, a.Co, a.K, kk + BK);
            gather<NPT, Gather>(rx, px, a, kk + BK + kg * NPT);
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
        float* dst = Part::dest(a, Part::out(a), b, r, HoWo);
        const int cp = Part::pitch(a, HoWo);                 // the epilogue's `HoWo`: the element is dst[m * cp]
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (m < a.Co) {
                float v = Part::finish(a, acc[i][e], m);
                v = Epi::apply(a, v, dst, m, cp);
                dst[(int64_t)m * cp] = v;
            }
        }
    }
}

// BN = 128 where that still fills the chip, else 64 (the result does not depend on the choice)
inline bool wide_grid(int64_t P, int Co) { return te::cdiv(P, 128) * te::cdiv(Co, BM) >= kWideGridMin; }

template <int BN, bool ALIGNED, class Gather, class Epi, class Part, class Args>
void launch_tile(const Args& a, int S, hipStream_t st) {
    const dim3 grid((unsigned)te::cdiv(a.P, BN), (unsigned)te::cdiv(a.Co, BM), (unsigned)S);
    if (ALIGNED && a.K % 4 == 0 && te::aligned16(a.w)) conv2d_kernel<BN, ALIGNED, Gather, Epi, Part, Args><<<grid, NT, 0, st>>>(a);
    else conv2d_kernel<BN, false, Gather, Epi, Part, Args><<<grid, NT, 0, st>>>(a);
}

// THE launch of the loop: the tile (wide_grid), the weight loads (16-byte ones where K % 4 == 0 and w is aligned) and the grid, S
// workgroups deep for a part that splits the k chain.  The library holds the kernel forms that the two flags allow and no others:
// ALIGNED = false for an entry point whose K is fixed and no multiple of 4 (the pose and AlexNet stems; the identity stem has always
// carried its unused aligned forms and goes on doing so), WIDE = false for one that was tuned at BN = 64 alone (the heads' split part).
template <class Gather, class Epi, class Part = PartWhole, bool ALIGNED = true, bool WIDE = true, class Args>
void launch(const Args& a, hipStream_t st, int S = 1) {
    if (WIDE && wide_grid(a.P, a.Co)) launch_tile<WIDE ? 128 : 64, ALIGNED, Gather, Epi, Part>(a, S, st);
    else launch_tile<64, ALIGNED, Gather, Epi, Part>(a, S, st);
}

// The geometry of a convolution, checked: -> Ho, Wo.  `who` names the entry point in the messages.  The loop itself takes any kernel
// size and stride; `max_kernel` and `stride4` are the entry point's own limits (the AlexNet stem of lpips_alex.hip is 11 x 11 with
// stride 4, every other entry point keeps 7 x 7 and strides 1 and 2).
inline int check_geometry(const char* who, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px, int& Ho, int& Wo,
                          int max_kernel = kMaxKernel, bool stride4 = false) {
    TE_REQUIRE(B >= 1 && Ci >= 1 && Co >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE, "%s: B, Ci, Co, H, W must be positive (got %d, %d, %d, %d, %d)", who,
               B, Ci, Co, H, W);
    TE_REQUIRE(kh >= 1 && kh <= max_kernel && kw >= 1 && kw <= max_kernel, TE_ERR_UNSUPPORTED, "%s: 1 <= kh, kw <= %d (got %d x %d)", who,
               max_kernel, kh, kw);
    TE_REQUIRE(s == 1 || s == 2 || (stride4 && s == 4), TE_ERR_UNSUPPORTED, "%s: the stride must be 1 or 2 (got %d)", who, s);
    TE_REQUIRE(py >= 0 && py < kh && px >= 0 && px < kw, TE_ERR_SHAPE,
               "%s: 0 <= py < kh and 0 <= px < kw (got padding %d, %d for a %d x %d kernel)", who, py, px, kh, kw);
    TE_REQUIRE(H + 2 * py >= kh && W + 2 * px >= kw, TE_ERR_SHAPE,
               "%s: a %d x %d kernel with padding %d, %d does not fit a %d x %d image (Ho, Wo >= 1)", who, kh, kw, py, px, H, W);
    Ho = (H + 2 * py - kh) / s + 1;
    Wo = (W + 2 * px - kw) / s + 1;
    return 0;
}

// What the loop indexes with an int and what the grid can hold, for a launch that gathers kh x kw patches of [B,Ci,H,W] images into
// Co channels of Ho x Wo pixels.  The data gradient (irse_bwd.hip) runs the loop the other way round and calls this with the roles swapped.
inline int check_limits(const char* who, int B, int Ci, int Co, int H, int W, int kh, int kw, int Ho, int Wo) {
    TE_REQUIRE((int64_t)Ci * H * W <= 0x7fffffff && (int64_t)Ci * kh * kw <= 0x7fffffff - BK && (int64_t)Ho * Wo <= 0x7fffffff, TE_ERR_SHAPE,
               "%s: one image (%d * %d * %d), a patch (%d * %d * %d) and a plane of pixels (%d * %d) must fit 31 bits", who, Ci, H, W, Ci, kh, kw,
               Ho, Wo);
    const int64_t P = (int64_t)B * Ho * Wo;
    TE_REQUIRE(te::cdiv(P, 64) <= 0x7fffffff && te::cdiv(Co, BM) <= 65535, TE_ERR_SHAPE, "%s: too many outputs (%lld pixels, %d channels)", who,
               (long long)P, Co);
    return 0;
}

// the checks and the fill of ConvArgs that every forward entry point on this loop shares
inline int fill_args(ConvArgs& a, const char* who, int B, int Ci, int Co, int H, int W, int kh, int kw, int s, int py, int px, int Ctot, int c0,
                     int act, int max_kernel = kMaxKernel, bool stride4 = false) {
    int Ho, Wo;
    if (const int rc = check_geometry(who, B, Ci, Co, H, W, kh, kw, s, py, px, Ho, Wo, max_kernel, stride4)) return rc;
    TE_REQUIRE(act == 0 || act == 1, TE_ERR_UNSUPPORTED, "%s: act must be 0 (none) or 1 (ReLU), got %d", who, act);
    TE_REQUIRE(c0 >= 0 && Ctot >= 1 && (int64_t)c0 + Co <= Ctot, TE_ERR_SHAPE, "%s: the slice [%d, %d + %d) is outside the %d output channels",
               who, c0, c0, Co, Ctot);
    if (const int rc = check_limits(who, B, Ci, Co, H, W, kh, kw, Ho, Wo)) return rc;
    a.P = (int64_t)B * Ho * Wo;
    a.Ci = Ci; a.Co = Co; a.H = H; a.W = W; a.kh = kh; a.kw = kw; a.s = s; a.py = py; a.px = px;
    a.Ho = Ho; a.Wo = Wo; a.Ctot = Ctot; a.c0 = c0; a.act = act; a.K = Ci * kh * kw;
    return 0;
}

}  // namespace conv2d
}  // namespace te
