// The feature moments of the Frechet inception distance (metrics/fid_query.py:162-163, metrics/calc_inception.py:110-111), streamed:
//
//     te_fid_moments_f64  : S (+)= X^T X,  s (+)= sum of the rows of X      X [N, D] fp32 on the device, S / s fp64
//     te_fid_finalize_f64 : mean = s / n,  cov = (S - s s^T / n) / (n - 1)  (np.mean / np.cov(rowvar=False) of everything folded in)
//
// The product is a symmetric rank-N update on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64): the sample index is the reduction index,
// so a K-slab of 32 rows of X is a coalesced read along D and lands in LDS as fp32, [32 samples][64 features].  Lane l of an MFMA takes
// A = X[k0 + (l >> 4)][i0 + (l & 15)] and B = X[k0 + (l >> 4)][j0 + (l & 15)]: 16 consecutive floats of one LDS row, converted to fp64
// on the way into the operand register (exact; the fp32 image halves the LDS traffic).  Every product of two fp32 values is exact in
// fp64 (24 + 24 < 53 bits), so only the summation rounds.
//
// A workgroup (4 waves) owns one 64 x 64 tile (ti, tj >= ti) of S and one of SPLIT ranges of the K-slabs; a wave owns a 32 x 32 quarter
// as 2 x 2 independent 16 x 16 accumulators.  C/D of the fp64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg (NOT the fp32 map).
// The diagonal tiles also sum their 64 columns of the slab into s.  SPLIT == 1: the tile is written (or added) straight into S; else the
// partial tiles go to the workspace and a second kernel adds them in split order: one owner and one summation order per element, no
// atomics, bit-reproducible.  Only the upper triangle (j >= i) of S is written.
#include "te_common.h"

namespace {

constexpr int BT = 64;           // tile rows = tile columns of S
constexpr int BK = 32;           // samples per slab
constexpr int LD = 80;           // LDS row pitch in floats: 80 mod 32 == 16, so the two 16-float rows a 32-lane group of ds_read_b32 touches
                                 // fall on disjoint banks; 320 B keeps the 16-byte stores aligned
constexpr int NT = 256;
constexpr int kMaxSplit = 8;
constexpr int kTargetWG = 2048;  // 8 workgroups per compute unit: below that the sample index is split
constexpr int kMaxD = 8192;

using f64x4 = __attribute__((ext_vector_type(4))) double;

// rows [k0, k0 + 32) x columns [c0, c0 + 64) of x; rows >= kend and columns >= D read as zero
template <bool AL>
__device__ __forceinline__ void load_slab(float4 (&r)[2], const float* __restrict__ x, int64_t k0, int64_t kend, int c0, int D) {
    const int t = threadIdx.x;
    const int c = c0 + (t & 15) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t row = k0 + (t >> 4) + 16 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < kend) {
            const float* p = x + row * D + c;
            if (AL) {
                if (c < D) v = *reinterpret_cast<const float4*>(p);      // D % 4 == 0: the four are inside the row or all past it
            } else {
                if (c < D) v.x = p[0];
                if (c + 1 < D) v.y = p[1];
                if (c + 2 < D) v.z = p[2];
                if (c + 3 < D) v.w = p[3];
            }
        }
        r[i] = v;
    }
}

__device__ __forceinline__ void store_slab(float* s, const float4 (&r)[2]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(s + ((t >> 4) + 16 * i) * LD + (t & 15) * 4) = r[i];
}

// linear index of the upper tile (ti, tj >= ti) among the TD (TD + 1) / 2 of them, row by row
__device__ __host__ __forceinline__ int64_t tile_id(int ti, int tj, int TD) { return (int64_t)ti * TD - (int64_t)ti * (ti - 1) / 2 + (tj - ti); }

// DIRECT: out = S [D, D] and sout = s [D] (accumulate: add to what is there);  else out = the workspace's partial tiles
// [split][tile][64][64] and sout = its partial sums [split][TD * 64]
template <bool AL, bool DIRECT>
__global__ __launch_bounds__(NT, 2) void fid_moments_kernel(double* __restrict__ out, double* __restrict__ sout,
                                                            const float* __restrict__ x, int64_t N, int D, int accumulate) {
    const int ti = blockIdx.y, tj = blockIdx.x, sp = blockIdx.z, TD = gridDim.x, SPLIT = gridDim.z;
    if (tj < ti) return;
    __shared__ __attribute__((aligned(16))) float As[BK * LD];
    __shared__ __attribute__((aligned(16))) float Bs[BK * LD];
    __shared__ double ssum[4][BT];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 15, q = lane >> 4;
    const int64_t NS = (N + BK - 1) / BK;
    const int64_t s0 = sp * NS / SPLIT, s1 = (sp + 1) * NS / SPLIT;
    const int64_t kend = s1 * BK < N ? s1 * BK : N;
    const bool diag = ti == tj;

    f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;                                     // diagonal tiles: column t & 63 over the slab rows 8 (t >> 6) ... + 7

    float4 ra[2], rb[2];
    if (s0 < s1) {
        load_slab<AL>(ra, x, s0 * BK, kend, ti * BT, D);
        load_slab<AL>(rb, x, s0 * BK, kend, tj * BT, D);
    }
    const float* ap = As + q * LD + wm * 32 + c;
    const float* bp = Bs + q * LD + wn * 32 + c;
    for (int64_t sl = s0; sl < s1; ++sl) {
        __syncthreads();                                     // the previous slab's LDS reads are done
        store_slab(As, ra);
        store_slab(Bs, rb);
        __syncthreads();
        if (sl + 1 < s1) {                                   // in flight behind the MFMAs below
            load_slab<AL>(ra, x, (sl + 1) * BK, kend, ti * BT, D);
            load_slab<AL>(rb, x, (sl + 1) * BK, kend, tj * BT, D);
        }
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            double a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = (double)ap[ks * 4 * LD + m * 16];
#pragma unroll
            for (int n = 0; n < 2; ++n) b[n] = (double)bp[ks * 4 * LD + n * 16];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        if (diag) {
            const float* p = As + (t >> 6) * 8 * LD + (t & 63);
#pragma unroll
            for (int r = 0; r < 8; ++r) colsum += (double)p[r * LD];
        }
    }

    // ---- the tile: acc[m][n][r] is row (q + 4 r), column c of the 16 x 16 fragment (m, n) of this wave's 32 x 32 quarter
    if (DIRECT) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ti * BT + wm * 32 + m * 16 + q + 4 * r;
                    const int j = tj * BT + wn * 32 + n * 16 + c;
                    if (i < D && j < D && j >= i) {
                        double* d = out + (int64_t)i * D + j;
                        *d = accumulate ? *d + acc[m][n][r] : acc[m][n][r];
                    }
                }
    } else {
        double* tile = out + ((int64_t)sp * (tile_id(TD - 1, TD - 1, TD) + 1) + tile_id(ti, tj, TD)) * (BT * BT);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    tile[(wm * 32 + m * 16 + q + 4 * r) * BT + wn * 32 + n * 16 + c] = acc[m][n][r];
    }
    if (diag) {
        ssum[t >> 6][t & 63] = colsum;
        __syncthreads();
        if (t < BT) {
            const double v = ((ssum[0][t] + ssum[1][t]) + ssum[2][t]) + ssum[3][t];
            const int j = tj * BT + t;
            if (DIRECT) {
                if (j < D) sout[j] = accumulate ? sout[j] + v : v;
            } else {
                sout[(int64_t)sp * TD * BT + j] = v;
            }
        }
    }
}

// S[i][j] (+)= sum over the splits, in split order, of the partial tiles; s likewise.  One thread per element of an upper tile.
__global__ __launch_bounds__(NT) void fid_combine_kernel(double* __restrict__ S, double* __restrict__ s, const double* __restrict__ part,
                                                         const double* __restrict__ spart, int D, int SPLIT, int accumulate) {
    const int ti = blockIdx.y, tj = blockIdx.x, TD = gridDim.x;
    if (tj < ti) return;
    const int64_t T = tile_id(TD - 1, TD - 1, TD) + 1;
    const double* tile = part + tile_id(ti, tj, TD) * (BT * BT);
    for (int e = threadIdx.x; e < BT * BT; e += NT) {
        const int i = ti * BT + e / BT, j = tj * BT + e % BT;
        if (i < D && j < D && j >= i) {
            double v = tile[e];
            for (int sp = 1; sp < SPLIT; ++sp) v += tile[(int64_t)sp * T * (BT * BT) + e];
            double* d = S + (int64_t)i * D + j;
            *d = accumulate ? *d + v : v;
        }
    }
    if (ti == tj && threadIdx.x < BT) {
        const int j = tj * BT + threadIdx.x;
        if (j < D) {
            double v = spart[j];
            for (int sp = 1; sp < SPLIT; ++sp) v += spart[(int64_t)sp * TD * BT + j];
            s[j] = accumulate ? s[j] + v : v;
        }
    }
}

__global__ __launch_bounds__(NT) void fid_finalize_kernel(double* __restrict__ mean, double* __restrict__ cov, const double* __restrict__ S,
                                                          const double* __restrict__ s, double n, int D) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= D) return;
    const int a = i < j ? i : j, b = i < j ? j : i;
    cov[(int64_t)i * D + j] = (S[(int64_t)a * D + b] - s[a] * s[b] / n) / (n - 1.0);
    if (i == 0) mean[j] = s[j] / n;
}

inline int tiles(int D) { return (D + BT - 1) / BT; }
inline int64_t upper_tiles(int D) { return (int64_t)tiles(D) * (tiles(D) + 1) / 2; }
inline int split(int64_t N, int D) {
    const int64_t NS = (N + BK - 1) / BK, T = upper_tiles(D);
    int64_t S = (kTargetWG + T - 1) / T;
    if (S > kMaxSplit) S = kMaxSplit;
    if (S > NS) S = NS;
    return (int)S;
}

}  // namespace

extern "C" int64_t te_fid_moments_ws_bytes(int64_t N, int D) {
    if (N < 1 || D < 1 || D > kMaxD) return TE_ERR_SHAPE;
    const int S = split(N, D);
    return S == 1 ? 0 : (int64_t)S * (upper_tiles(D) * BT * BT + (int64_t)tiles(D) * BT) * 8;
}

extern "C" int te_fid_moments_f64(double* S, double* s, void* ws, const float* x, int64_t N, int D, int accumulate, te_stream_t stream) {
    TE_REQUIRE(S && s && x, TE_ERR_NULL, "te_fid_moments_f64: NULL pointer");
    TE_REQUIRE(N >= 1 && D >= 1 && D <= kMaxD, TE_ERR_SHAPE, "te_fid_moments_f64: N >= 1, 1 <= D <= %d (got N %lld, D %d)", kMaxD,
               (long long)N, D);
    const int SP = split(N, D), TD = tiles(D);
    TE_REQUIRE(SP == 1 || ws, TE_ERR_NULL, "te_fid_moments_f64: a workspace of te_fid_moments_ws_bytes(N, D) bytes is required");
    hipStream_t st = (hipStream_t)stream;
    const bool al = D % 4 == 0 && te::aligned16(x);
    const dim3 grid(TD, TD, SP);
    const int acc = accumulate ? 1 : 0;
    if (SP == 1) {
        if (al) fid_moments_kernel<true, true><<<grid, NT, 0, st>>>(S, s, x, N, D, acc);
        else fid_moments_kernel<false, true><<<grid, NT, 0, st>>>(S, s, x, N, D, acc);
    } else {
        double* part = (double*)ws;
        double* spart = part + (int64_t)SP * upper_tiles(D) * BT * BT;
        if (al) fid_moments_kernel<true, false><<<grid, NT, 0, st>>>(part, spart, x, N, D, acc);
        else fid_moments_kernel<false, false><<<grid, NT, 0, st>>>(part, spart, x, N, D, acc);
        fid_combine_kernel<<<dim3(TD, TD), NT, 0, st>>>(S, s, part, spart, D, SP, acc);
    }
    return te::launch_status("te_fid_moments_f64");
}

extern "C" int te_fid_finalize_f64(double* mean, double* cov, const double* S, const double* s, int64_t n, int D, te_stream_t stream) {
    TE_REQUIRE(mean && cov && S && s, TE_ERR_NULL, "te_fid_finalize_f64: NULL pointer");
    TE_REQUIRE(D >= 1 && D <= kMaxD, TE_ERR_SHAPE, "te_fid_finalize_f64: 1 <= D <= %d (got %d)", kMaxD, D);
    TE_REQUIRE(n >= 2, TE_ERR_SHAPE, "te_fid_finalize_f64: a covariance needs n >= 2 samples (got %lld)", (long long)n);
    fid_finalize_kernel<<<dim3((D + NT - 1) / NT, D), NT, 0, (hipStream_t)stream>>>(mean, cov, S, s, (double)n, D);
    return te::launch_status("te_fid_finalize_f64");
}
