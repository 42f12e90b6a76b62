// Precision / recall / density / coverage (metrics/prdc.py) on squared distances, without ever writing a distance matrix:
//
//     te_row_sqnorm_f32  : nx[i] = sum_k x[i,k]^2
//     te_prdc_knn_f32    : r2[i] = the (k+1)-th smallest of d2(i, :) over the set itself, diagonal exactly 0 (prdc.py:41-51)
//     te_prdc_counts_f32 : col_count / row_any / row_min of the real x fake matrix against the two radii (prdc.py:75-93)
//
//     d2(i,j) = max(nx[i] + ny[j] - 2 dot(x_i, y_j), 0)
//
// One NT GEMM main loop (gemm_nt_f32.h, shared with svm.hip) serves both: a 128 x 128 x 32 LDS tile, 4 waves, each wave 2 x 2 tiles
// of v_mfma_f32_32x32x2_f32 (an fp32 fma chain in a fixed k order, so dot(x_i, y_j) == dot(y_j, x_i) bit for bit and the
// self-distance matrix is exactly symmetric).  A
// workgroup owns one block of 128 COLUMNS (the B operand) and walks a chunk of the row tiles; a column's reduction over rows is over
// the accumulator registers of one lane and stays in registers across the whole walk:
//   - knn: the self-distance matrix is symmetric, so the k+1 smallest of row i are the k+1 smallest of COLUMN i: every lane keeps a
//     sorted list of KP >= k+1 values per column;
//   - counts: col_count is a per-lane counter; row_min / row_any are reduced over the 32 lanes of a tile row by shuffles and written
//     once per (column block, row) to the workspace.
// The partials (row chunks x columns, column blocks x rows) are combined by a second, fixed-order kernel: no atomics anywhere, every
// output is bit-reproducible.  Rows >= N and columns >= M are loaded as zeros and masked before they reach any reduction.
#include "gemm_nt_f32.h"

namespace {

using namespace te::nt;      // BT, BK, LD, NT, gemm_tile, acc_row: the 128 x 128 x 32 main loop

constexpr int kMaxSplit = 8;     // row chunks per column block: 8 keeps an XCD's resident workgroups on few operand panels
constexpr int kMaxK = 15;

// Workgroup p of the launch -> (column block, row chunk).  Workgroup ids go round-robin over the 8 XCDs; the remap hands every XCD one
// contiguous eighth of the (column block, row chunk) list, so the workgroups resident on one L2 share few operand panels.
__device__ __forceinline__ void block_coords(int S, int& cb, int& chunk) {
    const int nwg = gridDim.x, p = blockIdx.x;
    const int q = nwg / te::kNumXCD, r = nwg % te::kNumXCD, xcd = p % te::kNumXCD;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + p / te::kNumXCD;
    cb = id / S;
    chunk = id % S;
}

template <int KP>
__device__ __forceinline__ void list_insert(float (&lst)[KP], float v) {
    if (v < lst[KP - 1]) {
#pragma unroll
        for (int s = 0; s < KP; ++s) {
            const float lo = fminf(lst[s], v);
            v = fmaxf(lst[s], v);
            lst[s] = lo;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- k nearest neighbours
// part[chunk][j][0 .. KP): the KP smallest d2(i, j) over the rows i of the chunk, ascending (+inf where the chunk has fewer rows)
template <int KP, bool AL>
__global__ __launch_bounds__(NT, 2) void prdc_knn_kernel(float* __restrict__ part, const float* __restrict__ x,
                                                         const float* __restrict__ nx, int N, int D, int S) {
    __shared__ __attribute__((aligned(16))) float lds[2 * BT * LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
    int cb, chunk;
    block_coords(S, cb, chunk);
    const int col0 = cb * BT;
    const int RT = (N + BT - 1) / BT;
    const int t0 = (int)((int64_t)chunk * RT / S), t1 = (int)((int64_t)(chunk + 1) * RT / S);
    int col[2];
    float nyj[2];
    float lst[2][KP];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        col[n] = col0 + wn * 64 + n * 32 + c;
        nyj[n] = col[n] < N ? nx[col[n]] : 0.f;
#pragma unroll
        for (int s = 0; s < KP; ++s) lst[n][s] = INFINITY;
    }
    for (int rt = t0; rt < t1; ++rt) {
        f32x16 acc[2][2];
        gemm_tile<AL>(acc, lds, lds + BT * LD, x, rt * BT, N, x, col0, N, D);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = rt * BT + wm * 64 + m * 32 + acc_row(e, h);
                if (row < N) {                               // a row past the end never reaches a list
                    const float nxi = nx[row];
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const float v = row == col[n] ? 0.f : fmaxf((nxi + nyj[n]) - 2.f * acc[m][n][e], 0.f);
                        list_insert<KP>(lst[n], v);
                    }
                }
            }
    }
    // the four lists of a column (two row halves of the wave tile x two waves) -> one
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int s = 0; s < KP; ++s) lds[((wn * 64 + n * 32 + c) * 4 + wm * 2 + h) * KP + s] = lst[n][s];
    __syncthreads();
    if (threadIdx.x < BT && col0 + threadIdx.x < N) {
        float out[KP];
        const float* src = lds + threadIdx.x * 4 * KP;
#pragma unroll
        for (int s = 0; s < KP; ++s) out[s] = src[s];
        for (int s = KP; s < 4 * KP; ++s) list_insert<KP>(out, src[s]);
        float* dst = part + ((int64_t)chunk * N + col0 + threadIdx.x) * KP;
#pragma unroll
        for (int s = 0; s < KP; ++s) dst[s] = out[s];
    }
}

template <int KP>
__global__ __launch_bounds__(256) void prdc_knn_reduce_kernel(float* __restrict__ r2, const float* __restrict__ part, int N, int S, int k) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float out[KP];
#pragma unroll
    for (int s = 0; s < KP; ++s) out[s] = part[(int64_t)j * KP + s];
    for (int ch = 1; ch < S; ++ch)
        for (int s = 0; s < KP; ++s) list_insert<KP>(out, part[((int64_t)ch * N + j) * KP + s]);
    float v = out[0];
#pragma unroll
    for (int s = 1; s < KP; ++s) v = s == k ? out[s] : v;
    r2[j] = v;
}

// ---------------------------------------------------------------------------------------------------- the three counts
// cc[chunk][j]: the chunk's share of col_count[j];  pmin / pany[cb][i]: row i's minimum / any over the columns of block cb
template <bool AL>
__global__ __launch_bounds__(NT, 2) void prdc_counts_kernel(int* __restrict__ cc, float* __restrict__ pmin, int* __restrict__ pany,
                                                            const float* __restrict__ x, const float* __restrict__ nx,
                                                            const float* __restrict__ rr2, const float* __restrict__ y,
                                                            const float* __restrict__ ny, const float* __restrict__ rf2, int N, int M,
                                                            int D, int S) {
    __shared__ __attribute__((aligned(16))) float lds[2 * BT * LD];
    __shared__ float rowmin_s[2][BT];
    __shared__ int rowany_s[2][BT];
    __shared__ int cc_s[2][BT];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
    int cb, chunk;
    block_coords(S, cb, chunk);
    const int col0 = cb * BT;
    const int RT = (N + BT - 1) / BT;
    const int t0 = (int)((int64_t)chunk * RT / S), t1 = (int)((int64_t)(chunk + 1) * RT / S);
    bool colok[2];
    float nyj[2], rfj[2];
    int cnt[2] = {0, 0};
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int col = col0 + wn * 64 + n * 32 + c;
        colok[n] = col < M;
        nyj[n] = colok[n] ? ny[col] : 0.f;
        rfj[n] = colok[n] ? rf2[col] : 0.f;
    }
    for (int rt = t0; rt < t1; ++rt) {
        f32x16 acc[2][2];
        gemm_tile<AL>(acc, lds, lds + BT * LD, x, rt * BT, N, y, col0, M, D);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int lrow = wm * 64 + m * 32 + acc_row(e, h);
                const int row = rt * BT + lrow;
                const bool rowok = row < N;
                const float nxi = rowok ? nx[row] : 0.f;
                const float rri = rowok ? rr2[row] : 0.f;
                float vmin = INFINITY;
                int any = 0;
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const float v = fmaxf((nxi + nyj[n]) - 2.f * acc[m][n][e], 0.f);
                    const bool ok = rowok && colok[n];       // a padded row or column never reaches a reduction
                    cnt[n] += (ok && v < rri) ? 1 : 0;
                    any |= (ok && v < rfj[n]) ? 1 : 0;
                    vmin = ok ? fminf(vmin, v) : vmin;
                }
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) {     // over the 32 lanes (columns) that hold this row
                    vmin = fminf(vmin, __shfl_xor(vmin, off, 64));
                    any |= __shfl_xor(any, off, 64);
                }
                if (c == 0) { rowmin_s[wn][lrow] = vmin; rowany_s[wn][lrow] = any; }
            }
        __syncthreads();
        if (threadIdx.x < BT && rt * BT + threadIdx.x < N) {
            const int64_t o = (int64_t)cb * N + rt * BT + threadIdx.x;
            pmin[o] = fminf(rowmin_s[0][threadIdx.x], rowmin_s[1][threadIdx.x]);
            pany[o] = rowany_s[0][threadIdx.x] | rowany_s[1][threadIdx.x];
        }
        // (the next write to rowmin_s / rowany_s lies behind the barriers of the next tile's main loop)
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        cnt[n] += __shfl_xor(cnt[n], 32, 64);
        if (h == 0) cc_s[wm][wn * 64 + n * 32 + c] = cnt[n];
    }
    __syncthreads();
    if (threadIdx.x < BT && col0 + threadIdx.x < M)
        cc[(int64_t)chunk * M + col0 + threadIdx.x] = cc_s[0][threadIdx.x] + cc_s[1][threadIdx.x];
}

__global__ __launch_bounds__(256) void prdc_counts_reduce_kernel(int* __restrict__ col_count, int* __restrict__ row_any,
                                                                  float* __restrict__ row_min, const int* __restrict__ cc,
                                                                  const float* __restrict__ pmin, const int* __restrict__ pany, int N,
                                                                  int M, int S, int CB) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < M) {
        int s = 0;
        for (int ch = 0; ch < S; ++ch) s += cc[(int64_t)ch * M + t];
        col_count[t] = s;
    }
    if (t < N) {
        float v = INFINITY;
        int any = 0;
        for (int b = 0; b < CB; ++b) {
            v = fminf(v, pmin[(int64_t)b * N + t]);
            any |= pany[(int64_t)b * N + t];
        }
        row_min[t] = v;
        row_any[t] = any;
    }
}

__global__ __launch_bounds__(256) void row_sqnorm_kernel(float* __restrict__ out, const float* __restrict__ x, int N, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* p = x + (int64_t)row * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s = fmaf(p[k], p[k], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[row] = s;
}

// ---------------------------------------------------------------------------------------------------- host side
constexpr int kMaxRows = 1 << 24;                             // keeps every int index of the kernels far from overflow

inline int tiles(int n) { return (n + BT - 1) / BT; }
inline int split(int n) { return tiles(n) < kMaxSplit ? tiles(n) : kMaxSplit; }
inline int list_len(int k) { return k < 2 ? 2 : k < 4 ? 4 : k < 8 ? 8 : 16; }
inline int64_t up256(int64_t b) { return (b + 255) / 256 * 256; }

inline int64_t knn_bytes(int n, int k) { return up256((int64_t)split(n) * n * list_len(k) * 4); }
inline int64_t counts_bytes(int N, int M) { return up256((int64_t)split(N) * M * 4) + 2 * up256((int64_t)tiles(M) * N * 4); }


template <int KP>
int launch_knn(float* r2, const float* x, const float* nx, int N, int D, int k, float* part, hipStream_t st) {
    const int S = split(N), grid = tiles(N) * S;
    if (D % 4 == 0 && te::aligned16(x))
        prdc_knn_kernel<KP, true><<<grid, NT, 0, st>>>(part, x, nx, N, D, S);
    else
        prdc_knn_kernel<KP, false><<<grid, NT, 0, st>>>(part, x, nx, N, D, S);
    prdc_knn_reduce_kernel<KP><<<(N + 255) / 256, 256, 0, st>>>(r2, part, N, S, k);
    return te::launch_status("te_prdc_knn_f32");
}

}  // namespace

extern "C" int64_t te_prdc_ws_bytes(int N, int M, int D, int k) {
    if (k < 1 || k > kMaxK || N <= k || M <= k || D < 1 || N > kMaxRows || M > kMaxRows) return TE_ERR_SHAPE;
    const int64_t a = knn_bytes(N, k), b = knn_bytes(M, k), c = counts_bytes(N, M);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

extern "C" int te_row_sqnorm_f32(float* out, const float* x, int N, int D, te_stream_t stream) {
    TE_REQUIRE(out && x, TE_ERR_NULL, "te_row_sqnorm_f32: NULL pointer");
    TE_REQUIRE(N >= 1 && N <= kMaxRows && D >= 1, TE_ERR_SHAPE, "te_row_sqnorm_f32: 1 <= N <= %d, D >= 1 (got %d, %d)", kMaxRows, N, D);
    row_sqnorm_kernel<<<(N + 3) / 4, 256, 0, (hipStream_t)stream>>>(out, x, N, D);
    return te::launch_status("te_row_sqnorm_f32");
}

extern "C" int te_prdc_knn_f32(float* r2, const float* x, const float* nx, int N, int D, int k, void* ws, te_stream_t stream) {
    TE_REQUIRE(r2 && x && nx && ws, TE_ERR_NULL, "te_prdc_knn_f32: NULL pointer");
    TE_REQUIRE(k >= 1 && k <= kMaxK, TE_ERR_SHAPE, "te_prdc_knn_f32: 1 <= k <= %d (got %d)", kMaxK, k);
    TE_REQUIRE(N > k && N <= kMaxRows && D >= 1, TE_ERR_SHAPE, "te_prdc_knn_f32: k + 1 <= N <= %d, D >= 1 (got N %d, D %d, k %d)",
               kMaxRows, N, D, k);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    switch (list_len(k)) {
        case 2: return launch_knn<2>(r2, x, nx, N, D, k, part, st);
        case 4: return launch_knn<4>(r2, x, nx, N, D, k, part, st);
        case 8: return launch_knn<8>(r2, x, nx, N, D, k, part, st);
        default: return launch_knn<16>(r2, x, nx, N, D, k, part, st);
    }
}

extern "C" int te_prdc_counts_f32(int32_t* col_count, int32_t* row_any, float* row_min, const float* x, const float* nx,
                                  const float* rr2, const float* y, const float* ny, const float* rf2, int N, int M, int D, void* ws,
                                  te_stream_t stream) {
    TE_REQUIRE(col_count && row_any && row_min && x && nx && rr2 && y && ny && rf2 && ws, TE_ERR_NULL,
               "te_prdc_counts_f32: NULL pointer");
    TE_REQUIRE(N >= 1 && M >= 1 && N <= kMaxRows && M <= kMaxRows && D >= 1, TE_ERR_SHAPE,
               "te_prdc_counts_f32: 1 <= N, M <= %d, D >= 1 (got %d, %d, %d)", kMaxRows, N, M, D);
    hipStream_t st = (hipStream_t)stream;
    const int S = split(N), CB = tiles(M), grid = CB * S;
    char* w = (char*)ws;
    int* cc = (int*)w;
    float* pmin = (float*)(w + up256((int64_t)S * M * 4));
    int* pany = (int*)(w + up256((int64_t)S * M * 4) + up256((int64_t)CB * N * 4));
    if (D % 4 == 0 && te::aligned16(x) && te::aligned16(y))
        prdc_counts_kernel<true><<<grid, NT, 0, st>>>(cc, pmin, pany, x, nx, rr2, y, ny, rf2, N, M, D, S);
    else
        prdc_counts_kernel<false><<<grid, NT, 0, st>>>(cc, pmin, pany, x, nx, rr2, y, ny, rf2, N, M, D, S);
    const int n = N > M ? N : M;
    prdc_counts_reduce_kernel<<<(n + 255) / 256, 256, 0, st>>>(col_count, row_any, row_min, cc, pmin, pany, N, M, S, CB);
    return te::launch_status("te_prdc_counts_f32");
}
