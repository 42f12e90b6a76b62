// The NT GEMM main loop on the fp32-input MFMA that prdc.hip's distance kernels and svm.hip's Gram kernel share: one 128 x 128 tile of
// X . Y^T for row-major X [N,D] and Y [M,D], staged through a 128 x 32 LDS panel per operand, 4 waves, each wave 2 x 2 tiles of
// v_mfma_f32_32x32x2_f32.  The products of one output element are summed as ONE fp32 fma chain in a fixed permutation of k that is the
// same for A and B, so dot(x_i, y_j) == dot(y_j, x_i) bit for bit.  Rows >= N / M and the k tail are loaded as zeros.
#pragma once
#include "te_common.h"

namespace te {
namespace nt {

constexpr int BT = 128;          // tile rows = tile columns
constexpr int BK = 32;
constexpr int LD = 36;           // LDS row pitch in floats: 144 B keeps the 16-byte stores aligned and ds_read_b128 conflict-free
constexpr int NT = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

template <bool AL>
__device__ __forceinline__ void load_panel(float4 (&r)[4], const float* __restrict__ base, int row0, int nrows, int D, int k0) {
    const int t = threadIdx.x;
    const int k = k0 + (t & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + (t >> 3) + 32 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < nrows) {
            const float* p = base + (int64_t)row * D + k;
            if (AL) {
                if (k < D) v = *reinterpret_cast<const float4*>(p);      // D % 4 == 0: the four are inside the row or all past it
            } else {
                if (k < D) v.x = p[0];
                if (k + 1 < D) v.y = p[1];
                if (k + 2 < D) v.z = p[2];
                if (k + 3 < D) v.w = p[3];
            }
        }
        r[i] = v;
    }
}

__device__ __forceinline__ void store_panel(float* s, const float4 (&r)[4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(s + ((t >> 3) + 32 * i) * LD + (t & 7) * 4) = r[i];
}

// acc[m][n] = the 32 x 32 tile (m, n) of this wave's 64 x 64 quarter of X[row0 : row0 + 128] . Y[col0 : col0 + 128]^T.
// Lane (c = lane & 31, h = lane >> 5) feeds k = 8q + 4h + u of every 32-deep step to MFMA (q, u): the same for A and B, so the order
// in which the products are summed is one fixed permutation of k.
template <bool AL>
__device__ __forceinline__ void gemm_tile(f32x16 (&acc)[2][2], float* As, float* Bs, const float* __restrict__ x, int row0, int N,
                                          const float* __restrict__ y, int col0, int M, int D) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
    float4 ra[4], rb[4];
    load_panel<AL>(ra, x, row0, N, D, 0);
    load_panel<AL>(rb, y, col0, M, D, 0);
    const float* ap = As + (wm * 64 + c) * LD + 4 * h;
    const float* bp = Bs + (wn * 64 + c) * LD + 4 * h;
    for (int k0 = 0; k0 < D; k0 += BK) {
        __syncthreads();                                     // the previous step's (or the previous epilogue's) LDS reads are done
        store_panel(As, ra);
        store_panel(Bs, rb);
        __syncthreads();
        if (k0 + BK < D) {                                   // in flight behind the MFMAs below
            load_panel<AL>(ra, x, row0, N, D, k0 + BK);
            load_panel<AL>(rb, y, col0, M, D, k0 + BK);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const float4*>(ap + m * 32 * LD + 8 * q);
#pragma unroll
            for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const float4*>(bp + n * 32 * LD + 8 * q);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].x, b[n].x, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].y, b[n].y, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].z, b[n].z, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].w, b[n].w, acc[m][n], 0, 0, 0);
                }
        }
    }
}

// row of accumulator register e inside a 32 x 32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

}  // namespace nt
}  // namespace te
