// The linear C-SVC behind an editing boundary (our_interfaceGAN/train_boundary.py:113-114 and :138: sklearn's SVC(kernel='linear'),
// i.e. libsvm's SMO on the host), from the training rows on:
//
//     te_gram_f32     : K = x x^T                                  fp32-input MFMA, fp32 accumulation (libsvm's Qfloat cache is fp32)
//     te_svm_smo_f64  : min 1/2 a^T Q a - e^T a,  0 <= a <= C,  y^T a = 0,  Q_ij = y_i y_j K_ij      libsvm's Solver, no shrinking
//     te_svm_coef_f32 : w[d] = sum_i a_i y_i x[i,d]                the un-normalised coef_
//
// Gram: the 128 x 128 x 32 main loop of gemm_nt_f32.h (prdc.hip's) over the tiles with tj >= ti; the epilogue writes every element it
// owns to K[i][j] AND K[j][i] (on a diagonal tile only the lanes with j >= i write), so the two triangles hold the same bits by
// construction.  One owner and one summation order per element, no atomics.
//
// SMO: ONE workgroup of 1024 threads; thread t owns the elements t, t + 1024, ... (at most 8 for n <= 8192): their gradient and alpha
// in fp64 registers.  Labels and the fp32 diagonal of K sit in LDS.  One iteration is
//     A  i = argmax over I_up of -y_t G_t                                                   -> barrier 1
//     B  row i of K (global memory / cache), j = argmax over I_low with b > 0 of b^2 / a,  Gmin  -> barrier 2
//        the owners of i and j publish alpha_i, alpha_j, G_j, K_ij; thread 0 publishes the stop decision -> barrier 3
//     C  every thread reads the decision; the two-variable update (computed redundantly by every thread from the published values),
//        row j of K, G += Q_i da_i + Q_j da_j.
// Both reductions prefer the LOWEST index among equal values (libsvm's loops keep the highest; the optimum does not depend on it), at
// every level: per thread ascending, across lanes, across waves.  All threads reach all barriers; the loop is bounded by max_iter.
//
// The labels are a HOST array of n values +-1: they are validated on the host and travel as 8192 bits of kernel argument.
#include <limits.h>

#include "gemm_nt_f32.h"

namespace {

using namespace te::nt;

constexpr int kMaxGramRows = 1 << 22;     // 32768 tile rows: inside the grid limits
constexpr int kMaxN = 8192;               // SMO / coef rows: 8 per thread of the one workgroup
constexpr int SNT = 1024;
constexpr int kWaves = SNT / 64;
constexpr int kMaxR = kMaxN / SNT;
constexpr double kTau = 1e-12;            // libsvm's TAU

struct Labels {
    uint32_t w[kMaxN / 32];               // bit t set: y_t = +1
};

// ---------------------------------------------------------------------------------------------------- Gram
template <bool AL>
__global__ __launch_bounds__(NT, 2) void gram_kernel(float* __restrict__ K, const float* __restrict__ x, int n, int D) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;
    __shared__ __attribute__((aligned(16))) float lds[2 * BT * LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1, c = lane & 31, h = lane >> 5;
    f32x16 acc[2][2];
    gemm_tile<AL>(acc, lds, lds + BT * LD, x, ti * BT, n, x, tj * BT, n, D);
    const bool diag = ti == tj;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
            const int col = tj * BT + wn * 64 + nn * 32 + c;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = ti * BT + wm * 64 + m * 32 + acc_row(e, h);
                if (row < n && col < n && (!diag || col >= row)) {
                    const float v = acc[m][nn][e];
                    K[(int64_t)row * n + col] = v;
                    if (col != row) K[(int64_t)col * n + row] = v;
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------------- SMO
// (v, idx) <- the better of it and (ov, oi): the larger value, the lower index among equals
__device__ __forceinline__ void take_better(double& v, int& idx, double ov, int oi) {
    if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
    }
}

__device__ __forceinline__ void wave_argmax(double& v, int& idx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        take_better(v, idx, ov, oi);
    }
}

template <int R>
__global__ __launch_bounds__(SNT) void smo_kernel(double* __restrict__ alpha_out, double* __restrict__ rho_out, int32_t* __restrict__ info,
                                                  const float* __restrict__ K, Labels lab, int n, double C, double eps,
                                                  int64_t max_iter) {
    __shared__ float qd_s[kMaxN];
    __shared__ signed char y_s[kMaxN];
    __shared__ double ra_v[kWaves], rb_v[kWaves], rb_g[kWaves];
    __shared__ int ra_i[kWaves], rb_i[kWaves];
    __shared__ double pub[4];                                // alpha_i, alpha_j, G_j, K_ij
    __shared__ int stop_s;
    __shared__ double fin_ub[kWaves], fin_lb[kWaves], fin_sf[kWaves];
    __shared__ int fin_nf[kWaves];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;

    double G[R], a[R];
    float ki[R], kj[R];
    int yv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int idx = t + SNT * r;
        G[r] = -1.0;
        a[r] = 0.0;
        ki[r] = kj[r] = 0.f;
        yv[r] = 1;
        if (idx < n) {
            yv[r] = (lab.w[idx >> 5] >> (idx & 31)) & 1 ? 1 : -1;
            y_s[idx] = (signed char)yv[r];
            qd_s[idx] = K[(int64_t)idx * n + idx];
        }
    }
    __syncthreads();

    int64_t it = 0;
    int converged = 0;
    for (; it < max_iter; ++it) {
        // ---- A: i = argmax of -y_t G_t over I_up = {y = +1, a < C} u {y = -1, a > 0}
        double bv = -INFINITY;
        int bi = INT_MAX;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = t + SNT * r;
            if (idx < n) {
                const bool up = yv[r] > 0 ? a[r] < C : a[r] > 0.0;
                const double v = yv[r] > 0 ? -G[r] : G[r];
                if (up && v > bv) {
                    bv = v;
                    bi = idx;
                }
            }
        }
        wave_argmax(bv, bi);
        if (lane == 0) {
            ra_v[wid] = bv;
            ra_i[wid] = bi;
        }
        __syncthreads();                                     // 1
        bv = ra_v[0];
        bi = ra_i[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) take_better(bv, bi, ra_v[w], ra_i[w]);
        const int i = bi;
        const double Gmax = bv;
        const bool have_i = i != INT_MAX;

        // ---- B: j = argmax of b^2 / a over I_low = {y = +1, a > 0} u {y = -1, a < C} with b = Gmax + y_t G_t > 0; Gmax2 = max y_t G_t
        double gv = -INFINITY, g2 = -INFINITY;
        int gj = INT_MAX, yi = 1;
        if (have_i) {
            yi = y_s[i];
            const double qdi = qd_s[i];
            const float* Ki = K + (int64_t)i * n;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int idx = t + SNT * r;
                if (idx < n) ki[r] = Ki[idx];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int idx = t + SNT * r;
                if (idx < n) {
                    const bool low = yv[r] > 0 ? a[r] > 0.0 : a[r] < C;
                    if (low) {
                        const double yG = yv[r] > 0 ? G[r] : -G[r];
                        g2 = fmax(g2, yG);
                        const double b = Gmax + yG;
                        if (b > 0.0) {
                            double q = (qdi + (double)qd_s[idx]) - 2.0 * (double)ki[r];
                            if (!(q > 0.0)) q = kTau;
                            const double gain = b * b / q;
                            if (gain > gv) {
                                gv = gain;
                                gj = idx;
                            }
                        }
                    }
                }
            }
        }
        wave_argmax(gv, gj);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) g2 = fmax(g2, __shfl_xor(g2, off, 64));
        if (lane == 0) {
            rb_v[wid] = gv;
            rb_i[wid] = gj;
            rb_g[wid] = g2;
        }
        __syncthreads();                                     // 2
        gv = rb_v[0];
        gj = rb_i[0];
        g2 = rb_g[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            take_better(gv, gj, rb_v[w], rb_i[w]);
            g2 = fmax(g2, rb_g[w]);
        }
        const int j = gj;
        const bool have_j = j != INT_MAX;
        if (have_j) {                                        // row j is in flight behind the barrier
            const float* Kj = K + (int64_t)j * n;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int idx = t + SNT * r;
                if (idx < n) kj[r] = Kj[idx];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = t + SNT * r;
            if (idx == i) pub[0] = a[r];
            if (idx == j) {
                pub[1] = a[r];
                pub[2] = G[r];
                pub[3] = (double)ki[r];
            }
        }
        if (t == 0) stop_s = (!have_i || !have_j || Gmax + g2 < eps) ? 1 : 0;
        __syncthreads();                                     // 3
        if (stop_s) {                                        // the one decision, read by every thread
            converged = 1;
            break;
        }

        // ---- C: the two-variable update (svm.cpp Solver::Solve), the same arithmetic in every thread
        const int yj = y_s[j];
        const double old_ai = pub[0], old_aj = pub[1], Gj = pub[2], Kij = pub[3];
        const double Gi = yi > 0 ? -Gmax : Gmax;
        double q = ((double)qd_s[i] + (double)qd_s[j]) - 2.0 * Kij;      // Q_ij = y_i y_j K_ij: the same a = K_ii + K_jj - 2 K_ij in both branches
        if (!(q > 0.0)) q = kTau;
        double ai = old_ai, aj = old_aj;
        if (yi != yj) {
            const double delta = (-Gi - Gj) / q;
            const double diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) {
                if (aj < 0.0) { aj = 0.0; ai = diff; }
            } else {
                if (ai < 0.0) { ai = 0.0; aj = -diff; }
            }
            if (diff > 0.0) {                                // C_i - C_j = 0
                if (ai > C) { ai = C; aj = C - diff; }
            } else {
                if (aj > C) { aj = C; ai = C + diff; }
            }
        } else {
            const double delta = (Gi - Gj) / q;
            const double sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > C) {
                if (ai > C) { ai = C; aj = sum - C; }
            } else {
                if (aj < 0.0) { aj = 0.0; ai = sum; }
            }
            if (sum > C) {
                if (aj > C) { aj = C; ai = sum - C; }
            } else {
                if (ai < 0.0) { ai = 0.0; aj = sum; }
            }
        }
        const double dai = ai - old_ai, daj = aj - old_aj;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = t + SNT * r;
            if (idx < n) {
                if (idx == i) a[r] = ai;
                if (idx == j) a[r] = aj;
                const double qi = yv[r] == yi ? (double)ki[r] : -(double)ki[r];
                const double qj = yv[r] == yj ? (double)kj[r] : -(double)kj[r];
                G[r] += qi * dai + qj * daj;
            }
        }
    }

    // ---- rho (svm.cpp Solver::calculate_rho): the mean of y_t G_t over the free variables, else the midpoint of the two bounds
    double ub = INFINITY, lb = -INFINITY, sf = 0.0;
    int nf = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int idx = t + SNT * r;
        if (idx < n) {
            const double yG = yv[r] > 0 ? G[r] : -G[r];
            if (a[r] >= C) {
                if (yv[r] < 0) ub = fmin(ub, yG); else lb = fmax(lb, yG);
            } else if (a[r] <= 0.0) {
                if (yv[r] > 0) ub = fmin(ub, yG); else lb = fmax(lb, yG);
            } else {
                ++nf;
                sf += yG;
            }
            alpha_out[idx] = a[r];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ub = fmin(ub, __shfl_xor(ub, off, 64));
        lb = fmax(lb, __shfl_xor(lb, off, 64));
        sf += __shfl_xor(sf, off, 64);
        nf += __shfl_xor(nf, off, 64);
    }
    if (lane == 0) {
        fin_ub[wid] = ub;
        fin_lb[wid] = lb;
        fin_sf[wid] = sf;
        fin_nf[wid] = nf;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) {
            ub = fmin(ub, fin_ub[w]);
            lb = fmax(lb, fin_lb[w]);
            sf += fin_sf[w];
            nf += fin_nf[w];
        }
        rho_out[0] = nf > 0 ? sf / nf : (ub + lb) / 2.0;
        info[0] = it > INT_MAX ? INT_MAX : (int32_t)it;
        info[1] = converged;
    }
}

// ---------------------------------------------------------------------------------------------------- coef
// one owner thread per d; i ascending in fp64, one rounding to fp32.  alpha_i is uniform, so a row with alpha_i == 0 (it adds an exact
// zero for finite x) is skipped by all threads together.
__global__ __launch_bounds__(64) void coef_kernel(float* __restrict__ w, const float* __restrict__ x, const double* __restrict__ alpha,
                                                  Labels lab, int n, int D) {
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const double ai = alpha[i];
        if (ai != 0.0) {
            const double c = (lab.w[i >> 5] >> (i & 31)) & 1 ? ai : -ai;
            s = fma(c, (double)x[(int64_t)i * D + d], s);
        }
    }
    w[d] = (float)s;
}

// the n host labels -> bits; TE_ERR_SHAPE unless every label is +1 or -1
int pack_labels(Labels& L, const char* what, const int8_t* y, int n, int& n_pos) {
    for (int k = 0; k < kMaxN / 32; ++k) L.w[k] = 0;
    n_pos = 0;
    for (int t = 0; t < n; ++t) {
        TE_REQUIRE(y[t] == 1 || y[t] == -1, TE_ERR_SHAPE, "%s: labels must be +1 or -1 (got %d at %d)", what, (int)y[t], t);
        if (y[t] == 1) {
            L.w[t >> 5] |= 1u << (t & 31);
            ++n_pos;
        }
    }
    return 0;
}

}  // namespace

extern "C" int te_gram_f32(float* K, const float* x, int n, int D, te_stream_t stream) {
    TE_REQUIRE(K && x, TE_ERR_NULL, "te_gram_f32: NULL pointer");
    TE_REQUIRE(n >= 1 && n <= kMaxGramRows && D >= 1, TE_ERR_SHAPE, "te_gram_f32: 1 <= n <= %d, D >= 1 (got %d, %d)", kMaxGramRows, n, D);
    const int T = (n + BT - 1) / BT;
    if (D % 4 == 0 && te::aligned16(x))
        gram_kernel<true><<<dim3(T, T), NT, 0, (hipStream_t)stream>>>(K, x, n, D);
    else
        gram_kernel<false><<<dim3(T, T), NT, 0, (hipStream_t)stream>>>(K, x, n, D);
    return te::launch_status("te_gram_f32");
}

extern "C" int te_svm_smo_f64(double* alpha, double* rho, int32_t* info, const float* K, const int8_t* y, int n, double C, double eps,
                              int64_t max_iter, te_stream_t stream) {
    TE_REQUIRE(alpha && rho && info && K && y, TE_ERR_NULL, "te_svm_smo_f64: NULL pointer");
    TE_REQUIRE(n >= 2 && n <= kMaxN, TE_ERR_SHAPE, "te_svm_smo_f64: 2 <= n <= %d (got %d)", kMaxN, n);
    TE_REQUIRE(C > 0.0 && eps > 0.0 && max_iter >= 0, TE_ERR_SHAPE, "te_svm_smo_f64: C > 0, eps > 0, max_iter >= 0 (got %g, %g, %lld)", C,
               eps, (long long)max_iter);
    Labels L;
    int n_pos = 0;
    if (int rc = pack_labels(L, "te_svm_smo_f64", y, n, n_pos)) return rc;
    TE_REQUIRE(n_pos >= 1 && n_pos < n, TE_ERR_SHAPE, "te_svm_smo_f64: both labels must be present (%d of %d are +1)", n_pos, n);
    hipStream_t st = (hipStream_t)stream;
    switch ((n + SNT - 1) / SNT) {
#define TE_SMO_CASE(R) \
    case R: smo_kernel<R><<<1, SNT, 0, st>>>(alpha, rho, info, K, L, n, C, eps, max_iter); break;
        TE_SMO_CASE(1) TE_SMO_CASE(2) TE_SMO_CASE(3) TE_SMO_CASE(4) TE_SMO_CASE(5) TE_SMO_CASE(6) TE_SMO_CASE(7)
        default: static_assert(kMaxR == 8, "one case per owned-element count"); smo_kernel<8><<<1, SNT, 0, st>>>(alpha, rho, info, K, L, n, C, eps, max_iter);
#undef TE_SMO_CASE
    }
    return te::launch_status("te_svm_smo_f64");
}

extern "C" int te_svm_coef_f32(float* w, const float* x, const double* alpha, const int8_t* y, int n, int D, te_stream_t stream) {
    TE_REQUIRE(w && x && alpha && y, TE_ERR_NULL, "te_svm_coef_f32: NULL pointer");
    TE_REQUIRE(n >= 1 && n <= kMaxN && D >= 1, TE_ERR_SHAPE, "te_svm_coef_f32: 1 <= n <= %d, D >= 1 (got %d, %d)", kMaxN, n, D);
    Labels L;
    int n_pos = 0;
    if (int rc = pack_labels(L, "te_svm_coef_f32", y, n, n_pos)) return rc;
    coef_kernel<<<(D + 63) / 64, 64, 0, (hipStream_t)stream>>>(w, x, alpha, L, n, D);
    return te::launch_status("te_svm_coef_f32");
}
