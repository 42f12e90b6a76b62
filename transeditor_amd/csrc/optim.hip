// T2: multi-tensor Adam and EMA — ONE launch over all parameter tensors of a module.
//
// Reference: train_spatial_query.py:458-473 (two torch.optim.Adam over 257 / 38 tensors, betas (0, 0.99 ** c)) and
// accumulate(), :56-61 (g_ema <- decay * g_ema + (1 - decay) * g, one mul_ + add_ pair per tensor): hundreds of tiny
// launches per iteration.  Here the tensors are described by a DEVICE table (pointers + sizes) and split into fixed-size
// chunks; block c processes chunk c of tensor chunk_tensor[c].  Pure HBM streaming: Adam reads p, g, v (+ m when
// beta1 != 0) and writes p, m, v once; EMA reads dst, src and writes dst.  16-byte accesses whenever every pointer of
// the tensor is 16-byte aligned (gradients that live inside a GradSync bucket may only be 4-byte aligned: scalar path).
#include "te_common.h"

namespace {

constexpr int THREADS = 256;

struct AdamK {       // scalar prefactors, formed in double on the host (as torch.optim.Adam does) and applied in fp32
    float lr_step, beta1, beta2, w1, w2, eps, bc2_sqrt;      // w1 = 1 - beta1, w2 = 1 - beta2
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, bool has_m, const AdamK& k) {
    // torch.optim.Adam (non-amsgrad, no weight decay), same operation order:
    //   m = lerp(m, g, 1 - beta1);  v = v * beta2 + (1 - beta2) * g * g;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
    float mm;
    if (!has_m) mm = g;                                   // beta1 == 0: lerp weight 1 returns g exactly
    else mm = (k.w1 < 0.5f) ? m + k.w1 * (g - m) : g - (g - m) * (1.f - k.w1);
    float vv = v * k.beta2;
    vv = vv + k.w2 * g * g;
    const float denom = sqrtf(vv) / k.bc2_sqrt + k.eps;
    p = p - k.lr_step * (mm / denom);
    m = mm;
    v = vv;
}

__global__ __launch_bounds__(THREADS) void mt_adam_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ chunks,
                                                           int n, int n_chunks, int chunk_elems, const AdamK k) {
    const int c = blockIdx.x;
    const int t = chunks[c];
    const int64_t off = (int64_t)chunks[n_chunks + c] * chunk_elems;
    float* p = reinterpret_cast<float*>(table[t]);
    const float* g = reinterpret_cast<const float*>(table[n + t]);
    float* m = reinterpret_cast<float*>(table[2 * n + t]);
    float* v = reinterpret_cast<float*>(table[3 * n + t]);
    const int64_t numel = table[4 * n + t];
    if (g == nullptr) return;                              // parameter without gradient this step: skipped, as torch does
    const bool has_m = k.beta1 != 0.f;
    const int64_t len = min((int64_t)chunk_elems, numel - off);
    p += off; g += off; m += off; v += off;
    const bool aligned = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                           reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    if (aligned) {
        const int64_t n4 = len >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += THREADS) {
            float4 P = reinterpret_cast<float4*>(p)[i];
            const float4 G = reinterpret_cast<const float4*>(g)[i];
            float4 M = has_m ? reinterpret_cast<float4*>(m)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 V = reinterpret_cast<float4*>(v)[i];
            adam_elem(P.x, G.x, M.x, V.x, has_m, k);
            adam_elem(P.y, G.y, M.y, V.y, has_m, k);
            adam_elem(P.z, G.z, M.z, V.z, has_m, k);
            adam_elem(P.w, G.w, M.w, V.w, has_m, k);
            reinterpret_cast<float4*>(p)[i] = P;
            reinterpret_cast<float4*>(m)[i] = M;
            reinterpret_cast<float4*>(v)[i] = V;
        }
        for (int64_t i = (n4 << 2) + threadIdx.x; i < len; i += THREADS) {
            float P = p[i], M = has_m ? m[i] : 0.f, V = v[i];
            adam_elem(P, g[i], M, V, has_m, k);
            p[i] = P; m[i] = M; v[i] = V;
        }
    } else {
        for (int64_t i = threadIdx.x; i < len; i += THREADS) {
            float P = p[i], M = has_m ? m[i] : 0.f, V = v[i];
            adam_elem(P, g[i], M, V, has_m, k);
            p[i] = P; m[i] = M; v[i] = V;
        }
    }
}

__global__ __launch_bounds__(THREADS) void mt_ema_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ chunks,
                                                          int n, int n_chunks, int chunk_elems, float decay, float one_minus) {
    const int c = blockIdx.x;
    const int t = chunks[c];
    const int64_t off = (int64_t)chunks[n_chunks + c] * chunk_elems;
    float* d = reinterpret_cast<float*>(table[t]) + off;
    const float* s = reinterpret_cast<const float*>(table[n + t]) + off;
    const int64_t len = min((int64_t)chunk_elems, table[2 * n + t] - off);
    // accumulate(): par1.mul_(decay).add_(1 - decay, par2)  (train_spatial_query.py:60-61)
    if (((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0) {
        const int64_t n4 = len >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += THREADS) {
            float4 D = reinterpret_cast<float4*>(d)[i];
            const float4 S = reinterpret_cast<const float4*>(s)[i];
            D.x = D.x * decay + one_minus * S.x;
            D.y = D.y * decay + one_minus * S.y;
            D.z = D.z * decay + one_minus * S.z;
            D.w = D.w * decay + one_minus * S.w;
            reinterpret_cast<float4*>(d)[i] = D;
        }
        for (int64_t i = (n4 << 2) + threadIdx.x; i < len; i += THREADS) d[i] = d[i] * decay + one_minus * s[i];
    } else {
        for (int64_t i = threadIdx.x; i < len; i += THREADS) d[i] = d[i] * decay + one_minus * s[i];
    }
}

// ----------------------------------------------------------------------------------------------------------- Ranger
// te_mt_ranger_f32: RAdam + Lookahead + gradient centralisation (reference pSp/training/ranger.py:79-165, one parameter at a
// time there) as ONE launch over every tensor of a parameter group.  table[7][n] = p, g (0: skipped), exp_avg, exp_avg_sq,
// slow_buffer, numel, L.  L = numel / shape[0] is the length of a row of the gradient seen as [shape[0], L]; the reference
// subtracts each row's mean from the gradient (ranger.py:118-119) before anything else, so a block owns WHOLE rows:
// work[3][n_work] = tensor, first row, row count.  L == 0: no centralisation, and the "rows" are chunks of tile_elems elements.
//
// A block stages its rows of g in LDS (one 32 KiB array: 4 floats for the wave partials, up to 3 of alignment pad, the tile;
// five workgroups fit a CU), forms each row's sum, writes g - mean back into LDS and runs the element update from there: g
// comes from HBM once.  A row longer than the tile goes through LDS in pieces of RG_LONG elements for its sum, and the update
// then re-reads g from global memory (L2 at these sizes).  No atomics, no workspace.
//
// REDUCTION ORDER.  The sum of a row x[0..L) is a fixed function of L and the element index alone; it does not depend on
// the alignment path, on where the row sits in its block, on the other tensors or on the grid:
//   K = 1 for L <= 32, 64 for L <= 2048, 256 above (constants: the caller's tile, at least 2048, decides only which rows go
//   through LDS in pieces, and those have K = 256 either way);
//   partial_j = (((0 + x[j]) + x[j + K]) + x[j + 2K]) + ...   for j = 0..K-1, in increasing index (j >= L: partial_j = 0);
//   K = 64 : for d = 32, 16, 8, 4, 2, 1:  partial_j <- partial_j + partial_(j xor d)  (every j ends with the same value);
//   K = 256: that butterfly inside each group of 64 consecutive j, giving S0..S3; the sum is (S0 + S1) + (S2 + S3);
//   mean = sum / (float)L (one division), g' = g - mean (one subtraction per element).
// One lane owns a row for K = 1, one wave for K = 64, the block for K = 256.
//
// Element arithmetic: fp32, one rounding per operation in the reference's order (no contraction into fma):
//   v = v * beta2 + ((1 - beta2) * g') * g';  m = m * beta1 + (1 - beta1) * g';  decay != 0: p = p + (-decay) * p;
//   rectified: p = p + (-step_lr) * (m / (sqrt(v) + eps)), else p = p + (-step_lr) * m;
//   lookahead: slow = slow + alpha * (p - slow), p = slow  (slow_buffer is touched on lookahead steps only).
// The schedule (N_sma, step_size, which branch, whether lookahead fires) is the host's: the kernel sees no step count.
constexpr int RG_LDS = 8192;                      // floats of LDS per block: all of 32 KiB
constexpr int RG_TILE_MAX = RG_LDS - 8;           // what is left for the tile
constexpr int RG_LONG = RG_TILE_MAX & ~(THREADS - 1);   // piece of a long row: a multiple of THREADS, so thread t always
                                                        // meets the elements j = t (mod 256) of the row
constexpr int RG_K1 = 32, RG_K64 = 2048;

struct RangerK {
    float beta1, beta2, w1, w2, eps, neg_step_lr, neg_decay, alpha;
    int decay_on, rectified, lookahead;
};

__device__ __forceinline__ void ranger_elem(float& p, float g, float mean, float& m, float& v, float& s, const RangerK& k) {
#pragma clang fp contract(off)
    const float gc = g - mean;
    const float t2 = k.w2 * gc;
    v = v * k.beta2 + t2 * gc;
    m = m * k.beta1 + k.w1 * gc;
    if (k.decay_on) p = p + k.neg_decay * p;
    if (k.rectified) p = p + k.neg_step_lr * (m / (sqrtf(v) + k.eps));
    else p = p + k.neg_step_lr * m;
    if (k.lookahead) {
        s = s + k.alpha * (p - s);
        p = s;
    }
}

// the tensors are global memory (said so in the pointer type: global_load / global_store, which leave the LDS counter alone)
typedef float rg4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float GF;
typedef __attribute__((address_space(1))) rg4 GF4;
__device__ __forceinline__ GF4* rg_v4(GF* x) { return (GF4*)x; }
__device__ __forceinline__ const GF4* rg_v4(const GF* x) { return (const GF4*)x; }
__device__ __forceinline__ rg4* rg_v4(float* x) { return reinterpret_cast<rg4*>(x); }
__device__ __forceinline__ const rg4* rg_v4(const float* x) { return reinterpret_cast<const rg4*>(x); }

// every pointer of the range sits at the same offset inside its 16 bytes: after `head` = (4 - res) & 3 scalar elements all of
// them are 16-byte aligned.  res = that offset in floats.
__device__ __forceinline__ bool rg_aligned(const GF* p, const GF* g, const GF* m, const GF* v, const GF* s, bool with_s, int& res) {
    const uintptr_t a = (uintptr_t)p & 15;
    bool same = ((uintptr_t)g & 15) == a && ((uintptr_t)m & 15) == a && ((uintptr_t)v & 15) == a;
    if (with_s) same = same && ((uintptr_t)s & 15) == a;
    res = same ? (int)(a >> 2) : 0;
    return same;
}

// st[e] = g[e] for e < len; vec: g + head and st + head are 16-byte aligned
__device__ __forceinline__ void rg_stage(float* st, const GF* g, int len, int head, bool vec) {
    if (vec) {
        const int h = min(head, len);
        if ((int)threadIdx.x < h) st[threadIdx.x] = g[threadIdx.x];
        const int n4 = (len - h) >> 2;
        const GF4* g4 = rg_v4(g + h);
        rg4* s4 = rg_v4(st + h);
        for (int i = threadIdx.x; i < n4; i += THREADS) s4[i] = g4[i];
        for (int i = h + (n4 << 2) + threadIdx.x; i < len; i += THREADS) st[i] = g[i];
    } else {
        for (int i = threadIdx.x; i < len; i += THREADS) st[i] = g[i];
    }
}

// the element update of [0, len); g (G = const GF or const float) is global memory, or the staged tile in LDS, which is
// already centralised (mean = 0 then)
template <typename G>
__device__ __forceinline__ void rg_update(GF* p, G* g, GF* m, GF* v, GF* s, int64_t len, int head, bool vec, float mean,
                                          const RangerK& k) {
    auto one = [&](int64_t i) {
        float P = p[i], M = m[i], V = v[i], S = k.lookahead ? s[i] : 0.f;
        ranger_elem(P, g[i], mean, M, V, S, k);
        p[i] = P; m[i] = M; v[i] = V;
        if (k.lookahead) s[i] = S;
    };
    if (!vec) {
        for (int64_t i = threadIdx.x; i < len; i += THREADS) one(i);
        return;
    }
    const int64_t h = min((int64_t)head, len);
    if ((int64_t)threadIdx.x < h) one(threadIdx.x);
    const int64_t n4 = (len - h) >> 2;
    GF4* p4 = rg_v4(p + h);
    auto g4 = rg_v4(g + h);
    GF4* m4 = rg_v4(m + h);
    GF4* v4 = rg_v4(v + h);
    GF4* s4 = rg_v4(s + h);
    for (int64_t i = threadIdx.x; i < n4; i += THREADS) {
        rg4 P = p4[i], M = m4[i], V = v4[i];
        const rg4 G4 = g4[i];
        rg4 S = {0.f, 0.f, 0.f, 0.f};
        if (k.lookahead) S = s4[i];
        float Px = P.x, Py = P.y, Pz = P.z, Pw = P.w, Mx = M.x, My = M.y, Mz = M.z, Mw = M.w;
        float Vx = V.x, Vy = V.y, Vz = V.z, Vw = V.w, Sx = S.x, Sy = S.y, Sz = S.z, Sw = S.w;
        ranger_elem(Px, G4.x, mean, Mx, Vx, Sx, k);
        ranger_elem(Py, G4.y, mean, My, Vy, Sy, k);
        ranger_elem(Pz, G4.z, mean, Mz, Vz, Sz, k);
        ranger_elem(Pw, G4.w, mean, Mw, Vw, Sw, k);
        p4[i] = rg4{Px, Py, Pz, Pw}; m4[i] = rg4{Mx, My, Mz, Mw}; v4[i] = rg4{Vx, Vy, Vz, Vw};
        if (k.lookahead) s4[i] = rg4{Sx, Sy, Sz, Sw};
    }
    for (int64_t i = h + (n4 << 2) + threadIdx.x; i < len; i += THREADS) one(i);
}

__device__ __forceinline__ float rg_wave_sum(float a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = a + __shfl_xor(a, d, 64);
    return a;
}

// K = 256: the block's partials -> the row sum, the same value in every thread.  Ends with the block in step.
__device__ __forceinline__ float rg_block_sum(float a, float* wred) {
    a = rg_wave_sum(a);
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = a;
    __syncthreads();
    const float tot = (wred[0] + wred[1]) + (wred[2] + wred[3]);
    __syncthreads();                                   // wred is free again
    return tot;
}

__global__ __launch_bounds__(THREADS) void mt_ranger_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ work,
                                                             int n, int n_work, int tile, const RangerK k) {
    __shared__ __align__(16) float sh[RG_LDS];
    float* wred = sh;
    float* stage = sh + 4;
    const int c = blockIdx.x;
    const int t = work[c];
    if (t < 0 || t >= n) return;
    const int64_t r0 = work[n_work + c];
    const int64_t nr = work[2 * n_work + c];
    GF* p = (GF*)table[t];
    const GF* g = (const GF*)table[n + t];
    GF* m = (GF*)table[2 * n + t];
    GF* v = (GF*)table[3 * n + t];
    GF* s = (GF*)table[4 * n + t];
    const int64_t numel = table[5 * n + t];
    const int64_t L = table[6 * n + t];
    if (g == nullptr || r0 < 0 || nr <= 0) return;       // no gradient this step: skipped, as the reference does
    int res;
    if (L <= 0) {                                        // no centralisation: a flat chunk, g straight from global memory
        const int64_t off = r0 * tile;
        if (off >= numel) return;
        const int64_t len = min(nr * tile, numel - off);
        const bool vec = rg_aligned(p + off, g + off, m + off, v + off, s + off, k.lookahead, res);
        rg_update(p + off, g + off, m + off, v + off, s + off, len, (4 - res) & 3, vec, 0.f, k);
        return;
    }
    const int64_t r_end = min(r0 + nr, numel / L);       // (a map that names rows past the tensor's end is cut, not followed)
    const float fL = (float)L;
    if (L > tile) {                                      // a long row (K = 256: tile >= RG_K64): its sum through LDS in pieces, then the update from global
        for (int64_t r = r0; r < r_end; ++r) {
            const int64_t off = r * L;
            float a = 0.f;
            for (int64_t q = 0; q < L; q += RG_LONG) {
                const int len = (int)min((int64_t)RG_LONG, L - q);
                const GF* gq = g + off + q;
                const int rq = (int)(((uintptr_t)gq & 15) >> 2);
                __syncthreads();                         // the previous piece has been read
                rg_stage(stage + rq, gq, len, (4 - rq) & 3, true);
                __syncthreads();
                for (int i = threadIdx.x; i < len; i += THREADS) a = a + stage[rq + i];
            }
            const float mean = rg_block_sum(a, wred) / fL;
            const bool vec = rg_aligned(p + off, g + off, m + off, v + off, s + off, k.lookahead, res);
            rg_update(p + off, g + off, m + off, v + off, s + off, L, (4 - res) & 3, vec, mean, k);
        }
        return;
    }
    const int iL = (int)L;
    const int cap = tile / iL;                           // whole rows a tile holds (>= 1)
    for (int64_t rs = r0; rs < r_end; rs += cap) {
        const int cnt = (int)min((int64_t)cap, r_end - rs);
        const int len = cnt * iL;
        const int64_t off = rs * L;
        const bool vec = rg_aligned(p + off, g + off, m + off, v + off, s + off, k.lookahead, res);
        const int head = (4 - res) & 3;
        float* st = stage + res;
        __syncthreads();                                 // the previous group's update has read its tile
        rg_stage(st, g + off, len, head, vec);
        __syncthreads();
        if (iL <= RG_K1) {                               // K = 1: a lane per row
            for (int r = threadIdx.x; r < cnt; r += THREADS) {
                float* x = st + r * iL;
                float a = 0.f;
                for (int i = 0; i < iL; ++i) a = a + x[i];
                const float mean = a / fL;
                for (int i = 0; i < iL; ++i) x[i] = x[i] - mean;
            }
        } else if (iL <= RG_K64) {                       // K = 64: a wave per row
            const int lane = threadIdx.x & 63;
            for (int r = threadIdx.x >> 6; r < cnt; r += THREADS / 64) {
                float* x = st + r * iL;
                float a = 0.f;
                for (int i = lane; i < iL; i += 64) a = a + x[i];
                const float mean = rg_wave_sum(a) / fL;
                for (int i = lane; i < iL; i += 64) x[i] = x[i] - mean;
            }
        } else {                                         // K = 256: the block per row
            for (int r = 0; r < cnt; ++r) {
                float* x = st + r * iL;
                float a = 0.f;
                for (int i = threadIdx.x; i < iL; i += THREADS) a = a + x[i];
                const float mean = rg_block_sum(a, wred) / fL;
                for (int i = threadIdx.x; i < iL; i += THREADS) x[i] = x[i] - mean;
            }
        }
        __syncthreads();
        rg_update(p + off, (const float*)st, m + off, v + off, s + off, len, head, vec, 0.f, k);
    }
}

}  // namespace

extern "C" int te_mt_adam_f32(const int64_t* table, const int32_t* chunks, int n_tensors, int n_chunks, int chunk_elems,
                              double lr, double beta1, double beta2, double eps, int step, te_stream_t stream_) {
    TE_REQUIRE(table && chunks, TE_ERR_NULL, "te_mt_adam_f32: NULL table");
    TE_REQUIRE(n_tensors > 0 && n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0 && step > 0, TE_ERR_SHAPE,
               "te_mt_adam_f32: bad table dims / step");
    // scalar prefactors in double, as torch.optim.Adam computes them on the host
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    AdamK k;
    k.lr_step = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.beta1 = (float)beta1; k.beta2 = (float)beta2; k.w1 = (float)(1.0 - beta1); k.w2 = (float)(1.0 - beta2); k.eps = (float)eps;
    mt_adam_kernel<<<n_chunks, THREADS, 0, (hipStream_t)stream_>>>(table, chunks, n_tensors, n_chunks, chunk_elems, k);
    return te::launch_status("te_mt_adam_f32");
}

extern "C" int te_mt_ema_f32(const int64_t* table, const int32_t* chunks, int n_tensors, int n_chunks, int chunk_elems,
                             double decay, te_stream_t stream_) {
    TE_REQUIRE(table && chunks, TE_ERR_NULL, "te_mt_ema_f32: NULL table");
    TE_REQUIRE(n_tensors > 0 && n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0, TE_ERR_SHAPE, "te_mt_ema_f32: bad table dims");
    mt_ema_kernel<<<n_chunks, THREADS, 0, (hipStream_t)stream_>>>(table, chunks, n_tensors, n_chunks, chunk_elems, (float)decay,
                                                                  (float)(1.0 - decay));
    return te::launch_status("te_mt_ema_f32");
}

extern "C" int te_mt_ranger_f32(const int64_t* table, const int32_t* work, int n_tensors, int n_work, int tile_elems,
                                double step_lr, double decay, double beta1, double beta2, double eps, double alpha, int rectified,
                                int lookahead, te_stream_t stream_) {
    TE_REQUIRE(table && work, TE_ERR_NULL, "te_mt_ranger_f32: NULL table");
    TE_REQUIRE(n_tensors > 0 && n_work > 0, TE_ERR_SHAPE, "te_mt_ranger_f32: bad table dims");
    TE_REQUIRE(tile_elems >= RG_K64 && tile_elems % 4 == 0 && tile_elems <= RG_TILE_MAX, TE_ERR_SHAPE,
               "te_mt_ranger_f32: the tile must be a multiple of 4 from 2048 to 8184 elements");
    TE_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, TE_ERR_SHAPE, "te_mt_ranger_f32: beta outside [0, 1)");
    TE_REQUIRE(eps > 0.0, TE_ERR_SHAPE, "te_mt_ranger_f32: eps must be positive");
    TE_REQUIRE(alpha >= 0.0 && alpha <= 1.0, TE_ERR_SHAPE, "te_mt_ranger_f32: alpha outside [0, 1]");
    // the scalars arrive formed in double (ranger.py:147,152,154 form them as python floats) and are applied in fp32
    RangerK k;
    k.beta1 = (float)beta1; k.beta2 = (float)beta2; k.w1 = (float)(1.0 - beta1); k.w2 = (float)(1.0 - beta2); k.eps = (float)eps;
    k.neg_step_lr = (float)(-step_lr); k.neg_decay = (float)(-decay); k.alpha = (float)alpha;
    k.decay_on = decay != 0.0; k.rectified = rectified != 0; k.lookahead = lookahead != 0;
    mt_ranger_kernel<<<n_work, THREADS, 0, (hipStream_t)stream_>>>(table, work, n_tensors, n_work, tile_elems, k);
    return te::launch_status("te_mt_ranger_f32");
}
