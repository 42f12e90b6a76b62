// Noise regulariser of the projector (projector_optimization.py:21-49) over the WHOLE list of noise maps, one launch per direction:
//
//     te_noise_reg_fwd_f32   : loss = sum_maps sum_scales (mean(n * roll(n,1,3)))^2 + (mean(n * roll(n,1,2)))^2, 2x2 mean between scales,
//                              stop after the first scale with size <= 8.  ONE block walks every map and scale in the reference's order
//                              (the per-scale means and the downsampled maps are kept in the workspace for the backward)
//     te_noise_reg_bwd_f32   : d loss / d map, one block per map (coarsest scale first, each scale's gradient spread over its 2x2 cells)
//     te_noise_normalize_f32 : in place, (n - mean) / std with the unbiased std, one block per map
//
// Fixed-shape block reductions only: bit-reproducible, no atomics.
#include "te_common.h"

namespace {

constexpr int kMaxMaps = 32;
constexpr int kThreads = 1024;

struct NoiseList {
    float* p[kMaxMaps];
    float* g[kMaxMaps];       // gradients (backward only)
    int size[kMaxMaps];
    int64_t pyr[kMaxMaps];    // offset of the map's first downsampled level in the pyramid workspace
    int stat[kMaxMaps];       // offset of the map's first (A, B) pair in the statistics workspace
    int n;
    int B;
    int nstat;                // floats of statistics (2 per scale of every map)
};

// sum of `v` over the block (1024 threads, 16 waves, fixed order); every thread gets the result
__device__ float block_sum(float v, float* part) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                       // part[] may still be read by the previous call
    if (lane == 0) part[wid] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) s += part[i];
    return s;
}

__global__ __launch_bounds__(kThreads) void noise_reg_fwd_kernel(float* __restrict__ loss, float* __restrict__ stats,
                                                                  float* __restrict__ pyr, NoiseList L) {
    __shared__ float part[kThreads / 64];
    float acc = 0.f;
    for (int i = 0; i < L.n; ++i) {
        const float* cur = L.p[i];
        float* nxt = pyr + L.pyr[i];
        int s = L.size[i], k = 0;
        while (true) {
            const int64_t plane = (int64_t)s * s, M = plane * L.B;
            float sa = 0.f, sb = 0.f;
            for (int64_t e = threadIdx.x; e < M; e += kThreads) {
                const int64_t b = e / plane;
                const int r = (int)(e - b * plane), y = r / s, x = r % s;
                const float* q = cur + b * plane;
                const float v = q[r];
                sa = fmaf(v, q[(int64_t)y * s + (x + s - 1) % s], sa);          // roll(n, 1, dims=3)[y, x] = n[y, x - 1]
                sb = fmaf(v, q[(int64_t)((y + s - 1) % s) * s + x], sb);        // roll(n, 1, dims=2)[y, x] = n[y - 1, x]
            }
            const float A = block_sum(sa, part) / (float)M;
            const float Bm = block_sum(sb, part) / (float)M;
            if (threadIdx.x == 0) { stats[L.stat[i] + 2 * k] = A; stats[L.stat[i] + 2 * k + 1] = Bm; }
            acc = (acc + A * A) + Bm * Bm;
            if (s <= 8) break;
            const int h = s / 2;
            const int64_t M2 = (int64_t)h * h * L.B;
            for (int64_t e = threadIdx.x; e < M2; e += kThreads) {
                const int64_t b = e / ((int64_t)h * h);
                const int r = (int)(e - b * h * h), y = r / h, x = r % h;
                const float* q = cur + b * plane + (int64_t)(2 * y) * s + 2 * x;
                nxt[e] = ((q[0] + q[1]) + (q[s] + q[s + 1])) * 0.25f;
            }
            __syncthreads();
            cur = nxt;
            nxt += M2;
            s = h;
            ++k;
        }
    }
    if (threadIdx.x == 0) loss[0] = acc;
}

// level gradient of (A^2 + B^2) at scale k, plus the (already scaled) gradient of the coarser scales spread over the 2x2 cell
__device__ __forceinline__ float level_grad(const float* q, int s, int y, int x, float ca, float cb) {
    return ca * (q[(int64_t)y * s + (x + s - 1) % s] + q[(int64_t)y * s + (x + 1) % s]) +
           cb * (q[(int64_t)((y + s - 1) % s) * s + x] + q[(int64_t)((y + 1) % s) * s + x]);
}

__global__ __launch_bounds__(kThreads) void noise_reg_bwd_kernel(const float* __restrict__ gloss,
                                                                  const float* __restrict__ stats, const float* __restrict__ pyr,
                                                                  float* __restrict__ tpyr, NoiseList L) {
    const int i = blockIdx.x;
    const int s0 = L.size[i];
    int K = 1;
    for (int s = s0; s > 8; s /= 2) ++K;
    const float gl = gloss[0];
    // coarsest scale first: T_k = G_k + up(T_{k+1}) / 4, T_k (k >= 1) in tpyr (same layout as the pyramid), T_0 * gl -> the gradient
    for (int k = K - 1; k >= 0; --k) {
        const int s = s0 >> k;
        const int64_t plane = (int64_t)s * s, M = plane * L.B;
        int64_t off = L.pyr[i];
        for (int j = 1; j < k; ++j) off += (int64_t)(s0 >> j) * (s0 >> j) * L.B;
        const float* q = k == 0 ? L.p[i] : pyr + off;
        float* out = k == 0 ? L.g[i] : tpyr + off;
        const float* coarse = k + 1 < K ? tpyr + off + (k == 0 ? 0 : M) : nullptr;
        const float A = stats[L.stat[i] + 2 * k], Bm = stats[L.stat[i] + 2 * k + 1];
        const float ca = 2.f * A / (float)M, cb = 2.f * Bm / (float)M;
        const int h = s / 2;
        for (int64_t e = threadIdx.x; e < M; e += kThreads) {
            const int64_t b = e / plane;
            const int r = (int)(e - b * plane), y = r / s, x = r % s;
            float g = level_grad(q + b * plane, s, y, x, ca, cb);
            if (coarse) g += coarse[b * h * h + (int64_t)(y / 2) * h + x / 2] * 0.25f;
            out[e] = k == 0 ? g * gl : g;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void noise_normalize_kernel(NoiseList L) {
    __shared__ float part[kThreads / 64];
    const int i = blockIdx.x;
    float* p = L.p[i];
    const int64_t M = (int64_t)L.size[i] * L.size[i] * L.B;
    float s = 0.f;
    for (int64_t e = threadIdx.x; e < M; e += kThreads) s += p[e];
    const float mean = block_sum(s, part) / (float)M;
    float v = 0.f;
    for (int64_t e = threadIdx.x; e < M; e += kThreads) { const float d = p[e] - mean; v = fmaf(d, d, v); }
    const float sd = sqrtf(block_sum(v, part) / (float)(M - 1));
    for (int64_t e = threadIdx.x; e < M; e += kThreads) p[e] = (p[e] - mean) / sd;
}

int fill_list(NoiseList& L, const char* what, float* const* maps, const int* sizes, int n, int B) {
    TE_REQUIRE(maps && sizes, TE_ERR_NULL, "%s: NULL pointer", what);
    TE_REQUIRE(n >= 1 && n <= kMaxMaps && B >= 1, TE_ERR_SHAPE, "%s: 1 <= maps <= %d, batch >= 1", what, kMaxMaps);
    L = NoiseList{};
    L.n = n;
    L.B = B;
    int64_t pyr = 0;
    int stat = 0;
    for (int i = 0; i < n; ++i) {
        TE_REQUIRE(maps[i], TE_ERR_NULL, "%s: map %d is NULL", what, i);
        int s = sizes[i];
        TE_REQUIRE(s >= 2 && (s <= 8 || (s & (s - 1)) == 0), TE_ERR_SHAPE, "%s: map %d has size %d (a power of two, or <= 8)", what, i, s);
        L.p[i] = maps[i];
        L.size[i] = s;
        L.pyr[i] = pyr;
        L.stat[i] = stat;
        stat += 2;
        while (s > 8) { s /= 2; pyr += (int64_t)s * s * B; stat += 2; }
    }
    L.nstat = stat;
    return 0;
}

}  // namespace

extern "C" int64_t te_noise_reg_ws_floats(const int* sizes, int n, int B) {
    if (!sizes || n < 1 || n > kMaxMaps || B < 1) return TE_ERR_SHAPE;
    int64_t pyr = 0, stat = 0;
    for (int i = 0; i < n; ++i) {
        int s = sizes[i];
        stat += 2;
        while (s > 8) { s /= 2; pyr += (int64_t)s * s * B; stat += 2; }
    }
    return stat + pyr;
}

extern "C" int te_noise_reg_fwd_f32(float* loss, float* ws, float* const* maps, const int* sizes, int n, int B, te_stream_t stream) {
    NoiseList L;
    if (int rc = fill_list(L, "te_noise_reg_fwd_f32", maps, sizes, n, B)) return rc;
    TE_REQUIRE(loss && ws, TE_ERR_NULL, "te_noise_reg_fwd_f32: NULL loss / workspace");
    // workspace: the (A, B) statistics of every scale, then the downsampled levels
    noise_reg_fwd_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(loss, ws, ws + L.nstat, L);
    return te::launch_status("te_noise_reg_fwd_f32");
}

extern "C" int te_noise_reg_bwd_f32(float* const* grads, float* tws, const float* gloss, const float* ws, float* const* maps,
                                    const int* sizes, int n, int B, te_stream_t stream) {
    NoiseList L;
    if (int rc = fill_list(L, "te_noise_reg_bwd_f32", maps, sizes, n, B)) return rc;
    TE_REQUIRE(grads && tws && gloss && ws, TE_ERR_NULL, "te_noise_reg_bwd_f32: NULL pointer");
    for (int i = 0; i < n; ++i) {
        TE_REQUIRE(grads[i], TE_ERR_NULL, "te_noise_reg_bwd_f32: gradient %d is NULL", i);
        L.g[i] = grads[i];
    }
    noise_reg_bwd_kernel<<<n, kThreads, 0, (hipStream_t)stream>>>(gloss, ws, ws + L.nstat, tws, L);
    return te::launch_status("te_noise_reg_bwd_f32");
}

extern "C" int te_noise_normalize_f32(float* const* maps, const int* sizes, int n, int B, te_stream_t stream) {
    NoiseList L;
    if (int rc = fill_list(L, "te_noise_normalize_f32", maps, sizes, n, B)) return rc;
    noise_normalize_kernel<<<n, kThreads, 0, (hipStream_t)stream>>>(L);
    return te::launch_status("te_noise_normalize_f32");
}
