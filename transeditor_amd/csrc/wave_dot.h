// One wave's reductions and its row dot product, shared by the score heads (csrc/dex.hip, csrc/celeba_attr.hip) and the IR-SE50
// identity network (csrc/irse.hip, csrc/irse_bwd.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace te {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// all 64 lanes end with the same value: a butterfly whose shape does not depend on the data
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// sum_k f(a[k]) * w[k] over k < K (a multiple of 4; a and w 16-byte aligned), in every lane: lane l takes k = 4 l, 4 l + 256, ... as
// 16-byte loads into four fma chains (one per vector component), summed (x + y) + (z + w); the lanes' sums meet in the butterfly.
// UNROLL is the caller's: the heads were tuned with different factors.
template <int UNROLL, class F>
__device__ __forceinline__ float wave_dot(const float* __restrict__ a, const float* __restrict__ w, int K, int lane, F f) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll UNROLL
    for (int k = 4 * lane; k < K; k += 256) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(a + k);
        const f32x4 y = *reinterpret_cast<const f32x4*>(w + k);
        acc.x = fmaf(f(x.x), y.x, acc.x);
        acc.y = fmaf(f(x.y), y.y, acc.y);
        acc.z = fmaf(f(x.z), y.z, acc.z);
        acc.w = fmaf(f(x.w), y.w, acc.w);
    }
    return wave_sum((acc.x + acc.y) + (acc.z + acc.w));
}

}  // namespace te
