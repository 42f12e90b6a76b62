// The editing scripts' image preprocessing, shared by the scorers' stems (csrc/dex.hip, csrc/celeba_attr.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace te {

// clamp(-1, 1).add(1).div(2).mul(255).round() of torch, step by step in fp32 (division by 2 and multiplication by 0.5 are the same
// exact operation; round is to nearest, ties to even).  The comparisons leave a NaN as it is, as torch's clamp does.
__device__ __forceinline__ float to_byte_level(float x) {
#pragma clang fp contract(off)
    const float c = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
    return rintf(__fmul_rn(__fmul_rn(__fadd_rn(c, 1.f), 0.5f), 255.f));
}

}  // namespace te
