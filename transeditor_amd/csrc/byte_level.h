// The editing scripts' image preprocessing, shared by the scorers' stems (csrc/dex.hip, csrc/celeba_attr.hip, csrc/resnet.hip).
#pragma once
#include "te_common.h"

namespace te {

// the checks of a stem that reads the centre crop x crop window of N images [3,H,W] into Co channels; `who` names the entry point
inline int check_centre_crop(const char* who, int N, int H, int W, int crop, int Co) {
    TE_REQUIRE(N > 0 && H > 0 && W > 0 && N < 65536 && Co >= 1, TE_ERR_SHAPE, "%s: 1 <= N < 65536 and positive H, W, Co (got %d, %d, %d, %d)", who,
               N, H, W, Co);
    TE_REQUIRE(crop >= 1 && crop <= H && crop <= W && crop <= 32768, TE_ERR_SHAPE, "%s: the crop (%d) must be positive and fit the %d x %d image",
               who, crop, H, W);
    TE_REQUIRE((H - crop) % 2 == 0 && (W - crop) % 2 == 0, TE_ERR_SHAPE, "%s: a centre crop of %d needs H - crop and W - crop even (got %d x %d)",
               who, crop, H, W);
    return 0;
}

// clamp(-1, 1).add(1).div(2).mul(255).round() of torch, step by step in fp32 (division by 2 and multiplication by 0.5 are the same
// exact operation; round is to nearest, ties to even).  The comparisons leave a NaN as it is, as torch's clamp does.
__device__ __forceinline__ float to_byte_level(float x) {
#pragma clang fp contract(off)
    const float c = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
    return rintf(__fmul_rn(__fmul_rn(__fadd_rn(c, 1.f), 0.5f), 255.f));
}

}  // namespace te
