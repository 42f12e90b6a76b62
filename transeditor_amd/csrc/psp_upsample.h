// What te_upsample_add_f32 (psp_heads.hip) and its adjoint te_upsample_add_bwd_f32 (psp_heads_bwd.hip) must agree on, written once: the two
// taps of an output position and their weights.  The adjoint sums with the very weights the forward formed.
#pragma once
#include "te_common.h"

namespace te {
namespace psp {

// align_corners=True: src = o * (in - 1) / (out - 1) (0 where out == 1), in integers: the quotient is the first tap, the remainder
// over out - 1 the second tap's weight, rounded once; l0 = 1 - l1
__device__ __forceinline__ void corner_tap(int o, int in_size, int out_size, int& i0, int& i1, float& l0, float& l1) {
    if (out_size == 1) { i0 = i1 = 0; l0 = 1.f; l1 = 0.f; return; }
    const int64_t num = (int64_t)o * (in_size - 1), den = out_size - 1;
    i0 = (int)(num / den);
    const int64_t rem = num - (int64_t)i0 * den;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = (float)rem / (float)den;
    l0 = 1.f - l1;
}

}  // namespace psp
}  // namespace te
