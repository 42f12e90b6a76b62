// What the forward pass (irse.hip) and the backward pass (irse_bwd.hip) of the IR-SE50 identity network must agree on, written once:
// the identity stem's window checks and the first step of squeeze-and-excitation, which the backward pass recomputes bit for bit.
#pragma once
#include "te_common.h"
#include "wave_dot.h"

namespace te {
namespace irse {

// the checks of the identity stem, forwards and backwards: the window [y0, y1) x [x0, x1) of N images [3,H,W], pooled to Pn x Pn
inline int check_id_window(const char* who, int N, int H, int W, int y0, int y1, int x0, int x1, int Pn, int Co) {
    TE_REQUIRE(N >= 1 && N < 65536 && H >= 1 && W >= 1 && Co >= 1, TE_ERR_SHAPE, "%s: 1 <= N < 65536 and positive H, W, Co (got %d, %d, %d, %d)", who,
               N, H, W, Co);
    TE_REQUIRE(y0 >= 0 && y0 < y1 && y1 <= H && x0 >= 0 && x0 < x1 && x1 <= W, TE_ERR_SHAPE,
               "%s: the window [%d, %d) x [%d, %d) must be non-empty and inside the %d x %d image", who, y0, y1, x0, x1, H, W);
    TE_REQUIRE(Pn >= 1 && Pn <= 32768 && y1 - y0 <= 32768 && x1 - x0 <= 32768, TE_ERR_SHAPE,
               "%s: 1 <= Pn <= 32768 and a window of at most 32768 x 32768 (got Pn = %d, %d x %d)", who, Pn, y1 - y0, x1 - x0);
    TE_REQUIRE((int64_t)3 * H * W <= 0x7fffffff, TE_ERR_SHAPE, "%s: one image (3 * H * W) must fit 31 bits", who);
    return 0;
}

// squeeze-and-excitation runs one workgroup of four waves per image; its R hidden units live in LDS
constexpr int kSeThreads = 256;
constexpr int kSeMaxR = 1024;

// Step 1 of se_excite_kernel and of se_bwd_kernel: the pre-activation of hidden unit r, in every lane: one wave's dot product of w1[r]
// with the image's C pooled values p (lane l takes k = l, l + 64, ... as one fma chain, the lanes' sums meet in a butterfly).  The
// forward pass stores its ReLU, the backward pass the value itself (it takes the unit's sign from it).  The loop over r and the store
// stay in the two kernels: moved in here, they change both instruction streams.
__device__ __forceinline__ float se_unit(const float* p, const float* w1, int C, int r, int lane) {
    const float* w = w1 + (int64_t)r * C;
    float acc = 0.f;
    for (int k = lane; k < C; k += 64) acc = fmaf(w[k], p[k], acc);
    return wave_sum(acc);
}

}  // namespace irse
}  // namespace te
