// The AlexNet LPIPS as a LOSS (pSp/criteria/lpips/lpips.py:29-35 LPIPS('alex').forward, the lpips_lambda term of
// pSp/training/coach_new.py:285-320 calc_loss): the two adjoints of its backward pass that no other entry point covers.  The heads are
// te_lpips_head_bwd_f32 (lpips.hip: the eps-beside-the-root form, which is this LPIPS's), the data gradients of conv2 ... conv5
// te_conv2d_dgrad_f32; here:
//
//     te_pool3s2_max_bwd_f32  : MaxPool2d(3, 2) backwards as a gather.  The windows overlap, so an input pixel lies in up to 2 x 2 of
//                               them; it recomputes each one's argmax under torch's rule and sums the gradients of those it wins
//     te_alex_stem_dgrad_f32  : the data gradient of Conv2d(3, Co, 11, stride 4, padding 2) through (x - mu) / sigma.  Per axis and
//                               output parity r < 4 only the taps k0 + 4 j reach a pixel: 16 dense phases of 3 x 3 down to 2 x 2 taps,
//                               never a walk over the zero-inserted plane
//
// NCHW fp32, no atomics, no workspace; every output element is one fma chain in a fixed order that sees its own image alone: results
// are bit-reproducible and an image's gradient does not depend on its batch.
#include "te_common.h"

namespace {

// --------------------------------------------------------------------------------------------------------- the pool backwards
// One thread per INPUT pixel (y, x) of a plane.  The windows that hold it are oy in [ceil((y - 2) / 2), y / 2] and ox likewise, cut to
// the output plane: none for the last row / column where (H - 3) % 2 == 1, one for an odd coordinate, two for an even one inside.
// The argmax scan is torch's max_pool2d: ky then kx ascending, the first element is the start, a later one replaces it if it is
// greater or a NaN.
__global__ __launch_bounds__(256) void pool3s2_bwd_kernel(float* __restrict__ gx, const float* __restrict__ g, const float* __restrict__ x,
                                                          int64_t total, int H, int W, int Ho, int Wo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t HW = (int64_t)H * W;
    const int64_t plane = i / HW;
    const int r = (int)(i - plane * HW);
    const int y = r / W, xx = r - y * W;
    const float* xp = x + plane * HW;
    const float* gp = g + plane * Ho * Wo;
    const int oy0 = max(0, (y - 1) >> 1), oy1 = min(Ho - 1, y >> 1);        // (y - 1) >> 1 == ceil((y - 2) / 2) for y >= 1
    const int ox0 = max(0, (xx - 1) >> 1), ox1 = min(Wo - 1, xx >> 1);
    float s = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const float* win = xp + (int64_t)(2 * oy) * W + 2 * ox;
            float m = -INFINITY;
            int idx = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = win[ky * W + kx];
                    if (v > m || v != v) { m = v; idx = ky * 3 + kx; }
                }
            if (idx == (y - 2 * oy) * 3 + (xx - 2 * ox)) s += gp[oy * Wo + ox];
        }
    gx[i] = s;
}

// ------------------------------------------------------------------------------------------------------ the stem's data gradient
// Output row y = 4 yy + ry is reached by the kernel rows ky = k0 + 4 jy, k0 = (ry + 2) % 4, jy < ny = (3, 2, 3, 3)[ry], from the
// gradient rows oy = yy + dy - jy, dy = (ry + 2) / 4; columns likewise.  A workgroup of four waves takes a tile of 8 x 8 positions
// (yy, xx) = 32 x 32 pixels of one image: wave ry owns the row phase ry, and a lane owns one position and all four column phases of
// it, 3 channels x 4 pixels = 12 accumulators.  The four column phases together read the gradient columns xx - 2 ... xx + 1, so per
// gradient channel a lane loads ny x 4 values from LDS and spends ny x 11 x 3 fmas on them (8 per load); a lane per single phase would
// get 3.  The weight index (ry, co, jy, kx, c) is wave-uniform: the weights come through the scalar cache as fma operands and use no
// LDS bandwidth.  The gradient tile with its halo (rows yy - 2 ... yy + 1: 11 x 11 values per channel) is staged kStemCC channels at a
// time; positions outside the gradient plane and channels past Co are zeros, so every lane runs the same chain.
// An output element is the chain co ascending, then ky, then kx ascending, from 0; then one division by sigma.
constexpr int kStemT = 8;                    // positions per tile side
constexpr int kStemHalo = kStemT + 3;        // 11
constexpr int kStemPlane = kStemHalo * kStemHalo;
constexpr int kStemCC = 32;                  // gradient channels per LDS stage: 32 * 121 floats = 15.1 KiB

// floats of wt in front of row phase ry's block [Co, ny, 11, 3], ny = (3, 2, 3, 3)[ry]
__device__ __forceinline__ int64_t stem_wt_offset(int ry, int Co) { return (int64_t)Co * 33 * (ry == 0 ? 0 : ry == 1 ? 3 : ry == 2 ? 5 : 8); }

// one stage of a row phase with NY kernel rows.  tile: this lane's LDS element of gradient row yy + dy, column xx - 2 (the caller's
// jy = 0, d = 0); wp: the row phase's weights at the stage's first channel
template <int NY>
__device__ __forceinline__ void stem_phase_rows(float (&acc)[3][4], const float* __restrict__ tile, const float* __restrict__ wp, int nco) {
    for (int co = 0; co < nco; ++co) {
        float gv[NY][4];
#pragma unroll
        for (int jy = 0; jy < NY; ++jy)
#pragma unroll
            for (int d = 0; d < 4; ++d) gv[jy][d] = tile[co * kStemPlane - jy * kStemHalo + d];
        const float* w = wp + (int64_t)co * (NY * 33);
#pragma unroll
        for (int jy = 0; jy < NY; ++jy)
#pragma unroll
            for (int kx = 0; kx < 11; ++kx) {
                constexpr int kTwo = 2;
                const int rx = (kx + kTwo) & 3;                 // the column phase this tap reaches
                const int d = (rx + kTwo - kx) / 4 + kTwo;      // its gradient column, as an index into xx - 2 ... xx + 1  (the dividend is a multiple of 4)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c][rx] = fmaf(w[(jy * 11 + kx) * 3 + c], gv[jy][d], acc[c][rx]);
            }
    }
}

__global__ __launch_bounds__(256) void alex_stem_dgrad_kernel(float* __restrict__ gimg, const float* __restrict__ g, const float* __restrict__ wt,
                                                              int H, int W, int Co, int Ho, int Wo, int tiles_x, int vec4) {
    __shared__ float lds[kStemCC * kStemPlane];
    const int n = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy_base = ty * kStemT - 2, ox_base = tx * kStemT - 2;          // the gradient position of the tile's LDS element (0, 0)
    const int ry = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // wave-uniform: the weights are scalar operands
    const int lane = threadIdx.x & 63;
    const int ly = lane >> 3, lx = lane & 7;
    const int dy = ry >> 1;                                                   // (ry + 2) / 4
    const float* gn = g + (int64_t)n * Co * Ho * Wo;
    const float* wry = wt + stem_wt_offset(ry, Co);
    const float* tile = lds + (ly + 2 + dy) * kStemHalo + lx;               // jy = 0, d = 0: row oy = yy + dy, column xx - 2
    float acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[c][k] = 0.f;
    for (int c0 = 0; c0 < Co; c0 += kStemCC) {
        const int nco = min(kStemCC, Co - c0);
        if (c0) __syncthreads();                                             // the previous stage has been read
        for (int e = threadIdx.x; e < nco * kStemPlane; e += 256) {
            const int cc = e / kStemPlane, p = e - cc * kStemPlane;
            const int r = p / kStemHalo, col = p - r * kStemHalo;
            const int oy = oy_base + r, ox = ox_base + col;
            lds[e] = (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) ? gn[((int64_t)(c0 + cc) * Ho + oy) * Wo + ox] : 0.f;
        }
        __syncthreads();
        if (ry == 1) stem_phase_rows<2>(acc, tile, wry + (int64_t)c0 * (2 * 33), nco);
        else stem_phase_rows<3>(acc, tile, wry + (int64_t)c0 * (3 * 33), nco);
    }
    const int y = 4 * (ty * kStemT + ly) + ry, x0 = 4 * (tx * kStemT + lx);
    if (y >= H || x0 >= W) return;
    float* o = gimg + (int64_t)n * 3 * H * W + (int64_t)y * W + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sigma = c == 0 ? 0.458f : c == 1 ? 0.448f : 0.450f;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fdiv_rn(acc[c][k], sigma);
        float* oc = o + (int64_t)c * H * W;
        if (vec4) {                                                          // W % 4 == 0 and gimg 16-byte aligned: x0 + 3 < W
            *reinterpret_cast<float4*>(oc) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < W) oc[k] = v[k];
        }
    }
}

}  // namespace

extern "C" int te_pool3s2_max_bwd_f32(float* gx, const float* g, const float* x, int64_t planes, int H, int W, te_stream_t stream) {
    TE_REQUIRE(gx && g && x, TE_ERR_NULL, "te_pool3s2_max_bwd_f32: NULL pointer");
    TE_REQUIRE(planes >= 1 && H >= 1 && W >= 1, TE_ERR_SHAPE, "te_pool3s2_max_bwd_f32: planes, H, W must be positive (got %lld, %d, %d)",
               (long long)planes, H, W);
    TE_REQUIRE(H >= 3 && W >= 3, TE_ERR_SHAPE, "te_pool3s2_max_bwd_f32: an unpadded 3 x 3 window does not fit a %d x %d plane", H, W);
    TE_REQUIRE((int64_t)H * W <= 0x7fffffff && planes <= ((int64_t)0x7fffffff * 256) / ((int64_t)H * W), TE_ERR_SHAPE,
               "te_pool3s2_max_bwd_f32: too many pixels (%lld planes of %d x %d)", (long long)planes, H, W);
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const int64_t total = planes * H * W;
    pool3s2_bwd_kernel<<<(unsigned)te::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(gx, g, x, total, H, W, Ho, Wo);
    return te::launch_status("te_pool3s2_max_bwd_f32");
}

extern "C" int te_alex_stem_dgrad_f32(float* gimg, const float* g, const float* wt, int N, int H, int W, int Co, te_stream_t stream) {
    TE_REQUIRE(gimg && g && wt, TE_ERR_NULL, "te_alex_stem_dgrad_f32: NULL pointer");
    TE_REQUIRE(N >= 1 && N < 65536 && H >= 1 && W >= 1 && Co >= 1, TE_ERR_SHAPE,
               "te_alex_stem_dgrad_f32: 1 <= N < 65536 and positive H, W, Co (got %d, %d, %d, %d)", N, H, W, Co);
    TE_REQUIRE(H + 4 >= 11 && W + 4 >= 11, TE_ERR_SHAPE, "te_alex_stem_dgrad_f32: an 11 x 11 kernel with padding 2 does not fit a %d x %d image", H,
               W);
    TE_REQUIRE((int64_t)3 * H * W <= 0x7fffffff, TE_ERR_SHAPE, "te_alex_stem_dgrad_f32: one image (3 * H * W) must fit 31 bits");
    const int Ho = (H - 7) / 4 + 1, Wo = (W - 7) / 4 + 1;
    TE_REQUIRE((int64_t)Co * Ho * Wo <= 0x7fffffff && (int64_t)Co * 363 <= 0x7fffffff, TE_ERR_SHAPE,
               "te_alex_stem_dgrad_f32: one image's gradient (Co * Ho * Wo) and the weight must fit 31 bits (Co = %d)", Co);
    const int tiles_y = (int)te::cdiv(te::cdiv(H, 4), kStemT), tiles_x = (int)te::cdiv(te::cdiv(W, 4), kStemT);   // (tiles_y * tiles_x < 2^21: H * W < 2^31)
    const int vec4 = (W % 4 == 0 && te::aligned16(gimg)) ? 1 : 0;
    alex_stem_dgrad_kernel<<<dim3((unsigned)(tiles_y * tiles_x), N), 256, 0, (hipStream_t)stream>>>(gimg, g, wt, H, W, Co, Ho, Wo, tiles_x, vec4);
    return te::launch_status("te_alex_stem_dgrad_f32");
}
