// conv1_1 + bias + ReLU of a VGG16 (3 -> 64 channels, 3x3, pad 1), written once for its three callers: te_vgg_stem_fwd_f32 (the raw
// image), te_lpips_stem_fwd_f32 (LPIPS's ScalingLayer in front; csrc/lpips.hip) and te_dex_stem_fwd_f32 (BGR byte levels of a centre
// crop; csrc/dex.hip).  What differs between them is the input rule, a type with
//
//     static __device__ int channel(int c)              the image channel that the convolution's input channel c reads
//     static __device__ float value(float v, int c)     the pixel v of that channel as the convolution sees it
//     static constexpr bool kWindow                     false: the window is the whole image, known when the kernel is compiled
//
// defined next to its caller, in that file's anonymous namespace (so that the instantiation stays local to the file).
#pragma once
#include "te_common.h"

namespace te {

// out[n,o,y,x] = relu(b[o] + sum_{c,ky,kx} w[o,c,ky,kx] * value(x[n, channel(c), y0 + y + ky - 1, x0 + x + kx - 1], c)) for (y, x) in
// the h x wd window at (y0, x0) of the H x W image; a tap outside the WINDOW is zero (the rule and the crop come BEFORE nn.Conv2d's
// zero padding).  One thread per output pixel, w [64,3,3,3] in LDS, the 27 inputs in registers, one fma chain over k = 0..26 per
// output channel.
template <class Rule>
__global__ __launch_bounds__(256) void vgg_stem_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, int H, int W, int h_, int w_, int y0_, int x0_) {
    const int h = Rule::kWindow ? h_ : H, wd = Rule::kWindow ? w_ : W, y0 = Rule::kWindow ? y0_ : 0, x0 = Rule::kWindow ? x0_ : 0;
    __shared__ float ws[64 * 27];
    __shared__ float bs[64];
    for (int i = threadIdx.x; i < 64 * 27; i += 256) ws[i] = w[i];
    if (threadIdx.x < 64) bs[threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.y;
    const int64_t HW = (int64_t)H * W, hw = (int64_t)h * wd;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int yy = (int)(p / wd), xx = (int)(p % wd);
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* xc = x + ((int64_t)n * 3 + Rule::channel(c)) * HW;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = yy + ky - 1, ix = xx + kx - 1;
                const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < wd;
                in[c * 9 + ky * 3 + kx] = ok ? Rule::value(xc[(int64_t)(y0 + iy) * W + (x0 + ix)], c) : 0.f;
            }
        }
    }
    float* o = out + (int64_t)n * 64 * hw + p;
    for (int m = 0; m < 64; ++m) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = fmaf(ws[m * 27 + k], in[k], acc);
        acc += bs[m];
        o[(int64_t)m * hw] = relu_nan(acc);
    }
}

template <class Rule>
inline void launch_vgg_stem(float* out, const float* x, const float* w, const float* b, int N, int H, int W, int h, int wd, int y0,
                            int x0, te_stream_t stream) {
    vgg_stem_kernel<Rule><<<dim3((unsigned)cdiv((int64_t)h * wd, 256), N), 256, 0, (hipStream_t)stream>>>(out, x, w, b, H, W, h, wd, y0, x0);
}

}  // namespace te
