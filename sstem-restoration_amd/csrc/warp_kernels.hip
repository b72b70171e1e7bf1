// Bilinear back-warp of an image by a dense flow field (one gather kernel, HBM-bound).
//
// Replaces the ~20 torch ops of the reference's SpatialTransformation
// (sff_scripts_fusion/utils/image_warp_torch.py:5-112: NHWC permute, 1-px zero pad, meshgrid, floor,
// clamp, four gathers on a flattened copy, weighted sum) used between the frozen flow network and the
// fusion UNet (sff_scripts_fusion/main_fusion.py:229-235).  Semantics kept exactly:
//   x = dx + col + 1, y = dy + row + 1                      (:104-105, :44-45; +1 = the zero border)
//   x0 = floor(x), x1 = x0 + 1, both clamped to [0, W+1]; same for y         (:50-58)
//   weights from the CLAMPED x1, y1:  wx = x1 - x, wy = y1 - y                (:87-93)
//   out = wx*wy*I(y0,x0) + wx*(1-wy)*I(y1,x0) + (1-wx)*wy*I(y0,x1) + (1-wx)*(1-wy)*I(y1,x1)   (:95-98)
//   I(.) reads the zero-padded image: indices 0 and W+1 / H+1 are the border.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "warp_kernels.h"

namespace sstem {

__global__ __launch_bounds__(256) void warp_bilinear(
    const float* __restrict__ img, const float* __restrict__ flow, float* __restrict__ out,
    int B, int C, int H, int W)
{
    const int64_t plane = (int64_t)H * W;
    const int64_t n = (int64_t)B * plane;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = p / plane;
        const int64_t yx = p - b * plane;
        const int row = (int)(yx / W), col = (int)(yx - (int64_t)row * W);
        const float x = (flow[(b * 2 + 0) * plane + yx] + (float)col) + 1.0f;
        const float y = (flow[(b * 2 + 1) * plane + yx] + (float)row) + 1.0f;
        // floor -> int64 like torch's .long(); clamp to the padded image
        const float fx0 = floorf(x), fy0 = floorf(y);
        const float lim = 4.0e18f;   // keep the float->int64 conversion defined for absurd flows
        int64_t x0 = (int64_t)fminf(fmaxf(fx0, -lim), lim), y0 = (int64_t)fminf(fmaxf(fy0, -lim), lim);
        int64_t x1 = x0 + 1, y1 = y0 + 1;
        const int64_t max_x = W + 1, max_y = H + 1;
        x0 = x0 < 0 ? 0 : (x0 > max_x ? max_x : x0);
        x1 = x1 < 0 ? 0 : (x1 > max_x ? max_x : x1);
        y0 = y0 < 0 ? 0 : (y0 > max_y ? max_y : y0);
        y1 = y1 < 0 ? 0 : (y1 > max_y ? max_y : y1);
        const float wx = (float)x1 - x, wy = (float)y1 - y;
        const float wa = wx * wy, wb = wx * (1.0f - wy), wc = (1.0f - wx) * wy, wd = (1.0f - wx) * (1.0f - wy);
        const bool x0in = x0 >= 1 && x0 <= W, x1in = x1 >= 1 && x1 <= W;
        const bool y0in = y0 >= 1 && y0 <= H, y1in = y1 >= 1 && y1 <= H;
        const int64_t oa = (y0 - 1) * W + (x0 - 1), ob = (y1 - 1) * W + (x0 - 1);
        const int64_t oc = (y0 - 1) * W + (x1 - 1), od = (y1 - 1) * W + (x1 - 1);
        for (int c = 0; c < C; ++c) {
            const float* ip = img + (b * C + c) * plane;
            const float ia = (y0in && x0in) ? ip[oa] : 0.f;
            const float ib = (y1in && x0in) ? ip[ob] : 0.f;
            const float ic = (y0in && x1in) ? ip[oc] : 0.f;
            const float id = (y1in && x1in) ? ip[od] : 0.f;
            // separate products, then summed in stack order (torch.sum over the 4 stacked terms)
            const float s = ((__fmul_rn(wa, ia) + __fmul_rn(wb, ib)) + __fmul_rn(wc, ic)) + __fmul_rn(wd, id);
            out[(b * C + c) * plane + yx] = s;
        }
    }
}

hipError_t launch_warp_bilinear(const float* img, const float* flow, float* out, int B, int C, int H, int W,
                                hipStream_t s)
{
    int64_t n = (int64_t)B * H * W;
    int64_t g = (n + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(warp_bilinear, dim3((unsigned)g), dim3(256), 0, s, img, flow, out, B, C, H, W);
    return hipGetLastError();
}

// ---- gradients of the back-warp (include/sstem_warp.h: sstem_warp_bilinear_backward_f32) ------------------------------------------
// What autograd derives from the reference's :32-95 with x0, x1, y0, y1 constants and d wx / dx = d wy / dy = -1 (floor and clamp have
// zero derivative), g = dL/dout:
//   dL/dflow[b,0] = sum_ch g * ( wy*(Ic - Ia) + (1-wy)*(Id - Ib) )        dL/dflow[b,1] = sum_ch g * ( wx*(Ib - Ia) + (1-wx)*(Id - Ic) )
//   dL/dimage    += wx*wy*g at (y0,x0), wx*(1-wy)*g at (y1,x0), (1-wx)*wy*g at (y0,x1), (1-wx)*(1-wy)*g at (y1,x1); border taps dropped
// Whenever a clamp changes an index both taps of that axis are border taps, so a weight outside [0,1] only ever meets zeros.

// The taps of one output pixel: warp_bilinear's own expressions (coordinates, floor, the 4e18 guard, clamp, weights from the CLAMPED
// x1 / y1, in-plane predicates, offsets into the unpadded plane).  An offset is meaningful only under its two predicates.
struct WarpTaps {
    float wx, wy;
    bool x0in, x1in, y0in, y1in;
    int64_t oa, ob, oc, od;
};

__device__ __forceinline__ WarpTaps warp_taps(const float* __restrict__ flow, int64_t b, int64_t plane, int64_t yx, int H, int W)
{
    WarpTaps t;
    const int row = (int)(yx / W), col = (int)(yx - (int64_t)row * W);
    const float x = (flow[(b * 2 + 0) * plane + yx] + (float)col) + 1.0f;
    const float y = (flow[(b * 2 + 1) * plane + yx] + (float)row) + 1.0f;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float lim = 4.0e18f;   // keep the float->int64 conversion defined for absurd flows
    int64_t x0 = (int64_t)fminf(fmaxf(fx0, -lim), lim), y0 = (int64_t)fminf(fmaxf(fy0, -lim), lim);
    int64_t x1 = x0 + 1, y1 = y0 + 1;
    const int64_t max_x = W + 1, max_y = H + 1;
    x0 = x0 < 0 ? 0 : (x0 > max_x ? max_x : x0);
    x1 = x1 < 0 ? 0 : (x1 > max_x ? max_x : x1);
    y0 = y0 < 0 ? 0 : (y0 > max_y ? max_y : y0);
    y1 = y1 < 0 ? 0 : (y1 > max_y ? max_y : y1);
    t.wx = (float)x1 - x; t.wy = (float)y1 - y;
    t.x0in = x0 >= 1 && x0 <= W; t.x1in = x1 >= 1 && x1 <= W;
    t.y0in = y0 >= 1 && y0 <= H; t.y1in = y1 >= 1 && y1 <= H;
    t.oa = (y0 - 1) * W + (x0 - 1); t.ob = (y1 - 1) * W + (x0 - 1);
    t.oc = (y0 - 1) * W + (x1 - 1); t.od = (y1 - 1) * W + (x1 - 1);
    return t;
}

// Flow gradient: one lane per pixel, channels summed in ascending order, both planes stored (zeros included); no atomics, no workspace:
// the bits repeat from run to run.  Roundings per element, separate multiplies and adds (a contraction to fma only removes some):
//   per channel  sub (Ic - Ia | Id - Ib), mul by the weight, add of the two products, mul by g   = 4 on the path of any one tap,
//   then C - 1 adds of the channel sum                                                            -> n = C + 4 bounds it (tests)
// 1 - wx and 1 - wy are exact for in-plane samples; out of the plane every tap is a zero and the result is a zero.
__global__ __launch_bounds__(256) void warp_bilinear_grad_flow(
    const float* __restrict__ img, const float* __restrict__ flow, const float* __restrict__ gout, float* __restrict__ gflow,
    int B, int C, int H, int W)
{
    const int64_t plane = (int64_t)H * W;
    const int64_t n = (int64_t)B * plane;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = p / plane;
        const int64_t yx = p - b * plane;
        const WarpTaps t = warp_taps(flow, b, plane, yx, H, W);
        const float ux = 1.0f - t.wx, uy = 1.0f - t.wy;
        const bool ina = t.y0in && t.x0in, inb = t.y1in && t.x0in, inc = t.y0in && t.x1in, ind = t.y1in && t.x1in;
        float gx = 0.f, gy = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* ip = img + (b * C + c) * plane;
            const float ia = ina ? ip[t.oa] : 0.f;
            const float ib = inb ? ip[t.ob] : 0.f;
            const float ic = inc ? ip[t.oc] : 0.f;
            const float id = ind ? ip[t.od] : 0.f;
            const float g = gout[(b * C + c) * plane + yx];
            gx += g * (t.wy * (ic - ia) + uy * (id - ib));
            gy += g * (t.wx * (ib - ia) + ux * (id - ic));
        }
        gflow[(b * 2 + 0) * plane + yx] = gx;
        gflow[(b * 2 + 1) * plane + yx] = gy;
    }
}

// Image gradient: one lane per pixel adds its in-plane taps with fp32 atomicAdd (one global_atomic_add_f32 each, no compare-and-swap
// loop).  Each term takes two roundings (the weight product, times g); the order of the adds is not fixed.
__global__ __launch_bounds__(256) void warp_bilinear_grad_image(
    const float* __restrict__ flow, const float* __restrict__ gout, float* __restrict__ gimg, int B, int C, int H, int W)
{
    const int64_t plane = (int64_t)H * W;
    const int64_t n = (int64_t)B * plane;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = p / plane;
        const int64_t yx = p - b * plane;
        const WarpTaps t = warp_taps(flow, b, plane, yx, H, W);
        const bool ina = t.y0in && t.x0in, inb = t.y1in && t.x0in, inc = t.y0in && t.x1in, ind = t.y1in && t.x1in;
        if (!(ina || inb || inc || ind)) continue;
        const float wa = t.wx * t.wy, wb = t.wx * (1.0f - t.wy), wc = (1.0f - t.wx) * t.wy, wd = (1.0f - t.wx) * (1.0f - t.wy);
        for (int c = 0; c < C; ++c) {
            float* gp = gimg + (b * C + c) * plane;
            const float g = gout[(b * C + c) * plane + yx];
            if (ina) atomicAdd(gp + t.oa, __fmul_rn(wa, g));
            if (inb) atomicAdd(gp + t.ob, __fmul_rn(wb, g));
            if (inc) atomicAdd(gp + t.oc, __fmul_rn(wc, g));
            if (ind) atomicAdd(gp + t.od, __fmul_rn(wd, g));
        }
    }
}

static unsigned warp_grid(int B, int H, int W)
{
    int64_t n = (int64_t)B * H * W;
    int64_t g = (n + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;       // the forward's cap
    if (g < 1) g = 1;
    return (unsigned)g;
}

hipError_t launch_warp_bilinear_backward(const float* img, const float* flow, const float* gout, float* gflow, float* gimg,
                                         int accumulate_image, int B, int C, int H, int W, hipStream_t s)
{
    const dim3 grid(warp_grid(B, H, W));
    if (gflow) {
        hipLaunchKernelGGL(warp_bilinear_grad_flow, grid, dim3(256), 0, s, img, flow, gout, gflow, B, C, H, W);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (gimg) {
        if (!accumulate_image) {
            hipError_t e = hipMemsetAsync(gimg, 0, sizeof(float) * (size_t)B * C * H * W, s);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(warp_bilinear_grad_image, grid, dim3(256), 0, s, flow, gout, gimg, B, C, H, W);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace sstem
