// SFF fold synthesis (include/sstem_fold.h): gen_flow, the numpy image_warp on bytes, and the two fused into one training sample.
//
// Replaces the host arithmetic of the reference's Train.degradation (sff_scripts_fusion/data/data_provider.py:183-248): ~30 float64
// numpy passes over a 400 x 400 plane per candidate fold (utils/flow_synthesis.py:20-87), a bilinear back-warp of the uint8 crop
// (utils/image_warp.py:3-112), the mask product, the centre crop and the /255 replication to six fp32 channels.  A pure per-pixel map
// with a 4-point byte gather: streaming kernels, no MFMA, no LDS (but the 256-byte jitter table of fold_degrade<true>).  256 threads, one pixel per thread, x innermost (every store is
// coalesced), the sample from blockIdx.y so a block's fold row is wave-uniform (scalar loads), a grid-stride walk under a capped grid.
//
// The contract is bit for bit with the reference, so every expression below restates numpy's operation order literally: separate
// multiplies and adds in double (the multiplications by the 0/1 masks and by the sign kept: they make the negative zeros the reference
// stores), four separate fp32 products in the warp.  hipcc's default contraction would fuse k * x - y and ndk * a + dis_b into FMAs;
// the pragma below takes the contract flag off every operation of this translation unit, so no pass may fuse them.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sstem_fold.h"
#include "fold_kernels.h"
#include "wg_reduce.h"

namespace sstem {

namespace {

constexpr int FOLD_GRID_CAP = 4096;      // workgroups per launch: 16 per CU; larger problems walk by the grid's stride

struct FoldPixel {
    float fx, fy;        // flow  (dx, dy)
    float gx, gy;        // flow2 (dx, dy)
    int mask;            // 0 on the fold line, 1 elsewhere
};

// gen_flow at pixel (x = column, y = row); f = the fold's row of doubles (wave-uniform)
__device__ __forceinline__ FoldPixel fold_pixel(const double* __restrict__ f, int x, int y)
{
    const double k = f[0], b = f[1], norm = f[2], lw = f[3], fw = f[4], ndk = f[5], dis_b = f[6], cos_p = f[7], sin_p = f[8];
    const bool k_pos = f[9] != 0.0;
    const double d = (((k * (double)x) - (double)y) + b) / norm;             // flow_synthesis.py:25
    const double sign = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);              // :28-31
    const double a = fabs(d);                                                // :33
    const double m1 = a < lw ? 0.0 : 1.0;                                    // :46-47 mask_dis
    const double m2 = a < fw ? 0.0 : 1.0;                                    // :48-49 mask_dis2
    double s = ndk * a + dis_b;                                              // :56
    if (s < 0.0) s = 0.0;                                                    // :57
    const double s2 = s * m2 + a * (1.0 - m2);                               // :58
    const double s1 = s * m1 + a * (1.0 - m1);                               // :59
    const double dis = s1 * sign;                                            // :61
    const double dis2 = s2 * (-sign);                                        // :62
    const double c1 = dis * cos_p, n1 = dis * sin_p, c2 = dis2 * cos_p, n2 = dis2 * sin_p;
    FoldPixel p;
    if (k_pos) { p.fx = (float)c1; p.fy = (float)(-n1); p.gx = (float)c2; p.gy = (float)(-n2); }       // :75-79
    else       { p.fx = (float)(-c1); p.fy = (float)n1; p.gx = (float)(-c2); p.gy = (float)n2; }       // :80-84
    p.mask = a > lw ? 1 : 0;                                                 // :34-35 (zeros, then 1 where dis_abs > line_width)
    return p;
}

// the four taps and weights of image_warp at pixel (col, row) of an H x W plane
struct WarpTaps {
    int64_t a, b, c, d;          // offsets inside the plane, in pixels: (y0,x0) (y1,x0) (y0,x1) (y1,x1)
    float wa, wb, wc, wd;
};

__device__ __forceinline__ int64_t floor_to_int(float fl)
{
    // np.floor(flow).astype(np.int32); saturated outside the int32 range, 0 for NaN (outside the contract, kept in bounds)
    if (!(fl == fl)) return 0;
    return (int64_t)fminf(fmaxf(fl, -2147483648.0f), 2147483520.0f);
}

__device__ __forceinline__ WarpTaps warp_taps(float fx, float fy, int col, int row, int H, int W)
{
    const float flx = floorf(fx), fly = floorf(fy);                          // image_warp.py:44
    int64_t x0 = (int64_t)col + floor_to_int(flx), y0 = (int64_t)row + floor_to_int(fly);      // :54-55
    x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);                             // :57-58
    y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
    const int64_t x1 = x0 + 1 > W - 1 ? W - 1 : x0 + 1;                      // :84-88, from the clamped x0
    const int64_t y1 = y0 + 1 > H - 1 ? H - 1 : y0 + 1;
    const float xw = fx - flx, yw = fy - fly;                                // :72 the unclamped fraction
    WarpTaps t;
    t.wa = (1.0f - xw) * (1.0f - yw);                                        // :79-82
    t.wb = (1.0f - xw) * yw;
    t.wc = xw * (1.0f - yw);
    t.wd = xw * yw;
    t.a = y0 * W + x0; t.b = y1 * W + x0; t.c = y0 * W + x1; t.d = y1 * W + x1;
    return t;
}

// :101 wa * Ia + wb * Ib + wc * Ic + wd * Id in fp32, left to right, then :110 astype(np.uint8) (truncation; the sum is in [0, 256))
__device__ __forceinline__ uint8_t warp_blend(const WarpTaps& t, float ia, float ib, float ic, float id)
{
    const float v = ((t.wa * ia + t.wb * ib) + t.wc * ic) + t.wd * id;
    return v == v ? (uint8_t)((int)v & 0xFF) : (uint8_t)0;
}

// grid (gx, gy): blockIdx.y walks the samples, blockIdx.x the pixels of one
__global__ __launch_bounds__(256) void fold_flow(const double* __restrict__ folds, int n, int H, int W, float* __restrict__ flow,
                                                 float* __restrict__ flow2, uint8_t* __restrict__ mask)
{
    const int64_t plane = (int64_t)H * W;
    for (int s = blockIdx.y; s < n; s += gridDim.y) {
        const double* f = folds + (int64_t)s * SSTEM_FOLD_PARAMS;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (int64_t)gridDim.x * 256) {
            const int y = (int)((uint32_t)p / (uint32_t)W), x = (int)((uint32_t)p - (uint32_t)y * (uint32_t)W);   // planes stay below 2^30 pixels
            const FoldPixel px = fold_pixel(f, x, y);
            const int64_t o = (int64_t)s * plane + p;
            if (flow) { flow[2 * o] = px.fx; flow[2 * o + 1] = px.fy; }
            if (flow2) { flow2[2 * o] = px.gx; flow2[2 * o + 1] = px.gy; }
            if (mask) mask[o] = (uint8_t)px.mask;
        }
    }
}

__global__ __launch_bounds__(256) void image_warp_u8(const uint8_t* __restrict__ im, const float* __restrict__ flow,
                                                     uint8_t* __restrict__ out, int n, int H, int W, int C, int bilinear)
{
    const int64_t plane = (int64_t)H * W;
    for (int s = blockIdx.y; s < n; s += gridDim.y) {
        const uint8_t* src = im + (int64_t)s * plane * C;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (int64_t)gridDim.x * 256) {
            const int y = (int)((uint32_t)p / (uint32_t)W), x = (int)((uint32_t)p - (uint32_t)y * (uint32_t)W);   // planes stay below 2^30 pixels
            const int64_t o = (int64_t)s * plane + p;
            const WarpTaps t = warp_taps(flow[2 * o], flow[2 * o + 1], x, y, H, W);
            for (int c = 0; c < C; ++c) {
                uint8_t v;
                if (bilinear) v = warp_blend(t, (float)src[t.a * C + c], (float)src[t.b * C + c], (float)src[t.c * C + c], (float)src[t.d * C + c]);
                else v = src[t.a * C + c];
                out[o * C + c] = v;
            }
        }
    }
}

// zero_count[slot of sample i] = 0 for the launched samples, ahead of fold_degrade's adds
__global__ __launch_bounds__(256) void fold_clear_counts(const int32_t* __restrict__ slot, int n, int slots, int32_t* __restrict__ zero_count)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int sl = slot ? slot[i] : i;
        if (sl >= 0 && sl < slots) zero_count[sl] = 0;
    }
}

// The fused sample.  LUT (include/sstem_jitter.h): the four bytes gathered for the warp go through the slot's 256-entry table, staged in
// LDS once per sample; the label still reads the plane itself.  Without LUT it is the kernel it always was (lut is not read).
template <bool LUT>
__global__ __launch_bounds__(256) void fold_degrade(const uint8_t* __restrict__ clean, const uint8_t* __restrict__ interp,
                                                    const double* __restrict__ folds, const int32_t* __restrict__ slot, int n, int slots,
                                                    int SH, int SW, int off_y, int off_x, int out_h, int out_w, int gt_line,
                                                    uint8_t* __restrict__ deformed, float* __restrict__ flow2, float* __restrict__ im,
                                                    float* __restrict__ lb, int32_t* __restrict__ zero_count, const uint8_t* __restrict__ lut)
{
    __shared__ uint8_t table[LUT ? 256 : 1];
    const int64_t plane = (int64_t)SH * SW, win = (int64_t)out_h * out_w;
    for (int s = blockIdx.y; s < n; s += gridDim.y) {
        const int sl = slot ? slot[s] : s;                                   // block-uniform
        if (sl < 0 || sl >= slots) continue;
        const double* f = folds + (int64_t)s * SSTEM_FOLD_PARAMS;
        const uint8_t* src = clean + (int64_t)sl * plane;
        if (LUT) {
            __syncthreads();                                                 // the previous sample's reads of the table are done
            table[threadIdx.x] = lut[(int64_t)sl * 256 + threadIdx.x];
            __syncthreads();
        }
        int zeros = 0;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < win; p += (int64_t)gridDim.x * 256) {
            const int wy = (int)((uint32_t)p / (uint32_t)out_w), wx = (int)((uint32_t)p - (uint32_t)wy * (uint32_t)out_w);
            const int y = off_y + wy, x = off_x + wx;
            const FoldPixel px = fold_pixel(f, x, y);
            const WarpTaps t = warp_taps(px.fx, px.fy, x, y, SH, SW);
            const uint8_t w = LUT ? warp_blend(t, (float)table[src[t.a]], (float)table[src[t.b]], (float)table[src[t.c]], (float)table[src[t.d]])
                                  : warp_blend(t, (float)src[t.a], (float)src[t.b], (float)src[t.c], (float)src[t.d]);
            const uint8_t d = px.mask ? w : (uint8_t)0;                      // data_provider.py:233 (deformed * mask).astype(np.uint8)
            zeros += d == 0 ? 1 : 0;                                         // :239-240
            const int64_t o = (int64_t)sl * win + p;
            if (deformed) deformed[o] = d;
            if (flow2) {                                                     // np.transpose(flow2, (2, 0, 1))
                flow2[2 * (int64_t)sl * win + p] = px.gx;
                flow2[(2 * (int64_t)sl + 1) * win + p] = px.gy;
            }
            const int64_t q = (int64_t)y * SW + x;                           // the window's pixel in the plane
            if (im) {                                                        // :157-164 repeat, concatenate, astype(np.float32) / 255.0
                const float dv = __fdiv_rn((float)d, 255.0f);
                const float iv = __fdiv_rn((float)interp[(int64_t)sl * plane + q], 255.0f);
                float* o6 = im + 6 * (int64_t)sl * win + p;
                o6[0] = dv; o6[win] = dv; o6[2 * win] = dv;
                o6[3 * win] = iv; o6[4 * win] = iv; o6[5 * win] = iv;
            }
            if (lb) lb[o] = (gt_line && d == 0) ? 0.0f : __fdiv_rn((float)src[q], 255.0f);          // :152-155, :167-169
        }
        if (zero_count) {                                                    // integer adds: the same total in any order
            zeros = wave_sum(zeros);
            if ((threadIdx.x & 63) == 0 && zeros != 0) atomicAdd(zero_count + sl, zeros);
        }
    }
}

// (pixel workgroups, sample rows) of a launch over n samples of `pixels` each, under FOLD_GRID_CAP workgroups in all
dim3 fold_grid(int64_t n, int64_t pixels)
{
    int64_t gx = (pixels + 255) / 256;
    if (gx > FOLD_GRID_CAP) gx = FOLD_GRID_CAP;
    if (gx < 1) gx = 1;
    int64_t gy = FOLD_GRID_CAP / gx;
    if (gy > n) gy = n;
    if (gy < 1) gy = 1;
    return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

hipError_t launch_fold_flow(const double* folds, int n, int H, int W, float* flow, float* flow2, uint8_t* mask, hipStream_t s)
{
    hipLaunchKernelGGL(fold_flow, fold_grid(n, (int64_t)H * W), dim3(256), 0, s, folds, n, H, W, flow, flow2, mask);
    return hipGetLastError();
}

hipError_t launch_image_warp_u8(const uint8_t* im, const float* flow, uint8_t* out, int n, int H, int W, int C, int bilinear, hipStream_t s)
{
    hipLaunchKernelGGL(image_warp_u8, fold_grid(n, (int64_t)H * W), dim3(256), 0, s, im, flow, out, n, H, W, C, bilinear);
    return hipGetLastError();
}

hipError_t launch_fold_degrade(const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int n, int slots, int SH,
                               int SW, int off_y, int off_x, int out_h, int out_w, int gt_line, uint8_t* deformed, float* flow2, float* im,
                               float* lb, int32_t* zero_count, hipStream_t s, const uint8_t* lut)
{
    if (zero_count) {
        int g = (n + 255) / 256;
        if (g > FOLD_GRID_CAP) g = FOLD_GRID_CAP;
        hipLaunchKernelGGL(fold_clear_counts, dim3((unsigned)g), dim3(256), 0, s, slot, n, slots, zero_count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (out_h == 0 || out_w == 0) return hipSuccess;
    const dim3 grid = fold_grid(n, (int64_t)out_h * out_w);
    if (lut)
        hipLaunchKernelGGL(fold_degrade<true>, grid, dim3(256), 0, s, clean, interp, folds, slot, n, slots, SH, SW, off_y, off_x, out_h, out_w,
                           gt_line, deformed, flow2, im, lb, zero_count, lut);
    else
        hipLaunchKernelGGL(fold_degrade<false>, grid, dim3(256), 0, s, clean, interp, folds, slot, n, slots, SH, SW, off_y, off_x, out_h, out_w,
                           gt_line, deformed, flow2, im, lb, zero_count, lut);
    return hipGetLastError();
}

}  // namespace sstem
