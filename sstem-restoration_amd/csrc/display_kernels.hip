// The image outputs of the SFF inference scripts and the unfolding monitor (include/sstem_display.h): the Middlebury colour code of a
// flow field, and the uint8 images the scripts save.
//
// Replaces the host tail of sff_scripts_fusion/inference.py:161-172, sff_scripts_unfolding/inference.py:146-153 and
// main_flowfusionnet.py:256-257,297-298: fp32 tensors downloaded, utils/flow_display.py's dense_flow in numpy, (x * 255).astype(uint8),
// PIL's convert('L'), the < 2 mask and the stitch.  Here the flow is read where the net left it and 3 bytes per pixel come out.
//
// The colour code is two launches on the stream: flow_maxrad leaves up to 128 partial maxima of every image's radius in the workspace
// (a maximum over the bits of non-negative floats: the same in any order), every workgroup of flow_colour takes the maximum of its
// image's partials and colours its pixels in float64.  Every word that is read was written by the same call, so the workspace is
// never cleared.  (A first version took one atomic maximum per workgroup and image and counted arrivals to reset the word; at
// 8 x 1024^2 those 16384 atomics on eight addresses were 570 of the entry's 668 us.)
//
// The contract is the reference's arithmetic operation by operation (the header lists it): float32 products and sums, then float64
// products, sums and divisions, each rounded on its own.  hipcc's default contraction would fuse them; the pragma below takes the
// contract flag off every operation of this translation unit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sstem_display.h"
#include "display_kernels.h"
#include "numpy_u8.h"

namespace sstem {

namespace {

constexpr int DISPLAY_GRID_CAP = 4096;   // workgroups per launch, a lane takes a pixel; larger planes walk by the stride
constexpr int PARTS = FLOW_MAXRAD_PARTS; // workgroups of flow_maxrad per image = partial maxima per image in the workspace
constexpr int WHEEL = SSTEM_FLOW_WHEEL_COLS;
constexpr unsigned MAXRAD_NAN = 0xFFFFFFFFu;   // above the bits of every non-negative float: some radius of the image was NaN

// The colour wheel: six arcs between the primaries, on each arc one channel ramps by floor(255 i / n) while another holds 255.
//   red -> yellow 15 (G up), yellow -> green 6 (R down), green -> cyan 4 (B up), cyan -> blue 11 (G down), blue -> magenta 13 (R up),
//   magenta -> red 6 (B down).  255 i / n in integers is the floor of the exact quotient.
struct Wheel {
    uint8_t rgb[WHEEL][3];
};

constexpr Wheel make_wheel()
{
    constexpr int arcs[6][3] = {{15, 1, +1}, {6, 0, -1}, {4, 2, +1}, {11, 1, -1}, {13, 0, +1}, {6, 2, -1}};   // length, ramping channel, direction
    constexpr int held[6][3] = {{255, 0, 0}, {0, 255, 0}, {0, 255, 0}, {0, 0, 255}, {0, 0, 255}, {255, 0, 0}};   // the channels that do not ramp
    Wheel w{};
    int col = 0;
    for (int a = 0; a < 6; ++a) {
        for (int i = 0; i < arcs[a][0]; ++i, ++col) {
            for (int c = 0; c < 3; ++c) w.rgb[col][c] = (uint8_t)held[a][c];
            const int ramp = 255 * i / arcs[a][0];
            w.rgb[col][arcs[a][1]] = (uint8_t)(arcs[a][2] > 0 ? ramp : 255 - ramp);
        }
    }
    return w;
}

__constant__ Wheel d_wheel = make_wheel();
const Wheel h_wheel = make_wheel();

// u, v of pixel p of one image; an unknown pixel (|u| or |v| above 1e7, infinities included; a NaN compares false) counts as (0, 0)
struct FlowPixel {
    float u, v;
    bool unknown;
};

__device__ __forceinline__ FlowPixel flow_pixel(const float* __restrict__ image, int64_t plane, int64_t p, int hwc)
{
    FlowPixel px;
    px.u = hwc ? image[2 * p] : image[p];
    px.v = hwc ? image[2 * p + 1] : image[plane + p];
    px.unknown = fabsf(px.u) > 1.0e7f || fabsf(px.v) > 1.0e7f;
    if (px.unknown) px.u = px.v = 0.0f;
    return px;
}

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// the maximum over the workgroup, to every thread; red is free again after the call
__device__ __forceinline__ unsigned block_umax(unsigned m, unsigned (&red)[4])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = umax(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = umax(umax(red[0], red[1]), umax(red[2], red[3]));
    __syncthreads();
    return m;
}

// grid (parts, gy): blockIdx.y walks the images, the parts workgroups of a row share the pixels of one.  ws[b][blockIdx.x] takes the
// workgroup's maximum of image b: the bits of the float32 radius, or MAXRAD_NAN.
__global__ __launch_bounds__(256) void flow_maxrad(const float* __restrict__ flow, int B, int64_t plane, int hwc, unsigned* __restrict__ ws)
{
    __shared__ unsigned red[4];
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* image = flow + (int64_t)b * 2 * plane;
        unsigned m = 0u;
#pragma unroll 4
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (int64_t)gridDim.x * 256) {
            const FlowPixel px = flow_pixel(image, plane, p, hwc);
            const float uu = px.u * px.u, vv = px.v * px.v;
            const float sum = uu + vv;
            // the float32 square root, correctly rounded: the float64 root is, and rounding it again cannot differ (53 >= 2 * 24 + 2)
            const float rad = (float)sqrt((double)sum);
            m = umax(m, rad != rad ? MAXRAD_NAN : __float_as_uint(rad));     // rad >= +0 otherwise: its bits order as it does
        }
        m = block_umax(m, red);
        if (threadIdx.x == 0) ws[(int64_t)b * PARTS + blockIdx.x] = m;
    }
}

// grid (gx, gy) as above with a lane per pixel.  parts: the row length of flow_maxrad's grid, the words of ws[b] that hold this call's maxima.
__global__ __launch_bounds__(256) void flow_colour(const float* __restrict__ flow, int B, int64_t plane, int hwc, uint8_t* __restrict__ rgb,
                                                   const unsigned* __restrict__ ws, int parts)
{
    __shared__ double wheel[WHEEL * 3];                                      // wheel[k][c] / 255, the division made once
    __shared__ unsigned red[4];
    if (threadIdx.x < WHEEL * 3) wheel[threadIdx.x] = (double)d_wheel.rgb[threadIdx.x / 3][threadIdx.x % 3] / 255.0;
    static_assert(PARTS <= 256, "one partial per thread");
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const unsigned bits = block_umax((int)threadIdx.x < parts ? ws[(int64_t)b * PARTS + threadIdx.x] : 0u, red);   // its barriers also order the wheel
        float maxrad = bits == MAXRAD_NAN ? -1.0f : __uint_as_float(bits);
        if (!(maxrad > -1.0f)) maxrad = -1.0f;
        const double d = (double)maxrad + 2.220446049250313e-16;            // np.finfo(float).eps = 2^-52
        const float* image = flow + (int64_t)b * 2 * plane;
        uint8_t* out = rgb + (int64_t)b * 3 * plane;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (int64_t)gridDim.x * 256) {
            const FlowPixel px = flow_pixel(image, plane, p, hwc);
            double u = (double)px.u / d, v = (double)px.v / d;
            const bool nan = u != u || v != v;
            if (nan) u = v = 0.0;
            const double uu = u * u, vv = v * v;
            const double rad = sqrt(uu + vv);
            const double a = atan2(-v, -u) / 3.141592653589793;             // np.pi
            const double fk = (a + 1.0) / 2.0 * (double)(WHEEL - 1) + 1.0;
            const double fl = floor(fk);
            int k0 = (int)fl;
            k0 = k0 < 1 ? 1 : (k0 > WHEEL ? WHEEL : k0);                     // 1 <= fk <= 55 for |a| <= 1: the index stays in the wheel
            const int k1 = k0 == WHEEL ? 1 : k0 + 1;
            const double f = fk - (double)k0;
            const double live = nan ? 0.0 : 1.0;
            uint8_t byte[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double lo = (1.0 - f) * wheel[(k0 - 1) * 3 + c], hi = f * wheel[(k1 - 1) * 3 + c];
                double col = lo + hi;
                if (rad <= 1.0) {
                    const double fade = rad * (1.0 - col);
                    col = 1.0 - fade;
                } else {
                    col = col * 0.75;
                }
                const double scaled = 255.0 * col;
                byte[c] = px.unknown ? (uint8_t)0 : (uint8_t)((int)floor(scaled * live) & 0xFF);
            }
            out[3 * p + 0] = byte[0];
            out[3 * p + 1] = byte[1];
            out[3 * p + 2] = byte[2];
        }
    }
}

// The same grid; each output is made where its pointer is given (the entry has checked the inputs it needs)
__global__ __launch_bounds__(256) void sff_outputs(const float* __restrict__ pred, const float* __restrict__ warped,
                                                   const uint8_t* __restrict__ interp, int B, int64_t plane, uint8_t* __restrict__ pred_u8,
                                                   uint8_t* __restrict__ warped_rgb, uint8_t* __restrict__ stitch_u8)
{
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int64_t base = (int64_t)b * plane;
        for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (int64_t)gridDim.x * 256) {
            const int64_t i = base + p;
            if (pred_u8) pred_u8[i] = numpy_u8_of(pred[i]);
            if (warped_rgb || stitch_u8) {
                const float* w = warped + 3 * base + p;
                const uint8_t r = numpy_u8_of(w[0]), g = numpy_u8_of(w[plane]), bl = numpy_u8_of(w[2 * plane]);
                if (warped_rgb) {
                    warped_rgb[3 * i + 0] = r;
                    warped_rgb[3 * i + 1] = g;
                    warped_rgb[3 * i + 2] = bl;
                }
                if (stitch_u8) {
                    const unsigned L = (19595u * r + 38470u * g + 7471u * bl + 32768u) >> 16;   // PIL's convert('L')
                    stitch_u8[i] = L < 2u ? interp[i] : (uint8_t)L;
                }
            }
        }
    }
}

// a row of up to `row_cap` workgroups per image, and as many rows as the cap and the batch allow
dim3 image_grid(int B, int64_t pixels_per_workgroup, int64_t plane, int row_cap)
{
    int64_t gx = (plane + pixels_per_workgroup - 1) / pixels_per_workgroup;
    if (gx > row_cap) gx = row_cap;
    int64_t gy = DISPLAY_GRID_CAP / gx;
    if (gy > B) gy = B;
    return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

const uint8_t* flow_color_wheel() { return &h_wheel.rgb[0][0]; }

hipError_t launch_flow_color(const float* flow, int B, int64_t plane, int hwc, uint8_t* rgb, unsigned* workspace, hipStream_t s)
{
    const dim3 parts = image_grid(B, 256 * 8, plane, PARTS);                 // eight pixels a lane before a row grows: few, fat workgroups
    hipLaunchKernelGGL(flow_maxrad, parts, dim3(256), 0, s, flow, B, plane, hwc, workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flow_colour, image_grid(B, 256, plane, DISPLAY_GRID_CAP), dim3(256), 0, s, flow, B, plane, hwc, rgb, workspace, (int)parts.x);
    return hipGetLastError();
}

hipError_t launch_sff_outputs(const float* pred, const float* warped, const uint8_t* interp, int B, int64_t plane, uint8_t* pred_u8,
                              uint8_t* warped_rgb, uint8_t* stitch_u8, hipStream_t s)
{
    hipLaunchKernelGGL(sff_outputs, image_grid(B, 256, plane, DISPLAY_GRID_CAP), dim3(256), 0, s, pred, warped, interp, B, plane, pred_u8, warped_rgb,
                       stitch_u8);
    return hipGetLastError();
}

}  // namespace sstem
