// Colour jitter as a byte table (include/sstem_jitter.h): the histogram of every sample's plane, then one 256-entry table per sample.
//
// Replaces the host's PIL chain of the reference's Train._color_jitter (sff_scripts_fusion/data/data_provider.py:309-313): up to three
// ImageEnhance blends over a 400 x 400 crop, one of them behind a mean of the whole image.  Every blend maps a byte to a byte, so the
// device needs the crop's histogram once (256 counts) and then works on 256 values per sample; the fold degradation reads its section
// through the table (fold_kernels.hip).  Three launches on the stream, ordered by their boundaries: clear, histogram, tables.
//
// The contract is bit for bit with PIL's Blend.c: a float32 product and a float32 sum, each rounded on its own.  hipcc's default
// contraction would fuse them; the pragma below takes the contract flag off every operation of this translation unit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sstem_jitter.h"
#include "jitter_kernels.h"
#include "wg_reduce.h"

namespace sstem {

namespace {

constexpr int JITTER_GRID_CAP = 1024;    // workgroups per launch: 4 per CU, each leaves 256 global adds; larger problems walk by the stride

__global__ __launch_bounds__(256) void jitter_clear(uint32_t* __restrict__ hist, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) hist[i] = 0u;
}

// grid (gx, gy): blockIdx.y walks the samples, blockIdx.x the dwords of one.  A sample's base is wherever n * S_h * S_w bytes put it:
// the bytes ahead of the first aligned dword and behind the last whole one go to workgroup 0, one byte per lane.
__global__ __launch_bounds__(256) void jitter_hist(const uint8_t* __restrict__ planes, int n, int64_t plane, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t bins[256];
    for (int s = blockIdx.y; s < n; s += gridDim.y) {
        bins[threadIdx.x] = 0u;
        __syncthreads();
        const uint8_t* src = planes + (int64_t)s * plane;
        int64_t head = (int64_t)((4u - (unsigned)((uintptr_t)src & 3u)) & 3u);
        if (head > plane) head = plane;
        const int64_t words = (plane - head) >> 2;
        const uint32_t* mid = reinterpret_cast<const uint32_t*>(src + head);
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
            const uint32_t w = mid[i];
            atomicAdd(&bins[w & 255u], 1u);
            atomicAdd(&bins[(w >> 8) & 255u], 1u);
            atomicAdd(&bins[(w >> 16) & 255u], 1u);
            atomicAdd(&bins[w >> 24], 1u);
        }
        if (blockIdx.x == 0) {
            const int64_t body = head + 4 * words, t = threadIdx.x;          // plane - body < 4 bytes follow the last dword
            if (t < head) atomicAdd(&bins[src[t]], 1u);
            else if (t - head < plane - body) atomicAdd(&bins[src[body + (t - head)]], 1u);
        }
        __syncthreads();
        const uint32_t c = bins[threadIdx.x];
        if (c != 0u) atomicAdd(hist + (int64_t)s * 256 + threadIdx.x, c);     // integer adds: the same total in any order
        __syncthreads();                                                     // bins are cleared again for the next sample
    }
}

// Blend.c on bytes: the degenerate d, the byte v, alpha the float32 factor
__device__ __forceinline__ int jitter_blend(int d, int v, float alpha)
{
    const float p = alpha * (float)(v - d);
    const float t = (float)d + p;
    if (!(fabsf(t) <= 3.4028234664e38f)) return 0;                           // NaN or infinite: outside the contract
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 0xFF;                // interpolation: t lies between d and v
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);                     // extrapolation, clipped
}

// one workgroup per sample, lane = byte value
__global__ __launch_bounds__(256) void jitter_table(const uint32_t* __restrict__ hist, int n, int64_t count, const int32_t* __restrict__ op_code,
                                                    const float* __restrict__ op_factor, uint8_t* __restrict__ lut)
{
    __shared__ unsigned long long red[4][1];
    for (int s = blockIdx.x; s < n; s += gridDim.x) {
        const int32_t* code = op_code + (int64_t)s * SSTEM_JITTER_OPS;      // block-uniform
        const float* factor = op_factor + (int64_t)s * SSTEM_JITTER_OPS;
        bool known = true;
        for (int q = 0; q < SSTEM_JITTER_OPS; ++q) known = known && code[q] >= SSTEM_JITTER_NONE && code[q] <= SSTEM_JITTER_SATURATION;
        if (!known) continue;
        const unsigned long long h = hist[(int64_t)s * 256 + threadIdx.x];
        int cur = threadIdx.x;
        for (int q = 0; q < SSTEM_JITTER_OPS; ++q) {
            if (code[q] == SSTEM_JITTER_BRIGHTNESS) {
                cur = jitter_blend(0, cur, factor[q]);
            } else if (code[q] == SSTEM_JITTER_CONTRAST) {
                const unsigned long long part[1] = {h * (unsigned long long)cur};
                block_sum(part, red);
                const unsigned long long sum = block_tree(red, 0);           // of the image as it is at this step, below 2^38
                __syncthreads();                                             // red is written again by a later contrast step
                const int d = (int)((2ull * sum + (unsigned long long)count) / (2ull * (unsigned long long)count));
                cur = jitter_blend(d, cur, factor[q]);
            }
        }
        lut[(int64_t)s * 256 + threadIdx.x] = (uint8_t)cur;
    }
}

}  // namespace

hipError_t launch_jitter_lut(const uint8_t* planes, int n, int64_t plane, const int32_t* op_code, const float* op_factor, uint8_t* lut,
                             uint32_t* hist, hipStream_t s)
{
    const int64_t bins = (int64_t)n * 256;
    int64_t g = (bins + 255) / 256;
    if (g > JITTER_GRID_CAP) g = JITTER_GRID_CAP;
    hipLaunchKernelGGL(jitter_clear, dim3((unsigned)g), dim3(256), 0, s, hist, bins);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    int64_t gx = (plane / 4 + 255) / 256;                                    // a lane takes a dword
    if (gx > JITTER_GRID_CAP) gx = JITTER_GRID_CAP;
    if (gx < 1) gx = 1;
    int64_t gy = JITTER_GRID_CAP / gx;
    if (gy > n) gy = n;
    hipLaunchKernelGGL(jitter_hist, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, planes, n, plane, hist);
    e = hipGetLastError();
    if (e != hipSuccess) return e;

    hipLaunchKernelGGL(jitter_table, dim3((unsigned)(n < JITTER_GRID_CAP ? n : JITTER_GRID_CAP)), dim3(256), 0, s, hist, n, plane, op_code, op_factor,
                       lut);
    return hipGetLastError();
}

}  // namespace sstem
