// Validation scores of the reference's loops as launches: compute_psnr / compute_ssim of utils/psnr_ssim.py:7-71 per image, and EPE of
// loss/multiscaleloss.py:5-16.  The reference copies every prediction to the host and scores it with numpy / scipy.signal.convolve2d in
// float64; here the results stay on the device and nothing synchronises.
//
// score_images<T>, T = float or uint8_t, B independent single-channel pairs [B,H,W], two launches:
//   1. score_stats   per image: max a, max b (the reference's range branch `np.max(img1) <= 1.0 and np.max(img2) <= 1.0`, decided here),
//                    sum (a - b)^2 and sum (a / 255 - b / 255)^2 in float64; the image's last workgroup picks the branch, writes
//                    mse and psnr = 20 log10(1 / sqrt(mse)) (1e12, the reference's sentinel, where mse < 1e-10) and leaves the flag.
//   2. score_ssim_map  per 32 x 16 tile of the (H - 10) x (W - 10) 'valid' map: both images staged as fp32 (quantised as
//                    (uint8)(x * 255.f) when the flag says unit range -- one IEEE multiply and a truncation, numpy's
//                    (im * 255).astype(np.uint8) on a float32 array; used as they are otherwise), the five blurred moments, the map
//                    ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) and its sum in float64.
// The window is 11 taps of exp(-k^2 / (2 1.5^2)), normalised; the reference's 2-D window (matlab_style_gauss2D) is the outer product of
// this, and its `h < eps * h.max()` cut zeroes nothing at sigma = 1.5 (the smallest entry is exp(-50 / 4.5) = 1.5e-5).
// A NaN among the values makes the maximum NaN and so selects the `> 1` branch, as np.max does.
//
// Sums: per-workgroup double partials; the last workgroup of a launch to arrive (wg_reduce.h; one counter per launch) finishes every
// image, one wave per image: lane l adds the image's partials l, l + 64, ... in index order.  An image's result depends on its own partials
// only, so it is the same bits whatever its neighbours in the batch.  No float atomics, the same bits run to run.  The three counters
// sit in the workspace's first 64 bytes whatever the shape and everything behind them is written before it is read, so one zeroed
// workspace serves calls of any shapes (up to the size it was asked for) and graph replays without another fill.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "score_kernels.h"
#include "wg_reduce.h"

namespace sstem {

namespace {

constexpr int TW = SCORE_TILE_W, TH = SCORE_TILE_H;
constexpr int HALO = SCORE_TAPS - 1;            // 10
constexpr int SW = TW + HALO, SH = TH + HALO;   // staged extent, 42 x 26

struct DTaps { double g[SCORE_TAPS]; };
constexpr int CNT_EPE = 0, CNT_STATS = 1, CNT_MAP = 2;      // the workspace's first words

// np.max: a NaN, once met, stays
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// pred[pred > 1] = 1; pred[pred < 0] = 0 (a NaN passes, as there)
__device__ __forceinline__ float clamp01(float v) { return v > 1.f ? 1.f : (v < 0.f ? 0.f : v); }

// (uint8)(x * 255.f) for x <= 1; below 0, where numpy's cast is undefined, 0
__device__ __forceinline__ float quantise(float v) { return v > 0.f ? (float)(int)(v * 255.f) : 0.f; }

__device__ __forceinline__ float wave_nan_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_down(v, o, 64));
    return v;
}

// Launch 1.  Workgroup = chunk c of image b: elements c * 256 + tid, stepping by chunks * 256.
// For bytes the reference's `(img1 - img2) ** 2` wraps modulo 256; that branch is reached only by images of 0 and 1, where the wrapped
// square is the true one.
template <class T>
__global__ __launch_bounds__(256) void score_stats(const T* __restrict__ a, const T* __restrict__ b, int64_t B, int64_t HW, int chunks,
                                                   int clamp01_a, double* __restrict__ scores, unsigned* counters, int* unit_range,
                                                   double* partials)
{
    __shared__ double red[4][4];
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x / chunks;
    const int c = blockIdx.x - (int)img * chunks;
    const T* pa = a + img * HW;
    const T* pb = b + img * HW;
    float ma = -INFINITY, mb = -INFINITY;
    double s_unit = 0.0, s_255 = 0.0;
    for (int64_t i = (int64_t)c * 256 + tid; i < HW; i += (int64_t)chunks * 256) {
        float va = (float)pa[i];
        const float vb = (float)pb[i];
        if (clamp01_a) va = clamp01(va);
        ma = nan_max(ma, va); mb = nan_max(mb, vb);
        const double d = (double)va - (double)vb;
        const double e = (double)va / 255. - (double)vb / 255.;
        s_unit += d * d;
        s_255 += e * e;
    }
    wave_slot(red, 0, (double)wave_nan_max(ma)); wave_slot(red, 1, (double)wave_nan_max(mb));
    wave_slot(red, 2, wave_sum(s_unit)); wave_slot(red, 3, wave_sum(s_255));
    __syncthreads();
    double* mine = partials + 4 * (int64_t)blockIdx.x;
    if (tid == 0) {
        agent_store(mine + 0, (double)nan_max(nan_max((float)red[0][0], (float)red[1][0]), nan_max((float)red[2][0], (float)red[3][0])));
        agent_store(mine + 1, (double)nan_max(nan_max((float)red[0][1], (float)red[1][1]), nan_max((float)red[2][1], (float)red[3][1])));
        agent_store(mine + 2, block_tree(red, 2));
        agent_store(mine + 3, block_tree(red, 3));
    }
    if (!arrive_last(counters + CNT_STATS)) return;

    // the launch's last workgroup: one wave per image, lane l takes the image's partial l (chunks <= 64), then the fixed tree
    const int lane = tid & 63;
    for (int64_t i = tid >> 6; i < B; i += 4) {
        const double* first = partials + 4 * i * chunks;
        float xa = -INFINITY, xb = -INFINITY;
        double t_unit = 0.0, t_255 = 0.0;
        if (lane < chunks) {
            xa = (float)agent_load(first + 4 * lane);
            xb = (float)agent_load(first + 4 * lane + 1);
            t_unit = agent_load(first + 4 * lane + 2);
            t_255 = agent_load(first + 4 * lane + 3);
        }
        xa = wave_nan_max(xa); xb = wave_nan_max(xb);
        t_unit = wave_sum(t_unit); t_255 = wave_sum(t_255);
        if (lane == 0) {
            const int unit = xa <= 1.f && xb <= 1.f;
            const double mse = (unit ? t_unit : t_255) / (double)HW;
            scores[3 * i] = mse;
            scores[3 * i + 1] = mse < 1.0e-10 ? 1.0e12 : 20.0 * log10(1.0 / sqrt(mse));
            unit_range[i] = unit;
        }
    }
    if (tid == 0) release_counter(counters + CNT_STATS);
}

// Launch 2.  Workgroup = one 32 x 16 tile of one image's map; map point (oy, ox) reads image rows oy .. oy + 10, columns ox .. ox + 10.
template <class T>
__global__ __launch_bounds__(256) void score_ssim_map(const T* __restrict__ a, const T* __restrict__ b, int H, int W, int oh, int ow,
                                                      int tiles_x, int tiles, DTaps taps, int clamp01_a, double count,
                                                      double* __restrict__ scores, unsigned* counters, const int* unit_range,
                                                      double* partials)
{
    __shared__ float sa[SH * SW], sb[SH * SW];
    __shared__ double hb[5][SH * TW];
    __shared__ double red[4][1];
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x / tiles;
    const int t = blockIdx.x - (int)img * tiles;
    const int Y0 = (t / tiles_x) * TH, X0 = (t % tiles_x) * TW;
    const int64_t base = img * H * W;
    const int unit = unit_range[img];              // left by score_stats, earlier on this stream

    for (int e = tid; e < SH * SW; e += 256) {
        const int r = e / SW, c = e - r * SW;
        const int iy = Y0 + r, ix = X0 + c;
        float va = 0.f, vb = 0.f;
        if (iy < H && ix < W) {
            const int64_t o = base + (int64_t)iy * W + ix;
            va = (float)a[o]; vb = (float)b[o];
            if (clamp01_a) va = clamp01(va);
            if (unit) { va = quantise(va); vb = quantise(vb); }
        }
        sa[e] = va; sb[e] = vb;
    }
    __syncthreads();

    for (int e = tid; e < SH * TW; e += 256) {
        const int r = e / TW, c = e - r * TW;
        double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
        for (int k = 0; k < SCORE_TAPS; ++k) {
            const double x = (double)sa[r * SW + c + k], y = (double)sb[r * SW + c + k], g = taps.g[k];
            m1 = fma(g, x, m1); m2 = fma(g, y, m2);
            s11 = fma(g, x * x, s11); s22 = fma(g, y * y, s22); s12 = fma(g, x * y, s12);
        }
        hb[0][e] = m1; hb[1][e] = m2; hb[2][e] = s11; hb[3][e] = s22; hb[4][e] = s12;
    }
    __syncthreads();

    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const int tx = tid & 31, ty = tid >> 5;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < TH / 8; ++i) {
        const int ly = ty + 8 * i;
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < SCORE_TAPS; ++k) s = fma(taps.g[k], hb[q][(ly + k) * TW + tx], s);
            v[q] = s;
        }
        if (Y0 + ly < oh && X0 + tx < ow) {
            const double mu1 = v[0], mu2 = v[1];
            const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
            sum += ((2.0 * m12 + C1) * (2.0 * (v[4] - m12) + C2)) / ((m11 + m22 + C1) * ((v[2] - m11) + (v[3] - m22) + C2));
        }
    }
    const double sums[1] = {sum};
    block_sum(sums, red);
    if (tid == 0) agent_store(partials + (int64_t)blockIdx.x, block_tree(red, 0));
    if (!arrive_last(counters + CNT_MAP)) return;

    // the launch's last workgroup: one wave per image, its tiles' partials in index order per lane, then the fixed tree
    const int lane = tid & 63;
    const int64_t B = gridDim.x / tiles;
    for (int64_t i = tid >> 6; i < B; i += 4) {
        const double* first = partials + i * tiles;
        double total = 0.0;
        for (int j = lane; j < tiles; j += 64) total += agent_load(first + j);
        total = wave_sum(total);
        if (lane == 0) scores[3 * i + 2] = total / count;             // np.mean divides: identical images give exactly 1
    }
    if (tid == 0) release_counter(counters + CNT_MAP);
}

// EPE(input_flow, target_flow, sparse, mean) for [B,2,H,W]: sqrt(dx^2 + dy^2) per pixel in float64; sparse skips the pixels whose two
// target components are both exactly 0.  One launch; the last workgroup divides by the kept count (mean; 0 / 0 = NaN when nothing is
// kept, the reference's empty mean) or by B.
__global__ __launch_bounds__(256) void flow_epe_kernel(const float* __restrict__ flow, const float* __restrict__ target, int64_t n, int64_t HW,
                                                       int sparse, int mean, double batch, double* __restrict__ value, unsigned* counter,
                                                       double* partials)
{
    __shared__ double red[4][2];
    const int tid = threadIdx.x;
    double sum = 0.0, kept = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t img = i / HW;
        const int64_t o = i + img * HW;            // [img][0][pixel]
        const float tx = target[o], ty = target[o + HW];
        if (sparse && tx == 0.f && ty == 0.f) continue;
        const double dx = (double)tx - (double)flow[o], dy = (double)ty - (double)flow[o + HW];
        sum += sqrt(dx * dx + dy * dy);
        kept += 1.0;
    }
    const double sums[2] = {sum, kept};
    block_sum(sums, red);
    if (tid == 0) {
        agent_store(partials + 2 * (int64_t)blockIdx.x, block_tree(red, 0));
        agent_store(partials + 2 * (int64_t)blockIdx.x + 1, block_tree(red, 1));
    }
    if (!arrive_last(counter)) return;

    block_total(partials, gridDim.x, red);
    if (tid != 0) return;
    const double total = block_tree(red, 0), count = block_tree(red, 1);
    *value = mean ? total / count : total / batch;
    release_counter(counter);
}

DTaps make_taps()
{
    // matlab_style_gauss2D's separable factor: float64 throughout, sigma fixed at 1.5 -- not ssim_kernels.hip's make_taps, which follows
    // torch's fp32 window with a sigma that shrinks with the window
    DTaps t;
    double sum = 0.0;
    for (int k = 0; k < SCORE_TAPS; ++k) {
        const double d = (double)(k - SCORE_TAPS / 2);
        t.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += t.g[k];
    }
    for (int k = 0; k < SCORE_TAPS; ++k) t.g[k] /= sum;
    return t;
}

}  // namespace

bool score_plan(int64_t B, int64_t H, int64_t W, ScorePlan* plan)
{
    if (B < 0 || H < 0 || W < 0) return false;
    if (H > (1 << 15) || W > (1 << 15) || B > ((int64_t)1 << 24)) return false;
    ScorePlan pl = {};
    const int64_t HW = H * W;
    const int64_t chunks = (HW + 4095) / 4096;
    pl.chunks = (int)(chunks < 1 ? 1 : (chunks > SCORE_MAX_CHUNKS ? SCORE_MAX_CHUNKS : chunks));
    if (H >= SCORE_TAPS && W >= SCORE_TAPS) {
        pl.tiles_x = (int)((W - 10 + SCORE_TILE_W - 1) / SCORE_TILE_W);
        pl.tiles = pl.tiles_x * (int)((H - 10 + SCORE_TILE_H - 1) / SCORE_TILE_H);
    }
    if (B * pl.tiles > ((int64_t)1 << 24)) return false;         // one grid dimension
    const int64_t epe = (B * HW + 2047) / 2048;
    pl.epe_wgs = (int)(epe < 1 ? 1 : (epe > SCORE_EPE_MAX_WGS ? SCORE_EPE_MAX_WGS : epe));
    int64_t off = 64;                                            // the three counters, then 8-byte aligned parts
    pl.off_epe_partials = off; off += 16 * (int64_t)SCORE_EPE_MAX_WGS;
    pl.off_unit_range = off; off += 8 * ((B + 1) / 2);
    pl.off_stat_partials = off; off += 32 * B * pl.chunks;
    pl.off_map_partials = off; off += 8 * B * pl.tiles;
    pl.total_bytes = off;
    *plan = pl;
    return true;
}

template <class T>
hipError_t launch_score_images(const T* a, const T* b, int64_t B, int64_t H, int64_t W, const ScorePlan& plan, int clamp01_a, double* scores,
                               void* ws, hipStream_t s)
{
    char* base = static_cast<char*>(ws);
    unsigned* counters = reinterpret_cast<unsigned*>(base);
    int* unit_range = reinterpret_cast<int*>(base + plan.off_unit_range);
    hipLaunchKernelGGL(score_stats<T>, dim3((unsigned)(B * plan.chunks)), dim3(256), 0, s, a, b, B, H * W, plan.chunks, clamp01_a, scores,
                       counters, unit_range, reinterpret_cast<double*>(base + plan.off_stat_partials));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int oh = (int)H - 10, ow = (int)W - 10;
    hipLaunchKernelGGL(score_ssim_map<T>, dim3((unsigned)(B * plan.tiles)), dim3(256), 0, s, a, b, (int)H, (int)W, oh, ow, plan.tiles_x,
                       plan.tiles, make_taps(), clamp01_a, (double)oh * ow, scores, counters, unit_range,
                       reinterpret_cast<double*>(base + plan.off_map_partials));
    return hipGetLastError();
}

template hipError_t launch_score_images<float>(const float*, const float*, int64_t, int64_t, int64_t, const ScorePlan&, int, double*, void*,
                                               hipStream_t);
template hipError_t launch_score_images<uint8_t>(const uint8_t*, const uint8_t*, int64_t, int64_t, int64_t, const ScorePlan&, int, double*,
                                                 void*, hipStream_t);

hipError_t launch_flow_epe(const float* flow, const float* target, int64_t B, int64_t H, int64_t W, const ScorePlan& plan, int sparse, int mean,
                           double* value, void* ws, hipStream_t s)
{
    char* base = static_cast<char*>(ws);
    hipLaunchKernelGGL(flow_epe_kernel, dim3((unsigned)plan.epe_wgs), dim3(256), 0, s, flow, target, B * H * W, H * W, sparse, mean, (double)B,
                       value, reinterpret_cast<unsigned*>(base) + CNT_EPE, reinterpret_cast<double*>(base + plan.off_epe_partials));
    return hipGetLastError();
}

}  // namespace sstem
