// Single-scale SSIM criterion of the SFF interpolation loop (cfg.TRAIN.loss = 'ssim': sff_scripts_interp/main_ms.py:27,153-155,203;
// SSIMLoss / _ssim of sff_scripts_interp/loss/loss_ssim.py:74-146): value and gradient, ONE launch each way.
//
// Images x, y of [B,C,H,W] are B C planes under one window (groups = channel): the 11 taps exp(-(k - 5)^2 / (2 1.5^2)) normalised in
// fp32 -- 11 whatever H and W are (the MS-SSIM entries shrink theirs) --, zero padding 5, so the map has the image's extent:
//   blur(t)[o] = sum_k g[k] t[o + k - 5]  (both axes);  mu1 = blur(x), mu2 = blur(y), e11 = blur(x x), e22 = blur(y y), e12 = blur(x y)
//   ssim = (2 mu1 mu2 + C1) (2 (e12 - mu1 mu2) + C2) / ((mu1^2 + mu2^2 + C1) ((e11 - mu1^2) + (e22 - mu2^2) + C2)),  C1 = 0.01^2, C2 = 0.03^2
//   value = 1 - mean(ssim) over everything, or per sample over its C H W points.
// Gradient with respect to x: with zero padding and an odd symmetric window the blur is its own adjoint, so with (a, b, c) the map's
// derivatives with respect to (mu1, e11, e12)
//   d value / d x = -(grad / N) (blur(a) + 2 x blur(b) + y blur(c)),  N = B C H W, or C H W per sample.
// It needs nothing the forward computed.
//
// Blur, staging and the map's formulas: ssim_blur.h.  Sums: a workgroup's map sum goes to the workspace as a double and the last
// workgroup to arrive adds them in index order (wg_reduce.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssim_blur.h"
#include "ssim_loss_kernels.h"
#include "wg_reduce.h"

namespace sstem {

namespace {

constexpr int T = 32;                           // tile edge, both kernels
constexpr int HALO = SSIM_BLUR_TAPS - 1;        // 10
constexpr int P = HALO / 2;                     // zero padding, 5
constexpr int FE = T + HALO;                    // forward: staged image extent, 42
constexpr int BM = T + HALO;                    // backward: map extent a tile's second blur reads, 42
constexpr int BE = BM + HALO;                   // backward: staged image extent, 52
constexpr float C1 = 0.0001f, C2 = 0.0009f;     // 0.01 ** 2, 0.03 ** 2 as fp32 scalars

// Forward.  Workgroup = one 32 x 32 tile of one plane's map.
__global__ __launch_bounds__(256) void ssim_loss_fwd(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int tiles_x,
                                                     int tiles, Taps taps, int per_sample, int64_t wgs_per_sample, double inv_count,
                                                     float* __restrict__ value, float* ws)
{
    __shared__ float sx[FE * FE], sy[FE * FE];
    __shared__ float hb[5 * FE * T];
    __shared__ double red[4][1];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / tiles;
    const int t = blockIdx.x - (int)plane * tiles;
    const int Y0 = (t / tiles_x) * T, X0 = (t % tiles_x) * T;

    stage_pair<FE>(x, y, plane * h * w, h, w, Y0 - P, X0 - P, sx, sy);
    __syncthreads();
    blur_rows_moments(sx, sy, FE, FE, T, taps, hb, FE * T);
    __syncthreads();

    const int tx = tid & 31, ty = tid >> 5;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ly = ty + 8 * i;
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = blur_point(hb + q * FE * T + ly * T + tx, T, taps);
        if (Y0 + ly < h && X0 + tx < w) sum += (double)ssim_point(v, C1, C2);
    }

    double* partials = reinterpret_cast<double*>(ws + SSIM_LOSS_HEADER_FLOATS);
    unsigned* counter = reinterpret_cast<unsigned*>(ws);
    const double sums[1] = {sum};
    block_sum(sums, red);
    if (tid == 0) agent_store(partials + (int64_t)blockIdx.x, block_tree(red, 0));
    if (!arrive_last(counter)) return;

    if (!per_sample) {
        // the last workgroup: every thread adds partials in index order, then the fixed tree
        block_total(partials, gridDim.x, red);
        if (tid != 0) return;
        *value = (float)(1.0 - block_tree(red, 0) * inv_count);
        release_counter(counter);
        return;
    }
    // per sample: one wave per sample, its workgroups' partials in index order per lane, then the wave's ladder
    const int lane = tid & 63;
    const int64_t B = gridDim.x / wgs_per_sample;
    for (int64_t i = tid >> 6; i < B; i += 4) {
        const double* first = partials + i * wgs_per_sample;
        double total = 0.0;
        for (int64_t j = lane; j < wgs_per_sample; j += 64) total += agent_load(first + j);
        total = wave_sum(total);
        if (lane == 0) value[i] = (float)(1.0 - total * inv_count);
    }
    if (tid == 0) release_counter(counter);
}

// Backward.  Workgroup = one 32 x 32 tile of one plane; it recomputes the blurred moments on the 42 x 42 map points its second blur
// reads (from a 52 x 52 staged window), forms (a, b, c) there -- zero outside the map --, blurs them and combines.
__global__ __launch_bounds__(256) void ssim_loss_bwd(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int tiles_x,
                                                     int tiles, Taps taps, int per_sample, int64_t planes_per_sample, float inv_count,
                                                     const float* __restrict__ grad_value, float* __restrict__ gout)
{
    constexpr int A_FLOATS = 2 * BE * BE > 3 * BM * BM ? 2 * BE * BE : 3 * BM * BM;
    constexpr int B_FLOATS = 5 * BE * BM;          // > 3 * BM * T
    __shared__ float ra[A_FLOATS];
    __shared__ float rb[B_FLOATS];
    float* sx = ra;
    float* sy = ra + BE * BE;
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / tiles;
    const int t = blockIdx.x - (int)plane * tiles;
    const int Y0 = (t / tiles_x) * T, X0 = (t % tiles_x) * T;
    const int64_t base = plane * h * w;

    stage_pair<BE>(x, y, base, h, w, Y0 - HALO, X0 - HALO, sx, sy);
    __syncthreads();

    const int tx = tid & 31, ty = tid >> 5;
    float cx[4], cy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cx[i] = sx[(ty + 8 * i + HALO) * BE + tx + HALO];
        cy[i] = sy[(ty + 8 * i + HALO) * BE + tx + HALO];
    }
    blur_rows_moments(sx, sy, BE, BE, BM, taps, rb, BE * BM);
    __syncthreads();

    // the map's derivatives on the 42 x 42 map points from (Y0 - 5, X0 - 5); zero outside the map
    float* ma = ra;
    float* mb = ra + BM * BM;
    float* mc = ra + 2 * BM * BM;
    for (int e = tid; e < BM * BM; e += 256) {
        const int m = e / BM, c = e - m * BM;
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = blur_point(rb + q * BE * BM + m * BM + c, BM, taps);
        const int oy = Y0 - P + m, ox = X0 - P + c;
        float da = 0.f, db = 0.f, dc = 0.f;
        if (oy >= 0 && oy < h && ox >= 0 && ox < w) ssim_point_derivs(v, C1, C2, da, db, dc);
        ma[e] = da; mb[e] = db; mc[e] = dc;
    }
    __syncthreads();

    // second blur, rows first: image column X0 + c reads map columns c .. c + 10 of this window
    for (int e = tid; e < BM * T; e += 256) {
        const int m = e / T, c = e - m * T;
        rb[e] = blur_point(ma + m * BM + c, 1, taps);
        rb[BM * T + e] = blur_point(mb + m * BM + c, 1, taps);
        rb[2 * BM * T + e] = blur_point(mc + m * BM + c, 1, taps);
    }
    __syncthreads();

    const float gv = grad_value ? grad_value[per_sample ? plane / planes_per_sample : 0] : 1.f;
    const float coef = -gv * inv_count;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ly = ty + 8 * i;
        const float s0 = blur_point(rb + ly * T + tx, T, taps);
        const float s1 = blur_point(rb + BM * T + ly * T + tx, T, taps);
        const float s2 = blur_point(rb + 2 * BM * T + ly * T + tx, T, taps);
        const int jy = Y0 + ly, jx = X0 + tx;
        if (jy < h && jx < w) gout[base + (int64_t)jy * w + jx] = coef * (s0 + 2.f * cx[i] * s1 + cy[i] * s2);
    }
}

}  // namespace

bool ssim_loss_plan(int64_t B, int64_t C, int64_t H, int64_t W, SsimLossPlan* plan)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return false;
    if (H > (1 << 15) || W > (1 << 15) || B > ((int64_t)1 << 24) || C > ((int64_t)1 << 24)) return false;
    SsimLossPlan pl = {};
    pl.planes = B * C;
    pl.h = (int)H; pl.w = (int)W;
    pl.tiles_x = (pl.w + 31) / 32;
    pl.tiles = pl.tiles_x * ((pl.h + 31) / 32);
    if (pl.planes > ((int64_t)1 << 24) || pl.planes * pl.tiles > ((int64_t)1 << 24)) return false;     // one grid dimension
    pl.wgs = pl.planes * pl.tiles;
    pl.wgs_per_sample = C * pl.tiles;
    pl.total_floats = SSIM_LOSS_HEADER_FLOATS + 2 * pl.wgs;          // one double per workgroup
    *plan = pl;
    return true;
}

hipError_t launch_ssim_loss_forward(const float* img1, const float* img2, int64_t B, const SsimLossPlan& plan, int per_sample, float* value,
                                    float* ws, hipStream_t s)
{
    const double points = (double)plan.h * plan.w * (double)(per_sample ? plan.planes / B : plan.planes);
    hipLaunchKernelGGL(ssim_loss_fwd, dim3((unsigned)plan.wgs), dim3(256), 0, s, img1, img2, plan.h, plan.w, plan.tiles_x, plan.tiles,
                       make_taps(SSIM_BLUR_TAPS), per_sample, plan.wgs_per_sample, 1.0 / points, value, ws);
    return hipGetLastError();
}

hipError_t launch_ssim_loss_backward(const float* img1, const float* img2, int64_t B, const SsimLossPlan& plan, int per_sample,
                                     const float* grad_value, float* grad_img1, hipStream_t s)
{
    const int64_t planes_per_sample = plan.planes / B;
    const double points = (double)plan.h * plan.w * (double)(per_sample ? planes_per_sample : plan.planes);
    hipLaunchKernelGGL(ssim_loss_bwd, dim3((unsigned)plan.wgs), dim3(256), 0, s, img1, img2, plan.h, plan.w, plan.tiles_x, plan.tiles,
                       make_taps(SSIM_BLUR_TAPS), per_sample, planes_per_sample, (float)(1.0 / points), grad_value, grad_img1);
    return hipGetLastError();
}

}  // namespace sstem
