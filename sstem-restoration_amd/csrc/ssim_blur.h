// The 11-tap separable Gaussian blur of the SSIM criteria (ssim_kernels.hip: MS-SSIM; ssim_loss_kernels.hip: single-scale SSIM) in one
// place: the taps, the staging of an image pair into LDS with a zero halo, the row pass over the five moments, the column pass, and the
// map point's value and derivatives.  Device code works on LDS arrays the kernel owns; workgroups of 256 threads.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace sstem {

constexpr int SSIM_BLUR_TAPS = 11;            // the longest window; shorter ones are zero-padded to it

struct Taps { float g[SSIM_BLUR_TAPS]; };

// gaussian() of loss_ssim.py: double exponentials rounded to fp32, divided by their fp32 sum, sigma = 1.5 ws / 11 (1.5 for the full
// window); taps past ws are zero -- not score_kernels.hip's make_taps, which is scipy's float64 window at a fixed sigma
inline Taps make_taps(int ws)
{
    Taps t;
    const double sigma = 1.5 * ws / 11;
    float f[SSIM_BLUR_TAPS], sum = 0.f;
    for (int k = 0; k < ws; ++k) {
        const double d = (double)(k - ws / 2);
        f[k] = (float)exp(-(d * d) / (2 * sigma * sigma));
        sum += f[k];
    }
    for (int k = 0; k < SSIM_BLUR_TAPS; ++k) t.g[k] = k < ws ? f[k] / sum : 0.f;
    return t;
}

// E x E window of images x, y (h x w at `base`) from (y0, x0) into sx, sy; zero outside the image.
template <int E>
__device__ __forceinline__ void stage_pair(const float* __restrict__ x, const float* __restrict__ y, int64_t base, int h, int w, int y0,
                                           int x0, float* sx, float* sy)
{
    for (int e = threadIdx.x; e < E * E; e += 256) {
        const int r = e / E, c = e - r * E;
        const int iy = y0 + r, ix = x0 + c;
        const bool in = iy >= 0 && iy < h && ix >= 0 && ix < w;
        const int64_t o = base + (int64_t)iy * w + ix;
        sx[e] = in ? x[o] : 0.f;
        sy[e] = in ? y[o] : 0.f;
    }
}

// Row pass of the five moments: rows x cols outputs, output (r, c) from staged elements (r, c .. c + 10) of sx, sy (row stride `in_stride`);
// quantity q of output e = r * cols + c goes to out[q * plane + e], q = x, y, xx, yy, xy.
__device__ __forceinline__ void blur_rows_moments(const float* sx, const float* sy, int in_stride, int rows, int cols, const Taps& taps,
                                                  float* out, int plane)
{
    for (int e = threadIdx.x; e < rows * cols; e += 256) {
        const int r = e / cols, c = e - r * cols;
        float m1 = 0.f, m2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_BLUR_TAPS; ++k) {
            const float a = sx[r * in_stride + c + k], bb = sy[r * in_stride + c + k], g = taps.g[k];
            m1 = fmaf(g, a, m1); m2 = fmaf(g, bb, m2);
            s11 = fmaf(g, a * a, s11); s22 = fmaf(g, bb * bb, s22); s12 = fmaf(g, a * bb, s12);
        }
        out[e] = m1; out[plane + e] = m2; out[2 * plane + e] = s11; out[3 * plane + e] = s22; out[4 * plane + e] = s12;
    }
}

// One output of a pass: sum_k g[k] p[k * stride]
__device__ __forceinline__ float blur_point(const float* p, int stride, const Taps& taps)
{
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_BLUR_TAPS; ++k) s = fmaf(taps.g[k], p[k * stride], s);
    return s;
}

// The SSIM map at one point from its five blurred moments v = (mu1, mu2, e11, e22, e12):
//   A1 = 2 mu1 mu2 + C1, A2 = 2 (e12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1, B2 = (e11 - mu1^2) + (e22 - mu2^2) + C2
__device__ __forceinline__ float ssim_point(const float (&v)[5], float C1, float C2)
{
    const float mu1 = v[0], mu2 = v[1];
    const float m12 = mu1 * mu2, m11 = mu1 * mu1, m22 = mu2 * mu2;
    const float A1 = 2.f * m12 + C1, A2 = 2.f * (v[4] - m12) + C2;
    const float B1 = m11 + m22 + C1, B2 = (v[2] - m11) + (v[3] - m22) + C2;
    return (A1 * A2) / (B1 * B2);
}

// ... and its derivatives with respect to (mu1, e11, e12): the ones the gradient for the first image needs
__device__ __forceinline__ void ssim_point_derivs(const float (&v)[5], float C1, float C2, float& da, float& db, float& dc)
{
    const float mu1 = v[0], mu2 = v[1];
    const float m12 = mu1 * mu2, m11 = mu1 * mu1, m22 = mu2 * mu2;
    const float A2 = 2.f * (v[4] - m12) + C2;
    const float B2 = (v[2] - m11) + (v[3] - m22) + C2;
    const float inv2 = 1.f / B2;
    const float mcs = A2 * inv2;
    const float A1 = 2.f * m12 + C1, B1 = m11 + m22 + C1;
    const float inv1 = 1.f / B1;
    const float r = A1 * inv1;
    da = 2.f * inv1 * (mu2 - mu1 * r) * mcs + r * (2.f * inv2 * (mu1 * mcs - mu2));
    db = r * (-mcs * inv2);
    dc = r * (2.f * inv2);
}

}  // namespace sstem
