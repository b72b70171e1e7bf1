// MS-SSIM criterion of the SFF fusion training loop (cfg.TRAIN.loss = 'ssim': sff_scripts_fusion/main_fusion.py:194-211,252-254;
// MS_SSIM(max_val=1) of sff_scripts_fusion/loss/loss_ssim.py:18-72): value and gradient, one launch per pyramid level each way.
//
// Per level, images x, y of [B,1,h,w]: window ws = min(h, w, 11), taps g[k] = exp(-(k - ws/2)^2 / (2 sigma^2)) normalised, sigma = 1.5 ws / 11,
// zero padding p = ws / 2, map extent oh = h + 2 p - ws + 1 (h + 1 for an even window, as F.conv2d(padding = ws // 2) gives it):
//   blur(t)[o] = sum_k g[k] t[o + k - p]  (both axes);  mu1 = blur(x), mu2 = blur(y), e11 = blur(x x), e22 = blur(y y), e12 = blur(x y)
//   A1 = 2 mu1 mu2 + C1, A2 = 2 (e12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1, B2 = (e11 - mu1^2) + (e22 - mu2^2) + C2
//   mcs = A2 / B2, ssim = A1 A2 / (B1 B2), the level's two terms are their means over B oh ow
// and the next level's images are the 2 x 2 averages ((a + b) + c) + d times 0.25 (pool2x2_forward's arithmetic).
//   value = prod_{i < L-1} mcs_i^w_i * ssim_{L-1}^w_{L-1}
// Gradient with respect to x: per level coef_i (blurT[a] + 2 x blurT[b] + y blurT[c]) with blurT[f][j] = sum_k g[k] f[j - k + p] over the map,
// (a, b, c) the map's derivatives with respect to (mu1, e11, e12), coef_i = w_i value / (term_i B oh ow), plus a quarter of the coarser level's
// gradient at [j / 2] wherever the floored 2 x 2 window covers j (a gather in this level's epilogue).
//
// Every window runs as 11 taps, the shorter ones padded with zero taps at the end, so the loops unroll with the taps in scalar registers;
// the staged halo is sized for 11 and zero outside the image (a zero tap then meets a finite number).
// Sums: a workgroup's two map sums go to the workspace as doubles and the level's last workgroup to arrive adds them (wg_reduce.h; one
// counter per level).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssim_blur.h"
#include "ssim_kernels.h"
#include "wg_reduce.h"

namespace sstem {

namespace {

constexpr int T = 32;                           // tile edge, both kernels
constexpr int HALO = SSIM_TAPS - 1;             // 10
constexpr int FE = T + HALO;                    // forward: staged image extent, 42
constexpr int BM = T + HALO;                    // backward: map extent a tile's adjoint blur reads, 42
constexpr int BE = BM + HALO;                   // backward: staged image extent, 52

// workspace header (float slots)
constexpr int HDR_VALUE = 0, HDR_TERMS = 2, HDR_COEF = 12, HDR_COUNTER = 20, HDR_IMG1 = 26, HDR_DTERMS = 32;

static_assert(SSIM_TAPS == SSIM_BLUR_TAPS, "one window length");     // Taps, stage_pair, make_taps: ssim_blur.h
struct Counts { double inv[SSIM_MAX_LEVELS]; };     // 1 / (B oh ow) per level

__device__ __forceinline__ float weight_of(int i)
{
    return i == 0 ? 0.0448f : i == 1 ? 0.2856f : i == 2 ? 0.3001f : i == 3 ? 0.2363f : 0.1333f;
}

// Forward of one level.  Workgroup = one 32 x 32 tile of one image's map (even origin, so it owns whole 2 x 2 pooling windows).
__global__ __launch_bounds__(256) void ms_ssim_level_fwd(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int oh, int ow,
                                                         int p, int tiles_x, int tiles, Taps taps, float C1, float C2,
                                                         float* __restrict__ nx, float* __restrict__ ny, int level, int levels, Counts counts,
                                                         float* ws, double* partials, float* value_out, float* terms_out,
                                                         unsigned long long img1_addr)
{
    __shared__ float sx[FE * FE], sy[FE * FE];
    __shared__ float hb[5][FE * T];
    __shared__ double red[4][2];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int Y0 = (t / tiles_x) * T, X0 = (t % tiles_x) * T;
    const int64_t base = (int64_t)b * h * w;

    stage_pair<FE>(x, y, base, h, w, Y0 - p, X0 - p, sx, sy);
    __syncthreads();

    for (int e = tid; e < FE * T; e += 256) {
        const int r = e / T, c = e - r * T;
        float m1 = 0.f, m2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            const float a = sx[r * FE + c + k], bb = sy[r * FE + c + k], g = taps.g[k];
            m1 = fmaf(g, a, m1); m2 = fmaf(g, bb, m2);
            s11 = fmaf(g, a * a, s11); s22 = fmaf(g, bb * bb, s22); s12 = fmaf(g, a * bb, s12);
        }
        hb[0][e] = m1; hb[1][e] = m2; hb[2][e] = s11; hb[3][e] = s22; hb[4][e] = s12;
    }
    __syncthreads();

    const int tx = tid & 31, ty = tid >> 5;
    double sum_ssim = 0.0, sum_mcs = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ly = ty + 8 * i;
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_TAPS; ++k) s = fmaf(taps.g[k], hb[q][(ly + k) * T + tx], s);
            v[q] = s;
        }
        if (Y0 + ly < oh && X0 + tx < ow) {
            const float mu1 = v[0], mu2 = v[1];
            const float m12 = mu1 * mu2, m11 = mu1 * mu1, m22 = mu2 * mu2;
            const float A1 = 2.f * m12 + C1, A2 = 2.f * (v[4] - m12) + C2;
            const float B1 = m11 + m22 + C1, B2 = (v[2] - m11) + (v[3] - m22) + C2;
            sum_mcs += (double)(A2 / B2);
            sum_ssim += (double)((A1 * A2) / (B1 * B2));
        }
    }

    // the next level's tile of both images: one pooled pixel per thread, from the staged tile
    if (nx) {
        const int py = tid >> 4, px = tid & 15;
        const int nh = h >> 1, nw = w >> 1;
        const int gy = (Y0 >> 1) + py, gx = (X0 >> 1) + px;
        if (gy < nh && gx < nw) {
            const int l = (2 * py + p) * FE + 2 * px + p;
            const int64_t o = ((int64_t)b * nh + gy) * nw + gx;
            nx[o] = (((sx[l] + sx[l + 1]) + sx[l + FE]) + sx[l + FE + 1]) * 0.25f;
            ny[o] = (((sy[l] + sy[l + 1]) + sy[l + FE]) + sy[l + FE + 1]) * 0.25f;
        }
    }

    const double sums[2] = {sum_ssim, sum_mcs};
    block_sum(sums, red);
    unsigned* counter = reinterpret_cast<unsigned*>(ws + HDR_COUNTER) + level;
    if (tid == 0) {
        agent_store(partials + 2 * (int64_t)blockIdx.x, block_tree(red, 0));
        agent_store(partials + 2 * (int64_t)blockIdx.x + 1, block_tree(red, 1));
    }
    if (!arrive_last(counter)) return;

    // the last workgroup of the level: every thread adds partials in index order, then the fixed tree
    block_total(partials, gridDim.x, red);
    if (tid != 0) return;
    double* dterms = reinterpret_cast<double*>(ws + HDR_DTERMS);
    const double mean_ssim = block_tree(red, 0) * counts.inv[level];
    const double mean_mcs = block_tree(red, 1) * counts.inv[level];
    dterms[2 * level] = mean_ssim; dterms[2 * level + 1] = mean_mcs;
    ws[HDR_TERMS + 2 * level] = (float)mean_ssim; ws[HDR_TERMS + 2 * level + 1] = (float)mean_mcs;
    if (terms_out) { terms_out[2 * level] = (float)mean_ssim; terms_out[2 * level + 1] = (float)mean_mcs; }
    if (level == 0) *reinterpret_cast<unsigned long long*>(ws + HDR_IMG1) = img1_addr;     // which image the first pyramid belongs to
    release_counter(counter);
    if (level != levels - 1) return;
    // the value and every level's coefficient; a non-positive mean gives NaN, as in the reference
    double term[SSIM_MAX_LEVELS];
    double value = 1.0;
#pragma unroll
    for (int i = 0; i < SSIM_MAX_LEVELS; ++i) {
        if (i < levels) {
            term[i] = i == level ? (i == levels - 1 ? mean_ssim : mean_mcs) : agent_load(dterms + 2 * i + 1);
            value *= pow(term[i], (double)weight_of(i));
        }
    }
#pragma unroll
    for (int i = 0; i < SSIM_MAX_LEVELS; ++i)
        if (i < levels) ws[HDR_COEF + i] = (float)((double)weight_of(i) * value / term[i] * counts.inv[i]);
    ws[HDR_VALUE] = (float)value;
    *value_out = (float)value;
}

// Backward of one level.  Workgroup = one 32 x 32 tile of one image; it recomputes the blurred quantities on the 42 x 42 map points its
// adjoint blur reads (from a 52 x 52 staged window), forms (a, b, c) there, blurs them back and adds the coarser level's share.
// first / second: the level's images in the forward's order; which of them is "x" here follows from the address the forward recorded
// (the gradient for the forward's second image is this launch with the operands exchanged).
__global__ __launch_bounds__(256) void ms_ssim_level_bwd(const float* __restrict__ first, const float* __restrict__ second, int h, int w, int oh,
                                                         int ow, int p, int tiles_x, int tiles, Taps taps, float C1, float C2, int level,
                                                         int use_ssim, const float* __restrict__ gcoarse, const float* __restrict__ grad_value,
                                                         float* __restrict__ gout, const float* __restrict__ ws, unsigned long long img1_addr)
{
    constexpr int A_FLOATS = 2 * BE * BE > 3 * BM * BM ? 2 * BE * BE : 3 * BM * BM;
    constexpr int B_FLOATS = 5 * BE * BM;          // > 3 * BM * T
    __shared__ float ra[A_FLOATS];
    __shared__ float rb[B_FLOATS];
    float* sx = ra;
    float* sy = ra + BE * BE;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int Y0 = (t / tiles_x) * T, X0 = (t % tiles_x) * T;
    const int64_t base = (int64_t)b * h * w;
    const bool swapped = level > 0 && *reinterpret_cast<const unsigned long long*>(ws + HDR_IMG1) != img1_addr;
    const float* x = swapped ? second : first;
    const float* y = swapped ? first : second;

    stage_pair<BE>(x, y, base, h, w, Y0 - HALO, X0 - HALO, sx, sy);
    __syncthreads();

    const int tx = tid & 31, ty = tid >> 5;
    float cx[4], cy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cx[i] = sx[(ty + 8 * i + HALO) * BE + tx + HALO];
        cy[i] = sy[(ty + 8 * i + HALO) * BE + tx + HALO];
    }
    for (int e = tid; e < BE * BM; e += 256) {
        const int r = e / BM, c = e - r * BM;
        float m1 = 0.f, m2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            const float a = sx[r * BE + c + k], bb = sy[r * BE + c + k], g = taps.g[k];
            m1 = fmaf(g, a, m1); m2 = fmaf(g, bb, m2);
            s11 = fmaf(g, a * a, s11); s22 = fmaf(g, bb * bb, s22); s12 = fmaf(g, a * bb, s12);
        }
        rb[e] = m1; rb[BE * BM + e] = m2; rb[2 * BE * BM + e] = s11; rb[3 * BE * BM + e] = s22; rb[4 * BE * BM + e] = s12;
    }
    __syncthreads();

    // the maps' derivatives on the 42 x 42 map points from (Y0 + p - 10, X0 + p - 10); zero outside the map
    float* ma = ra;
    float* mb = ra + BM * BM;
    float* mc = ra + 2 * BM * BM;
    for (int e = tid; e < BM * BM; e += 256) {
        const int m = e / BM, c = e - m * BM;
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_TAPS; ++k) s = fmaf(taps.g[k], rb[q * BE * BM + (m + k) * BM + c], s);
            v[q] = s;
        }
        const int oy = Y0 + p - HALO + m, ox = X0 + p - HALO + c;
        float da = 0.f, db = 0.f, dc = 0.f;
        if (oy >= 0 && oy < oh && ox >= 0 && ox < ow) {
            const float mu1 = v[0], mu2 = v[1];
            const float m12 = mu1 * mu2, m11 = mu1 * mu1, m22 = mu2 * mu2;
            const float A2 = 2.f * (v[4] - m12) + C2;
            const float B2 = (v[2] - m11) + (v[3] - m22) + C2;
            const float inv2 = 1.f / B2;
            const float mcs = A2 * inv2;
            da = 2.f * inv2 * (mu1 * mcs - mu2);          // d mcs / d mu1 = -2 mu2 / B2 + 2 mu1 A2 / B2^2
            db = -mcs * inv2;                             // d mcs / d e11
            dc = 2.f * inv2;                              // d mcs / d e12
            if (use_ssim) {
                const float A1 = 2.f * m12 + C1, B1 = m11 + m22 + C1;
                const float inv1 = 1.f / B1;
                const float r = A1 * inv1;
                da = 2.f * inv1 * (mu2 - mu1 * r) * mcs + r * da;
                db = r * db;
                dc = r * dc;
            }
        }
        ma[e] = da; mb[e] = db; mc[e] = dc;
    }
    __syncthreads();

    // adjoint blur, rows first: map column of image column j and tap k is (j - X0) + 10 - k
    for (int e = tid; e < BM * T; e += 256) {
        const int m = e / T, c = e - m * T;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            const int l = m * BM + c + HALO - k;
            const float g = taps.g[k];
            s0 = fmaf(g, ma[l], s0); s1 = fmaf(g, mb[l], s1); s2 = fmaf(g, mc[l], s2);
        }
        rb[e] = s0; rb[BM * T + e] = s1; rb[2 * BM * T + e] = s2;
    }
    __syncthreads();

    const float gv = grad_value ? *grad_value : 1.f;
    const float coef = ws[HDR_COEF + level] * gv;
    const int ch = h >> 1, cw = w >> 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ly = ty + 8 * i;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            const int l = (ly + HALO - k) * T + tx;
            const float g = taps.g[k];
            s0 = fmaf(g, rb[l], s0); s1 = fmaf(g, rb[BM * T + l], s1); s2 = fmaf(g, rb[2 * BM * T + l], s2);
        }
        const int jy = Y0 + ly, jx = X0 + tx;
        if (jy < h && jx < w) {
            float gr = coef * (s0 + 2.f * cx[i] * s1 + cy[i] * s2);
            if (gcoarse && jy < 2 * ch && jx < 2 * cw) gr += 0.25f * gcoarse[((int64_t)b * ch + (jy >> 1)) * cw + (jx >> 1)];
            gout[base + (int64_t)jy * w + jx] = gr;
        }
    }
}

}  // namespace

bool ms_ssim_plan(int64_t B, int64_t H, int64_t W, int levels, SsimPlan* plan)
{
    if (B < 0 || H < 1 || W < 1 || levels < 1 || levels > SSIM_MAX_LEVELS) return false;
    if (H > (1 << 15) || W > (1 << 15) || B > ((int64_t)1 << 24)) return false;
    SsimPlan pl = {};
    pl.levels = levels;
    int64_t off = SSIM_HEADER_FLOATS, max_wgs = 0;
    int h = (int)H, w = (int)W;
    for (int i = 0; i < levels; ++i) {
        if (h < 1 || w < 1) return false;
        pl.h[i] = h; pl.w[i] = w;
        const int ws = h < w ? (h < SSIM_TAPS ? h : SSIM_TAPS) : (w < SSIM_TAPS ? w : SSIM_TAPS);
        pl.ws[i] = ws;
        pl.oh[i] = h + 2 * (ws / 2) - ws + 1; pl.ow[i] = w + 2 * (ws / 2) - ws + 1;
        pl.tiles_x[i] = (pl.ow[i] + 31) / 32; pl.tiles[i] = pl.tiles_x[i] * ((pl.oh[i] + 31) / 32);
        pl.btiles_x[i] = (w + 31) / 32; pl.btiles[i] = pl.btiles_x[i] * ((h + 31) / 32);
        const int64_t wgs = B * pl.tiles[i];
        if (wgs > ((int64_t)1 << 24)) return false;          // one grid dimension, and the partials the last workgroup adds
        if (wgs > max_wgs) max_wgs = wgs;
        h >>= 1; w >>= 1;
    }
    pl.off_partials = off;                                   // 64 floats in: 8-byte aligned
    off += 4 * (max_wgs > 0 ? max_wgs : 1);
    for (int i = 1; i < levels; ++i) {
        const int64_t n = B * pl.h[i] * pl.w[i];
        pl.off_a[i] = off; pl.off_b[i] = off + n; pl.off_g[i] = off + 2 * n;
        off += 3 * n;
    }
    pl.total_floats = off;
    *plan = pl;
    return true;
}

static Counts make_counts(int64_t B, const SsimPlan& plan)
{
    Counts c = {};
    for (int i = 0; i < plan.levels; ++i) c.inv[i] = 1.0 / ((double)B * plan.oh[i] * plan.ow[i]);
    return c;
}

hipError_t launch_ms_ssim_forward(const float* img1, const float* img2, int64_t B, const SsimPlan& plan, float max_val, float* value,
                                  float* terms, float* ws, hipStream_t s)
{
    const float C1 = (float)((0.01 * max_val) * (0.01 * max_val)), C2 = (float)((0.03 * max_val) * (0.03 * max_val));
    const Counts counts = make_counts(B, plan);
    double* partials = reinterpret_cast<double*>(ws + plan.off_partials);
    for (int i = 0; i < plan.levels; ++i) {
        const float* x = i == 0 ? img1 : ws + plan.off_a[i];
        const float* y = i == 0 ? img2 : ws + plan.off_b[i];
        const bool more = i + 1 < plan.levels;
        float* nx = more ? ws + plan.off_a[i + 1] : nullptr;
        float* ny = more ? ws + plan.off_b[i + 1] : nullptr;
        hipLaunchKernelGGL(ms_ssim_level_fwd, dim3((unsigned)(B * plan.tiles[i])), dim3(256), 0, s, x, y, plan.h[i], plan.w[i], plan.oh[i],
                           plan.ow[i], plan.ws[i] / 2, plan.tiles_x[i], plan.tiles[i], make_taps(plan.ws[i]), C1, C2, nx, ny, i, plan.levels,
                           counts, ws, partials, value, terms, (unsigned long long)reinterpret_cast<uintptr_t>(img1));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_ms_ssim_backward(const float* img1, const float* img2, int64_t B, const SsimPlan& plan, float max_val,
                                   const float* grad_value, float* grad_img1, float* ws, hipStream_t s)
{
    const float C1 = (float)((0.01 * max_val) * (0.01 * max_val)), C2 = (float)((0.03 * max_val) * (0.03 * max_val));
    for (int i = plan.levels - 1; i >= 0; --i) {
        const float* first = i == 0 ? img1 : ws + plan.off_a[i];
        const float* second = i == 0 ? img2 : ws + plan.off_b[i];
        const float* gcoarse = i + 1 < plan.levels ? ws + plan.off_g[i + 1] : nullptr;
        float* gout = i == 0 ? grad_img1 : ws + plan.off_g[i];
        hipLaunchKernelGGL(ms_ssim_level_bwd, dim3((unsigned)(B * plan.btiles[i])), dim3(256), 0, s, first, second, plan.h[i], plan.w[i],
                           plan.oh[i], plan.ow[i], plan.ws[i] / 2, plan.btiles_x[i], plan.btiles[i], make_taps(plan.ws[i]), C1, C2, i,
                           i == plan.levels - 1 ? 1 : 0, gcoarse, grad_value, gout, ws,
                           (unsigned long long)reinterpret_cast<uintptr_t>(img1));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sstem
