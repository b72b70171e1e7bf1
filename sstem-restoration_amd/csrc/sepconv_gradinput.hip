// Input gradient of the separable local convolution for MI355X (gfx950 / CDNA4).  The reference's backward launcher
// (libs/sepconv/src/SeparableConvolution_kernel.cu:152-206) never writes gradInput; this is the library's own addition.
//
//     gI[b,c,Y,X] = sum_{fy,fx} g[b,c,Y-fy,X-fx] * V[b,fy;Y-fy,X-fx] * H[b,fx;Y-fy,X-fx]      (source pixel inside the image)
//
// ONE order for both kernels (sepconv_kernels.h): source rows y = Y-fy ascending, source columns x = X-fx ascending inside a
// row, one chain  acc = fmaf(V, fl(g * H), acc)  from +0.
//
// Tiled kernel: the adjoint of the forward's banded product.  For one source row y and a block of four target columns
// X_b..X_b+3, step t (source column x = X_b - 50 + t, t < 54) is the 4x4x1 product
//     D[i, j] += A[i] * B[j],   A[i] = V[Yg + i - y; y, x]  (target row Yg + i),   B[j] = g[c; y, x] * H[50 - t + j; y, x]
// -- one block of v_mfma_f32_4x4x1_16b_f32, 16 blocks = 64 target columns per instruction, each product one fmaf.  Taps outside
// 0..50 are zero rows of the LDS image, so off-band steps add A * 0 or 0 * B and leave the chain's value alone
// (finite data; an accumulator that has underflowed to -0 becomes +0, the one place where the direct kernel, which skips them, differs).  B is shared by the
// wave's four target-row groups; A by the channels.  A workgroup owns a 64 x 64 tile of the padded plane: wave w rows 16w..16w+15 as
// four groups of four, whose accumulators stay in registers while the workgroup walks the source rows y0-50 .. y0+63 that reach the
// tile.  One source row (51 V taps, 51 H taps, C rows of g, 114 columns) is staged per step into a double-buffered LDS image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sepconv_kernels.h"

namespace sstem {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// Direct kernel: one lane per grad_input element; any C, any filter length; 64-bit indexing.
// ---------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(256) void sepconv_gradinput_direct(
    const float* __restrict__ g, const float* __restrict__ ver, const float* __restrict__ hor, float* __restrict__ gi,
    int64_t B, int64_t C, int64_t H, int64_t W, int filt)
{
    const int64_t plane = H * W;
    const int64_t Hin = H + filt - 1, Win = W + filt - 1;
    const int64_t pin = Hin * Win;
    const int64_t n = B * C * pin;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bc = p / pin;
        const int64_t r = p - bc * pin;
        const int64_t Y = r / Win, X = r - Y * Win;
        const int64_t b = bc / C;
        const int64_t ylo = Y - (filt - 1) > 0 ? Y - (filt - 1) : 0, yhi = Y < H - 1 ? Y : H - 1;
        const int64_t xlo = X - (filt - 1) > 0 ? X - (filt - 1) : 0, xhi = X < W - 1 ? X : W - 1;
        const float* gp = g + bc * plane;
        const int64_t cb = b * filt * plane;
        float acc = 0.f;
        for (int64_t y = ylo; y <= yhi; ++y) {
            const int64_t vrow = cb + (Y - y) * plane + y * W;     // V[Y-y; y, .]
            for (int64_t x = xlo; x <= xhi; ++x) {
                const float gh = gp[y * W + x] * coef_at<BF>(hor, cb + (X - x) * plane + y * W + x);
                acc = fmaf(coef_at<BF>(ver, vrow + x), gh, acc);
            }
        }
        gi[p] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// Tiled kernel
// ---------------------------------------------------------------------------------------------
constexpr int F = 51;
constexpr int KSTEPS = 54;          // 51 taps + 3 skew positions of a 4-column block
constexpr int TS = 64;              // tile side, in grad_input elements
constexpr int COLS = TS + F - 1;    // 114 source columns reach a tile
constexpr int TAPROWS = F + 6;      // taps -3 .. 53; the six outside 0..50 stay zero
// Row pitch 117 = 1 (mod 4): the A read (lane (i, k): tap row d + i, column 4k + t) and the B read (tap row 50 - t + j, column
// 4k + t) both hit dword (row0 + i) * 117 + 4k + const -- i * 117 = i (mod 4) and 4k cover the 64 banks once.
constexpr int PITCH = 117;
constexpr int IMG = TAPROWS * PITCH;                 // dwords of one coefficient image
constexpr int GPITCH = 116;
template <int CH> constexpr int buf_dwords() { return 2 * IMG + CH * GPITCH; }
template <int CH> constexpr size_t gi_lds_bytes() { return 2 * (size_t)buf_dwords<CH>() * sizeof(float); }

struct GiArgs {
    int64_t B, C, H, W;
    int64_t tiles_x, tiles_y;
    int c0;                          // first channel of this launch's chunk
};

template <int CH>
__global__ __launch_bounds__(256, 1) void sepconv_gradinput_mfma(
    const float* __restrict__ g, const float* __restrict__ ver, const float* __restrict__ hor, float* __restrict__ gi, GiArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int BUF = buf_dwords<CH>();
    constexpr int NCOEF = 2 * F * COLS;                       // staged coefficient dwords per source row
    constexpr int NLD = (NCOEF + 255) / 256;                  // per thread
    constexpr int NG = (CH * GPITCH + 255) / 256;             // staged g dwords per thread

    const int64_t per_img = a.tiles_y * a.tiles_x;
    const int64_t b = blockIdx.x / per_img;
    const int64_t tr = blockIdx.x - b * per_img;
    const int ty = (int)(tr / a.tiles_x), tx = (int)(tr - (int64_t)ty * a.tiles_x);
    const int H = (int)a.H, W = (int)a.W;                     // gradinput_tiled_ok: every in-image offset fits 32 bits
    const int Hin = H + F - 1, Win = W + F - 1;
    const uint32_t plane = (uint32_t)H * (uint32_t)W;
    const int Y0 = ty * TS, X0 = tx * TS;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = lane >> 2, sub = lane & 3;

    const float* vb = ver + b * (int64_t)F * plane;
    const float* hb = hor + b * (int64_t)F * plane;
    const float* gb = g + (b * a.C + a.c0) * (int64_t)plane;

    // zero both buffers once: the six tap rows outside 0..50 are never written again
    for (int i = tid; i < 2 * BUF; i += 256) lds[i] = 0.f;

    // my staging slots: element e = tid + 256 q of [2 tensors][51 taps][114 columns]
    // source column of slot column cx: X0 - 50 + cx
    const int ys = Y0 - (F - 1) > 0 ? Y0 - (F - 1) : 0;       // source rows that reach the tile, inside the image
    const int ye = Y0 + TS - 1 < H - 1 ? Y0 + TS - 1 : H - 1;

    float st[NLD];
    float sg[NG];
    auto fetch = [&](int y) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int e = tid + 256 * q;
            const int ten = e >= F * COLS;
            const int r = e - ten * (F * COLS);
            const int tap = r / COLS, cx = r - tap * COLS;
            const int x = X0 - (F - 1) + cx;
            const bool ok = e < NCOEF && x >= 0 && x < W;
            const float* src = ten ? hb : vb;
            st[q] = ok ? src[(uint32_t)tap * plane + (uint32_t)y * (uint32_t)W + (uint32_t)x] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            const int e = tid + 256 * q;
            const int c = e / GPITCH, cx = e - c * GPITCH;
            const int x = X0 - (F - 1) + cx;
            const bool ok = e < CH * GPITCH && cx < COLS && x >= 0 && x < W;
            sg[q] = ok ? gb[(uint32_t)c * plane + (uint32_t)y * (uint32_t)W + (uint32_t)x] : 0.f;
        }
    };
    auto stash = [&](float* buf) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int e = tid + 256 * q;
            const int ten = e >= F * COLS;
            const int r = e - ten * (F * COLS);
            const int tap = r / COLS, cx = r - tap * COLS;
            if (e < NCOEF) buf[ten * IMG + (tap + 3) * PITCH + cx] = st[q];
        }
#pragma unroll
        for (int q = 0; q < NG; ++q)
            if (tid + 256 * q < CH * GPITCH) buf[2 * IMG + tid + 256 * q] = sg[q];
    };

    f32x4 acc[4][CH];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[q][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (ys <= ye) fetch(ys);
    __syncthreads();                                          // the zero-fill is complete
    if (ys <= ye) stash(lds);
    __syncthreads();

#pragma unroll 1
    for (int y = ys; y <= ye; ++y) {
        const float* cur = lds + ((y - ys) & 1) * BUF;
        float* nxt = lds + ((y - ys + 1) & 1) * BUF;
        const bool more = y < ye;                             // uniform
        if (more) fetch(y + 1);

        const float* vimg = cur;
        const float* himg = cur + IMG;
        const float* grow = cur + 2 * IMG;
        // B: tap row (50 - t + sub) + 3, column 4 blk + t  ->  base + t * (1 - PITCH)
        const float* bp = himg + (F - 1 + 3 + sub) * PITCH + 4 * blk;
        const float* gp = grow + 4 * blk;
        // B operands of 18 steps at a time, once for the wave's four groups: 18 x CH registers (all 54 x 3 at once do not
        // fit beside the staging set and would be parked in AGPRs).  Per accumulator the steps still come in ascending t.
        constexpr int TB = 18, AQ = 6;
        static_assert(KSTEPS % TB == 0 && TB % AQ == 0, "chunks");
#pragma unroll 1
        for (int t0 = 0; t0 < KSTEPS; t0 += TB) {
            float bop[CH][TB];
#pragma unroll
            for (int u = 0; u < TB; ++u) {
                const float hv = bp[(t0 + u) * (1 - PITCH)];
#pragma unroll
                for (int c = 0; c < CH; ++c) bop[c][u] = gp[c * GPITCH + t0 + u] * hv;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // target rows Yg .. Yg+3; source row y reaches them iff d = Yg - y in [-3, 50]  (wave-uniform)
                const int d = Y0 + 16 * wave + 4 * q - y;
                if (d >= -3 && d <= F - 1) {
                    const float* ap = vimg + (d + sub + 3) * PITCH + 4 * blk + t0;
                    // A operand through a two-deep register ring, six steps at a time: the reads of the next six are in flight
                    // under the MFMAs of these six (one wave per SIMD: nothing else covers the LDS latency)
                    float ar[2][AQ];
#pragma unroll
                    for (int u = 0; u < AQ; ++u) ar[0][u] = ap[u];
#pragma unroll
                    for (int k = 0; k < TB / AQ; ++k) {
                        if (k + 1 < TB / AQ) {
#pragma unroll
                            for (int u = 0; u < AQ; ++u) ar[(k + 1) & 1][u] = ap[(k + 1) * AQ + u];
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int u = 0; u < AQ; ++u)
#pragma unroll
                            for (int c = 0; c < CH; ++c)
                                acc[q][c] = __builtin_amdgcn_mfma_f32_4x4x1f32(ar[k & 1][u], bop[c][k * AQ + u], acc[q][c], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
        if (more) stash(nxt);
        __syncthreads();
    }

    // D row i = register i, column = lane: 256-byte row stores
    const int X = X0 + lane;
    if (X < Win) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int Y = Y0 + 16 * wave + 4 * q + i;
                if (Y < Hin) {
#pragma unroll
                    for (int c = 0; c < CH; ++c)
                        gi[((b * a.C + a.c0 + c) * (int64_t)Hin + Y) * Win + X] = acc[q][c][i];
                }
            }
    }
}

inline int grid_1d(int64_t n, int threads)
{
    int64_t g = (n + threads - 1) / threads;
    const int64_t cap = 256 * 32;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

template <int CH>
hipError_t launch_chunk(const float* g, const float* ver, const float* hor, float* gi, const GiArgs& a, hipStream_t s)
{
    static_assert(gi_lds_bytes<CH>() <= 160 * 1024, "LDS");
    // above the 64 KB default: an idempotent attribute of the (kernel, current device) pair, set before every launch
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sepconv_gradinput_mfma<CH>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)gi_lds_bytes<CH>());
    if (e != hipSuccess) return e;
    const int64_t nwg = a.B * a.tiles_y * a.tiles_x;
    hipLaunchKernelGGL(sepconv_gradinput_mfma<CH>, dim3((unsigned)nwg), dim3(256), gi_lds_bytes<CH>(), s, g, ver, hor, gi, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gradinput_direct(const float* g, const float* ver, const float* hor, float* gi,
                                   int64_t B, int64_t C, int64_t H, int64_t W, int filt, bool bf16coef, hipStream_t s)
{
    const int grid = grid_1d(B * C * (H + filt - 1) * (W + filt - 1), 256);
    if (bf16coef)
        hipLaunchKernelGGL(sepconv_gradinput_direct<true>, dim3(grid), dim3(256), 0, s, g, ver, hor, gi, B, C, H, W, filt);
    else
        hipLaunchKernelGGL(sepconv_gradinput_direct<false>, dim3(grid), dim3(256), 0, s, g, ver, hor, gi, B, C, H, W, filt);
    return hipGetLastError();
}

bool gradinput_tiled_ok(int64_t B, int64_t C, int64_t H, int64_t W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1 || !mfma_grid_ok(B, H, W)) return false;
    const int64_t nwg = B * ((H + F - 1 + TS - 1) / TS) * ((W + F - 1 + TS - 1) / TS);
    if (nwg > 0x7fffffffLL) return false;
    // in-image offsets are 32-bit: one image's coefficient tensor stays below 4 GiB, sizes below 2^31 - 128
    return (__int128)F * H * W * 4 < ((__int128)1 << 32) && H + 128 < 0x7fffffffLL && W + 128 < 0x7fffffffLL;
}

hipError_t launch_gradinput_tiled(const float* g, const float* ver, const float* hor, float* gi,
                                  int64_t B, int64_t C, int64_t H, int64_t W, hipStream_t s)
{
    if (!gradinput_tiled_ok(B, C, H, W)) return hipErrorInvalidValue;
    GiArgs a;
    a.B = B; a.C = C; a.H = H; a.W = W;
    a.tiles_x = (W + F - 1 + TS - 1) / TS;
    a.tiles_y = (H + F - 1 + TS - 1) / TS;
    for (int64_t c0 = 0; c0 < C; c0 += 3) {                  // chunks of three channels, as TileArgs::c0 elsewhere
        a.c0 = (int)c0;
        const int64_t ch = C - c0 < 3 ? C - c0 : 3;
        const hipError_t e = ch == 3 ? launch_chunk<3>(g, ver, hor, gi, a, s)
                           : ch == 2 ? launch_chunk<2>(g, ver, hor, gi, a, s)
                                     : launch_chunk<1>(g, ver, hor, gi, a, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sstem
