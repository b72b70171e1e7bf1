// Training crops from device-resident sections (include/sstem_batch.h): one oriented gather for the three training loops.
//
// Replaces the first host step of every training sample of the reference (sff_scripts_interp/data/data_provider.py:103-141,
// sff_scripts_fusion/data/data_provider.py:115-135, sp_scripts_train/dataset.py:161-171,217-236): the crop of each uint8 plane, its
// fliplr / flipud / transpose / rot90, the replication to channels and astype(np.float32) / 255.0 -- and with it the upload of the batch.
// A byte permutation, so no arithmetic but the one division; what matters is that both sides of the copy run along rows:
//   - one workgroup owns a 64 x 64-byte OUTPUT tile of one (sample, plane);
//   - it reads the SOURCE tile that maps onto it along source rows (the window origin is arbitrary, so those rows are not dword-aligned:
//     consecutive lanes read consecutive bytes) into LDS;
//   - it writes along output rows, reading the tile forwards, backwards or by columns as the code says.  The tile's pitch is padded so
//     that the column walk of each store path spreads over the banks (see PITCH below);
//   - the same path serves all eight codes; the fp32 entry converts on the way out and stores every channel of the plane from the one tile.
// 256 threads, a stride walk over (sample, plane, tile) under a capped grid, 64-bit offsets into the pool and the outputs, plain C++.
// A batch is 1-5 MB: the launch is most of its time, nothing here is tuned beyond the coalescing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sstem_batch.h"
#include "batch_kernels.h"

namespace sstem {

namespace {

constexpr int TILE = 64;
constexpr int BATCH_GRID_CAP = 4096;     // workgroups per launch: 16 per CU; larger problems walk by the grid's stride

// Byte pitch of the staged tile.  LDS byte reads bank by (address / 4) % 32 within a 32-lane half.
//   fp32 stores: a lane per output column, so a transposing read walks tile rows lane by lane: 17 dwords a row puts 32 lanes on 32 banks.
//   uint8 stores: a lane per output dword, so it walks four tile rows lane by lane: 65 bytes a row makes that step 65 dwords, odd again.
constexpr int PITCH_F32 = 68;
constexpr int PITCH_U8 = 65;

// the channel map of the fp32 entry, passed by value
struct ChanMap {
    int8_t plane[SSTEM_BATCH_MAX_CHANNELS];
    int c0, c1;
    uint32_t invert;                     // bit c: channel c stores 255 - byte
    uint32_t used;                       // bit p: some channel reads plane p
};

// what one workgroup needs of its (sample, plane, tile); everything block-uniform
struct TileJob {
    int i, p;                            // sample, plane
    int oy0, ox0, th, tw;                // the output tile inside the S_h x S_w window
    int fu, fl, tr;                      // the code's bits
};

// The sample's row and its P images: false when it must write nothing (include/sstem_batch.h).  oy, ox, code are its row.
__device__ __forceinline__ bool sample_ok(const int64_t* __restrict__ images, int n_images, const int32_t* __restrict__ samples,
                                          const int32_t* __restrict__ plane_image, int i, int P, int SH, int SW, int& oy, int& ox, int& code)
{
    const int32_t* s = samples + (int64_t)i * SSTEM_BATCH_SAMPLE_FIELDS;
    oy = s[0]; ox = s[1]; code = s[2];
    if (code < 0 || code > 7 || oy < 0 || ox < 0) return false;
    if ((code & SSTEM_ORIENT_TRANSPOSE) && SH != SW) return false;
    for (int q = 0; q < P; ++q) {
        const int id = plane_image[(int64_t)i * P + q];
        if (id < 0 || id >= n_images) return false;
        const int64_t* im = images + (int64_t)id * SSTEM_BATCH_IMAGE_FIELDS;
        if ((int64_t)oy + SH > im[1] || (int64_t)ox + SW > im[2]) return false;
    }
    return true;
}

// item -> (sample, plane, tile), plane-minor so that a sample's row is checked by neighbouring workgroups
__device__ __forceinline__ TileJob decode(int64_t item, int P, int tiles_y, int tiles_x, int SH, int SW)
{
    TileJob j;
    const int64_t tiles = (int64_t)tiles_y * tiles_x;
    const int64_t sp = item / tiles;
    const int t = (int)(item - sp * tiles);
    j.i = (int)(sp / P);
    j.p = (int)(sp - (int64_t)j.i * P);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    j.oy0 = ty * TILE; j.ox0 = tx * TILE;
    j.th = SH - j.oy0 < TILE ? SH - j.oy0 : TILE;
    j.tw = SW - j.ox0 < TILE ? SW - j.ox0 : TILE;
    j.fu = j.fl = j.tr = 0;
    return j;
}

// Stages the source tile of job j along source rows.  out[y][x] = window[a][b], or window[b][a] transposed, with a = y or S_h - 1 - y and
// b = x or S_w - 1 - x: the output tile's rows map onto window rows a0 .. a0 + th (columns b0 .. b0 + tw), those are source rows unless
// the code transposes, when they are source columns.
template <int PITCH>
__device__ __forceinline__ void stage(uint8_t* __restrict__ tile, const uint8_t* __restrict__ pool, const int64_t* __restrict__ image,
                                      const TileJob& j, int oy, int ox, int SH, int SW)
{
    const int a0 = j.fu ? SH - j.oy0 - j.th : j.oy0;
    const int b0 = j.fl ? SW - j.ox0 - j.tw : j.ox0;
    const int r0 = j.tr ? b0 : a0, c0 = j.tr ? a0 : b0, rows = j.tr ? j.tw : j.th, cols = j.tr ? j.th : j.tw;
    const int64_t W = image[2];
    const uint8_t* src = pool + image[0] + (int64_t)(oy + r0) * W + (ox + c0);
    const int lane = threadIdx.x & 63;
    if (lane < cols)
        for (int r = threadIdx.x >> 6; r < rows; r += 4) tile[r * PITCH + lane] = src[(int64_t)r * W + lane];
}

// the staged byte of output pixel (y, x) of the tile
template <int PITCH>
__device__ __forceinline__ uint8_t staged(const uint8_t* __restrict__ tile, const TileJob& j, int y, int x)
{
    const int la = j.fu ? j.th - 1 - y : y, lb = j.fl ? j.tw - 1 - x : x;
    return j.tr ? tile[lb * PITCH + la] : tile[la * PITCH + lb];
}

__global__ __launch_bounds__(256) void crop_orient_u8(const uint8_t* __restrict__ pool, const int64_t* __restrict__ images, int n_images,
                                                      const int32_t* __restrict__ samples, const int32_t* __restrict__ plane_image, int n, int P,
                                                      int SH, int SW, int tiles_y, int tiles_x, uint8_t* __restrict__ out)
{
    __shared__ uint8_t tile[TILE * PITCH_U8];
    const int64_t items = (int64_t)n * P * tiles_y * tiles_x;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        TileJob j = decode(item, P, tiles_y, tiles_x, SH, SW);
        int oy, ox, code;
        if (!sample_ok(images, n_images, samples, plane_image, j.i, P, SH, SW, oy, ox, code)) continue;      // block-uniform
        j.fl = code & SSTEM_ORIENT_FLIPLR; j.fu = code & SSTEM_ORIENT_FLIPUD; j.tr = code & SSTEM_ORIENT_TRANSPOSE;
        const int64_t* image = images + (int64_t)plane_image[(int64_t)j.i * P + j.p] * SSTEM_BATCH_IMAGE_FIELDS;
        stage<PITCH_U8>(tile, pool, image, j, oy, ox, SH, SW);
        __syncthreads();
        // a thread per output dword: 16 across a tile row, 16 rows a pass
        const int x = (threadIdx.x & 15) * 4;
        uint8_t* plane = out + ((int64_t)j.p * n + j.i) * SH * SW;
        if (x < j.tw)
            for (int y = threadIdx.x >> 4; y < j.th; y += 16) {
                uint8_t* dst = plane + (int64_t)(j.oy0 + y) * SW + (j.ox0 + x);
                if (x + 3 < j.tw && ((uintptr_t)dst & 3) == 0) {
                    const uint32_t v = (uint32_t)staged<PITCH_U8>(tile, j, y, x) | ((uint32_t)staged<PITCH_U8>(tile, j, y, x + 1) << 8) |
                                       ((uint32_t)staged<PITCH_U8>(tile, j, y, x + 2) << 16) | ((uint32_t)staged<PITCH_U8>(tile, j, y, x + 3) << 24);
                    *reinterpret_cast<uint32_t*>(dst) = v;
                } else {
                    for (int k = 0; k < 4 && x + k < j.tw; ++k) dst[k] = staged<PITCH_U8>(tile, j, y, x + k);
                }
            }
        __syncthreads();                                                     // the tile is free for the next item
    }
}

__global__ __launch_bounds__(256) void crop_orient_f32(const uint8_t* __restrict__ pool, const int64_t* __restrict__ images, int n_images,
                                                       const int32_t* __restrict__ samples, const int32_t* __restrict__ plane_image, int n, int P,
                                                       int SH, int SW, int tiles_y, int tiles_x, ChanMap chan, float* __restrict__ out0,
                                                       float* __restrict__ out1)
{
    __shared__ uint8_t tile[TILE * PITCH_F32];
    const int64_t items = (int64_t)n * P * tiles_y * tiles_x;
    const int64_t win = (int64_t)SH * SW;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        TileJob j = decode(item, P, tiles_y, tiles_x, SH, SW);
        if (!((chan.used >> j.p) & 1u)) continue;                            // no channel reads this plane
        int oy, ox, code;
        if (!sample_ok(images, n_images, samples, plane_image, j.i, P, SH, SW, oy, ox, code)) continue;      // block-uniform
        j.fl = code & SSTEM_ORIENT_FLIPLR; j.fu = code & SSTEM_ORIENT_FLIPUD; j.tr = code & SSTEM_ORIENT_TRANSPOSE;
        const int64_t* image = images + (int64_t)plane_image[(int64_t)j.i * P + j.p] * SSTEM_BATCH_IMAGE_FIELDS;
        stage<PITCH_F32>(tile, pool, image, j, oy, ox, SH, SW);
        __syncthreads();
        // a lane per output column, 4 rows a pass: a wave stores 256 consecutive bytes per channel
        const int x = threadIdx.x & 63;
        if (x < j.tw)
            for (int y = threadIdx.x >> 6; y < j.th; y += 4) {
                const int b = staged<PITCH_F32>(tile, j, y, x);
                const float v = __fdiv_rn((float)b, 255.0f), r = __fdiv_rn((float)(255 - b), 255.0f);
                const int64_t q = (int64_t)(j.oy0 + y) * SW + (j.ox0 + x);
                for (int c = 0; c < chan.c0 + chan.c1; ++c) {
                    if (chan.plane[c] != j.p) continue;
                    float* dst = c < chan.c0 ? out0 + ((int64_t)j.i * chan.c0 + c) * win : out1 + ((int64_t)j.i * chan.c1 + (c - chan.c0)) * win;
                    dst[q] = ((chan.invert >> c) & 1u) ? r : v;
                }
            }
        __syncthreads();                                                     // the tile is free for the next item
    }
}

// tiles of the window and the capped grid over (sample, plane, tile)
unsigned batch_grid(int n, int P, int SH, int SW, int& tiles_y, int& tiles_x)
{
    tiles_y = (SH + TILE - 1) / TILE;
    tiles_x = (SW + TILE - 1) / TILE;
    const int64_t items = (int64_t)n * P * tiles_y * tiles_x;
    return (unsigned)(items < BATCH_GRID_CAP ? items : BATCH_GRID_CAP);
}

}  // namespace

hipError_t launch_crop_orient_u8(const uint8_t* pool, const int64_t* images, int n_images, const int32_t* samples, const int32_t* plane_image,
                                 int n, int P, int SH, int SW, uint8_t* out, hipStream_t s)
{
    int tiles_y, tiles_x;
    const unsigned grid = batch_grid(n, P, SH, SW, tiles_y, tiles_x);
    hipLaunchKernelGGL(crop_orient_u8, dim3(grid), dim3(256), 0, s, pool, images, n_images, samples, plane_image, n, P, SH, SW, tiles_y, tiles_x,
                       out);
    return hipGetLastError();
}

hipError_t launch_crop_orient_f32(const uint8_t* pool, const int64_t* images, int n_images, const int32_t* samples, const int32_t* plane_image,
                                  int n, int P, int SH, int SW, const int32_t* chan_plane, int C0, int C1, uint32_t chan_invert, float* out0,
                                  float* out1, hipStream_t s)
{
    ChanMap chan = {};
    chan.c0 = C0; chan.c1 = C1; chan.invert = chan_invert;
    for (int c = 0; c < C0 + C1; ++c) {
        chan.plane[c] = (int8_t)chan_plane[c];
        chan.used |= 1u << chan_plane[c];
    }
    int tiles_y, tiles_x;
    const unsigned grid = batch_grid(n, P, SH, SW, tiles_y, tiles_x);
    hipLaunchKernelGGL(crop_orient_f32, dim3(grid), dim3(256), 0, s, pool, images, n_images, samples, plane_image, n, P, SH, SW, tiles_y, tiles_x,
                       chan, out0, out1);
    return hipGetLastError();
}

}  // namespace sstem
