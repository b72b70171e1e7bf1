#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

constexpr int SCORE_TAPS = 11;                 // compute_ssim's win_size; the 'valid' map is (H - 10) x (W - 10)
constexpr int SCORE_TILE_W = 32, SCORE_TILE_H = 16;
constexpr int SCORE_MAX_CHUNKS = 64;           // workgroups per image of the statistics launch
constexpr int SCORE_EPE_MAX_WGS = 1024;        // workgroups of the end-point-error launch

// Where everything sits in the workspace (bytes; host only, no HIP call).  One workspace serves the image scores and the end-point error
// of one (B, H, W): the image part is empty when H or W is below 11 (no 'valid' map there; the end-point error has no such floor).
struct ScorePlan {
    int chunks;                                // statistics launch: workgroups per image
    int tiles_x, tiles;                        // map launch: 32 x 16 tiles per image (0 below 11 x 11)
    int epe_wgs;                               // end-point-error launch: workgroups in all
    int64_t off_epe_partials;                  // doubles: {sum, kept} per workgroup; the launches' three counters are the workspace's first words
    int64_t off_unit_range;                    // one int per image: both maxima <= 1, left by the statistics launch for the map launch
    int64_t off_stat_partials;                 // doubles: {max a, max b, sum (a - b)^2, sum (a / 255 - b / 255)^2} per workgroup
    int64_t off_map_partials;                  // doubles: one per tile
    int64_t total_bytes;
};

// false: sizes the kernels cannot index (negative, H or W above 32768, B above 2^24, more than 2^24 tiles)
bool score_plan(int64_t B, int64_t H, int64_t W, ScorePlan* plan);

// scores[B][3] = {mse, psnr, ssim}; two launches (statistics, then the map, which reads the range flag the first one left)
template <class T>
hipError_t launch_score_images(const T* a, const T* b, int64_t B, int64_t H, int64_t W, const ScorePlan& plan, int clamp01_a, double* scores,
                               void* ws, hipStream_t s);

hipError_t launch_flow_epe(const float* flow, const float* target, int64_t B, int64_t H, int64_t W, const ScorePlan& plan, int sparse, int mean,
                           double* value, void* ws, hipStream_t s);
}
