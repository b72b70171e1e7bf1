#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

constexpr int SSIM_MAX_LEVELS = 5;
constexpr int SSIM_TAPS = 11;            // the longest window; shorter ones are zero-padded to it
constexpr int SSIM_HEADER_FLOATS = 64;   // value, terms, coefficients, counters, the forward's img1 address, the means in double

// What a call of given sizes does, level by level; everything the launchers and the workspace query need (host only, no HIP call).
struct SsimPlan {
    int levels;
    int h[SSIM_MAX_LEVELS], w[SSIM_MAX_LEVELS];          // level images
    int ws[SSIM_MAX_LEVELS];                             // window length min(h, w, 11)
    int oh[SSIM_MAX_LEVELS], ow[SSIM_MAX_LEVELS];        // map extent h + 2 (ws / 2) - ws + 1: one larger than the image for even ws
    int tiles_x[SSIM_MAX_LEVELS], tiles[SSIM_MAX_LEVELS];          // forward: 32 x 32 tiles of the map, per image
    int btiles_x[SSIM_MAX_LEVELS], btiles[SSIM_MAX_LEVELS];        // backward: 32 x 32 tiles of the image, per image
    int64_t off_a[SSIM_MAX_LEVELS], off_b[SSIM_MAX_LEVELS], off_g[SSIM_MAX_LEVELS];   // pyramids of both images and of the gradient (levels >= 1)
    int64_t off_partials;                                // doubles, two per workgroup of the largest level
    int64_t total_floats;
};

// false: sizes the kernels cannot index (the plan is then not to be used)
bool ms_ssim_plan(int64_t B, int64_t H, int64_t W, int levels, SsimPlan* plan);

hipError_t launch_ms_ssim_forward(const float* img1, const float* img2, int64_t B, const SsimPlan& plan, float max_val, float* value,
                                  float* terms, float* ws, hipStream_t s);
hipError_t launch_ms_ssim_backward(const float* img1, const float* img2, int64_t B, const SsimPlan& plan, float max_val,
                                   const float* grad_value, float* grad_img1, float* ws, hipStream_t s);
}
