#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

constexpr int SSIM_LOSS_HEADER_FLOATS = 16;   // the launch counter (word 0); the partial sums start 64 bytes in

// What a call of given sizes does; everything the launchers and the workspace query need (host only, no HIP call).
struct SsimLossPlan {
    int64_t planes;               // B * C
    int h, w;
    int tiles_x, tiles;           // 32 x 32 tiles per plane (the map has the image's extent)
    int64_t wgs;                  // planes * tiles: one workgroup each, forward and backward
    int64_t wgs_per_sample;       // C * tiles
    int64_t total_floats;
};

// false: sizes the kernels cannot index (negative, H or W above 32768, B or C above 2^24, more than 2^24 tiles) or an empty tensor
bool ssim_loss_plan(int64_t B, int64_t C, int64_t H, int64_t W, SsimLossPlan* plan);

hipError_t launch_ssim_loss_forward(const float* img1, const float* img2, int64_t B, const SsimLossPlan& plan, int per_sample, float* value,
                                    float* ws, hipStream_t s);
hipError_t launch_ssim_loss_backward(const float* img1, const float* img2, int64_t B, const SsimLossPlan& plan, int per_sample,
                                     const float* grad_value, float* grad_img1, hipStream_t s);
}
