#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {
hipError_t launch_warp_bilinear(const float* img, const float* flow, float* out, int B, int C, int H, int W,
                                hipStream_t s);
// gflow / gimg: either may be null (not both); img is read only for gflow.  gimg is cleared on the stream unless accumulate_image.
// gflow repeats bit for bit; gimg is summed by fp32 atomics in no fixed order, so its last bits can differ from run to run.
hipError_t launch_warp_bilinear_backward(const float* img, const float* flow, const float* gout, float* gflow, float* gimg,
                                         int accumulate_image, int B, int C, int H, int W, hipStream_t s);
}
