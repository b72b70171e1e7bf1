#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {
constexpr int FLOW_MAXRAD_PARTS = 128;                                      // workspace words per image of the colour code
// include/sstem_display.h; sizes already checked by the entries (1 <= B <= 2^24, 1 <= plane = H * W <= 2^30)
const uint8_t* flow_color_wheel();                                           // [55][3], the host's copy of the kernel's table
hipError_t launch_flow_color(const float* flow, int B, int64_t plane, int hwc, uint8_t* rgb, unsigned* workspace, hipStream_t s);
hipError_t launch_sff_outputs(const float* pred, const float* warped, const uint8_t* interp, int B, int64_t plane, uint8_t* pred_u8,
                              uint8_t* warped_rgb, uint8_t* stitch_u8, hipStream_t s);
}
