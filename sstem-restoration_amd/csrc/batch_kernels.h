#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {
// include/sstem_batch.h; sizes already checked by the entries (windows of at most 32768 x 32768, n and n_images at most 2^24,
// P and C0 + C1 at most 16, every chan_plane entry inside [0, P))
hipError_t launch_crop_orient_u8(const uint8_t* pool, const int64_t* images, int n_images, const int32_t* samples, const int32_t* plane_image,
                                 int n, int P, int SH, int SW, uint8_t* out, hipStream_t s);
hipError_t launch_crop_orient_f32(const uint8_t* pool, const int64_t* images, int n_images, const int32_t* samples, const int32_t* plane_image,
                                  int n, int P, int SH, int SW, const int32_t* chan_plane, int C0, int C1, uint32_t chan_invert, float* out0,
                                  float* out1, hipStream_t s);
}
