#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {
// include/sstem_jitter.h; sizes already checked by the entry (1 <= n <= 2^24, 1 <= plane = S_h * S_w <= 2^30)
hipError_t launch_jitter_lut(const uint8_t* planes, int n, int64_t plane, const int32_t* op_code, const float* op_factor, uint8_t* lut,
                             uint32_t* hist, hipStream_t s);
}
