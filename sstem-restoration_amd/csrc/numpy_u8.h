// (x * 255).astype(np.uint8) on a float32 value as numpy does it on x86-64 -- the conversion include/sstem_io.h states for
// sstem_f32_to_gray_u8, written once: an fp32 multiply by 255 rounded on its own, truncation toward zero to a wide integer, the low
// 8 bits, NO clamp (256.0 -> 0, -1.0 -> 255); NaN and |v| >= 2^63 give 0.  Device-only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

__device__ __forceinline__ uint8_t numpy_u8_of(float p)
{
#pragma clang fp contract(off)
    const float v = p * 255.0f;                                              // rounded on its own: nothing may fuse it
    long long w = 0;
    if (v == v && fabsf(v) < 9.0e18f) w = (long long)v;
    return (uint8_t)(w & 0xFF);
}

}  // namespace sstem
