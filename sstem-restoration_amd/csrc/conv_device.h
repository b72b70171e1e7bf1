// Device-side helpers shared by the convolution kernels (conv_kernels.hip, conv_bf16_kernels.hip, conv_split_kernels.hip,
// conv_split_wgrad.hip, convt_kernels.hip): the fused activation, the saddr-form lane accesses and the pins that keep wave-uniform
// values in SGPRs.  Every function is __forceinline__: one spelling, no code of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// "wave-uniform 64-bit base (SGPR pair) + one 32-bit per-lane byte offset" accesses: the saddr form, no per-lane 64-bit addresses
typedef __attribute__((address_space(1))) float gfloat_t;
template <typename T>
__device__ __forceinline__ void pin_uniform_ptr(T*& p) { asm volatile("" : "+s"(p)); }
__device__ __forceinline__ void store_lane(float* ubase, uint32_t lane_byte_off, float v)
{
    *reinterpret_cast<gfloat_t*>(reinterpret_cast<uint64_t>(ubase) + lane_byte_off) = v;
}
__device__ __forceinline__ float load_lane(const float* ubase, uint32_t lane_byte_off)
{
    return *reinterpret_cast<const gfloat_t*>(reinterpret_cast<uint64_t>(ubase) + lane_byte_off);
}
__device__ __forceinline__ void pin_sgpr(uint32_t& v) { asm volatile("" : "+s"(v)); }

// the fused activation of every convolution epilogue (ConvExtra: conv_kernels.h): 1 = ReLU, 2 = leaky ReLU with `slope`
__device__ __forceinline__ float act_apply(float v, int act, float slope)
{
    if (act == 1) return v > 0.f ? v : 0.f;
    if (act == 2) return v > 0.f ? v : v * slope;
    return v;
}

}  // namespace sstem
