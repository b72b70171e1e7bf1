// Internal launcher interface between the C-ABI (sstem_capi.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {

// one coefficient of a [B,taps,H,W] tensor: fp32, or bf16 widened exactly (the upper half of an fp32)
template <bool BF> __device__ __forceinline__ float coef_at(const float* t, int64_t i)
{
    if constexpr (BF) return __builtin_bit_cast(float, (uint32_t)reinterpret_cast<const uint16_t*>(t)[i] << 16);
    else return t[i];
}

hipError_t launch_fwd_direct(const float* in, const float* ver, const float* hor, float* out,
                             int64_t B, int64_t C, int64_t H, int64_t W, int filt, hipStream_t s);
hipError_t launch_bwd_direct(const float* g, const float* in, const float* ver, const float* hor,
                             float* gv, float* gh, int64_t B, int64_t C, int64_t H, int64_t W,
                             int filt, hipStream_t s);
hipError_t launch_fwd_mfma(const float* in, const float* ver, const float* hor, float* out,
                           int64_t B, int64_t C, int64_t H, int64_t W, hipStream_t s);
hipError_t launch_bwd_mfma(const float* g, const float* in, const float* ver, const float* hor,
                           float* gv, float* gh, int64_t B, int64_t C, int64_t H, int64_t W,
                           hipStream_t s);
bool mfma_grid_ok(int64_t B, int64_t H, int64_t W);
hipError_t launch_interp_fused(const float* i1, const float* i2, const float* k1v, const float* k1h,
                               const float* k2v, const float* k2h, float* out, int64_t B, int64_t H, int64_t W,
                               hipStream_t s);

bool interp_fused_gray_ok(int64_t H, int64_t W);
hipError_t launch_interp_fused_gray(const float* g1, const float* g2, const float* k1v, const float* k1h,
                                    const float* k2v, const float* k2h, float* out, int64_t B, int64_t H, int64_t W,
                                    hipStream_t s, uint8_t* out_u8 = nullptr);

// the same apply with the four coefficient tensors in the row-segment layout [B][H][ceil(W/64)][51][64]
int64_t coef_blocked_floats(int64_t B, int64_t H, int64_t W);
bool interp_fused_gray_blocked_ok(int64_t H, int64_t W);
hipError_t launch_coef_to_blocked(const float* src, float* dst, int64_t B, int64_t H, int64_t W, hipStream_t s);
hipError_t launch_interp_fused_gray_blocked(const float* g1, const float* g2, const float* k1v, const float* k1h,
                                            const float* k2v, const float* k2h, float* out, int64_t B, int64_t H, int64_t W,
                                            hipStream_t s, uint8_t* out_u8 = nullptr);

// bf16 coefficient tensors ([B,51,H,W] bf16), fp32 frames, gradients and sums
hipError_t launch_fwd_bf16coef(const float* in, const uint16_t* ver, const uint16_t* hor, float* out,
                               int64_t B, int64_t C, int64_t H, int64_t W, hipStream_t s);
hipError_t launch_bwd_bf16coef(const float* g, const float* in, const uint16_t* ver, const uint16_t* hor,
                               float* gv, float* gh, int64_t B, int64_t C, int64_t H, int64_t W, hipStream_t s);
bool interp_fused_gray_bf16coef_ok(int64_t H, int64_t W);
hipError_t launch_interp_fused_gray_bf16coef(const float* g1, const float* g2, const uint16_t* k1v, const uint16_t* k1h,
                                             const uint16_t* k2v, const uint16_t* k2h, float* out, int64_t B, int64_t H, int64_t W,
                                             hipStream_t s);

// Input gradient (sepconv_gradinput.hip; this library's addition, the reference leaves gradInput untouched):
//     gI[b,c,Y,X] = sum over source pixels (y,x), y in [Y-taps+1, Y] and [0,H), x in [X-taps+1, X] and [0,W), of
//                   V[b,Y-y;y,x] * (g[b,c,y,x] * H[b,X-x;y,x])
// ONE summation order for both kernels: source rows y ascending, source columns x ascending inside a row, one fmaf chain
// from +0:  acc = fmaf(V, fl(g * H), acc).  Source pixels outside the image contribute nothing.  So the tiled kernel equals
// the direct kernel bit for bit on finite data whose chains never underflow to -0: its off-band steps add A * 0 or 0 * B, which
// turns an infinite V or g * H into NaN and an accumulator that has underflowed to -0 into +0; the direct kernel skips those steps.
//   direct: one lane per grad_input element, any C, any filter length, fp32 or bf16 coefficients, 64-bit indexing.
//   tiled : 51 taps, fp32 coefficients; a gather by 64 x 64 tile of the padded plane, every element written once by plain
//           stores (no atomics, no workspace, no zero-fill).  C > 3 runs in chunks of three channels.
hipError_t launch_gradinput_direct(const float* g, const float* ver, const float* hor, float* gi,
                                   int64_t B, int64_t C, int64_t H, int64_t W, int filt, bool bf16coef, hipStream_t s);
bool gradinput_tiled_ok(int64_t B, int64_t C, int64_t H, int64_t W);
hipError_t launch_gradinput_tiled(const float* g, const float* ver, const float* hor, float* gi,
                                  int64_t B, int64_t C, int64_t H, int64_t W, hipStream_t s);

}  // namespace sstem
