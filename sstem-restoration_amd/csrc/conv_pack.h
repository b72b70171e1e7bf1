// 3x3 weight packing shared by the convolution families (conv_kernels.hip, conv_bf16_kernels.hip, conv_split_kernels.hip,
// convt_kernels.hip).  A packed layout is a contract between a pack kernel and the MFMA kernel that reads it, so each layout's slot
// function exists ONCE, in a layout policy next to the MFMA kernel and its constants; this header holds what every family repeats
// around it: the walk of the group-pack table, the two pack kernels, and the host side of both.  Templates and inline functions only.
//
// A layout policy L is a struct with
//   typedef ... elem_t;                                          element type of the packed image
//   static PackSide side(int cin, int cout);                     host: layout numbers of the packing that serves a (cin -> cout) convolution
//   static __device__ elem_t slot(const float* w, int64_t idx, int cin, int cout, int CO, int nchunks, bool transposed_flipped);
//                                                                element idx of that packing, read from W[cout][cin][3][3] or, transposed +
//                                                                flipped (data gradient), from W[cin][cout][3][3] with the taps reversed
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_launch.h"

namespace sstem {

// layout numbers of one orientation: output channels per block (or padded output channels), K chunks, channel blocks, elements
struct PackSide { int CO, nchunks, ncb; int64_t n; };

// The group-pack table: 16 int64 per entry -- w, wp_f, wp_t, Cin, Cout, CO_f, nchunks_f, ncb_f, n_fwd, CO_t, nchunks_t, ncb_t, n_t,
// [13] first 256-thread block of the entry in the pack launch (ascending), [14] first block in the fp16 bound launch, [15] the fp16
// bound's address.  Returns the last entry whose `column` value is <= blockIdx.x.
__device__ __forceinline__ const int64_t* pack_table_entry(const int64_t* __restrict__ table, int n_entries, int column)
{
    int lo = 0, hi = n_entries - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)mid * 16 + column] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)lo * 16;
}

// ---- fp32 layout (conv3x3_mfma, and the ConvTranspose kernels with 32-channel blocks): Wp[cb][chunk][k'][CO],
// k' = (cl%4)*9+ky*3+kx + 36*(cl/4), 8 input channels per chunk (zero-padded in co and ci)
constexpr int PACK_F32_KC = 8, PACK_F32_KK = PACK_F32_KC * 9;
struct PackF32Slot { int ci, co, tap; };
__device__ __forceinline__ PackF32Slot pack_f32_slot(int64_t idx, int CO, int nchunks)
{
    const int col = idx % CO;
    int64_t r = idx / CO;
    const int kp = r % PACK_F32_KK; r /= PACK_F32_KK;
    const int chunk = r % nchunks;
    const int cb = r / nchunks;
    const int half = kp / 36, rem = kp % 36;
    const int cl = rem / 9 + 4 * half;
    return PackF32Slot{chunk * PACK_F32_KC + cl, cb * CO + col, rem % 9};
}

// ---- the pack kernels -------------------------------------------------------------------------------------------------------------
// Forward and / or transposed packing of one layer's weights in ONE launch (training: the forward packing and the transposed + flipped
// one its data gradient needs): indices [0, n_fwd) are the forward layout, the rest the transposed one of the (Cout -> Cin) problem;
// either may be absent (n = 0).  A convolution's own pack launch is the forward side alone, which reads transposed + flipped when the
// caller's weights are the transposed ones (fwd_is_transposed).
template <class L>
__global__ void pack_weights_pair(const float* __restrict__ w, typename L::elem_t* __restrict__ wp_f, typename L::elem_t* __restrict__ wp_t,
                                  int Cin, int Cout, int CO_f, int nchunks_f, int64_t n_fwd, int CO_t, int nchunks_t, int64_t n_t,
                                  int fwd_is_transposed)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_fwd + n_t; i += (int64_t)gridDim.x * blockDim.x) {
        if (i >= n_fwd) wp_t[i - n_fwd] = L::slot(w, i - n_fwd, Cout, Cin, CO_t, nchunks_t, true);
        else wp_f[i] = L::slot(w, i, Cin, Cout, CO_f, nchunks_f, fwd_is_transposed != 0);
    }
}

// Both packings of MANY layers in one launch (training: after the optimiser step every layer's weights have changed; one pack launch
// per layer and step was 19 launches of the 2-sample fusion step and 46 of the IFNet step), one thread per slot.  The layout numbers
// of an entry come from pack_entry below, i.e. from the same L::side the per-layer launch uses.
template <class L>
__global__ __launch_bounds__(256) void pack_weights_table(const int64_t* __restrict__ table, int n_entries)
{
    const int64_t* en = pack_table_entry(table, n_entries, 13);
    const float* w = reinterpret_cast<const float*>(en[0]);
    typename L::elem_t* wp_f = reinterpret_cast<typename L::elem_t*>(en[1]);
    typename L::elem_t* wp_t = reinterpret_cast<typename L::elem_t*>(en[2]);
    const int Cin = (int)en[3], Cout = (int)en[4];
    const int64_t n_fwd = en[8], n_t = en[12];
    const int64_t i = ((int64_t)blockIdx.x - en[13]) * 256 + threadIdx.x;
    if (i >= n_fwd + n_t) return;
    if (i >= n_fwd) wp_t[i - n_fwd] = L::slot(w, i - n_fwd, Cout, Cin, (int)en[9], (int)en[10], true);
    else wp_f[i] = L::slot(w, i, Cin, Cout, (int)en[5], (int)en[6], false);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// layout numbers of one table entry (out[3..12]); returns the 256-thread blocks the entry needs at one thread per slot
template <class L>
inline int64_t pack_entry(int Cin, int Cout, int64_t* out)
{
    const PackSide f = L::side(Cin, Cout), t = L::side(Cout, Cin);
    out[3] = Cin; out[4] = Cout;
    out[5] = f.CO; out[6] = f.nchunks; out[7] = f.ncb; out[8] = f.n;
    out[9] = t.CO; out[10] = t.nchunks; out[11] = t.ncb; out[12] = t.n;
    return (out[8] + out[12] + 255) / 256;
}

// one launch of pack_weights_pair: either destination may be null
template <class L>
inline hipError_t launch_pack_pair(const float* w, float* wp_f, float* wp_t, int Cin, int Cout, bool fwd_is_transposed, hipStream_t s)
{
    int64_t en[16];
    (void)pack_entry<L>(Cin, Cout, en);
    const int64_t n_f = wp_f ? en[8] : 0, n_t = wp_t ? en[12] : 0;
    return launch_kernel<pack_weights_pair<L>>(dim3(grid_1d(n_f + n_t, 256)), dim3(256), 0, s, w, reinterpret_cast<typename L::elem_t*>(wp_f),
                                               reinterpret_cast<typename L::elem_t*>(wp_t), Cin, Cout, (int)en[5], (int)en[6], n_f, (int)en[9],
                                               (int)en[10], n_t, (int)fwd_is_transposed);
}

template <class L>
inline hipError_t launch_pack_table(const int64_t* table, int n_entries, int64_t total_blocks, hipStream_t s)
{
    if (n_entries <= 0 || total_blocks <= 0) return hipSuccess;
    if (total_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    return launch_kernel<pack_weights_table<L>>(dim3((unsigned)total_blocks), dim3(256), 0, s, table, n_entries);
}

}  // namespace sstem
