#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sstem {
// include/sstem_fold.h; sizes already checked by the entries (planes of at most 32768 x 32768, n and slots at most 2^24)
hipError_t launch_fold_flow(const double* folds, int n, int H, int W, float* flow, float* flow2, uint8_t* mask, hipStream_t s);
hipError_t launch_image_warp_u8(const uint8_t* im, const float* flow, uint8_t* out, int n, int H, int W, int C, int bilinear, hipStream_t s);
hipError_t launch_fold_degrade(const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int n, int slots, int SH,
                               int SW, int off_y, int off_x, int out_h, int out_w, int gt_line, uint8_t* deformed, float* flow2, float* im,
                               float* lb, int32_t* zero_count, hipStream_t s, const uint8_t* lut = nullptr);   // lut: include/sstem_jitter.h
}
