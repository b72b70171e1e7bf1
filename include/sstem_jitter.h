/*
 * sstem_jitter.h -- C-ABI of the colour jitter of libsstem_hip.so (MI355X / gfx950): the jitter of the SFF fusion and unfolding
 * providers as one 256-entry byte table per sample, and the fold degradation that reads its section through that table.
 *
 * Replaces, per sample, what the reference's Train._color_jitter does on the host
 * (sff_scripts_fusion/data/data_provider.py:146-148,309-313, sff_scripts_unfolding/data/data_provider.py:144-145):
 *   np.asarray(torchvision.transforms.ColorJitter(brightness, contrast, saturation, hue=0)(Image.fromarray(im)))
 * on a 2-D uint8 array, so on a PIL image of mode L.  There torchvision calls PIL's ImageEnhance, whose every enhancement is
 * Image.blend(degenerate, image, factor).  Drawing the factors and their order (the random module) stays on the host.
 *
 * The blend (PIL's Blend.c) of a byte v towards the degenerate byte d, alpha = (float)factor, everything in float32, the product and
 * the sum each rounded on their own (no contraction):
 *   t = (float)d + alpha * (float)(v - d)              v - d the exact integer
 *   0 <= alpha <= 1:   (uint8)t                        truncated; t lies between d and v
 *   otherwise:         0 where t <= 0, 255 where t >= 255, else (uint8)t
 * A step of a sample is (op code, factor):
 *   0 none         the byte stays
 *   1 brightness   d = 0
 *   2 contrast     d = int(mean + 0.5), mean = ImageStat's sum / count of the image as it is at that step
 *   3 saturation   the degenerate is the image itself: the byte stays (the step exists because the host draws a factor for it)
 * Each step maps a byte to a byte given one integer per sample, so the SSTEM_JITTER_OPS steps, applied left to right, are one table
 * lut[v] per sample, and the sum a contrast step needs is  sum over v of hist[v] * lut_so_far[v]  from the histogram of the plane
 * as it was given.  The sum is an exact 64-bit integer, and d = (2 sum + count) / (2 count) in integers.  That is ImageStat's
 * int(sum / count + 0.5) in doubles: count <= 2^30 and sum < 2^38, so sum / count + 0.5 is either an integer exactly or at least
 * 1 / (2 count) >= 2^-31 away from one, far above a double's resolution below 256 (2^-45): the two roundings cannot carry it across.
 *
 * sstem_jitter_lut_u8        planes [n,S_h,S_w] uint8, op_code / op_factor [n][SSTEM_JITTER_OPS] -> lut [n][256] uint8.  hist
 *                            [n][256] uint32 is workspace that need not be cleared: the entry enqueues its clear, then the histogram
 *                            (integer adds: the same counts every run), then the tables; three launches ordered by the stream.
 *                            A sample with an op code outside [0, 3] leaves its row of lut unwritten; its neighbours are written.
 * sstem_fold_degrade_lut_u8  sstem_fold_degrade_u8 (sstem_fold.h) with lut [slots][256] between gt_line and the outputs: every byte
 *                            gathered from clean for the warp goes through lut[slot] first, so deformed, im[:, 0:3], zero_count and
 *                            the gt_line zeros follow the jittered section.  lb reads the un-jittered window (the reference copies its
 *                            label ahead of the jitter, data_provider.py:143-148) and im[:, 3:6] reads interp untouched.  With
 *                            lut == NULL it is sstem_fold_degrade_u8 itself.
 *
 * Outside the contract: a t that is not finite (a NaN or infinite factor) stores 0 -- (uint8)NaN is undefined in C.
 *
 * The entries allocate, copy and synchronise nothing and may be captured into a graph.
 * Refused before any HIP call: negative sizes (SSTEM_ERR_BAD_SHAPE); S_h, S_w above 32768, n above 2^24 (SSTEM_ERR_UNSUPPORTED); NULL
 * planes / op_code / op_factor / lut / hist (SSTEM_ERR_NULL_POINTER).  n == 0 and an empty plane are successful no-ops.  The degrade
 * entry refuses what sstem_fold_degrade_u8 refuses.  Device pointers; same status codes / stream / ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_JITTER_H
#define SSTEM_JITTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSTEM_JITTER_OPS 4     /* steps per sample: 0 none, 1 brightness, 2 contrast, 3 saturation (identity) */

#define SSTEM_JITTER_NONE 0
#define SSTEM_JITTER_BRIGHTNESS 1
#define SSTEM_JITTER_CONTRAST 2
#define SSTEM_JITTER_SATURATION 3

int sstem_jitter_lut_u8(const uint8_t* planes, int64_t n, int64_t S_h, int64_t S_w, const int32_t* op_code, const float* op_factor,
                        uint8_t* lut, uint32_t* hist, void* stream);

int sstem_fold_degrade_lut_u8(const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int64_t n,
                              int64_t slots, int64_t S_h, int64_t S_w, int64_t off_y, int64_t off_x, int64_t out_h, int64_t out_w,
                              int gt_line, const uint8_t* lut, uint8_t* deformed, float* flow2, float* im, float* lb,
                              int32_t* zero_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_JITTER_H */
