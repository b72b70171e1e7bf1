/*
 * sstem_fold.h -- C-ABI of the SFF fold synthesis of libsstem_hip.so (MI355X / gfx950): the synthetic fold's flow field, the uint8
 * back-warp, and the two fused into the training sample of the fusion and unfolding loops.
 *
 * Replaces, per sample, what the reference's Train.degradation does on the host in numpy
 * (sff_scripts_fusion/data/data_provider.py:183-248, sff_scripts_unfolding/data/data_provider.py:180-245):
 *   gen_flow(height, width, k, b, line_width, fold_width, dis_k)    utils/flow_synthesis.py:20-87
 *   image_warp(im, flow, mode)                                      utils/image_warp.py:3-112
 *   (deformed * mask).astype(np.uint8), the centre crop, the count of black pixels, np.repeat(.., 3, 0), astype(np.float32) / 255.0
 * Drawing the fold (the random module) and reading files stay on the host; colour jitter is built in sstem_jitter.h (a byte table per
 * sample, read through by sstem_fold_degrade_lut_u8; only drawing its factors stays on the host).  The crops and flips ahead of the fold can
 * stay there too, or come from sstem_crop_orient_u8 (sstem_batch.h), whose planes 0 and 1 are this header's clean and interp.
 *
 * A fold is a row of SSTEM_FOLD_PARAMS doubles, derived on the host with the reference's own Python expressions (so the library
 * calls no libm function and the machine that derives them decides their last bits, as it does for the reference):
 *   [0] k            [1] b                    the fold line y = k x + b of gen_line
 *   [2] norm         math.sqrt(k ** 2 + 1)
 *   [3] line_width   [4] fold_width
 *   [5] ndk          -dis_k
 *   [6] dis_b        (fold_width - line_width) - ndk * line_width
 *   [7] cos_p        [8] sin_p                math.cos / math.sin of math.atan(1 / k), of math.atan(1 / 1e-9) when k == 0
 *   [9] k_pos        1.0 when k > 0, else 0.0 (the branch of flow_synthesis.py:75)
 * folds is a device array [n][SSTEM_FOLD_PARAMS].
 *
 * The arithmetic is the reference's, operation by operation in IEEE double / float with no contraction, so flow, flow2 (signed
 * zeros included), mask and the warped bytes are the reference's bit for bit.  Per pixel (x = column, y = row):
 *   d    = (((k * x) - y) + b) / norm                     sign = 1, -1 or 0 by d > 0, d < 0;   a = |d|
 *   mask = a <= line_width ? 0 : 1;   m1 = a < line_width ? 0 : 1;   m2 = a < fold_width ? 0 : 1
 *   s    = ndk * a + dis_b, 0 where s < 0;   s1 = s * m1 + a * (1 - m1);   s2 = s * m2 + a * (1 - m2)
 *   dis  = s1 * sign;   dis2 = s2 * (-sign)
 *   flow  = k_pos ? (dis * cos_p, -(dis * sin_p))   : (-(dis * cos_p), dis * sin_p)        rounded to fp32
 *   flow2 = the same of dis2
 *   warp: fl = floor(flow) in fp32;  x0 = clamp(x + (int)fl.x, 0, W - 1), x1 = min(x0 + 1, W - 1), likewise y;
 *         xw = flow.x - fl.x, yw = flow.y - fl.y in fp32 (the unclamped fraction);
 *         wa = (1 - xw)(1 - yw), wb = (1 - xw) yw, wc = xw (1 - yw), wd = xw yw;
 *         out = (uint8)(((wa I[y0,x0] + wb I[y1,x0]) + wc I[y0,x1]) + wd I[y1,x1]), four fp32 products, truncated;
 *         nearest: out = I[y0,x0]
 *   deformed = out * mask
 * A flow component that is NaN or beyond the int32 range is outside the contract (the reference's astype(np.int32) is undefined
 * there): its floor is saturated before the clamp and a NaN sum stores 0; nothing is read out of bounds.
 *
 * sstem_fold_flow       gen_flow on n full planes: flow, flow2 [n,H,W,2] fp32 (the reference's HWC layout), mask [n,H,W] uint8.
 *                       Any of the three may be NULL.  H != W is allowed.
 * sstem_image_warp_u8   image_warp: im [n,H,W,C] uint8, flow [n,H,W,2] fp32, out [n,H,W,C] uint8; mode SSTEM_WARP_NEAREST or
 *                       SSTEM_WARP_BILINEAR.
 * sstem_fold_degrade_u8 the fused training sample.  clean (and interp, needed only for im) are [slots,S_h,S_w] uint8 planes, one per
 *                       batch slot.  Launched sample i (fold row i) belongs to batch slot slot[i], or to slot i when slot is NULL: it
 *                       warps clean[slot] by its fold and writes that slot's outputs, so a redo launches only the rejected samples.
 *                       A slot value outside [0, slots) writes nothing.  Only the window's out_h x out_w pixels at (off_y, off_x)
 *                       are computed; flow and mask are never materialised; the gather reads the whole plane.  Outputs, any NULL:
 *     deformed   [slots,out_h,out_w] uint8
 *     flow2      [slots,2,out_h,out_w] fp32: the unfolding label np.transpose(flow2, (2, 0, 1))
 *     im         [slots,6,out_h,out_w] fp32: channels 0-2 deformed / 255, channels 3-5 interp's window / 255
 *     lb         [slots,1,out_h,out_w] fp32: clean's window / 255; with gt_line != 0 it is 0 where deformed == 0
 *     zero_count [slots] int32: the number of window pixels with deformed == 0 (what the reference's rejection rule reads)
 *                       The divisions are float32(byte) / float32(255), as sstem_gray_u8_to_f32.  zero_count is overwritten: the entry
 *                       enqueues a one-kernel clear of the launched samples' counts ahead of the map, whose waves then add with one
 *                       integer atomic each -- the same number every run, nothing for the caller to fill.
 *
 * The entries allocate, copy and synchronise nothing and may be captured into a graph.
 * Refused before any HIP call: negative sizes, C < 1, a window not inside the plane (SSTEM_ERR_BAD_SHAPE); an unknown mode, H, W,
 * S_h, S_w above 32768, n or slots above 2^24, C above 1024 (SSTEM_ERR_UNSUPPORTED); NULL folds / im / flow / out / clean, NULL interp
 * with im given (SSTEM_ERR_NULL_POINTER).  n == 0 is a successful no-op, and so is an empty plane for the first two entries.
 * Device pointers; same status codes / stream / ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_FOLD_H
#define SSTEM_FOLD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSTEM_FOLD_PARAMS 10

#define SSTEM_WARP_NEAREST 0
#define SSTEM_WARP_BILINEAR 1

int sstem_fold_flow(const double* folds, int64_t n, int64_t H, int64_t W, float* flow, float* flow2, uint8_t* mask, void* stream);

int sstem_image_warp_u8(const uint8_t* im, const float* flow, uint8_t* out, int64_t n, int64_t H, int64_t W, int64_t C, int mode,
                        void* stream);

int sstem_fold_degrade_u8(const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int64_t n, int64_t slots,
                          int64_t S_h, int64_t S_w, int64_t off_y, int64_t off_x, int64_t out_h, int64_t out_w, int gt_line,
                          uint8_t* deformed, float* flow2, float* im, float* lb, int32_t* zero_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_FOLD_H */
