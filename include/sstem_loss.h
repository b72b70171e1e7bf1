/*
 * sstem_loss.h -- C-ABI of the MS-SSIM criterion and of the single-scale SSIM criterion (libsstem_hip.so).
 *
 * Replaces MS_SSIM(max_val).forward(img1, img2) and its autograd backward
 * (sff_scripts_fusion/loss/loss_ssim.py:18-72; chosen by cfg.TRAIN.loss = 'ssim' in
 * sff_scripts_fusion/main_fusion.py:194-211 and descended at :252-254) for single-channel images [B,1,H,W], fp32:
 *
 *   per level  window ws = min(h, w, 11), sigma = 1.5 ws / 11, zero padding ws / 2 (an even window gives a map one larger
 *              than the image, as F.conv2d does there), ssim and mcs maps from the five blurred quantities, their means;
 *              the next level is the 2 x 2 average (floor extents)
 *   value    = prod_{i < levels-1} mcs_i^w_i * ssim_{levels-1}^w_{levels-1},  w = 0.0448, 0.2856, 0.3001, 0.2363, 0.1333
 *              (a non-positive level mean gives NaN, as in the reference)
 *
 * sstem_ms_ssim_forward_f32   one launch per level: *value, and terms[level][2] = {ssim mean, mcs mean} when terms is not NULL.
 *                             It leaves the pyramids of both images, the level means and the gradient's coefficients in `workspace`.
 * sstem_ms_ssim_backward_f32  one launch per level, coarsest first: grad_img1 = grad_value * d value / d img1 ([B,1,H,W]) from the
 *                             workspace AS THE FORWARD LEFT IT and the forward's two images.  The function is symmetric: the gradient with
 *                             respect to the forward's img2 is the same call with the two image pointers exchanged (the library knows
 *                             the exchange by the img1 address the forward recorded, so pass the forward's own two buffers).
 *                             grad_value: device scalar, NULL = 1.
 * sstem_ms_ssim_workspace_floats  floats of workspace for a shape (0 for sizes the entries refuse).  Zero it once before the first use;
 *                             every call leaves its counters clean, so calls and graph replays need no further fill.  8-byte aligned,
 *                             one per stream (two calls in flight on one workspace would share its counters and partial sums).
 *
 * Deterministic: every sum is taken in a fixed order (no float atomics), the same bits run to run.  The launches allocate, copy and
 * synchronise nothing and may be captured into a graph.
 * Refused before any HIP call: NULL pointers, levels outside 1..5, min(H, W) < 2^levels (the reference fails there too, in its trailing
 * avg_pool2d), a non-positive or non-finite max_val, sizes past the kernels' index range (H or W above 32768, more than 2^24 tiles).
 * B == 0 is a successful no-op.
 *
 * Single-scale SSIM criterion: replaces SSIMLoss(window_size=11, size_average).forward(img1, img2) and its autograd backward
 * (sff_scripts_interp/loss/loss_ssim.py:74-146; chosen by cfg.TRAIN.loss = 'ssim' in sff_scripts_interp/main_ms.py:153-155 and
 * descended at :203-206) for [B,C,H,W] fp32, any C >= 1 (B C planes under one window, groups = channel):
 *
 *   window     the 11 taps exp(-(k - 5)^2 / (2 1.5^2)) normalised in fp32 -- 11 whatever H and W are (the MS-SSIM entries shrink theirs
 *              to min(h, w, 11); this one does not), zero padding 5, so the map has the image's extent; C1 = 0.01^2, C2 = 0.03^2 (no
 *              max_val); images narrower or shorter than 11 are legal, as in the reference
 *   value    = 1 - mean(ssim map): one scalar (per_sample = 0, size_average=True), or B scalars, each 1 - the mean over that sample's
 *              C H W points (per_sample != 0, size_average=False)
 *
 * sstem_ssim_loss_forward_f32   ONE launch: value[1] or value[B].
 * sstem_ssim_loss_backward_f32  ONE launch: grad_img1 = grad_value * d value / d img1 ([B,C,H,W]); grad_value is a device pointer to one
 *                               scalar, or to B scalars when per_sample is set; NULL = ones.  It reads the two images only (nothing of the
 *                               forward's).  The function is symmetric: the gradient with respect to img2 is the same call with the two
 *                               image pointers exchanged.
 * sstem_ssim_loss_workspace_floats  floats of workspace for a shape (0 for sizes the entries refuse and for empty shapes).
 *
 * The launch rules are the MS-SSIM entries': every sum is taken in a fixed order (no float atomics), the same bits run to run; the
 * workspace is zeroed once before the first use and every call leaves it clean; it is 8-byte aligned, one per stream; nothing allocates,
 * copies or synchronises; the launches may be captured into a graph.  Refused before any HIP call: negative sizes, NULL pointers
 * (grad_value apart), sizes past the kernels' index range (H or W above 32768, B or C above 2^24, more than 2^24 tiles of 32 x 32), a
 * misaligned workspace.  B C H W == 0 is a successful no-op.
 * Device pointers; same status codes / stream / ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_LOSS_H
#define SSTEM_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t sstem_ms_ssim_workspace_floats(int64_t B, int64_t H, int64_t W, int levels);
int sstem_ms_ssim_forward_f32(const float* img1, const float* img2, int64_t B, int64_t H, int64_t W, int levels, float max_val,
                              float* value, float* terms, float* workspace, void* stream);
int sstem_ms_ssim_backward_f32(const float* img1, const float* img2, int64_t B, int64_t H, int64_t W, int levels, float max_val,
                               const float* grad_value, float* grad_img1, float* workspace, void* stream);

int64_t sstem_ssim_loss_workspace_floats(int64_t B, int64_t C, int64_t H, int64_t W);
int sstem_ssim_loss_forward_f32(const float* img1, const float* img2, int64_t B, int64_t C, int64_t H, int64_t W, int per_sample,
                                float* value, float* workspace, void* stream);
int sstem_ssim_loss_backward_f32(const float* img1, const float* img2, int64_t B, int64_t C, int64_t H, int64_t W, int per_sample,
                                 const float* grad_value, float* grad_img1, float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_LOSS_H */
