/*
 * sstem_display.h -- C-ABI of the image outputs of the SFF inference scripts and the unfolding monitor (libsstem_hip.so): the Middlebury
 * colour code of a flow field and the uint8 images the scripts save, as launches.
 *
 * Replaces, per image, what the reference does on the host after downloading fp32 tensors:
 *   dense_flow(pred_flow) = flow_to_image + compute_color + make_color_wheel of utils/flow_display.py:4-138, called by
 *     sff_scripts_fusion/inference.py:161-162,172,184, sff_scripts_unfolding/inference.py:146-149 and twice per monitor image by
 *     sff_scripts_unfolding/main_flowfusionnet.py:256-257,297-298;
 *   (x * 255).astype(np.uint8) of the prediction and of the three warped channels, Image.fromarray(...).convert('L'), the < 2 mask and
 *     the stitch with the interpolated section (sff_scripts_fusion/inference.py:163-171); the RGB image of the warped channels
 *     (sff_scripts_unfolding/inference.py:151-153).
 * sparse_flow (matplotlib plotting) and writing files stay on the host.
 *
 * sstem_flow_color_u8   flow fp32, [B,2,H,W] (hwc == 0: what the flow net emits) or [B,H,W,2] (hwc != 0: what the scripts hold after
 *     permute(0,2,3,1)); neither layout costs a copy launch.  rgb [B,H,W,3] uint8, interleaved: the array Image.fromarray takes.  Every
 *     image is normalised by its own maximum radius, because the reference is called per image.  Two launches: the first leaves
 *     partial maxima of every image in the workspace, the second takes each image's maximum of them and colours the pixels.
 *     The contract is the reference's arithmetic as it runs under NumPy 2.2.6:
 *       Unknown pixels.   |u| > 1e7 or |v| > 1e7 in float32 comparison makes a pixel unknown.  Infinities are therefore unknown.  Its u
 *                         and v count as 0 everywhere below and its three bytes are 0.
 *       First radius, in float32.   rad = sqrtf(u*u + v*v).  Each product and the sum is rounded to float32 on its own.
 *       maxrad.           It is the maximum of rad.  If any rad is NaN, the value is -1: np.max returns NaN, and Python's max(-1, nan)
 *                         keeps -1.  It is also -1 if the maximum is not greater than -1, which cannot occur otherwise.
 *       From here on, float64.   d = (double)maxrad + 2^-52, then u = (double)u / d and v = (double)v / d.  np.finfo(float).eps is a
 *                         float64 scalar.  Under NumPy 2 promotion it lifts the float32 arrays, so everything from this point is float64.
 *       NaN pixels.       A pixel where u or v is NaN has both set to 0, and its bytes are multiplied by 0.
 *       Second radius.    rad = sqrt(u*u + v*v) in float64, uncontracted.
 *       Angle.            a = atan2(-v, -u) / np.pi, then fk = (a + 1) / 2 * 54 + 1, k0 = floor(fk), k1 = k0 + 1 with 56 -> 1, and
 *                         f = fk - k0.
 *       Colour per channel.   col = (1 - f) * (wheel[k0-1] / 255) + f * (wheel[k1-1] / 255).
 *                         Then col = 1 - rad * (1 - col) where rad <= 1, else col * 0.75.
 *                         The byte is floor(255 * col * (1 - nan)).
 *       Wheel.            The 55-entry wheel of make_color_wheel is a constant table in the kernel: sstem_flow_color_wheel returns the
 *                         host's copy of it, [55][3] bytes, R G B.
 *     Deviation 1.  The reference zeroes the unknown pixels in the caller's array, because u is a view.  The entry never writes flow.
 *     Deviation 2.  Under NumPy 1.x the reference would run the second half in float32.  The contract is the float64 path.
 *     Deviation 3.  The only operation whose bits the device cannot promise is atan2.  Everything else is IEEE-exact and must match bit
 *                   for bit.  (k0 is held inside [1, 55] whatever atan2 returns, so a table index cannot leave the wheel.)
 *
 * sstem_flow_color_workspace_bytes   bytes of workspace for B images (512 per image: 128 partial maxima; 0 for a negative B).  The
 *     workspace need never be cleared: every word the second launch reads was written by the first launch of the same call, whatever
 *     an earlier call of any shape left there.  Image b's words sit at byte 512 b whatever the shape, so a workspace serves every call
 *     whose own query is not larger.  8-byte aligned, one per stream (two calls in flight on one workspace would read each other's
 *     maxima).
 *
 * sstem_sff_outputs_u8   the image tail of the two inference scripts, one launch.  pred [B,H,W], warped [B,3,H,W] fp32, interp [B,H,W]
 *     uint8 (the interpolated section as read from its file).
 *       pred_u8 [B,H,W]         (pred * 255).astype(np.uint8): the conversion of sstem_f32_to_gray_u8 (sstem_io.h) -- an fp32 multiply by
 *                               255, truncation, the low 8 bits, no clamp.  Needs pred.
 *       warped_rgb [B,H,W,3]    the same conversion of the three warped channels, interleaved.  Needs warped.
 *       stitch_u8 [B,H,W]       L = (19595 R + 38470 G + 7471 B + 32768) >> 16 of those three bytes (PIL's convert('L')), then
 *                               L < 2 ? interp : L.  The reference's float32 interp * (1 - mask) + L * mask with a 0/1 mask is exactly
 *                               this select.  Needs warped and interp.
 *     Each output may be NULL and is then not made; a requested output whose input is NULL is refused.  There is no PAD argument: every
 *     shipped configuration has pad: 0, and the fusion script's stitch only broadcasts with pad: 0.
 *
 * Deterministic: no atomics, the same bits run to run.  The launches allocate, copy and synchronise nothing and may be captured
 * into a graph.
 * Refused before any HIP call: negative sizes (SSTEM_ERR_BAD_SHAPE); H or W above 32768, B above 2^24, a workspace that is not 8-byte
 * aligned (SSTEM_ERR_UNSUPPORTED); NULL flow / rgb / workspace, a requested output whose input is NULL (SSTEM_ERR_NULL_POINTER).
 * B == 0 or H * W == 0 is a successful no-op (the reference raises on an empty array), and so is a call that asks for no output.
 * Device pointers; same status codes / stream / ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_DISPLAY_H
#define SSTEM_DISPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSTEM_FLOW_WHEEL_COLS 55     /* entries of the colour wheel: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 */

const uint8_t* sstem_flow_color_wheel(void);   /* [SSTEM_FLOW_WHEEL_COLS][3], host memory owned by the library */

int64_t sstem_flow_color_workspace_bytes(int64_t B);
int sstem_flow_color_u8(const float* flow, int64_t B, int64_t H, int64_t W, int hwc, uint8_t* rgb, void* workspace, void* stream);

int sstem_sff_outputs_u8(const float* pred, const float* warped, const uint8_t* interp, int64_t B, int64_t H, int64_t W,
                         uint8_t* pred_u8, uint8_t* warped_rgb, uint8_t* stitch_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_DISPLAY_H */
