/*
 * sstem_score.h -- C-ABI of the validation scores (libsstem_hip.so): PSNR, SSIM and the flow end-point error as launches.
 *
 * Replaces, per image, compute_psnr(img1, img2) and compute_ssim(im1, im2) of utils/psnr_ssim.py:7-71 -- what the reference's loops
 * report per validation image (sff_scripts_interp/main_ms.py:250-279, sff_scripts_fusion/main_fusion.py:309-355, after clamping the
 * prediction to [0, 1]) and its inference scripts on their uint8 outputs (sff_scripts_interp/inference.py:92-93,
 * sff_scripts_fusion/inference.py:177-178, sff_scripts_unfolding/inference.py:135,157-158) -- and EPE(input_flow, target_flow, sparse,
 * mean) of loss/multiscaleloss.py:5-16 (sff_scripts_unfolding/main_flowfusionnet.py:279, inference.py:135).  The reference copies every
 * prediction to the host and scores it with numpy / scipy.signal.convolve2d in float64; these entries leave the results on the device.
 *
 * sstem_score_images_f32 / _u8   B independent single-channel pairs a, b of [B,H,W]; scores[B][3] = {mse, psnr, ssim} in float64.
 *     range     both per-image maxima <= 1 (after the clamp below) selects the reference's unit-range branch, decided on the device:
 *               mse = mean((a - b)^2), and the SSIM runs on (uint8)(x * 255.f) of either image -- one fp32 multiply and a truncation,
 *               numpy's (im * 255).astype(np.uint8) on a float32 array.  Otherwise mse = mean((a / 255 - b / 255)^2) and the SSIM
 *               runs on the values as they are.  Bytes take the second branch unless both images hold only 0 and 1, as in the
 *               reference.  A NaN makes the maximum NaN (np.max) and so selects the second branch.
 *     psnr      20 log10(1 / sqrt(mse)); 1e12 where mse < 1e-10 (the reference returns the bare sentinel 1000000000000 there and no
 *               mse; the mse slot holds the mse all the same).
 *     ssim      11 x 11 Gaussian window, sigma 1.5, applied 'valid': the mean of the (H - 10) x (W - 10) map
 *               ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.
 *     clamp01_a non-zero: a is clamped to [0, 1] as it is read -- the loops' pred[pred > 1] = 1; pred[pred < 0] = 0 without a launch.
 *     Differences, the sums, the five blurred moments and the map are float64, every sum in a fixed order.
 *     Deviations from the reference: (1) with both maxima <= 1 a value below 0 quantises to 0; the reference is undefined there
 *     (numpy's cast of a negative float to uint8).  (2) For float32 images in the second branch the reference forms im1 * im1,
 *     im2 * im2, im1 * im2 in float32 before its float64 convolution; here the products are float64 (identical for integer-valued
 *     images up to 255, whose products are exact in float32).  (3) compute_psnr on float32 arrays squares and averages in float32;
 *     here float64.
 *     H or W < 11 is refused: the 'valid' map would be empty (scipy's convolve2d silently exchanges its operands there, so the
 *     reference returns a number that is no SSIM).
 *
 * sstem_flow_epe_f32   flow, target [B,2,H,W] fp32; *value (float64) = the mean over the kept pixels (mean != 0) or the sum over
 *     them divided by B (mean == 0) of sqrt(dx^2 + dy^2), in float64.  sparse != 0 skips the pixels whose two target components are
 *     both exactly 0; no kept pixel under mean gives NaN, as the reference's empty mean does.  One launch.  Any H, W >= 0.
 *
 * sstem_score_workspace_bytes   bytes of workspace for a (B, H, W); one workspace serves the three entries (0 for sizes they
 *     refuse).  Zero it once before the first use; every call leaves it clean, so calls and graph replays need no further fill.
 *     The counters sit at its start whatever the shape, so a workspace serves every call whose own query is not larger.
 *     8-byte aligned, one per stream (two calls in flight on one workspace would share its counters and partial sums).
 *
 * Deterministic: no float atomics, the same bits run to run.  The launches allocate, copy and synchronise nothing and may be captured
 * into a graph.
 * Refused before any HIP call: NULL pointers, negative sizes, H or W < 11 (image scores), sizes past the kernels' index range (H or W
 * above 32768, B above 2^24, more than 2^24 map tiles of 32 x 16), a workspace or result pointer that is not 8-byte aligned.
 * B == 0 is a successful no-op.
 * Device pointers; same status codes / stream / ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_SCORE_H
#define SSTEM_SCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t sstem_score_workspace_bytes(int64_t B, int64_t H, int64_t W);
int sstem_score_images_f32(const float* a, const float* b, int64_t B, int64_t H, int64_t W, int clamp01_a, double* scores, void* workspace,
                           void* stream);
int sstem_score_images_u8(const uint8_t* a, const uint8_t* b, int64_t B, int64_t H, int64_t W, int clamp01_a, double* scores, void* workspace,
                          void* stream);
int sstem_flow_epe_f32(const float* flow, const float* target, int64_t B, int64_t H, int64_t W, int sparse, int mean, double* value,
                       void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_SCORE_H */
