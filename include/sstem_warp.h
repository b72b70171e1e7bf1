/*
 * sstem_warp.h -- C-ABI of the bilinear back-warp of libsstem_hip.so (MI355X / gfx950).
 *
 * Replaces the reference's pure-torch module SpatialTransformation.forward / .interpolate
 * (sff_scripts_fusion/utils/image_warp_torch.py:35-112), the step between the frozen flow network and
 * the fusion UNet (sff_scripts_fusion/main_fusion.py:229-235, inference.py:150), with one gather kernel.
 *
 *   image  [B, C, H, W]  fp32 contiguous (the reference permutes to NHWC and zero-pads by 1 pixel; neither
 *                        copy is materialised here)
 *   flow   [B, 2, H, W]  fp32 contiguous; channel 0 = dx (columns), channel 1 = dy (rows) -- the layout the
 *                        flow network produces; the reference's deformation_matrix[b,y,x,k] is flow[b,k,y,x]
 *   output [B, C, H, W]
 * Same status codes / error reporting / stream and ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_WARP_H
#define SSTEM_WARP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int sstem_warp_bilinear_f32(const float* image, const float* flow, float* output,
                            int64_t B, int64_t C, int64_t H, int64_t W, void* stream);

/*
 * The gradients of the back-warp.  The reference has no code for them: they are what torch's autograd derives from
 * SpatialTransformation.interpolate (sff_scripts_fusion/utils/image_warp_torch.py:32-95) when the moving image or the
 * deformation field requires a gradient.  floor and clamp have zero derivative, so the indices x0, x1, y0, y1 are
 * constants and the weights wx = float(x1_clamped) - x, wy = float(y1_clamped) - y (:82-86) have d wx/dx = d wy/dy = -1.
 * With g = grad_output and Ia = P(y0,x0), Ib = P(y1,x0), Ic = P(y0,x1), Id = P(y1,x1) of the zero-bordered image P:
 *
 *   grad_flow[b,0,r,c] = sum_ch g * ( wy*(Ic - Ia) + (1-wy)*(Id - Ib) )
 *   grad_flow[b,1,r,c] = sum_ch g * ( wx*(Ib - Ia) + (1-wx)*(Id - Ic) )
 *   grad_image[b,ch,.] += wx*wy*g at (y0,x0), wx*(1-wy)*g at (y1,x0), (1-wx)*wy*g at (y0,x1), (1-wx)*(1-wy)*g at (y1,x1)
 *
 * Taps on the border (index 0, W+1 or H+1) are dropped.  Whenever a clamp changes an index both taps of that axis are
 * border taps, so a pixel whose sample lies outside the padded plane has zero gradients: a finite flow of any size is
 * as harmless as in the forward, and no load, store or atomic is issued outside its in-plane predicate.
 *
 *   grad_output [B, C, H, W]  fp32 contiguous
 *   grad_flow   [B, 2, H, W]  or NULL.  Written in full, zeros included; channels summed in ascending order by one lane
 *                             per pixel, no atomics, no workspace: bit-reproducible from run to run.  At most C + 4
 *                             roundings per element (sub, mul, add, mul by g, and C - 1 adds), each relative to
 *                             S = sum_ch |g| (|wy| (|Ia| + |Ic|) + |1-wy| (|Ib| + |Id|))   (and the y twin).
 *   grad_image  [B, C, H, W]  or NULL.  Cleared on the stream by the call (capturable), then summed with fp32 atomic
 *                             adds; accumulate_image != 0 skips the clear and adds to what is there (a caller's .grad
 *                             buffer, the convention of the convolution entries' accumulate).  The order of the adds is
 *                             NOT fixed: the bits can differ from run to run, inside (k + 2) 2^-24 A + k 2^-126 for an
 *                             element with k in-plane contributions w*g, A = sum |w*g| (two roundings per term, then
 *                             k - 1 adds in any order).  The absolute term allows for hardware that flushes a subnormal
 *                             partial sum; whether this chip's memory-side adder does has not been measured.
 *   image may be NULL when grad_flow is NULL (the image gradient does not read it).  Both outputs NULL: refused like
 *   any missing required pointer.  Sizes, empty shapes and limits: as sstem_warp_bilinear_f32.
 */
int sstem_warp_bilinear_backward_f32(const float* image, const float* flow, const float* grad_output,
                                     float* grad_flow /* nullable */, float* grad_image /* nullable */, int accumulate_image,
                                     int64_t B, int64_t C, int64_t H, int64_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_WARP_H */
