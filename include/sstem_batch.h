/*
 * sstem_batch.h -- C-ABI of the training crops of libsstem_hip.so (MI355X / gfx950): one oriented gather from a device-resident set of
 * uint8 sections to the batch tensors of the training loops.
 *
 * Replaces, per sample, what the reference's data providers do on the host in numpy before anything else
 * (sff_scripts_interp/data/data_provider.py:103-141, sff_scripts_fusion/data/data_provider.py:115-135, sp_scripts_train/dataset.py:161-171,
 * 217-236): the crop of each plane at one window, fliplr / flipud / transpose / rot90, the replication to channels and
 * astype(np.float32) / 255.0.  Drawing the sample (the random module), reading files, colour jitter, noise and the elastic transform stay
 * on the host; the swap of the outer frames is a permutation of plane_image and never reaches the kernel.
 *
 * The resident set:
 *   pool        device bytes holding every image, rows dense (pitch = W)
 *   images      device int64 [n_images][SSTEM_BATCH_IMAGE_FIELDS]: (byte offset into pool, H, W) of image k
 * The samples:
 *   samples     device int32 [n][SSTEM_BATCH_SAMPLE_FIELDS]: (oy, ox, code) -- the window's origin in its images and the orientation
 *   plane_image device int32 [n][P]: the image that plane p of sample i reads
 *
 * The orientation code has three bits and covers the dihedral group:
 *   out = fliplr^(code & 1)( flipud^(code & 2)( transpose^(code & 4)( window ) ) )
 * that is, with a = (code & 2) ? S_h - 1 - y : y and b = (code & 1) ? S_w - 1 - x : x,
 *   out[y][x] = (code & 4) ? window[b][a] : window[a][b]          window[r][c] = image[oy + r][ox + c]
 * The window is S_h x S_w; a transposing code needs S_h == S_w.
 *
 * sstem_crop_orient_u8   out [P][n][S_h][S_w] uint8, plane-major: out[0] and out[1] of a (clean, interp) pair are exactly the clean and
 *                        interp arguments of sstem_fold_degrade_u8 (include/sstem_fold.h), so the fold path has no per-batch upload.
 * sstem_crop_orient_f32  two outputs in one launch, out0 [n][C0][S_h][S_w] and out1 [n][C1][S_h][S_w] fp32 (out1 may be NULL with
 *                        C1 == 0).  chan_plane is a HOST array of C0 + C1 <= SSTEM_BATCH_MAX_CHANNELS plane indices, out0's channels
 *                        first; it is read during the call and passed to the kernel by value (nothing is copied to the device).  Bit c
 *                        of chan_invert stores 255 - byte in channel c (the reversed masks of the SP loops).  The value is
 *                        float32(byte) / float32(255), the division of sstem_gray_u8_to_f32, never a product by a reciprocal.  Channels
 *                        of one plane are stored from the one staged tile and are identical.
 *                        IFNet batch: P = 3, chan_plane = [0,0,0,2,2,2 | 1].  SP patch set: P <= 14, fourteen channels of one plane each.
 *
 * A sample writes NOTHING -- its outputs keep what they held, and its neighbours are written as usual -- when
 *   its code is outside [0, 8),
 *   its code transposes and S_h != S_w,
 *   one of its P image ids is outside [0, n_images), or
 *   its window is not inside every one of its P images (oy < 0, ox < 0, oy + S_h > H or ox + S_w > W).
 * This is the slot rule of sstem_fold_degrade_u8 (a slot outside [0, slots) writes nothing) for the gather: a table row is data, it
 * is checked where it is read, and a bad row costs its own sample only.
 *
 * The entries allocate, copy and synchronise nothing and may be captured into a graph.
 * Refused before any HIP call: negative sizes, P < 1, C0 < 1, a chan_plane entry outside [0, P) (SSTEM_ERR_BAD_SHAPE); P or C0 + C1
 * above 16, S_h or S_w above 32768, n or n_images above 2^24 (SSTEM_ERR_UNSUPPORTED); NULL pool / images / samples / plane_image / out /
 * chan_plane / out0, NULL out1 with C1 > 0 (SSTEM_ERR_NULL_POINTER).  n == 0 and an empty window (S_h == 0 or S_w == 0) are successful
 * no-ops.  Device pointers but chan_plane; same status codes / stream / ownership rules as sstem_sepconv.h.
 */
#ifndef SSTEM_BATCH_H
#define SSTEM_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSTEM_BATCH_IMAGE_FIELDS 3
#define SSTEM_BATCH_SAMPLE_FIELDS 3
#define SSTEM_BATCH_MAX_PLANES 16
#define SSTEM_BATCH_MAX_CHANNELS 16

#define SSTEM_ORIENT_FLIPLR 1
#define SSTEM_ORIENT_FLIPUD 2
#define SSTEM_ORIENT_TRANSPOSE 4

int sstem_crop_orient_u8(const uint8_t* pool, const int64_t* images, int64_t n_images, const int32_t* samples, const int32_t* plane_image,
                         int64_t n, int64_t P, int64_t S_h, int64_t S_w, uint8_t* out, void* stream);

int sstem_crop_orient_f32(const uint8_t* pool, const int64_t* images, int64_t n_images, const int32_t* samples, const int32_t* plane_image,
                          int64_t n, int64_t P, int64_t S_h, int64_t S_w, const int32_t* chan_plane, int64_t C0, int64_t C1,
                          uint32_t chan_invert, float* out0, float* out1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSTEM_BATCH_H */
