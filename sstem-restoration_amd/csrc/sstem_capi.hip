// C-ABI of libsstem_hip.so -- see include/sstem_sepconv.h for the contract and the reference
// interfaces (libs/sepconv/src/SeparableConvolution_cuda.{h,c}) each entry point replaces.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sstem_sepconv.h"
#include "../../include/sstem_conv.h"
#include "../../include/sstem_warp.h"
#include "../../include/sstem_io.h"
#include "../../include/sstem_resize.h"
#include "../../include/sstem_norm.h"
#include "../../include/sstem_loss.h"
#include "../../include/sstem_score.h"
#include "../../include/sstem_fold.h"
#include "../../include/sstem_jitter.h"
#include "../../include/sstem_batch.h"
#include "../../include/sstem_display.h"
#include "sepconv_kernels.h"
#include "conv_kernels.h"
#include "warp_kernels.h"
#include "misc_kernels.h"
#include "norm_kernels.h"
#include "ssim_kernels.h"
#include "ssim_loss_kernels.h"
#include "score_kernels.h"
#include "fold_kernels.h"
#include "jitter_kernels.h"
#include "batch_kernels.h"
#include "display_kernels.h"
#include <math.h>

namespace {

thread_local char g_last_error[512] = "";

int fail(int status, const char* fmt, const char* a = "", const char* b = "", const char* c = "")
{
    snprintf(g_last_error, sizeof(g_last_error), fmt, a, b, c);
    return status;
}

int hip_fail(const char* where, hipError_t e, const char* step = "")
{
    return fail(SSTEM_ERR_HIP, "%s%s: %s", where, step, hipGetErrorString(e));
}

// the end of every entry: the status of its last HIP call.  The shared bodies below pass their caller's prefix and " launch".
int launched(const char* where, hipError_t e, const char* step = "")
{
    return e == hipSuccess ? SSTEM_OK : hip_fail(where, e, step);
}

// all element counts of a call must be addressable in int64 (the reference used 32-bit int,
// kernel.cu:26,32 -- 64-bit here on purpose: B=64 x 51 x 1024^2 already exceeds 2^31).
bool sizes_ok(int64_t B, int64_t C, int64_t H, int64_t W)
{
    if (B < 0 || C < 0 || H < 0 || W < 0) return false;
    const int64_t lim = (int64_t)1 << 40;  // 1 Ti elements: far above 288 GB of fp32
    if (B > lim || C > lim || H > lim || W > lim) return false;
    const __int128 hw = (__int128)(H + 50) * (W + 50);
    const __int128 big = (__int128)B * (C > 51 ? C : 51) * hw;
    return big < ((__int128)1 << 46);
}

// the entries that take a filter length: 1..1024 taps, and the padded tensors addressable as in sizes_ok
bool taps_sizes_ok(int64_t B, int64_t C, int64_t H, int64_t W, int taps)
{
    return taps >= 1 && taps <= 1024 && B >= 0 && C >= 0 && H >= 0 && W >= 0 &&
           (__int128)B * (C > taps ? C : taps) * (H + taps) * (W + taps) < ((__int128)1 << 46);
}

// ---- fused interpolation apply: the `_supported` queries and the entries evaluate the same predicates, the five entries share a body --
enum ApplyKind { APPLY_RGB, APPLY_GRAY, APPLY_GRAY_BLOCKED, APPLY_GRAY_BF16COEF };

// one image's coefficients sit behind a 32-bit buffer resource (the rgb kernel has no such bound)
bool apply_range_ok(ApplyKind kind, int64_t H, int64_t W)
{
    switch (kind) {
        case APPLY_GRAY: return sstem::interp_fused_gray_ok(H, W);
        case APPLY_GRAY_BLOCKED: return sstem::interp_fused_gray_blocked_ok(H, W);
        case APPLY_GRAY_BF16COEF: return sstem::interp_fused_gray_bf16coef_ok(H, W);
        default: return true;
    }
}

int apply_supported(ApplyKind kind, int64_t B, int64_t H, int64_t W)
{
    return (sizes_ok(B, 3, H, W) && B > 0 && H > 0 && W > 0 && sstem::mfma_grid_ok(B, H, W) && apply_range_ok(kind, H, W)) ? 1 : 0;
}

// grid_note, range_note: the entry's own words for the two range refusals; launch(): its launcher on its tensors
template <class Launch>
int interp_apply(const char* what, ApplyKind kind, bool any_null, int64_t B, int64_t H, int64_t W, const char* grid_note,
                 const char* range_note, Launch launch)
{
    if (!sizes_ok(B, 3, H, W)) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative or oversized shape", what);
    if (B == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (any_null) return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    if (!sstem::mfma_grid_ok(B, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "%s: %s", what, grid_note);
    if (!apply_range_ok(kind, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "%s: %s", what, range_note);
    return launched(what, launch(), " launch");
}

// ---- dense convolutions: the small rules, written once -------------------------------------------------------------------------
bool conv_sizes_ok(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout)
{
    if (N < 0 || Cin < 0 || H < 0 || W < 0 || Cout < 0) return false;
    const int64_t lim = (int64_t)1 << 30;
    if (N > lim || Cin > lim || Cout > lim || H > lim || W > lim) return false;
    if (H * W >= ((int64_t)1 << 31)) return false;               // in-plane offsets are 32-bit
    if ((__int128)N * (Cin > Cout ? Cin : Cout) * H * W >= ((__int128)1 << 46)) return false;
    return true;
}

// ... and none of the five sizes is zero: the entries and queries with no empty-shape case
bool conv_sizes_positive(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout)
{
    return conv_sizes_ok(N, Cin, H, W, Cout) && N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0;
}

bool channels_ok(int64_t Cin, int64_t Cout) { return Cin > 0 && Cout > 0 && Cin <= (1 << 20) && Cout <= (1 << 20); }

// 0, or the refusal of an activation id / a weight-flags word outside the values of include/sstem_conv.h
bool act_ok(int act) { return act >= 0 && act <= 2; }
int check_act(const char* what, int act) { return act_ok(act) ? 0 : fail(SSTEM_ERR_UNSUPPORTED, "%s: unknown activation id", what); }
int check_weight_flags(const char* what, int flags)
{
    return flags >= 0 && flags <= 3 ? 0 : fail(SSTEM_ERR_UNSUPPORTED, "%s: unknown weight flags", what);
}

// weight-gradient launches: bit 0 = add into the gradient buffers, bit 1 (only with bit 0) = defer the slab reduce to
// sstem_wgrad_deferred_flush (include/sstem_conv.h)
int wgrad_flags(int accumulate) { return accumulate == 3 ? 3 : (accumulate ? 1 : 0); }

// An algorithm id of include/sstem_conv.h as the kernel family behind it; the split ids carry their pieces per operand and whether
// those are fp16.  SSTEM_CONV_AUTO and unknown ids are FAMILY_NONE: each entry says what it makes of them.
enum ConvFamily { FAMILY_NONE, FAMILY_DIRECT, FAMILY_FP32, FAMILY_BF16, FAMILY_SPLIT };
struct ConvAlgo {
    ConvFamily family;
    int pieces, f16;
    bool split_bf16() const { return family == FAMILY_SPLIT && !f16; }      // the two ids that every split entry takes
};
ConvAlgo conv_algo(int algo)
{
    switch (algo) {
        case SSTEM_CONV_DIRECT: return {FAMILY_DIRECT, 0, 0};
        case SSTEM_CONV_MFMA: return {FAMILY_FP32, 0, 0};
        case SSTEM_CONV_MFMA_BF16: return {FAMILY_BF16, 0, 0};
        case SSTEM_CONV_MFMA_BF16X3: return {FAMILY_SPLIT, 2, 0};
        case SSTEM_CONV_MFMA_BF16X6: return {FAMILY_SPLIT, 3, 0};
        case SSTEM_CONV_MFMA_F16X3: return {FAMILY_SPLIT, 2, 1};
        default: return {FAMILY_NONE, 0, 0};
    }
}

// the end of the three forward entries of the split kernels, after their own argument checks: range, workspace, launch
// (ex.f16: the pieces are fp16).  range_note: what the entry's range refusal adds
int split_forward(const char* what, const char* range_note, const float* input, const float* weight, const float* bias, const float* scale,
                  const float* shift, float* output, float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H,
                  int64_t W, int64_t Cout, int weight_flags, int act, float slope, int pieces, const sstem::ConvExtra& ex, void* stream)
{
    if (!sstem::conv3x3_split_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout) ||
        (ex.f16 && !sstem::conv3x3_split_f16_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout)))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: outside the split kernel's range%s", what, range_note);
    if (!workspace || workspace_floats < sstem::conv3x3_split_packed_floats((int)Cin, (int)Cout, pieces, ex.f16))
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: workspace too small (see sstem_conv3x3_forward_workspace_floats_algo)", what);
    return launched(what, sstem::launch_conv3x3_split_mfma(input, weight, bias, scale, shift, output, workspace, workspace_floats, (int)N,
                                                           (int)Cin, (int)H, (int)W, (int)Cout, act, slope, weight_flags, pieces,
                                                           static_cast<hipStream_t>(stream), ex), " launch");
}

// the bf16-operand forward with fp32 or bf16 tensors at either end; the plain entry is the masked one without masks
int forward_bf16io(const char* what, const void* input, int input_bf16, const uint8_t* input_mask, const float* weight, const float* bias,
                   const float* scale, const float* shift, void* output, int output_bf16, uint8_t* output_mask, float* workspace,
                   int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int weight_flags, int act,
                   float slope, void* stream)
{
    if (!conv_sizes_ok(N, Cin, H, W, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "%s: bad shape", what);
    if (int rc = check_act(what, act)) return rc;
    if (int rc = check_weight_flags(what, weight_flags)) return rc;
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    if (input_bf16 && input_mask) return fail(SSTEM_ERR_UNSUPPORTED, "%s: input_mask needs an fp32 input tensor", what);
    if ((input_mask || output_mask) && (reinterpret_cast<uintptr_t>(input) & 15) != 0)
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: the masks need a 16-byte aligned input", what);
    if (Cin == 0 || !sstem::conv3x3_bf16_io_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout, output_bf16))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: needs W %% 4 == 0, a channel plane below 2 GiB and, for a bf16 output, an unsplit launch "
                                           "(sstem_conv3x3_bf16io_supported)", what);
    if (!workspace || workspace_floats < sstem::conv3x3_bf16_packed_floats((int)Cin, (int)Cout))
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: workspace too small (see sstem_conv3x3_forward_workspace_floats_algo)", what);
    return launched(what, sstem::launch_conv3x3_bf16_mfma_io(input, input_bf16 ? 1 : 0, weight, bias, scale, shift, output, output_bf16 ? 1 : 0,
                                                             workspace, workspace_floats, (int)N, (int)Cin, (int)H, (int)W, (int)Cout, act,
                                                             slope, weight_flags, static_cast<hipStream_t>(stream), input_mask, output_mask),
                    " launch");
}

// the two weight-gradient entries of the split kernels.  pieces == 0: the caller's algorithm id is no split-bf16 id
int backward_weight_split(const char* what, int pieces, bool any_null, const float* input, const float* input_amax, const float* grad_output,
                          const float* grad_amax, const uint8_t* grad_mask, float* grad_weight, float* grad_bias, float* workspace,
                          int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int accumulate, void* stream)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "%s: bad shape", what);
    if (!pieces) return fail(SSTEM_ERR_UNSUPPORTED, "%s: a split-bf16 id is needed (SSTEM_CONV_MFMA_BF16X6 / _BF16X3)", what);
    if (any_null) return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    if (Cin * Cout >= ((int64_t)1 << 31)) return fail(SSTEM_ERR_BAD_SHAPE, "%s: Cin*Cout too large", what);
    if (!sstem::conv3x3_wgrad_split_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: outside the split kernel's range", what);
    if (!workspace || workspace_floats < sstem::conv3x3_wgrad_split_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: workspace too small (see sstem_conv3x3_wgrad_workspace_floats_algo)", what);
    return launched(what, sstem::launch_conv3x3_wgrad_split_mfma(input, grad_output, grad_weight, grad_bias, workspace, (int)N, (int)Cin,
                                                                 (int)H, (int)W, (int)Cout, pieces, static_cast<hipStream_t>(stream),
                                                                 wgrad_flags(accumulate), grad_mask, input_amax, grad_amax), " launch");
}

// ---- validation scores (include/sstem_score.h): the three entries make the same checks, in this order, before any HIP call ----------
int score_checked(const char* what, bool any_null, bool images, int64_t B, int64_t H, int64_t W, const void* result,
                         const void* workspace, sstem::ScorePlan* plan, bool* empty)
{
    *empty = false;
    if (B < 0 || H < 0 || W < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (B == 0) { *empty = true; return SSTEM_OK; }
    if (any_null) return fail(SSTEM_ERR_NULL_POINTER, "%s: null pointer", what);
    if (images && (H < sstem::SCORE_TAPS || W < sstem::SCORE_TAPS))
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: H and W must be at least 11 (the 'valid' map of the 11 x 11 window would be empty)", what);
    if (!sstem::score_plan(B, H, W, plan))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (H, W <= 32768, B <= 2^24, at most 2^24 tiles of 32 x 16)", what);
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(result)) & 7)
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: the workspace and the result must be 8-byte aligned", what);
    return SSTEM_OK;
}

template <class T>
int score_images(const char* what, const T* a, const T* b, int64_t B, int64_t H, int64_t W, int clamp01_a, double* scores,
                        void* workspace, void* stream)
{
    sstem::ScorePlan plan;
    bool empty;
    const int rc = score_checked(what, !a || !b || !scores || !workspace, true, B, H, W, scores, workspace, &plan, &empty);
    if (rc != SSTEM_OK || empty) return rc;
    const hipError_t e = sstem::launch_score_images<T>(a, b, B, H, W, plan, clamp01_a ? 1 : 0, scores, workspace, static_cast<hipStream_t>(stream));
    return launched(what, e, " launch");
}

// ---- fold synthesis (include/sstem_fold.h): the range the kernels index in 32 bits (a plane below 2^30 pixels) ------------------------
bool fold_range_ok(int64_t n, int64_t H, int64_t W) { return n <= (1 << 24) && H <= 32768 && W <= 32768; }

}  // namespace

extern "C" {

int sstem_wgrad_deferred_count(void) { return sstem::wgrad_deferred_count(); }
void sstem_wgrad_deferred_drop(void) { sstem::wgrad_deferred_drop(); }
int sstem_wgrad_deferred_flush(void* stream)
{
    hipError_t e = sstem::wgrad_deferred_flush(static_cast<hipStream_t>(stream));
    return launched("grouped weight-gradient reduce launch", e);
}

int sstem_version(void) { return 100; }  // 0.1.0

const char* sstem_status_string(int status)
{
    switch (status) {
        case SSTEM_OK: return "ok";
        case SSTEM_ERR_NULL_POINTER: return "null pointer argument";
        case SSTEM_ERR_BAD_SHAPE: return "bad shape";
        case SSTEM_ERR_UNSUPPORTED: return "unsupported configuration";
        case SSTEM_ERR_HIP: return "HIP runtime error";
        case SSTEM_ERR_NO_DEVICE: return "no usable gfx950 device";
        default: return "unknown status";
    }
}

const char* sstem_last_error(void) { return g_last_error; }

int64_t sstem_sepconv_forward_bytes(int64_t B, int64_t C, int64_t H, int64_t W)
{
    return 4 * (B * C * (H + 50) * (W + 50) + 2 * B * 51 * H * W + B * C * H * W);
}

int64_t sstem_sepconv_backward_bytes(int64_t B, int64_t C, int64_t H, int64_t W)
{
    return 4 * (B * C * H * W + B * C * (H + 50) * (W + 50) + 4 * B * 51 * H * W);
}

int sstem_sepconv_forward_f32_algo(const float* input, const float* vertical,
                                   const float* horizontal, float* output,
                                   int64_t B, int64_t C, int64_t H, int64_t W,
                                   void* stream, int algo)
{
    if (!sizes_ok(B, C, H, W)) return fail(SSTEM_ERR_BAD_SHAPE, "forward: negative or oversized shape");
    if (B == 0 || C == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !vertical || !horizontal || !output)
        return fail(SSTEM_ERR_NULL_POINTER, "forward: null tensor pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (algo == SSTEM_SEPCONV_AUTO)
        algo = sstem::mfma_grid_ok(B, H, W) ? SSTEM_SEPCONV_MFMA : SSTEM_SEPCONV_DIRECT;
    if (algo == SSTEM_SEPCONV_MFMA) {
        if (!sstem::mfma_grid_ok(B, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "forward: grid too large for the MFMA kernel");
        e = sstem::launch_fwd_mfma(input, vertical, horizontal, output, B, C, H, W, s);
    } else if (algo == SSTEM_SEPCONV_DIRECT) {
        e = sstem::launch_fwd_direct(input, vertical, horizontal, output, B, C, H, W,
                                     SSTEM_SEPCONV_FILTER, s);
    } else {
        return fail(SSTEM_ERR_UNSUPPORTED, "forward: unknown algorithm id");
    }
    return launched("sepconv forward launch", e);
}

int sstem_sepconv_forward_f32(const float* input, const float* vertical,
                              const float* horizontal, float* output,
                              int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    return sstem_sepconv_forward_f32_algo(input, vertical, horizontal, output, B, C, H, W,
                                          stream, SSTEM_SEPCONV_AUTO);
}

int sstem_sepconv_interp_apply_f32(const float* i1, const float* i2,
                                   const float* k1v, const float* k1h,
                                   const float* k2v, const float* k2h, float* output,
                                   int64_t B, int64_t H, int64_t W, void* stream)
{
    return interp_apply("interp apply", APPLY_RGB, !i1 || !i2 || !k1v || !k1h || !k2v || !k2h || !output, B, H, W, "grid too large", "", [&] {
        return sstem::launch_interp_fused(i1, i2, k1v, k1h, k2v, k2h, output, B, H, W, static_cast<hipStream_t>(stream));
    });
}

// the three fp32 gray entries: the NCHW or the blocked kernel, with or without the uint8 copy of the output
static int interp_apply_gray(const char* what, ApplyKind kind, const char* range_note, const float* g1, const float* g2, const float* k1v,
                             const float* k1h, const float* k2v, const float* k2h, float* output, uint8_t* output_u8, bool need_u8,
                             int64_t B, int64_t H, int64_t W, void* stream)
{
    const bool any_null = !g1 || !g2 || !k1v || !k1h || !k2v || !k2h || !output || (need_u8 && !output_u8);
    return interp_apply(what, kind, any_null, B, H, W, "grid too large", range_note, [&] {
        return (kind == APPLY_GRAY_BLOCKED ? sstem::launch_interp_fused_gray_blocked : sstem::launch_interp_fused_gray)(
            g1, g2, k1v, k1h, k2v, k2h, output, B, H, W, static_cast<hipStream_t>(stream), output_u8);
    });
}

int sstem_sepconv_interp_apply_gray_f32(const float* g1, const float* g2,
                                        const float* k1v, const float* k1h,
                                        const float* k2v, const float* k2h, float* output,
                                        int64_t B, int64_t H, int64_t W, void* stream)
{
    return interp_apply_gray("gray interp apply", APPLY_GRAY, "51*H*W*4 bytes per image must stay below 4 GiB "
                             "(use sstem_sepconv_interp_apply_f32 on the replicated frames)",
                             g1, g2, k1v, k1h, k2v, k2h, output, nullptr, false, B, H, W, stream);
}

int sstem_sepconv_interp_apply_gray_supported(int64_t B, int64_t H, int64_t W) { return apply_supported(APPLY_GRAY, B, H, W); }

int64_t sstem_sepconv_coef_blocked_floats(int64_t B, int64_t H, int64_t W)
{
    if (!sizes_ok(B, 3, H, W)) return 0;
    return sstem::coef_blocked_floats(B, H, W);
}

int sstem_sepconv_coef_to_blocked_f32(const float* coef, float* blocked, int64_t B, int64_t H, int64_t W, void* stream)
{
    if (!sizes_ok(B, 3, H, W)) return fail(SSTEM_ERR_BAD_SHAPE, "coef to blocked: negative or oversized shape");
    if (B == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!coef || !blocked) return fail(SSTEM_ERR_NULL_POINTER, "coef to blocked: null tensor pointer");
    hipError_t e = sstem::launch_coef_to_blocked(coef, blocked, B, H, W, static_cast<hipStream_t>(stream));
    return launched("coef to blocked launch", e);
}

int sstem_sepconv_interp_apply_gray_blocked_supported(int64_t B, int64_t H, int64_t W) { return apply_supported(APPLY_GRAY_BLOCKED, B, H, W); }

int sstem_sepconv_interp_apply_gray_blocked_f32(const float* g1, const float* g2,
                                                const float* k1v, const float* k1h,
                                                const float* k2v, const float* k2h, float* output,
                                                int64_t B, int64_t H, int64_t W, void* stream)
{
    return interp_apply_gray("blocked gray interp apply", APPLY_GRAY_BLOCKED, "one image's blocked coefficients must stay below 4 GiB",
                             g1, g2, k1v, k1h, k2v, k2h, output, nullptr, false, B, H, W, stream);
}

int sstem_sepconv_interp_apply_gray_u8_f32(const float* g1, const float* g2, const float* k1v, const float* k1h,
                                           const float* k2v, const float* k2h, float* output, uint8_t* output_u8,
                                           int64_t B, int64_t H, int64_t W, int blocked_coefficients, void* stream)
{
    return interp_apply_gray("gray interp apply (uint8 store)", blocked_coefficients ? APPLY_GRAY_BLOCKED : APPLY_GRAY,
                             "one image's coefficients must stay below 4 GiB", g1, g2, k1v, k1h, k2v, k2h, output, output_u8, true, B, H, W,
                             stream);
}

int64_t sstem_sepconv_interp_apply_bytes(int64_t B, int64_t H, int64_t W, int frame_planes)
{
    return 4 * (2 * B * frame_planes * H * W + 4 * B * 51 * H * W + B * H * W);
}

int sstem_sepconv_backward_f32_algo(const float* grad_output, const float* input,
                                    const float* vertical, const float* horizontal,
                                    float* grad_input, float* grad_vertical,
                                    float* grad_horizontal,
                                    int64_t B, int64_t C, int64_t H, int64_t W,
                                    void* stream, int algo)
{
    (void)grad_input;  // never written: kernel.cu:152-206 of the reference does not touch it either
    if (!sizes_ok(B, C, H, W)) return fail(SSTEM_ERR_BAD_SHAPE, "backward: negative or oversized shape");
    if (B == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (C > 3)
        return fail(SSTEM_ERR_UNSUPPORTED,
                    "backward: C > 3 (the reference kernels hard-code three channels, kernel.cu:100-108)");
    if (!vertical || !horizontal || !grad_vertical || !grad_horizontal || (C > 0 && (!grad_output || !input)))
        return fail(SSTEM_ERR_NULL_POINTER, "backward: null tensor pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (C == 0) {  // sum over zero channels
        const size_t bytes = (size_t)B * 51 * H * W * sizeof(float);
        hipError_t e = hipMemsetAsync(grad_vertical, 0, bytes, s);
        if (e == hipSuccess) e = hipMemsetAsync(grad_horizontal, 0, bytes, s);
        return launched("sepconv backward memset", e);
    }
    hipError_t e;
    if (algo == SSTEM_SEPCONV_AUTO)
        algo = sstem::mfma_grid_ok(B, H, W) ? SSTEM_SEPCONV_MFMA : SSTEM_SEPCONV_DIRECT;
    if (algo == SSTEM_SEPCONV_MFMA) {
        if (!sstem::mfma_grid_ok(B, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "backward: grid too large for the MFMA kernel");
        e = sstem::launch_bwd_mfma(grad_output, input, vertical, horizontal, grad_vertical,
                                   grad_horizontal, B, C, H, W, s);
    } else if (algo == SSTEM_SEPCONV_DIRECT) {
        e = sstem::launch_bwd_direct(grad_output, input, vertical, horizontal, grad_vertical,
                                     grad_horizontal, B, C, H, W, SSTEM_SEPCONV_FILTER, s);
    } else {
        return fail(SSTEM_ERR_UNSUPPORTED, "backward: unknown algorithm id");
    }
    return launched("sepconv backward launch", e);
}

int sstem_sepconv_backward_f32(const float* grad_output, const float* input,
                               const float* vertical, const float* horizontal,
                               float* grad_input, float* grad_vertical, float* grad_horizontal,
                               int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    return sstem_sepconv_backward_f32_algo(grad_output, input, vertical, horizontal, grad_input,
                                           grad_vertical, grad_horizontal, B, C, H, W, stream,
                                           SSTEM_SEPCONV_AUTO);
}

// ---- dense convolution blocks (include/sstem_conv.h) -------------------------------------------
int64_t sstem_conv3x3_workspace_floats(int64_t Cin, int64_t Cout)
{
    if (!channels_ok(Cin, Cout)) return 0;
    return sstem::conv3x3_workspace_floats((int)Cin, (int)Cout);
}

int64_t sstem_conv3x3_forward_workspace_floats(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout)
{
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || Cin <= 0 || Cout <= 0) return 0;
    return sstem::conv3x3_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
}

int64_t sstem_conv3x3_packed_floats(int64_t Cin, int64_t Cout, int algo)
{
    if (!channels_ok(Cin, Cout)) return 0;
    const ConvAlgo a = conv_algo(algo);
    switch (a.family) {
        case FAMILY_BF16: return sstem::conv3x3_bf16_packed_floats((int)Cin, (int)Cout);
        case FAMILY_SPLIT: return sstem::conv3x3_split_packed_floats((int)Cin, (int)Cout, a.pieces, a.f16);
        case FAMILY_FP32: return sstem::conv3x3_workspace_floats((int)Cin, (int)Cout);
        default: return 0;
    }
}

int sstem_conv3x3_pack_weights_f32(const float* weight, int64_t Cin, int64_t Cout, int algo, float* packed_forward,
                                   float* packed_transposed, void* stream)
{
    if (!channels_ok(Cin, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "pack_weights: bad shape");
    if (!weight) return fail(SSTEM_ERR_NULL_POINTER, "pack_weights: null weight");
    if (!packed_forward && !packed_transposed) return SSTEM_OK;
    const ConvAlgo a = conv_algo(algo);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    switch (a.family) {
        case FAMILY_BF16: e = sstem::launch_pack_weights_3x3_bf16_both(weight, packed_forward, packed_transposed, (int)Cin, (int)Cout, s); break;
        case FAMILY_SPLIT:
            e = a.f16 ? sstem::launch_pack_weights_3x3_split_f16_both(weight, packed_forward, packed_transposed, (int)Cin, (int)Cout, s)
                      : sstem::launch_pack_weights_3x3_split_both(weight, packed_forward, packed_transposed, (int)Cin, (int)Cout, a.pieces, s);
            break;
        case FAMILY_FP32: e = sstem::launch_pack_weights_3x3_both(weight, packed_forward, packed_transposed, (int)Cin, (int)Cout, s); break;
        default: return fail(SSTEM_ERR_UNSUPPORTED, "pack_weights: an explicit MFMA algorithm id is needed (SSTEM_CONV_MFMA or _MFMA_BF16)");
    }
    return launched("pack_weights launch", e);
}

int64_t sstem_conv3x3_pack_group_entry(int64_t Cin, int64_t Cout, int algo, int64_t* entry16)
{
    if (!entry16 || !channels_ok(Cin, Cout)) return 0;
    const ConvAlgo a = conv_algo(algo);
    switch (a.family) {
        case FAMILY_BF16: return sstem::pack_group_entry_bf16((int)Cin, (int)Cout, entry16);
        case FAMILY_SPLIT:
            return a.f16 ? sstem::pack_group_entry_split_f16((int)Cin, (int)Cout, entry16)
                         : sstem::pack_group_entry_split((int)Cin, (int)Cout, a.pieces, entry16);
        case FAMILY_FP32: return sstem::pack_group_entry((int)Cin, (int)Cout, entry16);
        default: return 0;
    }
}

int sstem_conv3x3_pack_weights_group_f32(const int64_t* table, int64_t n_entries, int64_t total_blocks, int algo, void* stream)
{
    if (n_entries < 0 || total_blocks < 0 || n_entries > (1 << 20)) return fail(SSTEM_ERR_BAD_SHAPE, "pack group: bad counts");
    if (n_entries == 0) return SSTEM_OK;
    if (!table) return fail(SSTEM_ERR_NULL_POINTER, "pack group: null table");
    const ConvAlgo a = conv_algo(algo);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (a.family == FAMILY_BF16)
        e = sstem::launch_pack_weights_3x3_bf16_group(table, (int)n_entries, total_blocks, s);
    else if (a.split_bf16())                                     // the fp16 id has its own group entry, below
        e = sstem::launch_pack_weights_3x3_split_group(table, (int)n_entries, total_blocks, a.pieces, s);
    else if (a.family == FAMILY_FP32)
        e = sstem::launch_pack_weights_3x3_group(table, (int)n_entries, total_blocks, s);
    else
        return fail(SSTEM_ERR_UNSUPPORTED, "pack group: an explicit MFMA algorithm id is needed");
    return launched("pack group launch", e);
}

int sstem_conv3x3_pack_weights_group_f16(const int64_t* table, int64_t n_entries, int64_t total_blocks, int64_t bound_blocks, float* bounds,
                                         void* stream)
{
    if (n_entries < 0 || total_blocks < 0 || bound_blocks < 0 || n_entries > (1 << 20)) return fail(SSTEM_ERR_BAD_SHAPE, "pack group f16: bad counts");
    if (n_entries == 0) return SSTEM_OK;
    if (!table || !bounds) return fail(SSTEM_ERR_NULL_POINTER, "pack group f16: null table / bounds");
    const hipError_t e = sstem::launch_pack_weights_3x3_split_f16_group(table, (int)n_entries, total_blocks, bound_blocks, bounds,
                                                                        static_cast<hipStream_t>(stream));
    return launched("pack group f16 launch", e);
}

int64_t sstem_conv3x3_forward_workspace_floats_algo(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int algo)
{
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || Cin <= 0 || Cout <= 0) return 0;
    const ConvAlgo a = conv_algo(algo);
    switch (a.family) {
        case FAMILY_BF16: return sstem::conv3x3_bf16_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
        case FAMILY_SPLIT: return sstem::conv3x3_split_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout, a.pieces, a.f16);
        case FAMILY_DIRECT: return 0;
        default: return sstem::conv3x3_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);      // AUTO and any other id: the fp32 plan
    }
}

int sstem_conv2d_forward_f32(const float* input, const float* weight, const float* bias,
                             const float* scale, const float* shift, float* output,
                             float* workspace, int64_t workspace_floats,
                             int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                             int KH, int KW, int pad_h, int pad_w, int weight_transposed,
                             int act, float slope, void* stream, int algo)
{
    return sstem_conv2d_forward_ex_f32(input, weight, bias, scale, shift, nullptr, 1.f, output, nullptr, workspace, workspace_floats,
                                       N, Cin, H, W, Cout, KH, KW, pad_h, pad_w, weight_transposed, act, slope, stream, algo);
}

int64_t sstem_conv_bn_partials(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int KH, int KW, int transposed, int algo)
{
    if (!conv_sizes_positive(N, Cin, transposed ? 2 * H : H, transposed ? 2 * W : W, Cout)) return 0;
    if (KH != 3 || KW != 3) return 0;
    if (algo == SSTEM_CONV_AUTO) algo = (N * ((Cout + 31) / 32) < 65536) ? SSTEM_CONV_MFMA : SSTEM_CONV_DIRECT;
    if (algo != SSTEM_CONV_MFMA) return 0;
    if (transposed) return sstem::convT3x3s2_bn_partials((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    return sstem::conv3x3_bn_partials((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
}

int sstem_conv2d_forward_ex_f32(const float* input, const float* weight, const float* bias,
                                const float* scale, const float* shift, const float* residual, float residual_scale,
                                float* output, float* bn_partials, float* workspace, int64_t workspace_floats,
                                int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                int KH, int KW, int pad_h, int pad_w, int weight_transposed,
                                int act, float slope, void* stream, int algo)
{
    const sstem::ConvExtra ex{residual, residual_scale, bn_partials, 0};
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || KH <= 0 || KW <= 0 || pad_h < 0 || pad_w < 0)
        return fail(SSTEM_ERR_BAD_SHAPE, "conv2d: bad shape");
    if (2 * pad_h != KH - 1 || 2 * pad_w != KW - 1)
        return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: only stride-1 'same' padding is supported");
    if (int rc = check_act("conv2d", act)) return rc;
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "conv2d: null tensor pointer");
    const bool is3x3 = (KH == 3 && KW == 3);
    if (weight_transposed && !is3x3) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: transposed weights need 3x3");
    if (weight_transposed < 0 || weight_transposed > 3) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: unknown weight_transposed flags");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (algo == SSTEM_CONV_AUTO) algo = (is3x3 && Cin > 0 && N * ((Cout + 31) / 32) < 65536) ? SSTEM_CONV_MFMA : SSTEM_CONV_DIRECT;
    const ConvAlgo a = conv_algo(algo);
    hipError_t e;
    if (a.family == FAMILY_FP32) {
        if (!is3x3 || Cin == 0) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: the MFMA kernel is 3x3/s1/p1 only");
        const int64_t need = sstem::conv3x3_workspace_floats((int)Cin, (int)Cout);
        if (!workspace || workspace_floats < need)
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d: workspace too small (see sstem_conv3x3_workspace_floats)");
        if (bn_partials && (scale || shift || act != 0 || residual))
            return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: bn_partials are the statistics of the raw conv + bias output (no affine, activation or residual)");
        if (bn_partials && workspace_floats < sstem::conv3x3_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d: bn_partials need the full workspace (sstem_conv3x3_forward_workspace_floats)");
        e = sstem::launch_conv3x3_mfma(input, weight, bias, scale, shift, output, workspace, workspace_floats, (int)N,
                                       (int)Cin, (int)H, (int)W, (int)Cout, act, slope, weight_transposed & 3, s, ex);
    } else if (a.split_bf16()) {                                 // the fp16 id is for sstem_conv3x3_forward_scaled_f32 only
        if (!is3x3 || Cin == 0) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: the split-bf16 MFMA kernel is 3x3/s1/p1 only");
        if (bn_partials) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: bn_partials need the fp32 3x3 MFMA kernel (SSTEM_CONV_MFMA)");
        if (!sstem::conv3x3_split_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
            return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: the split-bf16 MFMA kernel needs a channel plane (W % 4 == 0) or a whole input image below 2 GiB");
        if (!workspace || workspace_floats < sstem::conv3x3_split_packed_floats((int)Cin, (int)Cout, a.pieces))
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d: workspace too small (see sstem_conv3x3_forward_workspace_floats_algo)");
        e = sstem::launch_conv3x3_split_mfma(input, weight, bias, scale, shift, output, workspace, workspace_floats, (int)N, (int)Cin,
                                             (int)H, (int)W, (int)Cout, act, slope, weight_transposed & 3, a.pieces, s, ex);
    } else if (residual || bn_partials) {
        return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: residual / bn_partials need the fp32 3x3 MFMA kernel (SSTEM_CONV_MFMA)");
    } else if (a.family == FAMILY_BF16) {
        if (!is3x3 || Cin == 0) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: the bf16 MFMA kernel is 3x3/s1/p1 only");
        if (!sstem::conv3x3_bf16_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
            return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: the bf16 MFMA kernel needs a channel plane (W % 4 == 0) or a whole input image below 2 GiB");
        if (!workspace || workspace_floats < sstem::conv3x3_bf16_packed_floats((int)Cin, (int)Cout))
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d: workspace too small (see sstem_conv3x3_forward_workspace_floats_algo)");
        e = sstem::launch_conv3x3_bf16_mfma(input, weight, bias, scale, shift, output, workspace, workspace_floats, (int)N,
                                            (int)Cin, (int)H, (int)W, (int)Cout, act, slope, weight_transposed & 3, s);
    } else if (a.family == FAMILY_DIRECT) {
        if (weight_transposed) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: direct kernel takes plain [Cout,Cin,KH,KW] weights only");
        e = sstem::launch_conv2d_direct(input, weight, bias, scale, shift, output, (int)N, (int)Cin, (int)H,
                                        (int)W, (int)Cout, KH, KW, pad_h, pad_w, act, slope, s);
    } else {
        return fail(SSTEM_ERR_UNSUPPORTED, "conv2d: unknown algorithm id");
    }
    return launched("conv2d launch", e);
}

int sstem_conv3x3_forward_masked_f32(const float* input, const uint8_t* input_mask, const float* weight, const float* bias,
                                     const float* scale, const float* shift, float* output, uint8_t* output_mask,
                                     float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H, int64_t W,
                                     int64_t Cout, int weight_flags, int act, float slope, void* stream, int algo)
{
    const char* what = "conv3x3 masked";
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || Cin <= 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: bad shape", what);
    if (int rc = check_act(what, act)) return rc;
    if (int rc = check_weight_flags(what, weight_flags)) return rc;
    const ConvAlgo a = conv_algo(algo);
    if (!a.split_bf16()) return fail(SSTEM_ERR_UNSUPPORTED, "%s: a split-bf16 id is needed (SSTEM_CONV_MFMA_BF16X6 / _BF16X3)", what);
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    const sstem::ConvExtra ex{nullptr, 1.f, nullptr, 0, input_mask, output_mask};
    return split_forward(what, "", input, weight, bias, scale, shift, output, workspace, workspace_floats, N, Cin, H, W, Cout, weight_flags, act,
                         slope, a.pieces, ex, stream);
}

int64_t sstem_amax_word_floats(void) { return 1024; }

int sstem_amax_f32(const float* x, int64_t n, float* word, void* stream)
{
    if (n < 0) return fail(SSTEM_ERR_BAD_SHAPE, "amax: negative count");
    if (n == 0) return SSTEM_OK;
    if (!x || !word) return fail(SSTEM_ERR_NULL_POINTER, "amax: null pointer");
    const hipError_t e = sstem::launch_amax(x, n, word, static_cast<hipStream_t>(stream));
    return launched("amax launch", e);
}

int sstem_conv3x3_forward_scaled_f32(const float* input, const float* input_amax, const float* weight, const float* bias,
                                     const float* scale, const float* shift, const float* residual, float residual_scale,
                                     float* output, float* output_amax, float* workspace, int64_t workspace_floats,
                                     int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int weight_flags, int act, float slope,
                                     void* stream, int algo, int output_layout)
{
    return sstem_conv3x3_forward_scaled_strided_f32(input, input_amax, weight, bias, scale, shift, residual, residual_scale, output, output_amax,
                                                    workspace, workspace_floats, N, Cin, H, W, Cout, weight_flags, act, slope, stream, algo,
                                                    output_layout, 0, nullptr, SSTEM_POOL_NONE);
}

int sstem_conv3x3_forward_scaled_strided_f32(const float* input, const float* input_amax, const float* weight, const float* bias,
                                             const float* scale, const float* shift, const float* residual, float residual_scale,
                                             float* output, float* output_amax, float* workspace, int64_t workspace_floats,
                                             int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int weight_flags, int act, float slope,
                                             void* stream, int algo, int output_layout, int64_t output_image_stride, float* pooled_output,
                                             int pool_kind)
{
    if (pooled_output && (pool_kind != SSTEM_POOL_MAX && pool_kind != SSTEM_POOL_AVG))
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: unknown pooling kind");
    if (pooled_output && (algo != SSTEM_CONV_MFMA_F16X3 || output_layout != SSTEM_LAYOUT_NCHW || residual || H % 8 != 0 || W % 32 != 0))
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: a pooled copy needs SSTEM_CONV_MFMA_F16X3, the NCHW store without residual, H % 8 == 0 and W % 32 == 0");
    if (output_image_stride != 0 && (output_layout == SSTEM_LAYOUT_ROW_SEGMENTS || output_image_stride < Cout * H * W))
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: an output image stride is for NCHW / sub-pixel stores and cannot be smaller than one image");
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || Cin <= 0) return fail(SSTEM_ERR_BAD_SHAPE, "conv3x3 scaled: bad shape");
    if (output_layout != SSTEM_LAYOUT_NCHW && output_layout != SSTEM_LAYOUT_ROW_SEGMENTS && output_layout != SSTEM_LAYOUT_CONVT_PARITY)
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: unknown output layout");
    if (output_layout == SSTEM_LAYOUT_CONVT_PARITY &&
        (algo != SSTEM_CONV_MFMA_F16X3 || Cout % 128 != 0 || Cin % 16 != 0 || W % 4 != 0 || Cout * H * W * 4 >= ((int64_t)1 << 32)))
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: the sub-pixel ConvTranspose store needs SSTEM_CONV_MFMA_F16X3, Cout = 4 C with C a multiple "
                                           "of 32, Cin a multiple of 16, W a multiple of 4 and one output image below 4 GiB");
    if (output_layout == SSTEM_LAYOUT_ROW_SEGMENTS && (residual || H * ((W + 63) / 64) * Cout * 256 >= ((int64_t)1 << 32)))
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: the row-segment output takes no residual and one image of it must stay below 4 GiB");
    if (int rc = check_act("conv3x3 scaled", act)) return rc;
    if (int rc = check_weight_flags("conv3x3 scaled", weight_flags)) return rc;
    if (algo == SSTEM_CONV_DIRECT) {
        // the streaming fp32 kernel for a handful of output channels: exact fp32 products, so no input bound is read; it leaves the
        // output's bound like the split ids do (a link of an fp16 chain)
        if (residual || output_layout != SSTEM_LAYOUT_NCHW || pooled_output || weight_flags != 0 ||
            (output_image_stride != 0 && output_image_stride != Cout * H * W))
            return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: SSTEM_CONV_DIRECT takes plain weights and stores plain NCHW (no residual, pooled copy or image stride)");
        if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
        if (!input || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "conv3x3 scaled: null tensor pointer");
        if (!sstem::conv3x3_stream_small_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
            return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: SSTEM_CONV_DIRECT here is the streaming kernel (sstem_conv3x3_stream_small_supported)");
        const hipError_t e = sstem::launch_conv3x3_stream_small(input, weight, bias, scale, shift, output, (int)N, (int)Cin, (int)H, (int)W,
                                                                (int)Cout, act, slope, output_amax, static_cast<hipStream_t>(stream));
        return launched("conv3x3 scaled launch (streaming kernel)", e);
    }
    const ConvAlgo a = conv_algo(algo);
    if (a.family != FAMILY_SPLIT)
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 scaled: a split id (SSTEM_CONV_MFMA_F16X3 / _BF16X6 / _BF16X3) or SSTEM_CONV_DIRECT is needed");
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !weight || (!output && !pooled_output)) return fail(SSTEM_ERR_NULL_POINTER, "conv3x3 scaled: null tensor pointer");
    if (a.f16 && !input_amax) return fail(SSTEM_ERR_NULL_POINTER, "conv3x3 scaled: SSTEM_CONV_MFMA_F16X3 needs the input's amax word (sstem_amax_f32)");
    const sstem::ConvExtra ex{residual, residual_scale, nullptr, 0, nullptr, nullptr, input_amax, output_amax, a.f16,
                              output_layout == SSTEM_LAYOUT_ROW_SEGMENTS ? 1 : (output_layout == SSTEM_LAYOUT_CONVT_PARITY ? 2 : 0),
                              output_image_stride == Cout * H * W ? 0 : output_image_stride, pooled_output, pooled_output ? pool_kind : 0};
    return split_forward("conv3x3 scaled", " (sstem_conv3x3_algo_supported)", input, weight, bias, scale, shift, output, workspace,
                         workspace_floats, N, Cin, H, W, Cout, weight_flags, act, slope, a.pieces, ex, stream);
}

int sstem_conv3x3_forward_scaled_masked_f32(const float* input, const float* input_amax, const uint8_t* input_mask, const float* weight,
                                            const float* bias, const float* scale, const float* shift, float* output, float* output_amax,
                                            uint8_t* output_mask, float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin,
                                            int64_t H, int64_t W, int64_t Cout, int weight_flags, int act, float slope, void* stream)
{
    const char* what = "conv3x3 scaled masked";
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || Cin <= 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: bad shape", what);
    if (int rc = check_act(what, act)) return rc;
    if (int rc = check_weight_flags(what, weight_flags)) return rc;
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !input_amax || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    if ((input_mask || output_mask) && (W % 4 != 0 || (reinterpret_cast<uintptr_t>(input) & 15) != 0))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: the masked fp16 instances take W %% 4 == 0 and a 16-byte aligned input", what);
    const sstem::ConvExtra ex{nullptr, 1.f, nullptr, 0, input_mask, output_mask, input_amax, output_amax, 1, 0, 0, nullptr, 0};
    return split_forward(what, " (sstem_conv3x3_algo_supported)", input, weight, bias, scale, shift, output, workspace, workspace_floats, N, Cin,
                         H, W, Cout, weight_flags, act, slope, 2, ex, stream);
}

int sstem_conv3x3_backward_weight_masked_f32(const float* input, const float* grad_output, const uint8_t* grad_mask, float* grad_weight,
                                             float* grad_bias, float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin,
                                             int64_t H, int64_t W, int64_t Cout, int accumulate, void* stream, int algo)
{
    const ConvAlgo a = conv_algo(algo);
    return backward_weight_split("conv3x3 wgrad masked", a.split_bf16() ? a.pieces : 0, !input || !grad_output || !grad_weight, input, nullptr,
                                 grad_output, nullptr, grad_mask, grad_weight, grad_bias, workspace, workspace_floats, N, Cin, H, W, Cout,
                                 accumulate, stream);
}

int sstem_conv3x3_backward_weight_scaled_masked_f32(const float* input, const float* input_amax, const float* grad_output,
                                                    const float* grad_amax, const uint8_t* grad_mask, float* grad_weight, float* grad_bias,
                                                    float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H,
                                                    int64_t W, int64_t Cout, int accumulate, void* stream)
{
    return backward_weight_split("conv3x3 wgrad scaled", 2, !input || !input_amax || !grad_output || !grad_amax || !grad_weight, input,
                                 input_amax, grad_output, grad_amax, grad_mask, grad_weight, grad_bias, workspace, workspace_floats, N, Cin, H,
                                 W, Cout, accumulate, stream);
}

int sstem_conv3x3_algo_supported(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int algo)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout)) return 0;
    const ConvAlgo a = conv_algo(algo);
    if (a.family == FAMILY_DIRECT) return 1;
    if (a.family == FAMILY_SPLIT && a.f16) return sstem::conv3x3_split_f16_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout) ? 1 : 0;
    if (a.family == FAMILY_BF16 || a.family == FAMILY_SPLIT) return sstem::conv3x3_bf16_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout) ? 1 : 0;
    if (a.family == FAMILY_FP32 || algo == SSTEM_CONV_AUTO) return N * ((Cout + 31) / 32) < 65536 ? 1 : 0;
    return 0;
}

int sstem_conv3x3_first_layer_u8_supported(int64_t N, int64_t H, int64_t W, int64_t Cout)
{
    if (N < 0 || H < 0 || W < 0 || N > 65535 || H > (1 << 20) || W > (1 << 20)) return 0;
    return sstem::conv3x3_first_u8_supported((int)N, (int)H, (int)W, (int)Cout) ? 1 : 0;
}

int sstem_conv3x3_first_layer_u8(const uint8_t* frames, const float* weight, const float* bias, float* output, float* planes,
                                 float* output_amax, int64_t N, int64_t H, int64_t W, int64_t Cout, int act, float slope, void* stream)
{
    if (!sstem_conv3x3_first_layer_u8_supported(N, H, W, Cout))
        return fail(SSTEM_ERR_UNSUPPORTED, "first layer from uint8 frames: Conv2d(6 -> 6), W % 4 == 0, 2*H*W < 2^31");
    if (!frames || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "first layer from uint8 frames: null pointer");
    if (!act_ok(act)) return fail(SSTEM_ERR_UNSUPPORTED, "first layer from uint8 frames: unknown activation");
    hipError_t e = sstem::launch_conv3x3_first_u8(frames, weight, bias, output, planes, (int)N, (int)H, (int)W, (int)Cout, act, slope,
                                                  output_amax, static_cast<hipStream_t>(stream));
    return launched("first layer from uint8 frames launch", e);
}

int sstem_conv3x3_stream_small_supported(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout)) return 0;
    return sstem::conv3x3_stream_small_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout) ? 1 : 0;
}

int sstem_conv3x3_bf16io_supported(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int output_bf16)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout)) return 0;
    return sstem::conv3x3_bf16_io_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout, output_bf16) ? 1 : 0;
}

int sstem_conv3x3_forward_bf16io(const void* input, int input_bf16, const float* weight, const float* bias, const float* scale,
                                 const float* shift, void* output, int output_bf16, float* workspace, int64_t workspace_floats,
                                 int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int weight_flags, int act, float slope,
                                 void* stream)
{
    return forward_bf16io("conv3x3 bf16io", input, input_bf16, nullptr, weight, bias, scale, shift, output, output_bf16, nullptr, workspace,
                          workspace_floats, N, Cin, H, W, Cout, weight_flags, act, slope, stream);
}

int sstem_conv3x3_forward_bf16io_masked(const void* input, int input_bf16, const uint8_t* input_mask, const float* weight, const float* bias,
                                        const float* scale, const float* shift, void* output, int output_bf16, uint8_t* output_mask,
                                        float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H, int64_t W,
                                        int64_t Cout, int weight_flags, int act, float slope, void* stream)
{
    return forward_bf16io("conv3x3 bf16io masked", input, input_bf16, input_mask, weight, bias, scale, shift, output, output_bf16, output_mask,
                          workspace, workspace_floats, N, Cin, H, W, Cout, weight_flags, act, slope, stream);
}

int sstem_conv3x3_backward_weight_bf16_masked(const void* input, int input_bf16, const float* grad_output, const uint8_t* grad_mask,
                                              float* grad_weight, float* grad_bias, float* workspace, int64_t workspace_floats, int64_t N,
                                              int64_t Cin, int64_t H, int64_t W, int64_t Cout, int accumulate, void* stream)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout))
        return fail(SSTEM_ERR_BAD_SHAPE, "conv3x3 wgrad bf16 masked: bad shape");
    if (!input || !grad_output || !grad_weight) return fail(SSTEM_ERR_NULL_POINTER, "conv3x3 wgrad bf16 masked: null tensor pointer");
    if (W % 4 != 0 || ((reinterpret_cast<uintptr_t>(input) | reinterpret_cast<uintptr_t>(grad_output)) & 15) != 0)
        return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 wgrad bf16 masked: needs W % 4 == 0 and 16-byte aligned tensors");
    if (Cin * Cout >= ((int64_t)1 << 31)) return fail(SSTEM_ERR_BAD_SHAPE, "conv3x3 wgrad bf16 masked: Cin*Cout too large");
    const int64_t need = sstem::conv3x3_wgrad_bf16_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    if (!workspace || workspace_floats < need)
        return fail(SSTEM_ERR_BAD_SHAPE, "conv3x3 wgrad bf16 masked: workspace too small (see sstem_conv3x3_wgrad_workspace_floats_algo)");
    hipError_t e = sstem::launch_conv3x3_wgrad_bf16_mfma_in(input, input_bf16 ? 1 : 0, grad_output, grad_weight, grad_bias, workspace, (int)N,
                                                            (int)Cin, (int)H, (int)W, (int)Cout, static_cast<hipStream_t>(stream),
                                                            wgrad_flags(accumulate), grad_mask);
    return launched("conv3x3 wgrad bf16 masked launch", e);
}

int sstem_conv_transpose3x3s2_forward_f32(const float* input, const float* weight, const float* bias,
                                          const float* scale, const float* shift, float* output,
                                          int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                          int act, float slope, void* stream)
{
    if (!conv_sizes_ok(N, Cin, 2 * H, 2 * W, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose: bad shape");
    if (int rc = check_act("conv_transpose", act)) return rc;
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose: null tensor pointer");
    hipError_t e = sstem::launch_convT3x3s2_direct(input, weight, bias, scale, shift, output, (int)N, (int)Cin,
                                                   (int)H, (int)W, (int)Cout, act, slope,
                                                   static_cast<hipStream_t>(stream));
    return launched("conv_transpose launch", e);
}

int64_t sstem_conv_transpose3x3s2_workspace_floats(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int which)
{
    if (!conv_sizes_positive(N, Cin, 2 * H, 2 * W, Cout)) return 0;
    const int64_t f = sstem::convT3x3s2_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    const int64_t d = sstem::convT3x3s2_dgrad_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    const int64_t g = sstem::convT3x3s2_wgrad_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    if (which == 0) return f;
    if (which == 1) return d;
    if (which == 2) return g;
    if (which == 3) return d > g ? d : g;
    return 0;
}

int sstem_conv_transpose3x3s2_forward_ex_f32(const float* input, const float* weight, const float* bias,
                                             const float* scale, const float* shift, const float* residual, float residual_scale,
                                             float* output, float* bn_partials, float* workspace, int64_t workspace_floats,
                                             int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                             int weight_flags, int act, float slope, void* stream)
{
    if (!conv_sizes_ok(N, Cin, 2 * H, 2 * W, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose: bad shape");
    if (int rc = check_act("conv_transpose", act)) return rc;
    if (weight_flags != 0 && weight_flags != SSTEM_CONV_WEIGHT_PREPACKED) return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose: unknown weight flags");
    if (N == 0 || Cout == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !weight || !output) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose: null tensor pointer");
    if (Cin == 0) return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose: no input channels");
    if (8 * H * W * 4 >= ((int64_t)1 << 32)) return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose: plane too large for the MFMA kernel's 32-bit offsets");
    const int64_t need = sstem::convT3x3s2_forward_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    const int64_t packed = sstem::conv3x3_workspace_floats((int)Cin, (int)Cout);
    if (!workspace || workspace_floats < (bn_partials ? need : packed))
        return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose: workspace too small (see sstem_conv_transpose3x3s2_workspace_floats)");
    if (bn_partials && (scale || shift || act != 0 || residual))
        return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose: bn_partials are the statistics of the raw output (no affine, activation or residual)");
    if (bn_partials && sstem::convT3x3s2_bn_partials((int)N, (int)Cin, (int)H, (int)W, (int)Cout) == 0)
        return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose: this launch is split over K and writes no statistics (sstem_conv_bn_partials == 0)");
    const sstem::ConvExtra ex{residual, residual_scale, bn_partials, 0};
    hipError_t e = sstem::launch_convT3x3s2_mfma(input, weight, bias, scale, shift, output, workspace, workspace_floats, (int)N, (int)Cin,
                                                 (int)H, (int)W, (int)Cout, act, slope, weight_flags ? 1 : 0,
                                                 static_cast<hipStream_t>(stream), ex);
    return launched("conv_transpose launch", e);
}

int sstem_conv_transpose3x3s2_backward_ex_f32(const float* input, const float* weight, const float* grad_output,
                                              float* grad_input, float* grad_weight, float* grad_bias,
                                              float* workspace, int64_t workspace_floats,
                                              int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                              int accumulate, void* stream)
{
    if (!conv_sizes_ok(N, Cin, 2 * H, 2 * W, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose backward: bad shape");
    if (Cin == 0 || Cout == 0) return SSTEM_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0 || H == 0 || W == 0) {
        if (!accumulate) {
            hipError_t e = grad_weight ? hipMemsetAsync(grad_weight, 0, (size_t)Cout * Cin * 9 * sizeof(float), s) : hipSuccess;
            if (e == hipSuccess && grad_bias) e = hipMemsetAsync(grad_bias, 0, (size_t)Cout * sizeof(float), s);
            if (e != hipSuccess) return hip_fail("conv_transpose backward memset", e);
        }
        return SSTEM_OK;
    }
    if (!grad_output) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose backward: null grad_output");
    if (grad_bias && !grad_weight) return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose backward: the bias gradient rides along with the weight gradient");
    if (8 * 4 * H * W * 4 >= ((int64_t)1 << 32)) return fail(SSTEM_ERR_UNSUPPORTED, "conv_transpose backward: plane too large for 32-bit offsets");
    if (grad_input) {
        if (!weight) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose backward: null weight");
        if (!workspace || workspace_floats < sstem::conv3x3_workspace_floats((int)Cout, (int)Cin))
            return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose backward: workspace too small (see sstem_conv_transpose3x3s2_workspace_floats)");
        hipError_t e = sstem::launch_convT3x3s2_dgrad_mfma(grad_output, weight, grad_input, workspace, workspace_floats, (int)N, (int)Cin,
                                                           (int)H, (int)W, (int)Cout, s);
        if (e != hipSuccess) return hip_fail("conv_transpose dgrad launch", e);
    }
    if (grad_weight) {
        if (!input) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose backward: null input");
        if (!workspace || workspace_floats < sstem::convT3x3s2_wgrad_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
            return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose backward: workspace too small (see sstem_conv_transpose3x3s2_workspace_floats)");
        hipError_t e = sstem::launch_convT3x3s2_wgrad_mfma(input, grad_output, grad_weight, grad_bias, workspace, (int)N, (int)Cin, (int)H,
                                                           (int)W, (int)Cout, s, wgrad_flags(accumulate));
        if (e != hipSuccess) return hip_fail("conv_transpose wgrad launch", e);
    }
    return SSTEM_OK;
}

int64_t sstem_conv3x3_wgrad_workspace_floats(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout)) return 0;
    return sstem::conv3x3_wgrad_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
}

int64_t sstem_conv3x3_wgrad_workspace_floats_algo(int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int algo)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout)) return 0;
    const ConvAlgo a = conv_algo(algo);
    if (a.family == FAMILY_BF16) return sstem::conv3x3_wgrad_bf16_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    if (a.family == FAMILY_SPLIT && sstem::conv3x3_wgrad_split_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout))
        return sstem::conv3x3_wgrad_split_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    if (a.family == FAMILY_DIRECT) return 0;
    return sstem::conv3x3_wgrad_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
}

int sstem_conv2d_backward_weight_f32(const float* input, const float* grad_output, float* grad_weight,
                                     float* workspace, int64_t workspace_floats,
                                     int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                     int KH, int KW, int pad_h, int pad_w, void* stream, int algo)
{
    return sstem_conv2d_backward_weight_bias_f32(input, grad_output, grad_weight, nullptr, workspace, workspace_floats,
                                                 N, Cin, H, W, Cout, KH, KW, pad_h, pad_w, stream, algo);
}

int sstem_conv2d_backward_weight_bias_f32(const float* input, const float* grad_output, float* grad_weight,
                                          float* grad_bias, float* workspace, int64_t workspace_floats,
                                          int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                          int KH, int KW, int pad_h, int pad_w, void* stream, int algo)
{
    return sstem_conv2d_backward_weight_bias_ex_f32(input, grad_output, grad_weight, grad_bias, workspace, workspace_floats,
                                                    N, Cin, H, W, Cout, KH, KW, pad_h, pad_w, 0, stream, algo);
}

int sstem_conv2d_backward_weight_bias_ex_f32(const float* input, const float* grad_output, float* grad_weight,
                                             float* grad_bias, float* workspace, int64_t workspace_floats,
                                             int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                             int KH, int KW, int pad_h, int pad_w, int accumulate, void* stream, int algo)
{
    if (!conv_sizes_ok(N, Cin, H, W, Cout) || KH <= 0 || KW <= 0 || KH > 5 || KW > 5)
        return fail(SSTEM_ERR_BAD_SHAPE, "conv2d wgrad: bad shape (kernel up to 5x5)");
    if (2 * pad_h != KH - 1 || 2 * pad_w != KW - 1)
        return fail(SSTEM_ERR_UNSUPPORTED, "conv2d wgrad: only stride-1 'same' padding is supported");
    if (Cin == 0 || Cout == 0) return SSTEM_OK;
    if (!grad_weight) return fail(SSTEM_ERR_NULL_POINTER, "conv2d wgrad: null grad_weight");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0 || H == 0 || W == 0) {
        if (accumulate) return SSTEM_OK;
        hipError_t e = hipMemsetAsync(grad_weight, 0, (size_t)Cout * Cin * KH * KW * sizeof(float), s);
        if (e == hipSuccess && grad_bias) e = hipMemsetAsync(grad_bias, 0, (size_t)Cout * sizeof(float), s);
        return launched("conv2d wgrad memset", e);
    }
    if (!input || !grad_output) return fail(SSTEM_ERR_NULL_POINTER, "conv2d wgrad: null tensor pointer");
    if (Cin * Cout >= ((int64_t)1 << 31)) return fail(SSTEM_ERR_BAD_SHAPE, "conv2d wgrad: Cin*Cout too large");
    const bool is3x3 = (KH == 3 && KW == 3);
    if (algo == SSTEM_CONV_AUTO) algo = is3x3 ? SSTEM_CONV_MFMA : SSTEM_CONV_DIRECT;
    ConvAlgo a = conv_algo(algo);
    if (a.split_bf16() && (!is3x3 || !sstem::conv3x3_wgrad_split_supported((int)N, (int)Cin, (int)H, (int)W, (int)Cout)))
        a = conv_algo(SSTEM_CONV_MFMA);                         // outside the split kernel's range: the fp32 MFMA kernel
    hipError_t e;
    if (a.family == FAMILY_FP32) {
        if (!is3x3) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d wgrad: the MFMA kernel is 3x3 only");
        const int64_t need = sstem::conv3x3_wgrad_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
        if (!workspace || workspace_floats < need)
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d wgrad: workspace too small (see sstem_conv3x3_wgrad_workspace_floats)");
        e = sstem::launch_conv3x3_wgrad_mfma(input, grad_output, grad_weight, grad_bias, workspace, (int)N, (int)Cin, (int)H,
                                             (int)W, (int)Cout, s, wgrad_flags(accumulate));
    } else if (a.split_bf16()) {
        const int64_t need = sstem::conv3x3_wgrad_split_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
        if (!workspace || workspace_floats < need)
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d wgrad: workspace too small (see sstem_conv3x3_wgrad_workspace_floats_algo)");
        e = sstem::launch_conv3x3_wgrad_split_mfma(input, grad_output, grad_weight, grad_bias, workspace, (int)N, (int)Cin, (int)H,
                                                   (int)W, (int)Cout, a.pieces, s, wgrad_flags(accumulate));
    } else if (a.family == FAMILY_BF16) {
        if (!is3x3) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d wgrad: the bf16 MFMA kernel is 3x3 only");
        const int64_t need = sstem::conv3x3_wgrad_bf16_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
        if (!workspace || workspace_floats < need)
            return fail(SSTEM_ERR_BAD_SHAPE, "conv2d wgrad: workspace too small (see sstem_conv3x3_wgrad_workspace_floats_algo)");
        e = sstem::launch_conv3x3_wgrad_bf16_mfma(input, grad_output, grad_weight, grad_bias, workspace, (int)N, (int)Cin, (int)H,
                                                  (int)W, (int)Cout, s, wgrad_flags(accumulate));
    } else if (a.family == FAMILY_DIRECT) {
        if (grad_bias) return fail(SSTEM_ERR_UNSUPPORTED, "conv2d wgrad: the fused bias gradient needs the 3x3 MFMA kernel");
        e = sstem::launch_conv2d_wgrad_direct(input, grad_output, grad_weight, (int)N, (int)Cin, (int)H, (int)W,
                                              (int)Cout, KH, KW, pad_h, pad_w, s, accumulate ? 1 : 0);
    } else {
        return fail(SSTEM_ERR_UNSUPPORTED, "conv2d wgrad: unknown algorithm id");
    }
    return launched("conv2d wgrad launch", e);
}

int sstem_conv3x3_backward_weight_bf16in(const void* input_bf16, const float* grad_output, float* grad_weight, float* grad_bias,
                                         float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H, int64_t W,
                                         int64_t Cout, void* stream)
{
    return sstem_conv3x3_backward_weight_bf16in_ex(input_bf16, grad_output, grad_weight, grad_bias, workspace, workspace_floats,
                                                   N, Cin, H, W, Cout, 0, stream);
}

int sstem_conv3x3_backward_weight_bf16in_ex(const void* input_bf16, const float* grad_output, float* grad_weight, float* grad_bias,
                                            float* workspace, int64_t workspace_floats, int64_t N, int64_t Cin, int64_t H, int64_t W,
                                            int64_t Cout, int accumulate, void* stream)
{
    if (!conv_sizes_positive(N, Cin, H, W, Cout))
        return fail(SSTEM_ERR_BAD_SHAPE, "conv3x3 wgrad bf16in: bad shape");
    if (!input_bf16 || !grad_output || !grad_weight) return fail(SSTEM_ERR_NULL_POINTER, "conv3x3 wgrad bf16in: null tensor pointer");
    if (W % 4 != 0) return fail(SSTEM_ERR_UNSUPPORTED, "conv3x3 wgrad bf16in: needs W % 4 == 0");
    const int64_t need = sstem::conv3x3_wgrad_bf16_workspace_floats((int)N, (int)Cin, (int)H, (int)W, (int)Cout);
    if (!workspace || workspace_floats < need)
        return fail(SSTEM_ERR_BAD_SHAPE, "conv3x3 wgrad bf16in: workspace too small (see sstem_conv3x3_wgrad_workspace_floats_algo)");
    hipError_t e = sstem::launch_conv3x3_wgrad_bf16_mfma_in(input_bf16, 1, grad_output, grad_weight, grad_bias, workspace, (int)N, (int)Cin,
                                                            (int)H, (int)W, (int)Cout, static_cast<hipStream_t>(stream), wgrad_flags(accumulate));
    return launched("conv3x3 wgrad bf16in launch", e);
}

int sstem_conv_transpose3x3s2_backward_f32(const float* input, const float* weight,
                                           const float* grad_output, float* grad_input,
                                           float* grad_weight,
                                           int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                           void* stream)
{
    if (!conv_sizes_ok(N, Cin, 2 * H, 2 * W, Cout)) return fail(SSTEM_ERR_BAD_SHAPE, "conv_transpose backward: bad shape");
    if (Cin == 0 || Cout == 0) return SSTEM_OK;
    if (!grad_output && N > 0 && H > 0 && W > 0) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose backward: null grad_output");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (grad_input && N > 0 && H > 0 && W > 0) {
        if (!weight) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose backward: null weight");
        hipError_t e = sstem::launch_convT3x3s2_dgrad_direct(grad_output, weight, grad_input, (int)N, (int)Cin,
                                                             (int)H, (int)W, (int)Cout, s);
        if (e != hipSuccess) return hip_fail("conv_transpose dgrad launch", e);
    }
    if (grad_weight) {
        if (!input && N > 0 && H > 0 && W > 0) return fail(SSTEM_ERR_NULL_POINTER, "conv_transpose backward: null input");
        hipError_t e = sstem::launch_convT3x3s2_wgrad_direct(input, grad_output, grad_weight, (int)N, (int)Cin,
                                                             (int)H, (int)W, (int)Cout, s);
        if (e != hipSuccess) return hip_fail("conv_transpose wgrad launch", e);
    }
    return SSTEM_OK;
}

// ---- bilinear back-warp (include/sstem_warp.h) -------------------------------------------------
int sstem_warp_bilinear_f32(const float* image, const float* flow, float* output,
                            int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    if (!conv_sizes_ok(B, C, H, W, 2)) return fail(SSTEM_ERR_BAD_SHAPE, "warp: bad shape");
    if (B == 0 || C == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!image || !flow || !output) return fail(SSTEM_ERR_NULL_POINTER, "warp: null tensor pointer");
    hipError_t e = sstem::launch_warp_bilinear(image, flow, output, (int)B, (int)C, (int)H, (int)W,
                                               static_cast<hipStream_t>(stream));
    return launched("warp launch", e);
}

int sstem_warp_bilinear_backward_f32(const float* image, const float* flow, const float* grad_output,
                                     float* grad_flow, float* grad_image, int accumulate_image,
                                     int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    if (!conv_sizes_ok(B, C, H, W, 2)) return fail(SSTEM_ERR_BAD_SHAPE, "warp backward: bad shape");
    if (B == 0 || C == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!flow || !grad_output || (!grad_flow && !grad_image) || (grad_flow && !image))
        return fail(SSTEM_ERR_NULL_POINTER, "warp backward: null tensor pointer");
    hipError_t e = sstem::launch_warp_bilinear_backward(image, flow, grad_output, grad_flow, grad_image, accumulate_image,
                                                        (int)B, (int)C, (int)H, (int)W, static_cast<hipStream_t>(stream));
    return launched("warp backward launch", e);
}

// ---- uint8 edge + flat Adam (include/sstem_io.h) -----------------------------------------------
int sstem_gray_u8_to_f32(const uint8_t* image, float* output, int64_t npix, int64_t replicas, void* stream)
{
    if (npix < 0 || replicas < 0 || replicas > 1024 || npix > ((int64_t)1 << 40)) return fail(SSTEM_ERR_BAD_SHAPE, "u8->f32: bad size");
    if (npix == 0 || replicas == 0) return SSTEM_OK;
    if (!image || !output) return fail(SSTEM_ERR_NULL_POINTER, "u8->f32: null pointer");
    hipError_t e = sstem::launch_gray_u8_to_f32(image, output, npix, (int)replicas, static_cast<hipStream_t>(stream));
    return launched("u8->f32 launch", e);
}

static bool bn_sizes_ok(int64_t N, int64_t C, int64_t HW)
{
    return N >= 0 && C >= 0 && HW >= 0 && N <= (1 << 20) && C <= 65535 && HW <= ((int64_t)1 << 31) &&
           (__int128)N * C * HW < ((__int128)1 << 40);
}

int64_t sstem_batchnorm_workspace_floats(int64_t N, int64_t C, int64_t HW)
{
    if (!bn_sizes_ok(N, C, HW)) return 0;
    return sstem::bn_workspace_floats(N, C, HW);
}

int sstem_batchnorm_train_forward_f32(const float* x, const float* weight, const float* bias,
                                      float* running_mean, float* running_var, float* y,
                                      float* save_mean, float* save_invstd,
                                      float* workspace, int64_t workspace_floats,
                                      int64_t N, int64_t C, int64_t HW, float momentum, float eps,
                                      int act, float slope, void* stream)
{
    return sstem_batchnorm_train_forward_ex_f32(x, weight, bias, running_mean, running_var, nullptr, y, save_mean, save_invstd,
                                                nullptr, 0, workspace, workspace_floats, N, C, HW, momentum, eps, act, slope, stream);
}

int sstem_batchnorm_train_forward_ex_f32(const float* x, const float* weight, const float* bias,
                                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float* y,
                                         float* save_mean, float* save_invstd,
                                         const float* partials, int64_t n_partials,
                                         float* workspace, int64_t workspace_floats,
                                         int64_t N, int64_t C, int64_t HW, float momentum, float eps,
                                         int act, float slope, void* stream)
{
    return sstem_batchnorm_train_forward_amax_f32(x, weight, bias, running_mean, running_var, num_batches_tracked, y, nullptr, save_mean,
                                                  save_invstd, partials, n_partials, workspace, workspace_floats, N, C, HW, momentum, eps,
                                                  act, slope, stream);
}

int sstem_batchnorm_train_forward_amax_f32(const float* x, const float* weight, const float* bias,
                                           float* running_mean, float* running_var, int64_t* num_batches_tracked, float* y,
                                           float* y_amax, float* save_mean, float* save_invstd,
                                           const float* partials, int64_t n_partials,
                                           float* workspace, int64_t workspace_floats,
                                           int64_t N, int64_t C, int64_t HW, float momentum, float eps,
                                           int act, float slope, void* stream)
{
    if (!bn_sizes_ok(N, C, HW)) return fail(SSTEM_ERR_BAD_SHAPE, "batchnorm: bad shape");
    if (int rc = check_act("batchnorm", act)) return rc;
    if (N == 0 || C == 0 || HW == 0) return SSTEM_OK;
    if (!x || !y || !save_mean || !save_invstd) return fail(SSTEM_ERR_NULL_POINTER, "batchnorm: null tensor pointer");
    if (partials && n_partials <= 0) return fail(SSTEM_ERR_BAD_SHAPE, "batchnorm: partials without a count");
    if (!partials && (!workspace || workspace_floats < sstem::bn_workspace_floats(N, C, HW)))
        return fail(SSTEM_ERR_BAD_SHAPE, "batchnorm: workspace too small (see sstem_batchnorm_workspace_floats)");
    hipError_t e = sstem::launch_bn_train_forward(x, weight, bias, running_mean, running_var, y, save_mean, save_invstd,
                                                  workspace, (int)N, (int)C, HW, momentum, eps, act, slope,
                                                  static_cast<hipStream_t>(stream), partials, n_partials,
                                                  reinterpret_cast<long long*>(num_batches_tracked), y_amax);
    return launched("batchnorm forward launch", e);
}

int sstem_batchnorm_train_backward_f32(const float* dy, const float* x, const float* weight, const float* bias,
                                       const float* save_mean, const float* save_invstd,
                                       float* dx, float* dweight, float* dbias,
                                       float* workspace, int64_t workspace_floats,
                                       int64_t N, int64_t C, int64_t HW, int act, float slope, void* stream)
{
    return sstem_batchnorm_train_backward_ex_f32(dy, x, weight, bias, save_mean, save_invstd, dx, dweight, dbias, workspace,
                                                 workspace_floats, N, C, HW, act, slope, 0, stream);
}

int sstem_batchnorm_train_backward_ex_f32(const float* dy, const float* x, const float* weight, const float* bias,
                                          const float* save_mean, const float* save_invstd,
                                          float* dx, float* dweight, float* dbias,
                                          float* workspace, int64_t workspace_floats,
                                          int64_t N, int64_t C, int64_t HW, int act, float slope, int accumulate, void* stream)
{
    return sstem_batchnorm_train_backward_amax_f32(dy, x, weight, bias, save_mean, save_invstd, dx, nullptr, dweight, dbias, workspace,
                                                   workspace_floats, N, C, HW, act, slope, accumulate, stream);
}

int sstem_batchnorm_train_backward_amax_f32(const float* dy, const float* x, const float* weight, const float* bias,
                                            const float* save_mean, const float* save_invstd,
                                            float* dx, float* dx_amax, float* dweight, float* dbias,
                                            float* workspace, int64_t workspace_floats,
                                            int64_t N, int64_t C, int64_t HW, int act, float slope, int accumulate, void* stream)
{
    if (!bn_sizes_ok(N, C, HW)) return fail(SSTEM_ERR_BAD_SHAPE, "batchnorm: bad shape");
    if (int rc = check_act("batchnorm", act)) return rc;
    if (N == 0 || C == 0 || HW == 0) return SSTEM_OK;
    if (!dy || !x || !dx || !save_mean || !save_invstd) return fail(SSTEM_ERR_NULL_POINTER, "batchnorm: null tensor pointer");
    if (!workspace || workspace_floats < sstem::bn_workspace_floats(N, C, HW))
        return fail(SSTEM_ERR_BAD_SHAPE, "batchnorm: workspace too small (see sstem_batchnorm_workspace_floats)");
    hipError_t e = sstem::launch_bn_train_backward(dy, x, weight, bias, save_mean, save_invstd, dx, dweight, dbias, workspace,
                                                   (int)N, (int)C, HW, act, slope, static_cast<hipStream_t>(stream), accumulate ? 1 : 0, dx_amax);
    return launched("batchnorm backward launch", e);
}

int sstem_upsample_bilinear2x_f32(const float* input, float* output, int64_t planes, int64_t H, int64_t W, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || H > (1 << 14) || W > (1 << 14) || planes > ((int64_t)1 << 30))
        return fail(SSTEM_ERR_BAD_SHAPE, "upsample: bad shape");
    if (W % 2 != 0) return fail(SSTEM_ERR_UNSUPPORTED, "upsample: the input width must be even (16-byte output stores)");
    if (planes == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !output) return fail(SSTEM_ERR_NULL_POINTER, "upsample: null pointer");
    if ((reinterpret_cast<uintptr_t>(output) & 15) != 0) return fail(SSTEM_ERR_UNSUPPORTED, "upsample: output must be 16-byte aligned");
    hipError_t e = sstem::launch_upsample_bilinear2x(input, output, planes, (int)H, (int)W, static_cast<hipStream_t>(stream));
    return launched("upsample launch", e);
}

int sstem_upsample_bilinear2x_backward_f32(const float* grad_output, float* grad_input, int64_t planes, int64_t H, int64_t W, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || H > (1 << 14) || W > (1 << 14) || planes > ((int64_t)1 << 31) - 1)
        return fail(SSTEM_ERR_BAD_SHAPE, "upsample backward: bad shape");
    if (planes == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!grad_output || !grad_input) return fail(SSTEM_ERR_NULL_POINTER, "upsample backward: null pointer");
    hipError_t e = sstem::launch_upsample_bilinear2x_backward(grad_output, grad_input, planes, (int)H, (int)W, static_cast<hipStream_t>(stream));
    return launched("upsample backward launch", e);
}

int sstem_pool2x2_forward_f32(const float* input, float* output, uint8_t* argmax, int64_t planes, int64_t H, int64_t W, int is_max, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || H > (1 << 15) || W > (1 << 15) || planes > ((int64_t)1 << 31) - 1)
        return fail(SSTEM_ERR_BAD_SHAPE, "pool2x2: bad shape");
    if (planes == 0 || H < 2 || W < 2) return SSTEM_OK;
    if (!input || !output) return fail(SSTEM_ERR_NULL_POINTER, "pool2x2: null pointer");
    hipError_t e = sstem::launch_pool2x2_forward(input, output, is_max ? argmax : nullptr, planes, (int)H, (int)W, is_max ? 1 : 0,
                                                 static_cast<hipStream_t>(stream));
    return launched("pool2x2 launch", e);
}

int sstem_pool2x2_backward_f32(const float* grad_output, const uint8_t* argmax, float* grad_input, int64_t planes, int64_t H, int64_t W,
                               int is_max, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || H > (1 << 15) || W > (1 << 15) || planes > ((int64_t)1 << 31) - 1)
        return fail(SSTEM_ERR_BAD_SHAPE, "pool2x2 backward: bad shape");
    if (planes == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!grad_input || ((H >= 2 && W >= 2) && !grad_output)) return fail(SSTEM_ERR_NULL_POINTER, "pool2x2 backward: null pointer");
    if (is_max && H >= 2 && W >= 2 && !argmax) return fail(SSTEM_ERR_NULL_POINTER, "pool2x2 backward: the maximum needs its argmax bytes");
    hipError_t e = sstem::launch_pool2x2_backward(grad_output, argmax, grad_input, planes, (int)H, (int)W, is_max ? 1 : 0,
                                                  static_cast<hipStream_t>(stream));
    return launched("pool2x2 backward launch", e);
}

int sstem_f32_to_gray_u8(const float* pred, uint8_t* output, int64_t npix, int clamp01, void* stream)
{
    if (npix < 0 || npix > ((int64_t)1 << 40)) return fail(SSTEM_ERR_BAD_SHAPE, "f32->u8: bad size");
    if (npix == 0) return SSTEM_OK;
    if (!pred || !output) return fail(SSTEM_ERR_NULL_POINTER, "f32->u8: null pointer");
    hipError_t e = sstem::launch_f32_to_gray_u8(pred, output, npix, clamp01 ? 1 : 0, static_cast<hipStream_t>(stream));
    return launched("f32->u8 launch", e);
}

int sstem_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                        void* stream)
{
    if (n < 0 || n > ((int64_t)1 << 40) || step < 1) return fail(SSTEM_ERR_BAD_SHAPE, "adam: bad size or step < 1");
    if (n == 0) return SSTEM_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(SSTEM_ERR_NULL_POINTER, "adam: null pointer");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipError_t e = sstem::launch_adam_step(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                                           (float)bc1, (float)sqrt(bc2), static_cast<hipStream_t>(stream));
    return launched("adam launch", e);
}

// ---- any filter length (the reference's cupy spelling: sff_scripts_interp/model/sepconv.py:8-31, SIZE_1(vertical)) -----------------
int sstem_sepconv_forward_taps_f32(const float* input, const float* vertical, const float* horizontal, float* output,
                                   int64_t B, int64_t C, int64_t H, int64_t W, int taps, void* stream)
{
    if (taps == SSTEM_SEPCONV_FILTER) return sstem_sepconv_forward_f32(input, vertical, horizontal, output, B, C, H, W, stream);
    if (!taps_sizes_ok(B, C, H, W, taps)) return fail(SSTEM_ERR_BAD_SHAPE, "forward (any filter length): bad shape or filter length");
    if (B == 0 || C == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !vertical || !horizontal || !output) return fail(SSTEM_ERR_NULL_POINTER, "forward (any filter length): null tensor pointer");
    hipError_t e = sstem::launch_fwd_direct(input, vertical, horizontal, output, B, C, H, W, taps, static_cast<hipStream_t>(stream));
    return launched("sepconv forward (any filter length) launch", e);
}

int sstem_sepconv_backward_taps_f32(const float* grad_output, const float* input, const float* vertical, const float* horizontal,
                                    float* grad_vertical, float* grad_horizontal,
                                    int64_t B, int64_t C, int64_t H, int64_t W, int taps, void* stream)
{
    if (!taps_sizes_ok(B, C, H, W, taps)) return fail(SSTEM_ERR_BAD_SHAPE, "backward (any filter length): bad shape or filter length");
    if (B == 0 || C == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!grad_output || !input || !vertical || !horizontal || !grad_vertical || !grad_horizontal)
        return fail(SSTEM_ERR_NULL_POINTER, "backward (any filter length): null tensor pointer");
    hipError_t e = sstem::launch_bwd_direct(grad_output, input, vertical, horizontal, grad_vertical, grad_horizontal, B, C, H, W, taps,
                                            static_cast<hipStream_t>(stream));
    return launched("sepconv backward (any filter length) launch", e);
}

// ---- bf16 coefficient tensors (BASELINE config 5: "bf16 activations with fp32 sepconv accumulate") -------------------
int64_t sstem_sepconv_forward_bytes_bf16coef(int64_t B, int64_t C, int64_t H, int64_t W)
{
    return 4 * (B * C * (H + 50) * (W + 50) + B * C * H * W) + 2 * (2 * B * 51 * H * W);
}

int64_t sstem_sepconv_backward_bytes_bf16coef(int64_t B, int64_t C, int64_t H, int64_t W)
{
    return 4 * (B * C * H * W + B * C * (H + 50) * (W + 50) + 2 * B * 51 * H * W) + 2 * (2 * B * 51 * H * W);
}

int64_t sstem_sepconv_interp_apply_bytes_bf16coef(int64_t B, int64_t H, int64_t W, int frame_planes)
{
    return 4 * (2 * B * frame_planes * H * W + B * H * W) + 2 * (4 * B * 51 * H * W);
}

int sstem_sepconv_forward_bf16coef(const float* input, const uint16_t* vertical, const uint16_t* horizontal, float* output,
                                   int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    if (!sizes_ok(B, C, H, W)) return fail(SSTEM_ERR_BAD_SHAPE, "forward (bf16 coefficients): negative or oversized shape");
    if (B == 0 || C == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!input || !vertical || !horizontal || !output) return fail(SSTEM_ERR_NULL_POINTER, "forward (bf16 coefficients): null tensor pointer");
    if (!sstem::mfma_grid_ok(B, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "forward (bf16 coefficients): grid too large");
    hipError_t e = sstem::launch_fwd_bf16coef(input, vertical, horizontal, output, B, C, H, W, static_cast<hipStream_t>(stream));
    return launched("sepconv forward (bf16 coefficients) launch", e);
}

int sstem_sepconv_backward_bf16coef(const float* grad_output, const float* input, const uint16_t* vertical, const uint16_t* horizontal,
                                    float* grad_input, float* grad_vertical, float* grad_horizontal,
                                    int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    (void)grad_input;      // never written, as in the reference (kernel.cu:152-206) and in sstem_sepconv_backward_f32
    if (!sizes_ok(B, C, H, W)) return fail(SSTEM_ERR_BAD_SHAPE, "backward (bf16 coefficients): negative or oversized shape");
    if (C != 3) return fail(SSTEM_ERR_BAD_SHAPE, "backward: the gradient kernels are defined for 3 channels (kernel.cu:100-108)");
    if (B == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!grad_output || !input || !vertical || !horizontal || !grad_vertical || !grad_horizontal)
        return fail(SSTEM_ERR_NULL_POINTER, "backward (bf16 coefficients): null tensor pointer");
    if (!sstem::mfma_grid_ok(B, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "backward (bf16 coefficients): grid too large");
    hipError_t e = sstem::launch_bwd_bf16coef(grad_output, input, vertical, horizontal, grad_vertical, grad_horizontal, B, C, H, W,
                                              static_cast<hipStream_t>(stream));
    return launched("sepconv backward (bf16 coefficients) launch", e);
}

int sstem_sepconv_interp_apply_gray_bf16coef_supported(int64_t B, int64_t H, int64_t W) { return apply_supported(APPLY_GRAY_BF16COEF, B, H, W); }

int sstem_sepconv_interp_apply_gray_bf16coef(const float* g1, const float* g2, const uint16_t* k1v, const uint16_t* k1h,
                                             const uint16_t* k2v, const uint16_t* k2h, float* output,
                                             int64_t B, int64_t H, int64_t W, void* stream)
{
    const char* range = "grid too large or 51*H*W*4 bytes per image not below 4 GiB";      // one refusal for both range rules
    return interp_apply("gray interp apply (bf16 coefficients)", APPLY_GRAY_BF16COEF, !g1 || !g2 || !k1v || !k1h || !k2v || !k2h || !output,
                        B, H, W, range, range, [&] {
        return sstem::launch_interp_fused_gray_bf16coef(g1, g2, k1v, k1h, k2v, k2h, output, B, H, W, static_cast<hipStream_t>(stream));
    });
}

// ---- input gradient (the library's addition: the reference's launcher leaves gradInput untouched, kernel.cu:152-206) ---------------
int64_t sstem_sepconv_backward_input_bytes(int64_t B, int64_t C, int64_t H, int64_t W)
{
    return 4 * (B * C * H * W + 2 * B * 51 * H * W + B * C * (H + 50) * (W + 50));
}

// shared tail of the four entries: taps == 51 unless the _taps entry says otherwise; bf16: coefficient tensors are bf16 (direct kernel)
static int backward_input(const char* what, const float* grad_output, const float* vertical, const float* horizontal, float* grad_input,
                          int64_t B, int64_t C, int64_t H, int64_t W, int taps, bool bf16, void* stream, int algo)
{
    if (!sizes_ok(B, C, H, W) || !taps_sizes_ok(B, C, H, W, taps)) return fail(SSTEM_ERR_BAD_SHAPE, "%s: bad shape or filter length", what);
    if (algo != SSTEM_SEPCONV_AUTO && algo != SSTEM_SEPCONV_DIRECT && algo != SSTEM_SEPCONV_MFMA)
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: unknown algorithm id", what);
    if (B == 0 || C == 0) return SSTEM_OK;
    if (!grad_input || ((H > 0 && W > 0) && (!grad_output || !vertical || !horizontal)))
        return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (H == 0 || W == 0) {   // no source pixel: every grad_input element is an empty sum
        const size_t bytes = (size_t)B * C * (H + taps - 1) * (W + taps - 1) * sizeof(float);
        if (bytes == 0) return SSTEM_OK;
        return launched("sepconv input gradient memset", hipMemsetAsync(grad_input, 0, bytes, s));
    }
    const bool tiled_can = !bf16 && taps == SSTEM_SEPCONV_FILTER && sstem::gradinput_tiled_ok(B, C, H, W);
    if (algo == SSTEM_SEPCONV_AUTO) algo = tiled_can ? SSTEM_SEPCONV_MFMA : SSTEM_SEPCONV_DIRECT;
    hipError_t e;
    if (algo == SSTEM_SEPCONV_MFMA) {
        if (!tiled_can) return fail(SSTEM_ERR_UNSUPPORTED, "%s: shape outside the tiled kernel's grid or 32-bit offset range", what);
        e = sstem::launch_gradinput_tiled(grad_output, vertical, horizontal, grad_input, B, C, H, W, s);
    } else {
        e = sstem::launch_gradinput_direct(grad_output, vertical, horizontal, grad_input, B, C, H, W, taps, bf16, s);
    }
    return launched("sepconv input gradient launch", e);
}

int sstem_sepconv_backward_input_f32_algo(const float* grad_output, const float* vertical, const float* horizontal, float* grad_input,
                                          int64_t B, int64_t C, int64_t H, int64_t W, void* stream, int algo)
{
    return backward_input("backward input", grad_output, vertical, horizontal, grad_input, B, C, H, W, SSTEM_SEPCONV_FILTER, false, stream, algo);
}

int sstem_sepconv_backward_input_f32(const float* grad_output, const float* vertical, const float* horizontal, float* grad_input,
                                     int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    return sstem_sepconv_backward_input_f32_algo(grad_output, vertical, horizontal, grad_input, B, C, H, W, stream, SSTEM_SEPCONV_AUTO);
}

int sstem_sepconv_backward_input_taps_f32(const float* grad_output, const float* vertical, const float* horizontal, float* grad_input,
                                          int64_t B, int64_t C, int64_t H, int64_t W, int taps, void* stream)
{
    if (taps == SSTEM_SEPCONV_FILTER) return sstem_sepconv_backward_input_f32(grad_output, vertical, horizontal, grad_input, B, C, H, W, stream);
    return backward_input("backward input (any filter length)", grad_output, vertical, horizontal, grad_input, B, C, H, W, taps, false, stream,
                          SSTEM_SEPCONV_DIRECT);
}

int sstem_sepconv_backward_input_bf16coef(const float* grad_output, const uint16_t* vertical, const uint16_t* horizontal,
                                          float* grad_input, int64_t B, int64_t C, int64_t H, int64_t W, void* stream)
{
    return backward_input("backward input (bf16 coefficients)", grad_output, reinterpret_cast<const float*>(vertical),
                          reinterpret_cast<const float*>(horizontal), grad_input, B, C, H, W, SSTEM_SEPCONV_FILTER, true, stream,
                          SSTEM_SEPCONV_DIRECT);
}

int64_t sstem_l1_workspace_floats(void) { return 1024 + 1; }

int sstem_l1_mean_forward_grad_f32(const float* pred, const float* target, int64_t n, float* loss, float* grad, float* workspace,
                                   void* stream)
{
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(SSTEM_ERR_BAD_SHAPE, "l1: bad size");
    if (!pred || !target || !loss || !grad || !workspace) return fail(SSTEM_ERR_NULL_POINTER, "l1: null pointer");
    hipError_t e = sstem::launch_l1_mean_fwd_grad(pred, target, n, loss, grad, workspace, static_cast<hipStream_t>(stream));
    return launched("l1 launch", e);
}

int sstem_l2_mean_forward_grad_f32(const float* pred, const float* target, int64_t n, float* loss, float* grad, float* workspace,
                                   void* stream)
{
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(SSTEM_ERR_BAD_SHAPE, "l2: bad size");
    if (!pred || !target || !loss || !grad || !workspace) return fail(SSTEM_ERR_NULL_POINTER, "l2: null pointer");
    hipError_t e = sstem::launch_l2_mean_fwd_grad(pred, target, n, loss, grad, workspace, static_cast<hipStream_t>(stream));
    return launched("l2 launch", e);
}

// ---- MS-SSIM criterion (include/sstem_loss.h): both entries make the same checks, in this order, before any HIP call ----------------
static int ms_ssim_checked(const char* what, bool any_null, int64_t B, int64_t H, int64_t W, int levels, float max_val, const float* workspace,
                           sstem::SsimPlan* plan, bool* empty)
{
    *empty = false;
    if (B < 0 || H < 0 || W < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (levels < 1 || levels > sstem::SSIM_MAX_LEVELS) return fail(SSTEM_ERR_UNSUPPORTED, "%s: levels must be 1..5", what);
    if (!(max_val > 0.f) || isinf(max_val)) return fail(SSTEM_ERR_UNSUPPORTED, "%s: max_val must be positive and finite", what);
    if (B == 0) { *empty = true; return SSTEM_OK; }
    if (any_null) return fail(SSTEM_ERR_NULL_POINTER, "%s: null pointer", what);
    if ((H < W ? H : W) < ((int64_t)1 << levels))
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: min(H, W) must be at least 2^levels (every level is pooled 2 x 2 once more)", what);
    if (!sstem::ms_ssim_plan(B, H, W, levels, plan))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (H, W <= 32768 and at most 2^24 tiles of 32 x 32)", what);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(SSTEM_ERR_UNSUPPORTED, "%s: the workspace must be 8-byte aligned", what);
    return SSTEM_OK;
}

int64_t sstem_ms_ssim_workspace_floats(int64_t B, int64_t H, int64_t W, int levels)
{
    sstem::SsimPlan plan;
    if (levels < 1 || levels > sstem::SSIM_MAX_LEVELS || B < 0 || (H < W ? H : W) < ((int64_t)1 << levels)) return 0;
    return sstem::ms_ssim_plan(B, H, W, levels, &plan) ? plan.total_floats : 0;
}

int sstem_ms_ssim_forward_f32(const float* img1, const float* img2, int64_t B, int64_t H, int64_t W, int levels, float max_val, float* value,
                              float* terms, float* workspace, void* stream)
{
    sstem::SsimPlan plan;
    bool empty;
    const int rc = ms_ssim_checked("ms_ssim forward", !img1 || !img2 || !value || !workspace, B, H, W, levels, max_val, workspace, &plan, &empty);
    if (rc != SSTEM_OK || empty) return rc;
    hipError_t e = sstem::launch_ms_ssim_forward(img1, img2, B, plan, max_val, value, terms, workspace, static_cast<hipStream_t>(stream));
    return launched("ms_ssim forward launch", e);
}

int sstem_ms_ssim_backward_f32(const float* img1, const float* img2, int64_t B, int64_t H, int64_t W, int levels, float max_val,
                               const float* grad_value, float* grad_img1, float* workspace, void* stream)
{
    sstem::SsimPlan plan;
    bool empty;
    const int rc = ms_ssim_checked("ms_ssim backward", !img1 || !img2 || !grad_img1 || !workspace, B, H, W, levels, max_val, workspace, &plan, &empty);
    if (rc != SSTEM_OK || empty) return rc;
    hipError_t e = sstem::launch_ms_ssim_backward(img1, img2, B, plan, max_val, grad_value, grad_img1, workspace, static_cast<hipStream_t>(stream));
    return launched("ms_ssim backward launch", e);
}

// ---- single-scale SSIM criterion (include/sstem_loss.h): both entries make the same checks, in this order, before any HIP call ------
static int ssim_loss_checked(const char* what, bool any_null, int64_t B, int64_t C, int64_t H, int64_t W, const float* workspace,
                             sstem::SsimLossPlan* plan, bool* empty)
{
    *empty = false;
    if (B < 0 || C < 0 || H < 0 || W < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (B == 0 || C == 0 || H == 0 || W == 0) { *empty = true; return SSTEM_OK; }
    if (any_null) return fail(SSTEM_ERR_NULL_POINTER, "%s: null pointer", what);
    if (!sstem::ssim_loss_plan(B, C, H, W, plan))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (H, W <= 32768 and at most 2^24 tiles of 32 x 32)", what);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(SSTEM_ERR_UNSUPPORTED, "%s: the workspace must be 8-byte aligned", what);
    return SSTEM_OK;
}

int64_t sstem_ssim_loss_workspace_floats(int64_t B, int64_t C, int64_t H, int64_t W)
{
    sstem::SsimLossPlan plan;
    return sstem::ssim_loss_plan(B, C, H, W, &plan) ? plan.total_floats : 0;
}

int sstem_ssim_loss_forward_f32(const float* img1, const float* img2, int64_t B, int64_t C, int64_t H, int64_t W, int per_sample,
                                float* value, float* workspace, void* stream)
{
    sstem::SsimLossPlan plan;
    bool empty;
    const int rc = ssim_loss_checked("ssim_loss forward", !img1 || !img2 || !value || !workspace, B, C, H, W, workspace, &plan, &empty);
    if (rc != SSTEM_OK || empty) return rc;
    hipError_t e = sstem::launch_ssim_loss_forward(img1, img2, B, plan, per_sample != 0, value, workspace, static_cast<hipStream_t>(stream));
    return launched("ssim_loss forward launch", e);
}

int sstem_ssim_loss_backward_f32(const float* img1, const float* img2, int64_t B, int64_t C, int64_t H, int64_t W, int per_sample,
                                 const float* grad_value, float* grad_img1, float* workspace, void* stream)
{
    sstem::SsimLossPlan plan;
    bool empty;
    const int rc = ssim_loss_checked("ssim_loss backward", !img1 || !img2 || !grad_img1 || !workspace, B, C, H, W, workspace, &plan, &empty);
    if (rc != SSTEM_OK || empty) return rc;
    hipError_t e = sstem::launch_ssim_loss_backward(img1, img2, B, plan, per_sample != 0, grad_value, grad_img1, static_cast<hipStream_t>(stream));
    return launched("ssim_loss backward launch", e);
}

// ---- validation scores (include/sstem_score.h); the checks are score_checked, above --------------------------------------------
int64_t sstem_score_workspace_bytes(int64_t B, int64_t H, int64_t W)
{
    sstem::ScorePlan plan;
    return sstem::score_plan(B, H, W, &plan) ? plan.total_bytes : 0;
}

int sstem_score_images_f32(const float* a, const float* b, int64_t B, int64_t H, int64_t W, int clamp01_a, double* scores, void* workspace,
                           void* stream)
{
    return score_images<float>("score images (f32)", a, b, B, H, W, clamp01_a, scores, workspace, stream);
}

int sstem_score_images_u8(const uint8_t* a, const uint8_t* b, int64_t B, int64_t H, int64_t W, int clamp01_a, double* scores, void* workspace,
                          void* stream)
{
    return score_images<uint8_t>("score images (u8)", a, b, B, H, W, clamp01_a, scores, workspace, stream);
}

int sstem_flow_epe_f32(const float* flow, const float* target, int64_t B, int64_t H, int64_t W, int sparse, int mean, double* value,
                       void* workspace, void* stream)
{
    sstem::ScorePlan plan;
    bool empty;
    const int rc = score_checked("flow epe", !flow || !target || !value || !workspace, false, B, H, W, value, workspace, &plan, &empty);
    if (rc != SSTEM_OK || empty) return rc;
    const hipError_t e = sstem::launch_flow_epe(flow, target, B, H, W, plan, sparse ? 1 : 0, mean ? 1 : 0, value, workspace,
                                                static_cast<hipStream_t>(stream));
    return launched("flow epe", e, " launch");
}

}  // extern "C"

namespace {

// sstem_fold_degrade_u8 and, with a table, sstem_fold_degrade_lut_u8 (include/sstem_jitter.h): one set of checks, one launcher
int fold_degrade_entry(const char* what, const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int64_t n,
                       int64_t slots, int64_t S_h, int64_t S_w, int64_t off_y, int64_t off_x, int64_t out_h, int64_t out_w, int gt_line,
                       const uint8_t* lut, uint8_t* deformed, float* flow2, float* im, float* lb, int32_t* zero_count, void* stream)
{
    if (n < 0 || slots < 0 || S_h < 0 || S_w < 0 || off_y < 0 || off_x < 0 || out_h < 0 || out_w < 0)
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (off_y > S_h || out_h > S_h - off_y || off_x > S_w || out_w > S_w - off_x)
        return fail(SSTEM_ERR_BAD_SHAPE, "%s: the window is not inside the plane", what);
    if (n == 0) return SSTEM_OK;
    if (!clean || !folds) return fail(SSTEM_ERR_NULL_POINTER, "%s: null plane or fold table", what);
    if (im && !interp) return fail(SSTEM_ERR_NULL_POINTER, "%s: im needs the interp plane", what);
    if (!fold_range_ok(n, S_h, S_w) || slots > (1 << 24))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (S_h, S_w <= 32768, n, slots <= 2^24)", what);
    if (!deformed && !flow2 && !im && !lb && !zero_count) return SSTEM_OK;
    return launched(what, sstem::launch_fold_degrade(clean, interp, folds, slot, (int)n, (int)slots, (int)S_h, (int)S_w, (int)off_y, (int)off_x,
                                                     (int)out_h, (int)out_w, gt_line ? 1 : 0, deformed, flow2, im, lb, zero_count,
                                                     static_cast<hipStream_t>(stream), lut), " launch");
}

}  // namespace

extern "C" {

// ---- fold synthesis (include/sstem_fold.h) ---------------------------------------------------------------------------------------
int sstem_fold_flow(const double* folds, int64_t n, int64_t H, int64_t W, float* flow, float* flow2, uint8_t* mask, void* stream)
{
    const char* what = "fold flow";
    if (n < 0 || H < 0 || W < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (n == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!folds) return fail(SSTEM_ERR_NULL_POINTER, "%s: null fold table", what);
    if (!fold_range_ok(n, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (H, W <= 32768, n <= 2^24)", what);
    if (!flow && !flow2 && !mask) return SSTEM_OK;
    return launched(what, sstem::launch_fold_flow(folds, (int)n, (int)H, (int)W, flow, flow2, mask, static_cast<hipStream_t>(stream)), " launch");
}

int sstem_image_warp_u8(const uint8_t* im, const float* flow, uint8_t* out, int64_t n, int64_t H, int64_t W, int64_t C, int mode,
                        void* stream)
{
    const char* what = "image warp (u8)";
    if (n < 0 || H < 0 || W < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (C < 1) return fail(SSTEM_ERR_BAD_SHAPE, "%s: C must be at least 1", what);
    if (mode != SSTEM_WARP_NEAREST && mode != SSTEM_WARP_BILINEAR) return fail(SSTEM_ERR_UNSUPPORTED, "%s: unknown mode", what);
    if (n == 0 || H == 0 || W == 0) return SSTEM_OK;
    if (!im || !flow || !out) return fail(SSTEM_ERR_NULL_POINTER, "%s: null tensor pointer", what);
    if (!fold_range_ok(n, H, W) || C > 1024)
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (H, W <= 32768, n <= 2^24, C <= 1024)", what);
    return launched(what, sstem::launch_image_warp_u8(im, flow, out, (int)n, (int)H, (int)W, (int)C, mode == SSTEM_WARP_BILINEAR ? 1 : 0,
                                                      static_cast<hipStream_t>(stream)), " launch");
}

int sstem_fold_degrade_u8(const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int64_t n, int64_t slots,
                          int64_t S_h, int64_t S_w, int64_t off_y, int64_t off_x, int64_t out_h, int64_t out_w, int gt_line,
                          uint8_t* deformed, float* flow2, float* im, float* lb, int32_t* zero_count, void* stream)
{
    return fold_degrade_entry("fold degrade", clean, interp, folds, slot, n, slots, S_h, S_w, off_y, off_x, out_h, out_w, gt_line, nullptr,
                              deformed, flow2, im, lb, zero_count, stream);
}

// ---- colour jitter (include/sstem_jitter.h) -------------------------------------------------------------------------------------------
int sstem_jitter_lut_u8(const uint8_t* planes, int64_t n, int64_t S_h, int64_t S_w, const int32_t* op_code, const float* op_factor,
                        uint8_t* lut, uint32_t* hist, void* stream)
{
    const char* what = "jitter lut";
    if (n < 0 || S_h < 0 || S_w < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (!fold_range_ok(n, S_h, S_w)) return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (S_h, S_w <= 32768, n <= 2^24)", what);
    if (n == 0 || S_h == 0 || S_w == 0) return SSTEM_OK;
    if (!planes || !op_code || !op_factor || !lut || !hist) return fail(SSTEM_ERR_NULL_POINTER, "%s: null plane, step table, lut or hist", what);
    return launched(what, sstem::launch_jitter_lut(planes, (int)n, S_h * S_w, op_code, op_factor, lut, hist, static_cast<hipStream_t>(stream)),
                    " launch");
}

int sstem_fold_degrade_lut_u8(const uint8_t* clean, const uint8_t* interp, const double* folds, const int32_t* slot, int64_t n,
                              int64_t slots, int64_t S_h, int64_t S_w, int64_t off_y, int64_t off_x, int64_t out_h, int64_t out_w,
                              int gt_line, const uint8_t* lut, uint8_t* deformed, float* flow2, float* im, float* lb,
                              int32_t* zero_count, void* stream)
{
    return fold_degrade_entry("fold degrade (lut)", clean, interp, folds, slot, n, slots, S_h, S_w, off_y, off_x, out_h, out_w, gt_line, lut,
                              deformed, flow2, im, lb, zero_count, stream);
}

}  // extern "C"

// ---- training crops (include/sstem_batch.h) ----------------------------------------------------------------------------------------
namespace {

// the checks the two crop entries share; `done` is set when the call is a successful no-op
int crop_orient_checks(const char* what, const void* pool, const void* images, int64_t n_images, const void* samples, const void* plane_image,
                       int64_t n, int64_t P, int64_t S_h, int64_t S_w, int64_t C0, int64_t C1, bool* done)
{
    *done = false;
    if (n_images < 0 || n < 0 || S_h < 0 || S_w < 0 || C0 < 0 || C1 < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (P < 1) return fail(SSTEM_ERR_BAD_SHAPE, "%s: P must be at least 1", what);
    if (P > SSTEM_BATCH_MAX_PLANES || C0 + C1 > SSTEM_BATCH_MAX_CHANNELS)
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: more than 16 planes or channels", what);
    if (S_h > 32768 || S_w > 32768 || n > (1 << 24) || n_images > (1 << 24))
        return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (S_h, S_w <= 32768, n, n_images <= 2^24)", what);
    if (n == 0 || S_h == 0 || S_w == 0) { *done = true; return SSTEM_OK; }
    if (!pool || !images || !samples || !plane_image) return fail(SSTEM_ERR_NULL_POINTER, "%s: null pool or table", what);
    return SSTEM_OK;
}

}  // namespace

extern "C" {

int sstem_crop_orient_u8(const uint8_t* pool, const int64_t* images, int64_t n_images, const int32_t* samples, const int32_t* plane_image,
                         int64_t n, int64_t P, int64_t S_h, int64_t S_w, uint8_t* out, void* stream)
{
    const char* what = "crop orient (u8)";
    bool done;
    const int rc = crop_orient_checks(what, pool, images, n_images, samples, plane_image, n, P, S_h, S_w, 0, 0, &done);
    if (rc != SSTEM_OK || done) return rc;
    if (!out) return fail(SSTEM_ERR_NULL_POINTER, "%s: null output", what);
    return launched(what, sstem::launch_crop_orient_u8(pool, images, (int)n_images, samples, plane_image, (int)n, (int)P, (int)S_h, (int)S_w, out,
                                                       static_cast<hipStream_t>(stream)), " launch");
}

int sstem_crop_orient_f32(const uint8_t* pool, const int64_t* images, int64_t n_images, const int32_t* samples, const int32_t* plane_image,
                          int64_t n, int64_t P, int64_t S_h, int64_t S_w, const int32_t* chan_plane, int64_t C0, int64_t C1,
                          uint32_t chan_invert, float* out0, float* out1, void* stream)
{
    const char* what = "crop orient (f32)";
    bool done;
    const int rc = crop_orient_checks(what, pool, images, n_images, samples, plane_image, n, P, S_h, S_w, C0, C1, &done);
    if (rc != SSTEM_OK) return rc;
    if (C0 < 1) return fail(SSTEM_ERR_BAD_SHAPE, "%s: C0 must be at least 1", what);
    if (done) return SSTEM_OK;
    if (!chan_plane || !out0 || (C1 > 0 && !out1)) return fail(SSTEM_ERR_NULL_POINTER, "%s: null channel map or output", what);
    for (int64_t c = 0; c < C0 + C1; ++c)
        if (chan_plane[c] < 0 || chan_plane[c] >= P) return fail(SSTEM_ERR_BAD_SHAPE, "%s: a channel's plane is outside [0, P)", what);
    return launched(what, sstem::launch_crop_orient_f32(pool, images, (int)n_images, samples, plane_image, (int)n, (int)P, (int)S_h, (int)S_w,
                                                        chan_plane, (int)C0, (int)C1, chan_invert, out0, out1,
                                                        static_cast<hipStream_t>(stream)), " launch");
}

}  // extern "C"

// ---- image outputs (include/sstem_display.h) ------------------------------------------------------------------------------------------
namespace {

// the checks the two display entries share, ahead of their pointers; `done` is set when the call is a successful no-op
int display_checks(const char* what, int64_t B, int64_t H, int64_t W, bool* done)
{
    *done = false;
    if (B < 0 || H < 0 || W < 0) return fail(SSTEM_ERR_BAD_SHAPE, "%s: negative size", what);
    if (!fold_range_ok(B, H, W)) return fail(SSTEM_ERR_UNSUPPORTED, "%s: sizes past the index range (H, W <= 32768, B <= 2^24)", what);
    if (B == 0 || H == 0 || W == 0) *done = true;
    return SSTEM_OK;
}

}  // namespace

extern "C" {

const uint8_t* sstem_flow_color_wheel(void) { return sstem::flow_color_wheel(); }

int64_t sstem_flow_color_workspace_bytes(int64_t B) { return B < 0 ? 0 : 4 * sstem::FLOW_MAXRAD_PARTS * B; }

int sstem_flow_color_u8(const float* flow, int64_t B, int64_t H, int64_t W, int hwc, uint8_t* rgb, void* workspace, void* stream)
{
    const char* what = "flow colour";
    bool done;
    const int rc = display_checks(what, B, H, W, &done);
    if (rc != SSTEM_OK || done) return rc;
    if (!flow || !rgb || !workspace) return fail(SSTEM_ERR_NULL_POINTER, "%s: null flow, rgb or workspace", what);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(SSTEM_ERR_UNSUPPORTED, "%s: the workspace must be 8-byte aligned", what);
    return launched(what, sstem::launch_flow_color(flow, (int)B, H * W, hwc ? 1 : 0, rgb, static_cast<unsigned*>(workspace),
                                                   static_cast<hipStream_t>(stream)), " launch");
}

int sstem_sff_outputs_u8(const float* pred, const float* warped, const uint8_t* interp, int64_t B, int64_t H, int64_t W,
                         uint8_t* pred_u8, uint8_t* warped_rgb, uint8_t* stitch_u8, void* stream)
{
    const char* what = "sff outputs";
    bool done;
    const int rc = display_checks(what, B, H, W, &done);
    if (rc != SSTEM_OK || done) return rc;
    if (pred_u8 && !pred) return fail(SSTEM_ERR_NULL_POINTER, "%s: pred_u8 needs pred", what);
    if (warped_rgb && !warped) return fail(SSTEM_ERR_NULL_POINTER, "%s: warped_rgb needs warped", what);
    if (stitch_u8 && (!warped || !interp)) return fail(SSTEM_ERR_NULL_POINTER, "%s: stitch_u8 needs warped and interp", what);
    if (!pred_u8 && !warped_rgb && !stitch_u8) return SSTEM_OK;
    return launched(what, sstem::launch_sff_outputs(pred, warped, interp, (int)B, H * W, pred_u8, warped_rgb, stitch_u8,
                                                    static_cast<hipStream_t>(stream)), " launch");
}

}  // extern "C"
