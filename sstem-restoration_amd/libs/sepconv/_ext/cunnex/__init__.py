"""ctypes binding of ``csrc/libsstem_hip.so`` under the reference's FFI module name.

The reference exposes two callables here, produced by ``torch.utils.ffi._wrap_function``
around the cffi module ``_cunnex`` (``libs/sepconv/_ext/cunnex/__init__.py:1-15``):

    SeparableConvolution_cuda_forward(input, vertical, horizontal, output)
    SeparableConvolution_cuda_backward(gradLoss, input, vertical, horizontal,
                                       gradInput, gradVertical, gradHorizontal)

Both take torch tensors, write their outputs in place on the current stream and
return 1.  The same two names with the same argument order live here; they unwrap
the tensors to raw device pointers + sizes and call the C-ABI
(``sstem_sepconv_forward_f32`` / ``sstem_sepconv_backward_f32``).

There is NO fallback: if the shared library is missing or fails to load, every
call raises (``ImportError``/``RuntimeError``); a CPU tensor is refused by the
caller exactly as in the reference (``SeparableConvolution.py:47-48``).
"""
import torch

__all__ = [
    "SeparableConvolution_cuda_forward",
    "SeparableConvolution_cuda_backward",
    "SeparableConvolution_cuda_backward_input",
    "library_path",
    "load_library",
]

from sstem_native import C_ABI, check, library_path, load_library  # noqa: F401  (one loader for the whole C-ABI)

ALGO_AUTO, ALGO_DIRECT, ALGO_MFMA = 0, 1, 2
_forced_algo = ALGO_AUTO


def set_algorithm(algo):
    """Force a kernel family (tests / A-B benchmarks).  0 auto, 1 direct, 2 mfma."""
    global _forced_algo
    if algo not in (ALGO_AUTO, ALGO_DIRECT, ALGO_MFMA):
        raise ValueError("unknown sepconv algorithm id %r" % (algo,))
    _forced_algo = algo


def _dev_tensor(t, name, coef=False):
    """coef: a coefficient tensor (vertical / horizontal) -- float32, or bfloat16 for the ..._bf16coef entry points
    (include/sstem_sepconv.h: BASELINE config 5)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s)" % (name, t.device))
    if t.dtype != torch.float32 and not (coef and t.dtype == torch.bfloat16):
        raise TypeError("%s must be float32%s (got %s)" % (name, " or bfloat16" if coef else "", t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    return t


def _same_device(tensors):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError("all tensors must be on the same device (%s vs %s)" % (dev, t.device))
    return dev


def _checked(named, vertical, horizontal, then=()):
    """The prologue of the three entry points: every (tensor, name) of `named` is a usable device tensor, the two coefficient
    tensors have one dtype, then the tensors of `then`, and all live on one device.  -> (bfloat16 coefficients?, the device)"""
    ts = [_dev_tensor(t, name, coef=name in ("vertical", "horizontal")) for t, name in named]
    if vertical.dtype != horizontal.dtype:
        raise TypeError("vertical and horizontal must have one dtype (%s vs %s)" % (vertical.dtype, horizontal.dtype))
    ts += [_dev_tensor(t, name) for t, name in then]
    return vertical.dtype == torch.bfloat16, _same_device(ts)


def _launch(dev, entry, args, after_stream=(), what=None):
    """entry(*args, the current stream of dev, *after_stream); a status other than 0 raises under the entry's name, or `what`."""
    with torch.cuda.device(dev):
        rc = getattr(load_library(), entry)(*args, torch.cuda.current_stream().cuda_stream, *after_stream)
    check(rc, what or entry)
    return 1


def SeparableConvolution_cuda_forward(input, vertical, horizontal, output):
    load_library()
    bf16, dev = _checked([(input, "input"), (vertical, "vertical"), (horizontal, "horizontal"), (output, "output")], vertical, horizontal)
    B, C, H, W = output.shape
    if tuple(input.shape) != (B, C, H + 50, W + 50) or tuple(vertical.shape) != (B, 51, H, W) \
            or tuple(horizontal.shape) != (B, 51, H, W):
        raise RuntimeError("sepconv forward: inconsistent shapes in=%s v=%s h=%s out=%s" % (
            tuple(input.shape), tuple(vertical.shape), tuple(horizontal.shape), tuple(output.shape)))
    args = [input.data_ptr(), vertical.data_ptr(), horizontal.data_ptr(), output.data_ptr(), B, C, H, W]
    if bf16:
        return _launch(dev, "sstem_sepconv_forward_bf16coef", args)
    return _launch(dev, "sstem_sepconv_forward_f32_algo", args, (_forced_algo,), what="sstem_sepconv_forward_f32")


def SeparableConvolution_cuda_backward(gradLoss, input, vertical, horizontal,
                                       gradInput, gradVertical, gradHorizontal):
    load_library()
    bf16, dev = _checked([(gradLoss, "gradLoss"), (input, "input"), (vertical, "vertical"), (horizontal, "horizontal"),
                          (gradVertical, "gradVertical"), (gradHorizontal, "gradHorizontal")],      # gradients: always float32
                         vertical, horizontal, then=[(gradInput, "gradInput")] if gradInput is not None else [])
    B, C, H, W = gradLoss.shape
    if tuple(input.shape) != (B, C, H + 50, W + 50) or tuple(vertical.shape) != (B, 51, H, W) \
            or tuple(horizontal.shape) != (B, 51, H, W) \
            or gradVertical.shape != vertical.shape or gradHorizontal.shape != horizontal.shape:
        raise RuntimeError("sepconv backward: inconsistent shapes")
    args = [gradLoss.data_ptr(), input.data_ptr(), vertical.data_ptr(), horizontal.data_ptr(),
            gradInput.data_ptr() if gradInput is not None else None, gradVertical.data_ptr(), gradHorizontal.data_ptr(), B, C, H, W]
    if bf16:
        return _launch(dev, "sstem_sepconv_backward_bf16coef", args)
    return _launch(dev, "sstem_sepconv_backward_f32_algo", args, (_forced_algo,), what="sstem_sepconv_backward_f32")


def SeparableConvolution_cuda_backward_input(gradLoss, vertical, horizontal, gradInput):
    """gradInput[B,C,H+50,W+50] = the input gradient of the op -- this package's addition: the reference's backward never writes its
    gradInput (kernel.cu:152-206).  Every element is written; ``set_algorithm`` is honoured (fp32 coefficients)."""
    load_library()
    bf16, dev = _checked([(gradLoss, "gradLoss"), (vertical, "vertical"), (horizontal, "horizontal"), (gradInput, "gradInput")],
                         vertical, horizontal)
    B, C, H, W = gradLoss.shape
    if tuple(gradInput.shape) != (B, C, H + 50, W + 50) or tuple(vertical.shape) != (B, 51, H, W) \
            or tuple(horizontal.shape) != (B, 51, H, W):
        raise RuntimeError("sepconv backward input: inconsistent shapes g=%s v=%s h=%s gradInput=%s" % (
            tuple(gradLoss.shape), tuple(vertical.shape), tuple(horizontal.shape), tuple(gradInput.shape)))
    args = [gradLoss.data_ptr(), vertical.data_ptr(), horizontal.data_ptr(), gradInput.data_ptr(), B, C, H, W]
    if bf16:
        return _launch(dev, "sstem_sepconv_backward_input_bf16coef", args)
    return _launch(dev, "sstem_sepconv_backward_input_f32_algo", args, (_forced_algo,), what="sstem_sepconv_backward_input_f32")
