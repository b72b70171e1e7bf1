"""``SeparableConvolution`` -- the reference's operator API on MI355X.

Mirrors ``libs/sepconv/SeparableConvolution.py:11-78`` of the reference:

* ``SeparableConvolution.apply(input[B,C,H+50,W+50], vertical[B,51,H,W],
  horizontal[B,51,H,W]) -> output[B,C,H,W]``
* the same shape/contiguity assertions (reference ``:29-35``),
* GPU tensors go to the native library, CPU tensors raise
  ``NotImplementedError`` (reference ``:47-48``) -- there is deliberately no CPU or
  PyTorch fallback in the product path,
* ``backward`` returns ``(grad_input, grad_vertical, grad_horizontal)`` where
  ``grad_input`` is all zeros: the reference's launcher never writes it
  (``src/SeparableConvolution_kernel.cu:152-206``).

Extension (round 5): ``vertical`` / ``horizontal`` may be bfloat16 tensors (BASELINE config 5, "bf16 activations with fp32 sepconv
accumulate"): frames, output and all sums stay float32.

Differences: the native kernels overwrite every output element, so the outputs
are allocated with ``empty`` instead of three extra zero-fill passes (``:37,60-62``);
``grad_input`` is still a zero tensor.  A non-GPU ``grad_output`` raises instead of
silently returning zero gradients (reference ``:64,76``).

Addition (opt-in): the input gradient the reference leaves at zero.  ``set_input_gradient(True)``, the context manager
``input_gradient()`` or the environment variable ``SSTEM_SEPCONV_INPUT_GRAD=1`` (read once at import; default off) make ``backward``
compute ``grad_input`` with ``sstem_sepconv_backward_input_*`` (include/sstem_sepconv.h) when the input requires a gradient, and
return ``None`` for it -- no zero-fill, no launch -- when it does not.  Off, ``backward`` is what it always was.
"""
import contextlib
import os

import torch

import libs.sepconv._ext as _ext  # noqa: F401  (same import shape as the reference, :7-8)
import libs.sepconv._ext.cunnex

_input_gradient = os.environ.get("SSTEM_SEPCONV_INPUT_GRAD", "0").strip().lower() not in ("", "0", "false", "off", "no")


def set_input_gradient(enabled):
    """True: ``backward`` computes the input gradient; False (the default): it returns zeros, as the reference does."""
    global _input_gradient
    _input_gradient = bool(enabled)


def get_input_gradient():
    return _input_gradient


@contextlib.contextmanager
def input_gradient(enabled=True):
    """``with input_gradient(): loss.backward()`` -- the switch for one block; the previous state comes back on any exit."""
    previous = get_input_gradient()
    set_input_gradient(enabled)
    try:
        yield
    finally:
        set_input_gradient(previous)


class SeparableConvolution(torch.autograd.Function):
    FILTER = 51

    @staticmethod
    def forward(context, input, vertical, horizontal):
        context.save_for_backward(input, vertical, horizontal)

        batches, depth, in_h, in_w = input.shape
        taps = min(vertical.size(1), horizontal.size(1))
        out_h = min(vertical.size(2), horizontal.size(2))
        out_w = min(vertical.size(3), horizontal.size(3))

        assert in_h - 51 == out_h - 1
        assert in_w - 51 == out_w - 1
        assert taps == 51

        assert input.is_contiguous()
        assert vertical.is_contiguous()
        assert horizontal.is_contiguous()

        if not input.is_cuda:
            raise NotImplementedError()  # as the reference: no CPU version of the op

        output = input.new_empty((batches, depth, out_h, out_w))
        _ext.cunnex.SeparableConvolution_cuda_forward(input, vertical, horizontal, output)
        return output

    @staticmethod
    def backward(context, grad_output):
        _input, vertical, horizontal = context.saved_tensors

        if not grad_output.is_cuda:
            raise NotImplementedError()

        grad_output = grad_output.contiguous()
        if _input_gradient:
            return SeparableConvolution._backward_with_input(context, grad_output, _input, vertical, horizontal)
        grad_input = torch.zeros_like(_input)
        # bfloat16 coefficient tensors (BASELINE config 5; include/sstem_sepconv.h, ..._bf16coef): the kernels read them as they
        # are and write fp32 gradients; autograd wants a gradient of its input's dtype, so they are rounded on the way out
        grad_vertical = torch.empty_like(vertical, dtype=torch.float32)
        grad_horizontal = torch.empty_like(horizontal, dtype=torch.float32)

        _ext.cunnex.SeparableConvolution_cuda_backward(
            grad_output, _input, vertical, horizontal,
            grad_input, grad_vertical, grad_horizontal)

        if vertical.dtype != torch.float32:
            grad_vertical, grad_horizontal = grad_vertical.to(vertical.dtype), grad_horizontal.to(horizontal.dtype)
        return grad_input, grad_vertical, grad_horizontal

    @staticmethod
    def _backward_with_input(context, grad_output, _input, vertical, horizontal):
        """The switch is on: grad_input is computed (or None when the input does not require it) -- the kernel writes every element."""
        grad_input = None
        if context.needs_input_grad[0]:
            grad_input = torch.empty_like(_input)
            _ext.cunnex.SeparableConvolution_cuda_backward_input(grad_output, vertical, horizontal, grad_input)
        grad_vertical = grad_horizontal = None
        if context.needs_input_grad[1] or context.needs_input_grad[2]:
            grad_vertical = torch.empty_like(vertical, dtype=torch.float32)
            grad_horizontal = torch.empty_like(horizontal, dtype=torch.float32)
            _ext.cunnex.SeparableConvolution_cuda_backward(
                grad_output, _input, vertical, horizontal,
                None, grad_vertical, grad_horizontal)
            if vertical.dtype != torch.float32:
                grad_vertical, grad_horizontal = grad_vertical.to(vertical.dtype), grad_horizontal.to(horizontal.dtype)
        return grad_input, grad_vertical, grad_horizontal


class _SepconvGray(torch.autograd.Function):
    @staticmethod
    def forward(context, plane, vertical, horizontal):
        assert plane.dim() == 4 and plane.size(1) == 1
        if not plane.is_cuda:
            raise NotImplementedError()
        context.save_for_backward(plane, vertical, horizontal)
        B, _, in_h, in_w = plane.shape
        input3 = plane.expand(B, 3, in_h, in_w).contiguous()
        output = plane.new_empty((B, 3, vertical.size(2), vertical.size(3)))
        _ext.cunnex.SeparableConvolution_cuda_forward(input3, vertical, horizontal, output)
        return output

    @staticmethod
    def backward(context, grad_output):
        plane, vertical, horizontal = context.saved_tensors
        if not grad_output.is_cuda:
            raise NotImplementedError()
        grad_output = grad_output.contiguous()
        B, _, in_h, in_w = plane.shape
        grad_plane = None
        if context.needs_input_grad[0]:
            if _input_gradient:
                grad_plane = torch.empty_like(plane)
                _ext.cunnex.SeparableConvolution_cuda_backward_input(grad_output.sum(1, keepdim=True), vertical, horizontal, grad_plane)
            else:
                grad_plane = torch.zeros_like(plane)
        grad_vertical = grad_horizontal = None
        if context.needs_input_grad[1] or context.needs_input_grad[2]:
            grad_vertical = torch.empty_like(vertical, dtype=torch.float32)
            grad_horizontal = torch.empty_like(horizontal, dtype=torch.float32)
            _ext.cunnex.SeparableConvolution_cuda_backward(
                grad_output, plane.expand(B, 3, in_h, in_w).contiguous(), vertical, horizontal,
                None, grad_vertical, grad_horizontal)
            if vertical.dtype != torch.float32:
                grad_vertical, grad_horizontal = grad_vertical.to(vertical.dtype), grad_horizontal.to(horizontal.dtype)
        return grad_plane, grad_vertical, grad_horizontal


def sepconv_gray(plane, vertical, horizontal):
    """``SeparableConvolution`` on a grayscale frame: ``plane[B,1,H+50,W+50]``, coefficients ``[B,51,H,W]`` -> ``[B,3,H,W]``, the
    existing op on the plane expanded to three channels (the same output bits).

    Under the input-gradient switch the backward hands ``grad_output.sum(1, keepdim=True)`` to the one-channel kernel: a third of the
    work of differentiating through ``expand`` + ``SeparableConvolution``.  The two agree only to rounding: here the channel sum is
    taken BEFORE the products (one chain over fl(g0 + g1 + g2)), there AFTER them (three chains, then summed by ``expand``'s
    backward).  With the switch off the plane's gradient is zeros, as everywhere else."""
    assert plane.is_contiguous() and vertical.is_contiguous() and horizontal.is_contiguous()
    assert vertical.size(1) == 51 and horizontal.size(1) == 51
    assert plane.size(2) - 51 == vertical.size(2) - 1 and plane.size(3) - 51 == vertical.size(3) - 1
    return _SepconvGray.apply(plane, vertical, horizontal)
