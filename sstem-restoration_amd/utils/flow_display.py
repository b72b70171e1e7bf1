"""``dense_flow`` / ``flow_to_image`` -- the reference's Middlebury colour code of a flow field, on MI355X.

Mirrors ``utils/flow_display.py:96-138`` of the reference: the same import path (``from utils.flow_display import dense_flow``) and
names.  The reference downloads the predicted flow and colours it with numpy on one core; here the flow stays where the net left it
and two launches write the interleaved RGB bytes (``include/sstem_display.h``, ``csrc/display_kernels.hip``): the reference's
arithmetic as it runs under NumPy 2, float32 up to the maximum radius and float64 from the division on, every image normalised by its
own maximum.

* ``dense_flow(flow)`` = ``flow_to_image(flow)``: one ``[H,W,2]`` float32 GPU tensor (what the scripts hold after
  ``permute(0,2,3,1)`` and ``squeeze``) -> ``[H,W,3]`` uint8 GPU tensor, the array ``Image.fromarray`` takes once it is downloaded.
* ``flow_color_batch(flow)``: ``[B,2,H,W]`` float32, as the flow net emits it -> ``[B,H,W,3]`` uint8.  Neither layout is copied.
* GPU tensors only: a CPU tensor or a numpy array raises ``NotImplementedError``, like every native op of the package.  Nothing
  synchronises.  Unlike the reference, the call never writes ``flow`` (the reference zeroes its unknown pixels in place).
* One workspace per device and stream, owned by this module (512 bytes per image); it grows when a larger batch arrives -- outside graph
  capture, so run a batch size once before capturing it.
* ``sparse_flow`` is matplotlib plotting and is not provided.
"""
import torch

import sstem_native

_workspaces = {}


def _workspace(lib, B, device):
    """The workspace of (device, current stream), grown to the batch at hand; the library never needs it cleared."""
    need = int(lib.sstem_flow_color_workspace_bytes(B))
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("flow_display: the workspace has to grow for %d images -- run this batch size once before capturing" % B)
        buf = _workspaces[key] = torch.empty(max(need, 64), dtype=torch.uint8, device=device)
    return buf


def _gpu_f32(flow):
    if not isinstance(flow, torch.Tensor) or not flow.is_cuda:
        raise NotImplementedError("flow_display is GPU-only: flow must be a GPU tensor")
    if flow.dtype != torch.float32:
        raise TypeError("flow_display: flow must be float32 (got %s)" % flow.dtype)
    return flow.contiguous()


def _colour(flow, B, H, W, hwc):
    lib = sstem_native.load_library()
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=flow.device)
    with torch.cuda.device(flow.device):
        ws = _workspace(lib, B, flow.device)
        rc = lib.sstem_flow_color_u8(flow.data_ptr(), B, H, W, 1 if hwc else 0, rgb.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_flow_color_u8")
    return rgb


def flow_color_batch(flow):
    flow = _gpu_f32(flow)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("flow_display: flow must be [B,2,H,W], got %r" % (tuple(flow.shape),))
    return _colour(flow, flow.shape[0], flow.shape[2], flow.shape[3], False)


def flow_to_image(flow):
    flow = _gpu_f32(flow)
    if flow.dim() != 3 or flow.shape[2] != 2:
        raise ValueError("flow_display: flow must be [H,W,2], got %r" % (tuple(flow.shape),))
    return _colour(flow, 1, flow.shape[0], flow.shape[1], True)[0]


def dense_flow(flow):
    return flow_to_image(flow)
