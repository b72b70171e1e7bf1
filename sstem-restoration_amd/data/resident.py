"""A training set resident on the device, and the oriented gather that cuts batches out of it (``include/sstem_batch.h``).

A training set is a few dozen uint8 sections: uploaded once, it stays in HBM, and a batch then needs only integers from the host --
which image, where, which orientation.  ``crop_u8`` / ``crop_f32`` are one launch each, bit for bit what the reference's providers
compute in numpy (crop, ``fliplr`` / ``flipud`` / transpose / ``rot90``, replication, ``astype(np.float32) / 255.0``).

    resident = ResidentImages(sections, "cuda:0")              # list of 2-D uint8 arrays, one upload
    table = sample_table([(oy, ox, code)], [[3, 4, 5]], resident.device)
    im, lb = crop_f32(resident, table, 256, 256, [0, 0, 0, 2, 2, 2, 1], 6)

GPU only -- there is no CPU fallback.
"""
import collections
import ctypes

import numpy as np
import torch

import sstem_native

FLIPLR, FLIPUD, TRANSPOSE = 1, 2, 4
MAX_PLANES = MAX_CHANNELS = 16

# the simple augmentations of the SFF providers' config (DATA.AUG.random_fliplr, random_flipud, random_flipz, random_rotation, swap)
AugFlags = collections.namedtuple("AugFlags", "fliplr flipud flipz rotation swap")


def _lr(m):
    return [row[::-1] for row in m]


def _ud(m):
    return m[::-1]


def _tr(m):
    return [list(row) for row in zip(*m)]


def _rot90(m, r):
    for _ in range(r % 4):                                  # np.rot90(m, 1) == np.transpose(np.fliplr(m))
        m = _tr(_lr(m))
    return m


def _code_form(m, code):
    """fliplr^(code & 1)( flipud^(code & 2)( transpose^(code & 4)( m ) ) ): the kernel's form"""
    if code & TRANSPOSE:
        m = _tr(m)
    if code & FLIPUD:
        m = _ud(m)
    if code & FLIPLR:
        m = _lr(m)
    return m


_PROBE = [[0, 1], [2, 3]]                                   # its eight dihedral images are distinct
_CODE_OF = {repr(_code_form(_PROBE, code)): code for code in range(8)}


def orientation_code(fliplr, flipud, flipz, r):
    """The 3-bit code of the interp and fusion providers' sequence (``data_provider.py:115-125``): ``np.fliplr`` and ``np.flipud``, each
    if drawn, then ``np.transpose`` if drawn, then ``np.rot90(., r)``."""
    m = _PROBE
    if fliplr:
        m = _lr(m)
    if flipud:
        m = _ud(m)
    if flipz:
        m = _tr(m)
    return _CODE_OF[repr(_rot90(m, r))]


# sp_scripts_train/dataset.py:217-236 RotationFlip(image, case): identity, fliplr, rot90, fliplr(rot90), rot180, fliplr(rot180),
# rot270, fliplr(rot270)
SP_ROTATION_FLIP = (0, 1, 6, 7, 3, 2, 5, 4)
assert SP_ROTATION_FLIP == tuple(_CODE_OF[repr(_lr(_rot90(_PROBE, case // 2)) if case & 1 else _rot90(_PROBE, case // 2))] for case in range(8))


class ResidentImages(object):
    """The device byte pool of a list of 2-D uint8 images and its table ``[n_images][3]`` int64 of (byte offset, H, W); one upload."""

    def __init__(self, images, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("the resident set lives on the GPU")
        arrays = []
        for im in images:
            a = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 2:
                raise ValueError("images must be 2-D uint8 arrays")
            arrays.append(np.ascontiguousarray(a))
        self.shapes = [a.shape for a in arrays]
        rows, offset = [], 0
        for a in arrays:
            rows.append((offset, a.shape[0], a.shape[1]))
            offset += a.size
        self.device = device
        self.nbytes = offset
        host = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros((0,), np.uint8)
        self.pool = torch.from_numpy(host).to(device)
        self.table = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 3).to(device)

    def __len__(self):
        return len(self.shapes)


class SampleTable(object):
    """The integer tables of one batch on the device: ``samples [n][3]`` (oy, ox, code) and ``plane_image [n][P]`` int32."""

    def __init__(self, samples, plane_image):
        self.samples, self.plane_image = samples, plane_image
        self.n, self.P = plane_image.shape


def sample_table(samples, plane_image, device):
    """Host rows -> SampleTable, as ONE upload: both tables travel in one int32 tensor."""
    n = len(samples)
    P = len(plane_image[0]) if n else 1
    host = torch.tensor([list(s) + list(ids) for s, ids in zip(samples, plane_image)], dtype=torch.int32).reshape(n, 3 + P)
    # the kernel wants each table dense: they are laid end to end on the host and copied together
    flat = torch.cat([host[:, :3].reshape(-1), host[:, 3:].reshape(-1)]).to(device)
    return SampleTable(flat[:3 * n].view(n, 3), flat[3 * n:].view(n, P))


def _check(resident, table):
    if not isinstance(resident, ResidentImages):
        raise NotImplementedError("crops are cut from a ResidentImages set on the GPU")
    for t in (table.samples, table.plane_image):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise NotImplementedError("the crop kernels are GPU-only")
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == resident.device
    assert table.samples.shape == (table.n, 3) and table.plane_image.shape == (table.n, table.P)


def crop_u8(resident, table, S_h, S_w, out=None):
    """One launch, no synchronisation: ``out [P][n][S_h][S_w]`` uint8, plane-major (``out[0]``, ``out[1]`` are the ``clean`` and ``interp``
    of ``sstem_fold_degrade_u8``).  A sample with a bad row writes nothing (``include/sstem_batch.h``)."""
    _check(resident, table)
    if out is None:
        out = torch.empty((table.P, table.n, S_h, S_w), dtype=torch.uint8, device=resident.device)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (table.P, table.n, S_h, S_w) and out.is_contiguous()
    lib = sstem_native.load_library()
    with torch.cuda.device(resident.device):
        rc = lib.sstem_crop_orient_u8(resident.pool.data_ptr(), resident.table.data_ptr(), len(resident), table.samples.data_ptr(),
                                      table.plane_image.data_ptr(), table.n, table.P, S_h, S_w, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_crop_orient_u8")
    return out


def crop_f32(resident, table, S_h, S_w, chan_plane, C0, invert=0, out0=None, out1=None):
    """One launch, no synchronisation: ``out0 [n][C0][S_h][S_w]`` and ``out1 [n][C1][S_h][S_w]`` fp32 (``None`` when ``C1 == 0``), channel c
    = plane ``chan_plane[c]`` / 255, or (255 - it) / 255 where bit c of ``invert`` is set; ``C1 = len(chan_plane) - C0``."""
    _check(resident, table)
    C1 = len(chan_plane) - C0
    dev = resident.device
    if out0 is None:
        out0 = torch.empty((table.n, C0, S_h, S_w), dtype=torch.float32, device=dev)
    if out1 is None and C1 > 0:
        out1 = torch.empty((table.n, C1, S_h, S_w), dtype=torch.float32, device=dev)
    assert out0.is_cuda and out0.dtype == torch.float32 and tuple(out0.shape) == (table.n, C0, S_h, S_w) and out0.is_contiguous()
    assert C1 == 0 or (out1.is_cuda and out1.dtype == torch.float32 and tuple(out1.shape) == (table.n, C1, S_h, S_w) and out1.is_contiguous())
    chan = (ctypes.c_int32 * max(1, len(chan_plane)))(*chan_plane)
    lib = sstem_native.load_library()
    with torch.cuda.device(dev):
        rc = lib.sstem_crop_orient_f32(resident.pool.data_ptr(), resident.table.data_ptr(), len(resident), table.samples.data_ptr(),
                                       table.plane_image.data_ptr(), table.n, table.P, S_h, S_w, chan, C0, C1, invert, out0.data_ptr(),
                                       None if C1 == 0 else out1.data_ptr(), torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_crop_orient_f32")
    return out0, (out1 if C1 > 0 else None)
