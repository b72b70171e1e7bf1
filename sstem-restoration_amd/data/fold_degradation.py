"""The SFF training sample as native launches: the fold degradation of the reference's ``Train.degradation`` and the batch tensors of
its ``__getitem__`` (``sff_scripts_fusion/data/data_provider.py:142-169,183-248``, ``sff_scripts_unfolding/data/data_provider.py``).

The host keeps what is random or file-bound (reading, crop positions, flips, the jitter's factors -- and drawing the fold,
``draw_fold``); the device does the arithmetic: per attempt ONE call of ``sstem_fold_degrade_u8`` (``include/sstem_fold.h``) warps every sample's uint8 crop by its
fold, masks the fold line, crops the centre window, counts the black pixels and writes the fp32 batch -- bit for bit the reference's
numbers.  A batch leaves the host as two uint8 crops per sample instead of 6 + 1 fp32 planes -- or, with the sections resident on the
device (``data/resident.py``), as a few integers per sample: ``batch_resident`` draws the crops, cuts and orients them in one launch
of ``sstem_crop_orient_u8`` and runs the same rounds on its output.  With ``jitter=(brightness, contrast, saturation)`` the section that
gets folded is colour-jittered first, as the shipped configurations ask (``data/color_jitter.py``): one table launch per batch, and the
rounds read the section through the table (``sstem_fold_degrade_lut_u8``, ``include/sstem_jitter.h``).

    synth = FoldSynthesizer(det_size=256)
    batch = synth.batch(clean_u8, interp_u8, random)          # [B,400,400] uint8 GPU tensors -> im [B,6,256,256], lb [B,1,256,256]
    batch = synth.batch_resident(resident, pairs, random, 16, 400, flags)      # the same from a ResidentImages set
    step.load(batch.im, batch.lb)

GPU tensors only -- there is no CPU fallback.
"""
import torch

import sstem_native
from data.color_jitter import draw_jitter, jitter_luts
from data.interp_batch import draw_orientation
from data.resident import crop_u8, sample_table
from utils.flow_synthesis import FOLD_PARAMS, fold_scalars, gen_line


def draw_fold(rng, height, width):
    """One candidate fold ``(k, b, line_width, fold_width, dis_k)`` from ``rng`` (a ``random.Random`` or the ``random`` module),
    consuming it exactly as ``degradation`` does (``data_provider.py:188-228``)."""
    line_width = rng.randint(5, 20)
    fold_width = rng.randint(line_width + 1, 80)

    # two end points: 1 --> top line (0, x), 2 --> right line (x, width), 3 --> bottom line (height, x), 4 --> left line (x, 0)
    k1 = rng.randint(1, 4)
    k2 = rng.randint(1, 4)
    while k1 == k2:
        k2 = rng.randint(1, 4)
    points = []
    for side in (k1, k2):
        if side == 1:
            points.append([0, rng.randint(1, width - 1)])
        elif side == 2:
            points.append([rng.randint(1, height - 1), width])
        elif side == 3:
            points.append([height, rng.randint(1, width - 1)])
        else:
            points.append([rng.randint(1, height - 1), 0])
    dis_k = rng.uniform(0.00001, 0.1)
    k, b = gen_line(points[0], points[1])
    return k, b, line_width, fold_width, dis_k


def draw_fusion_crop(rng, flags, shapes, crop):
    """One crop ``(k, i, j, code)`` from ``rng``, consuming it exactly as the fusion and unfolding providers' ``__getitem__`` does
    (``data_provider.py:111-137``): the pair, the window's row and column, the flips, the rotation.  The provider's ``swap`` indexes a
    third plane that its two-plane stack does not have, so ``flags.swap`` is refused."""
    if flags.swap:
        raise ValueError("the fusion provider's swap indexes a third plane it does not have")
    k = rng.randint(0, len(shapes) - 1)
    H, W = shapes[k]
    i = rng.randint(0, H - crop[0])
    j = rng.randint(0, W - crop[1])
    return k, i, j, draw_orientation(rng, flags)


class FoldBatch(object):
    """The tensors of one degraded batch.  ``lb`` is the label the caller asked for: the clean window ``[B,1,h,w]`` (``'image'``) or
    the unfolding flow ``[B,2,h,w]`` (``'flow'``).  ``FoldSynthesizer.batch`` adds ``folds`` (the accepted fold per sample), ``drawn``
    (candidates drawn in all), ``rounds`` and ``launches`` -- and, for a jittered batch, ``lut`` (``[slots,256]`` uint8, the table each
    slot's section was read through) and ``jitter_steps`` (each slot's drawn ``[(code, factor), ...]``); both None otherwise."""

    def __init__(self, slots, window, label, device):
        _, _, h, w = window
        self.window, self.label = tuple(window), label
        self.deformed = torch.empty((slots, h, w), dtype=torch.uint8, device=device)
        self.im = torch.empty((slots, 6, h, w), dtype=torch.float32, device=device)
        self.lb = torch.empty((slots, 2 if label == "flow" else 1, h, w), dtype=torch.float32, device=device)
        self.zero_count = torch.empty((slots,), dtype=torch.int32, device=device)
        self.folds, self.drawn, self.rounds, self.launches = None, 0, 0, 0
        self.lut = self.jitter_steps = None


def fold_table(folds, device):
    """Folds ``(k, b, line_width, fold_width, dis_k)`` -> the device table ``[n, FOLD_PARAMS]`` float64 of ``fold_scalars`` rows."""
    return torch.tensor([fold_scalars(*f) for f in folds], dtype=torch.float64).reshape(len(folds), FOLD_PARAMS).to(device)


def degrade(clean_u8, interp_u8, folds, window, label="image", gt_line=False, slots=None, out=None, lut=None):
    """One launch, no synchronisation: sample i of ``folds`` degrades the plane of batch slot ``slots[i]`` (``i`` without ``slots``).

    clean_u8, interp_u8   ``[B,S_h,S_w]`` uint8 GPU tensors (``interp_u8`` may be None: ``im[:, 3:6]`` is then left unwritten)
    folds                 ``[n, FOLD_PARAMS]`` float64 GPU tensor (``fold_table``), or a list of fold tuples (copied up here)
    window                ``(off_y, off_x, out_h, out_w)`` inside the plane
    slots                 None, or n batch slots (int32 GPU tensor or a list): a redo launches only the rejected samples
    out                   a ``FoldBatch`` to write into (the slots not launched keep what they hold); a new one by default
    lut                   None, or ``[B,256]`` uint8 GPU tensor (``data.color_jitter.jitter_luts``): slot b's section is read through
                          ``lut[b]`` for the warp; the label still reads the section itself
    """
    if not isinstance(clean_u8, torch.Tensor) or not clean_u8.is_cuda or (interp_u8 is not None and not (isinstance(interp_u8, torch.Tensor) and interp_u8.is_cuda)):
        raise NotImplementedError("the fold kernels are GPU-only")
    if label not in ("image", "flow"):
        raise ValueError("label must be 'image' or 'flow'")
    assert clean_u8.dtype == torch.uint8 and clean_u8.dim() == 3 and clean_u8.is_contiguous()
    assert interp_u8 is None or (interp_u8.dtype == torch.uint8 and interp_u8.shape == clean_u8.shape and interp_u8.is_contiguous())
    dev = clean_u8.device
    B, S_h, S_w = clean_u8.shape
    if not isinstance(folds, torch.Tensor):
        folds = fold_table(folds, dev)
    assert folds.is_cuda and folds.dtype == torch.float64 and folds.dim() == 2 and folds.shape[1] == FOLD_PARAMS and folds.is_contiguous()
    n = folds.shape[0]
    if slots is not None and not isinstance(slots, torch.Tensor):
        slots = torch.tensor(list(slots), dtype=torch.int32).to(dev)
    assert slots is None or (slots.is_cuda and slots.dtype == torch.int32 and slots.numel() == n and slots.is_contiguous())
    assert slots is not None or n <= B, "more folds than batch slots"
    assert lut is None or (lut.is_cuda and lut.dtype == torch.uint8 and tuple(lut.shape) == (B, 256) and lut.is_contiguous())
    if out is None:
        out = FoldBatch(B, window, label, dev)
    assert out.window == tuple(window) and out.label == label and out.deformed.shape[0] == B
    off_y, off_x, out_h, out_w = window
    flow_label = label == "flow"
    lib = sstem_native.load_library()
    ins = (clean_u8.data_ptr(), None if interp_u8 is None else interp_u8.data_ptr(), folds.data_ptr(),
           None if slots is None else slots.data_ptr(), n, B, S_h, S_w, off_y, off_x, out_h, out_w, 1 if gt_line else 0)
    outs = (out.deformed.data_ptr(), out.lb.data_ptr() if flow_label else None, out.im.data_ptr(),
            None if flow_label else out.lb.data_ptr(), out.zero_count.data_ptr())
    with torch.cuda.device(dev):
        if lut is None:
            name = "sstem_fold_degrade_u8"
            rc = lib.sstem_fold_degrade_u8(*ins, *outs, torch.cuda.current_stream().cuda_stream)
        else:
            name = "sstem_fold_degrade_lut_u8"
            rc = lib.sstem_fold_degrade_lut_u8(*ins, lut.data_ptr(), *outs, torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, name)
    out.launches += 1
    return out


class FoldSynthesizer(object):
    """The reference's rejection loop over a batch: a sample is redrawn while fewer than ``min_zero`` of its window's pixels came out
    black (``data_provider.py:239-244``).  Per round: draw a fold for every pending sample, one launch, one readback of the B counts;
    only the rejected slots are redrawn and relaunched.  With one sample the random stream is consumed exactly as the reference's
    loop consumes it; with several, round by round in slot order (the reference's workers define no order between samples).

    The plane is square in the reference; like it, both extents of the drawn line and the crop offset come from the plane's height."""

    def __init__(self, det_size=256, min_zero=100):
        self.det_size, self.min_zero = det_size, min_zero

    def window(self, S_h):
        offset = (S_h - self.det_size) // 2
        return (offset, offset, S_h - 2 * offset, S_h - 2 * offset)

    def batch(self, clean_u8, interp_u8, rng, label="image", gt_line=False, jitter=None, jitter_steps=None):
        """``jitter``: None, or the strengths ``(brightness, contrast, saturation)`` of the providers' ColorJitter: every slot's steps are
        drawn in slot order ahead of the first fold round (``draw_jitter``; with B == 1 the reference's order), one table launch, and
        the rounds read ``clean_u8`` through the tables.  ``jitter_steps`` passes steps already drawn instead (``batch_resident``)."""
        B, S_h, _ = clean_u8.shape
        window = self.window(S_h)
        lut = None
        if jitter is not None and jitter_steps is None:
            jitter_steps = [draw_jitter(rng, *jitter) for _ in range(B)]
        if jitter_steps is not None and B > 0:
            lut = jitter_luts(clean_u8, jitter_steps)
        out, pending = None, list(range(B))
        folds = [None] * B
        drawn = rounds = 0
        while pending:
            draws = [draw_fold(rng, S_h, S_h) for _ in pending]
            drawn += len(draws)
            rounds += 1
            out = degrade(clean_u8, interp_u8, draws, window, label, gt_line, None if len(pending) == B else pending, out, lut)
            for s, f in zip(pending, draws):
                folds[s] = f
            counts = out.zero_count.cpu()                                    # the one readback of the round
            pending = [s for s in pending if int(counts[s]) < self.min_zero]
        if out is None:
            out = FoldBatch(0, window, label, clean_u8.device)
        out.folds, out.drawn, out.rounds = folds, drawn, rounds
        out.lut, out.jitter_steps = lut, jitter_steps
        return out

    def batch_resident(self, resident, pairs, rng, B, crop_size, flags, label="image", gt_line=False, jitter=None):
        """The batch from a device-resident set (``data/resident.py``): ``pairs[k]`` names the resident images (section, its
        interpolation) of training entry k.  Draws the B crops in slot order, cuts and orients them in one launch (``crop_u8``: its planes
        0 and 1 are ``clean`` and ``interp``), then runs ``batch`` on them -- no crop leaves the host.  With B == 1 the stream is
        consumed as the reference's ``__getitem__`` consumes it; with more, all crop draws come first, then the fold rounds.  With
        ``jitter`` (see ``batch``) each slot draws its crop, then its jitter -- with B == 1 the reference's crop, jitter, folds."""
        pairs = [tuple(p) for p in pairs]
        shapes = [resident.shapes[p[0]] for p in pairs]
        samples, planes = [], []
        steps = None if jitter is None else []
        for _ in range(B):
            k, i, j, code = draw_fusion_crop(rng, flags, shapes, (crop_size, crop_size))
            samples.append((i, j, code))
            planes.append(pairs[k])
            if jitter is not None:
                steps.append(draw_jitter(rng, *jitter))
        crops = crop_u8(resident, sample_table(samples, planes, resident.device), crop_size, crop_size)
        out = self.batch(crops[0], crops[1], rng, label, gt_line, jitter_steps=steps)
        out.crops = samples
        return out
