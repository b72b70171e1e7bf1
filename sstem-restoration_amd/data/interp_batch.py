"""The IFNet training batch of the SFF interpolation loop from a device-resident set: what the reference's ``Train.__getitem__`` builds
per sample on the host (``sff_scripts_interp/data/data_provider.py:93-141``) as one upload of integers and one launch per batch.

The host keeps what is random (``draw_interp_sample`` consumes the ``random`` stream exactly as ``__getitem__`` does); the device crops the
three planes of the drawn triplet, orients them, replicates the outer two to three channels each and divides by 255
(``sstem_crop_orient_f32``, ``include/sstem_batch.h``) -- bit for bit the reference's ``im`` and ``lb``.

    resident = ResidentImages(sections, "cuda:0")
    batcher = InterpBatcher(resident, triplets, 256, AugFlags(True, True, True, True, True))
    im, lb = batcher.batch(random, 8)                     # [8,6,256,256], [8,1,256,256] fp32
    step.load(im, lb)

Colour jitter, ``_gauss_noise`` and ``_elastic_transform`` are not built.  GPU only.
"""
from data.resident import AugFlags, crop_f32, orientation_code, sample_table

IFNET_CHANNELS = (0, 0, 0, 2, 2, 2, 1)                    # im = first x 3, last x 3 | lb = middle


def draw_orientation(rng, flags):
    """The draws of ``data_provider.py:115-125`` -> orientation code.  A disabled augmentation draws nothing (the ``and`` short-circuits)."""
    fliplr = bool(flags.fliplr) and rng.uniform(0, 1) < 0.5
    flipud = bool(flags.flipud) and rng.uniform(0, 1) < 0.5
    flipz = bool(flags.flipz) and rng.uniform(0, 1) < 0.5
    r = rng.randint(0, 3) if flags.rotation else 0
    return orientation_code(fliplr, flipud, flipz, r)


def draw_interp_sample(rng, flags, shapes, crop):
    """One sample ``(k, i, j, code, swap)`` from ``rng`` (a ``random.Random`` or the ``random`` module), consuming it exactly as
    ``__getitem__:99-127`` does: the triplet, the window's row and column, the flips, the rotation, the swap.  ``shapes[k]`` is the
    (H, W) of triplet k's first image; ``crop`` is (rows, columns)."""
    k = rng.randint(0, len(shapes) - 1)
    H, W = shapes[k]
    i = rng.randint(0, H - crop[0])
    j = rng.randint(0, W - crop[1])
    code = draw_orientation(rng, flags)
    swap = bool(flags.swap) and rng.uniform(0, 1) < 0.5
    return k, i, j, code, swap


class InterpBatcher(object):
    """``triplets[k]`` names the three resident images (first, middle, last) of training entry k.  ``batch`` draws B samples in slot
    order, uploads their integer tables once and launches once."""

    def __init__(self, resident, triplets, crop_size, flags=AugFlags(True, True, True, True, True)):
        self.resident, self.triplets, self.flags = resident, [tuple(t) for t in triplets], flags
        self.crop = (crop_size, crop_size) if isinstance(crop_size, int) else tuple(crop_size)
        if (flags.flipz or flags.rotation) and self.crop[0] != self.crop[1]:
            raise ValueError("transposing augmentations need a square crop")
        self.shapes = [resident.shapes[t[0]] for t in self.triplets]

    def draw(self, rng, B):
        samples, planes = [], []
        for _ in range(B):
            k, i, j, code, swap = draw_interp_sample(rng, self.flags, self.shapes, self.crop)
            first, middle, last = self.triplets[k]
            samples.append((i, j, code))
            planes.append((last, middle, first) if swap else (first, middle, last))          # :127-130, a permutation of the planes
        return samples, planes

    def batch(self, rng, B, out=None):
        samples, planes = self.draw(rng, B)
        table = sample_table(samples, planes, self.resident.device)
        im, lb = (None, None) if out is None else out
        return crop_f32(self.resident, table, self.crop[0], self.crop[1], IFNET_CHANNELS, 6, 0, im, lb)
