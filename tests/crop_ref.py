"""The training-crop contract of include/sstem_batch.h, restated in numpy: the oriented gather from a resident set of uint8 images, its
two output layouts, the samples that write nothing, and -- on top of it -- the sample of the reference's interpolation and fusion
providers as the Python layer composes it (draws, orientation code, swap as a permutation of the planes).

It is the project's own statement, not the reference's code: the gather works from the integer tables the kernel gets, and ``variant``
switches in the deliberate mistakes that tests/test_crop_batch_cpu.py shows the fixture (tests/golden/crop_batch.npz) to catch.  The
images of the fixture and of the GPU tests come from the seeded recipe ``image`` and are not stored."""
import numpy as np

FLIPLR, FLIPUD, TRANSPOSE = 1, 2, 4

# variants of the contract that the fixture must tell from it
MUTANTS = ("transpose_after_flips", "rot90_clockwise", "origin_exchanged", "label_from_plane0", "reciprocal_multiply")


def image(seed, H, W):
    """The seeded uint8 test image, every byte value."""
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def orient(window, code, variant=None):
    """fliplr^(code & 1)( flipud^(code & 2)( transpose^(code & 4)( window ) ) )"""
    out = window
    if variant == "transpose_after_flips":
        if code & FLIPUD:
            out = np.flipud(out)
        if code & FLIPLR:
            out = np.fliplr(out)
        return np.transpose(out) if code & TRANSPOSE else out
    if code & TRANSPOSE:
        out = np.transpose(out)
    if code & FLIPUD:
        out = np.flipud(out)
    if code & FLIPLR:
        out = np.fliplr(out)
    return out


def sample_writes(images, ids, oy, ox, code, S_h, S_w):
    """The rule of include/sstem_batch.h: False for a sample that must write nothing."""
    if not 0 <= code < 8 or oy < 0 or ox < 0:
        return False
    if code & TRANSPOSE and S_h != S_w:
        return False
    for k in ids:
        if not 0 <= k < len(images):
            return False
        H, W = images[k].shape
        if oy + S_h > H or ox + S_w > W:
            return False
    return True


def _plane(images, k, oy, ox, code, S_h, S_w, variant=None):
    src = images[k]
    if code & TRANSPOSE:                                   # the window is square
        return orient(src[oy:oy + S_w, ox:ox + S_h], code, variant)
    return orient(src[oy:oy + S_h, ox:ox + S_w], code, variant)


def crop_u8(images, samples, plane_image, S_h, S_w, out=None, variant=None):
    """out [P][n][S_h][S_w] uint8; samples [n][3] (oy, ox, code), plane_image [n][P].  `out` (sentinel-filled) keeps what it held where a
    sample writes nothing; a new zero array by default."""
    samples, plane_image = np.asarray(samples).reshape(-1, 3), np.asarray(plane_image)
    n, P = plane_image.shape
    if out is None:
        out = np.zeros((P, n, S_h, S_w), dtype=np.uint8)
    for i in range(n):
        oy, ox, code = (int(v) for v in samples[i])
        ids = [int(k) for k in plane_image[i]]
        if not sample_writes(images, ids, oy, ox, code, S_h, S_w):
            continue
        for p in range(P):
            out[p, i] = _plane(images, ids[p], oy, ox, code, S_h, S_w, variant)
    return out


def to_f32(b, variant=None):
    """float32(byte) / float32(255)"""
    if variant == "reciprocal_multiply":
        return b.astype(np.float32) * (np.float32(1) / np.float32(255))
    return b.astype(np.float32) / np.float32(255)


def crop_f32(images, samples, plane_image, S_h, S_w, chan_plane, C0, invert=0, out0=None, out1=None, variant=None):
    """out0 [n][C0][S_h][S_w], out1 [n][C1][S_h][S_w] float32 (out1 None when C1 == 0); channel c reads plane chan_plane[c], inverted
    (255 - byte) when bit c of `invert` is set."""
    samples, plane_image = np.asarray(samples).reshape(-1, 3), np.asarray(plane_image)
    n, P = plane_image.shape
    C1 = len(chan_plane) - C0
    if out0 is None:
        out0 = np.zeros((n, C0, S_h, S_w), dtype=np.float32)
    if out1 is None and C1:
        out1 = np.zeros((n, C1, S_h, S_w), dtype=np.float32)
    planes = crop_u8(images, samples, plane_image, S_h, S_w, variant=variant)
    for i in range(n):
        oy, ox, code = (int(v) for v in samples[i])
        if not sample_writes(images, [int(k) for k in plane_image[i]], oy, ox, code, S_h, S_w):
            continue
        for c, p in enumerate(chan_plane):
            b = planes[p, i]
            if (invert >> c) & 1:
                b = (255 - b.astype(np.int32)).astype(np.uint8)
            v = to_f32(b, variant)
            if c < C0:
                out0[i, c] = v
            else:
                out1[i, c - C0] = v
    return out0, out1


# ---- the providers' sample on top of the gather ----------------------------------------------------------------------------------------
def orientation_code(fliplr, flipud, flipz, r, variant=None):
    """The code of: fliplr, flipud (each if drawn), then transpose, then np.rot90(., r) -- found by pushing a 2 x 2 probe through both forms."""
    probe = np.arange(4).reshape(2, 2)
    m = probe
    if fliplr:
        m = np.fliplr(m)
    if flipud:
        m = np.flipud(m)
    if flipz:
        m = np.transpose(m)
    m = np.rot90(m, -r if variant == "rot90_clockwise" else r)
    for code in range(8):
        if np.array_equal(orient(probe, code), m):
            return code
    raise AssertionError("not a dihedral image")


def draw_sample(rng, flags, shapes, crop):
    """The draws of the interpolation provider's __getitem__ (the fusion provider's are the same with swap off), in its order and with its
    short-circuits: a disabled augmentation draws nothing.  flags: (fliplr, flipud, flipz, rotation, swap).  -> (k, i, j, code, swap)."""
    f_lr, f_ud, f_z, f_rot, f_swap = flags
    k = rng.randint(0, len(shapes) - 1)
    H, W = shapes[k]
    i = rng.randint(0, H - crop[0])
    j = rng.randint(0, W - crop[1])
    lr = bool(f_lr) and rng.uniform(0, 1) < 0.5
    ud = bool(f_ud) and rng.uniform(0, 1) < 0.5
    z = bool(f_z) and rng.uniform(0, 1) < 0.5
    r = rng.randint(0, 3) if f_rot else 0
    swap = bool(f_swap) and rng.uniform(0, 1) < 0.5
    return k, i, j, (lr, ud, z, r), swap


def interp_sample(images, triplets, draw, crop, variant=None):
    """im [6,S,S], lb [1,S,S] float32 of one drawn sample: planes (first, middle, last) of triplet k, the outer two exchanged by swap."""
    k, i, j, (lr, ud, z, r), swap = draw
    code = orientation_code(lr, ud, z, r, variant)
    if variant == "origin_exchanged":
        i, j = j, i
    ids = list(triplets[k])
    if swap:
        ids[0], ids[2] = ids[2], ids[0]
    chan = [0, 0, 0, 2, 2, 2, 0 if variant == "label_from_plane0" else 1]
    im, lb = crop_f32(images, [(i, j, code)], [ids], crop[0], crop[1], chan, 6, variant=variant)
    return im[0], lb[0]


def fusion_crops(images, pairs, draw, crop, variant=None):
    """clean, interp uint8 [S,S] of one drawn fusion sample (planes: the section, its interpolation)."""
    k, i, j, (lr, ud, z, r), _ = draw
    out = crop_u8(images, [(i, j, orientation_code(lr, ud, z, r, variant))], [list(pairs[k])], crop[0], crop[1], variant=variant)
    return out[0, 0], out[1, 0]


# ---- the fixture's cases (tests/golden/make_crop_batch_golden.py) ----------------------------------------------------------------------
ALL_FLAGS = (True, True, True, True, True)
# interp: three triplets over images of two sizes, crop 40
INTERP_IMAGES = [(500 + s, 96, 80) for s in range(4)] + [(510 + s, 64, 72) for s in range(3)]      # (seed, H, W)
INTERP_TRIPLETS = [(0, 1, 2), (1, 2, 3), (4, 5, 6)]
INTERP_CROP = (40, 40)
INTERP_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 16, 24, 29)  # all eight codes, both swap outcomes, every triplet (24, 29: code 7)
INTERP_OTHER_SEEDS = 2                                     # the flag sets other than "all" run the first two seeds
INTERP_FLAG_SETS = {"all": ALL_FLAGS, "noflip": (False, True, False, True, False), "none": (False, False, False, False, False)}
# fusion: pairs (section, interpolated section) of 120 x 110, crop 100, det_size 64
FUSION_IMAGES = [(600 + s, 120, 110) for s in range(4)]
FUSION_PAIRS = [(0, 1), (2, 3)]
FUSION_CROP = (100, 100)
FUSION_DET = 64
FUSION_FLAGS = (True, True, True, True, False)
FUSION_SEEDS = (0, 1, 2, 3)
# the SP loops' RotationFlip on a small non-symmetric square
SP_SQUARE = (700, 6, 6)


def images_of(recipe):
    return [image(*r) for r in recipe]
