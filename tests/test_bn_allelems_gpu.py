"""Every element of the train-mode BatchNorm2d (+ ReLU / LeakyReLU) kernels (csrc/norm_kernels.hip) through the C-ABI of
include/sstem_norm.h, against the float64 reference and the derived bounds of tests/bn_ref64.py: y, dx, save_mean, save_invstd,
running_mean, running_var, dweight, dbias at every element, num_batches_tracked, the amax words slot by slot.

The references are computed on the GPU itself from a device generator.  Every output lies inside a larger NaN-filled tensor whose guard
elements on both sides must stay untouched, and the workspace is NaN-filled before each call.  y is held against float64 computed from
the launch's OWN saved statistics, the backward against the mask of the forward launch's stored y (as torch takes it).

Shapes are (N, C, HW); bn_ref64.SHAPES states what each reaches and the geometry asserted for it (restated by bn_geometry and pinned
to the library through sstem_batchnorm_workspace_floats); bn_ref64.CONFIGS spreads the nullable arguments and flags over them:
weight = bias = NULL, running_* = NULL, num_batches_tracked NULL or not, momentum 0, 1 and 0.1, dweight = dbias = NULL, accumulate on
pre-filled and not on NaN-filled buffers.  The three spellings of each entry point (plain, _ex, _amax) must give the same bits.

Each test prints the worst err / bound it saw, per output (run with -s; DESIGN.md section 3 records them).
"""
import ctypes

import numpy as np
import pytest
import torch

import bn_ref64 as R
import sstem_native
from bn_ref64 import ACT_LEAKY, ACT_NONE, ACT_RELU, ACTS, CONFIGS, EPS, SHAPES
from stream_ref64 import assert_within_rounding

pytestmark = pytest.mark.gpu
WORST = {}
GUARD = 64                                        # floats on either side of every output: 256 bytes, so the outputs stay 16-byte aligned
NAN = float("nan")


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for family in sorted(WORST):
        print("\nWORST err / bound  %-48s %8.3f" % (family, WORST[family]))


def _note(worst, family, what):
    for name, v in worst.items():
        key = "%s, %s" % (family, name)
        WORST[key] = max(WORST.get(key, 0.0), v)
    print("%s [%s]: worst err / bound %s" % (what, family, {k: round(v, 3) for k, v in worst.items()}))


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(lib, name, *args):
    rc = getattr(lib, name)(*args, _stream())
    assert rc == 0, (name, rc, lib.sstem_last_error().decode("utf-8", "replace"))
    torch.cuda.synchronize()


class _Outputs:
    """Output tensors inside guard bands: ``new`` hands out the middle of a larger tensor filled with ``fill``; ``assert_intact`` checks
    that the GUARD elements on both sides of every one of them still hold it."""

    def __init__(self):
        self.held = []

    def new(self, n, fill=NAN, dtype=torch.float32, init=None):
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        mid = buf[GUARD:GUARD + n]
        if init is not None:
            mid.copy_(init)
        self.held.append((buf, n, fill))
        return mid

    def assert_intact(self):
        for buf, n, fill in self.held:
            sides = torch.cat([buf[:GUARD], buf[GUARD + n:]])
            assert bool(torch.isnan(sides).all() if fill != fill else (sides == fill).all()), (n, sides)


def _workspace_floats(lib, shape):
    """sstem_batchnorm_workspace_floats, which must be what the restated geometry gives: 3 floats per (channel, chunk)."""
    N, C, HW = shape
    ws_n = lib.sstem_batchnorm_workspace_floats(N, C, HW)
    assert ws_n == 3 * C * R.bn_geometry(N, C, HW)[2], (shape, ws_n, R.bn_geometry(N, C, HW))
    return ws_n


def _forward(lib, spelling, inp, cfg, act, slope, partials=None, workspace=True):
    """One forward launch through sstem_batchnorm_train_forward{,_ex,_amax}_f32 into guarded, NaN-filled outputs."""
    x = inp["x"]
    N, C, HW = x.shape
    o = _Outputs()
    ws_n = _workspace_floats(lib, (N, C, HW))
    ws = o.new(ws_n) if workspace else None
    y = o.new(N * C * HW)
    sm, si = o.new(C), o.new(C)
    rm = None if inp["running_mean"] is None else o.new(C, init=inp["running_mean"])
    rv = None if inp["running_var"] is None else o.new(C, init=inp["running_var"])
    nbt = o.new(1, fill=-77, dtype=torch.int64, init=torch.tensor([7])) if (cfg["nbt"] and spelling != "plain") else None
    word = o.new(1024, init=torch.zeros(1024)) if spelling == "amax" else None
    tail = (_p(ws), ws_n if workspace else 0, N, C, HW, cfg["momentum"], EPS, act, slope)
    head = (_p(x), _p(inp["weight"]), _p(inp["bias"]), _p(rm), _p(rv))
    n_partials = 0 if partials is None else partials.shape[1]
    if spelling == "plain":
        assert partials is None
        _call(lib, "sstem_batchnorm_train_forward_f32", *head, _p(y), _p(sm), _p(si), *tail)
    elif spelling == "ex":
        _call(lib, "sstem_batchnorm_train_forward_ex_f32", *head, _p(nbt), _p(y), _p(sm), _p(si), _p(partials), n_partials, *tail)
    else:
        _call(lib, "sstem_batchnorm_train_forward_amax_f32", *head, _p(nbt), _p(y), _p(word), _p(sm), _p(si), _p(partials), n_partials, *tail)
    o.assert_intact()
    if nbt is not None:
        assert int(nbt) == 8                       # one more per CALL: not per channel, not per chunk
    if partials is not None and ws is not None:
        assert bool(torch.isnan(ws).all())         # the statistics launch did not run
    return {"y": y.view(N, C, HW), "save_mean": sm, "save_invstd": si, "running_mean": rm, "running_var": rv, "word": word}


def _backward(lib, spelling, inp, cfg, fw, act, slope):
    """One backward launch through sstem_batchnorm_train_backward{,_ex,_amax}_f32; dweight / dbias NaN-filled, or pre-filled with the
    case's prior gradients under accumulate."""
    x = inp["x"]
    N, C, HW = x.shape
    o = _Outputs()
    ws_n = _workspace_floats(lib, (N, C, HW))
    ws = o.new(ws_n)
    dx = o.new(N * C * HW)
    acc = cfg["accumulate"]
    dw = o.new(C, init=inp["prior_dweight"] if acc else None) if cfg["pgrads"] else None
    db = o.new(C, init=inp["prior_dbias"] if acc else None) if cfg["pgrads"] else None
    word = o.new(1024, init=torch.zeros(1024)) if spelling == "amax" else None
    head = (_p(inp["dy"]), _p(x), _p(inp["weight"]), _p(inp["bias"]), _p(fw["save_mean"]), _p(fw["save_invstd"]), _p(dx))
    tail = (_p(dw), _p(db), _p(ws), ws_n, N, C, HW, act, slope)
    if spelling == "plain":
        assert not acc
        _call(lib, "sstem_batchnorm_train_backward_f32", *head, *tail)
    elif spelling == "ex":
        _call(lib, "sstem_batchnorm_train_backward_ex_f32", *head, *tail, acc)
    else:
        _call(lib, "sstem_batchnorm_train_backward_amax_f32", *head, _p(word), *tail, acc)
    o.assert_intact()
    return {"dx": dx.view(N, C, HW), "dweight": dw, "dbias": db, "word": word}


def _same_bits(a, b, names):
    for k in names:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k


FWD_OUT = ("y", "save_mean", "save_invstd", "running_mean", "running_var")
BWD_OUT = ("dx", "dweight", "dbias")


def _assert_amax_word(word, stored):
    """The word was zeroed by the caller: max(word) == max |stored| exactly, and slot by slot -- workgroup (chunk, channel) raises slot
    (channel * chunks + chunk) & 1023 to the largest magnitude of its chunk."""
    N, C, HW = stored.shape
    chunk_len, pieces, chunks = R.bn_geometry(N, C, HW)
    assert float(word.max()) == float(stored.abs().max())
    per = torch.nn.functional.pad(stored.abs(), (0, pieces * chunk_len - HW)).view(N, C, pieces, chunk_len).amax(-1)
    per = per.permute(1, 0, 2).reshape(C * chunks)
    slots = torch.arange(C * chunks, device="cuda") & 1023
    want = torch.zeros(1024, device="cuda").scatter_reduce(0, slots, per, "amax")
    assert torch.equal(word, want)


def _forward_backward_checked(lib, inp, cfg, act, slope, family, what, spellings=True):
    """The _amax spelling forward and backward with every check; the other spellings must give its bits.  Returns (fw, bw)."""
    shape = tuple(inp["x"].shape)
    T = R.threads_terms(R.bn_geometry(*shape)[0])
    fw = _forward(lib, "amax", inp, cfg, act, slope)
    worst = R.check_forward(fw, inp, cfg["momentum"], EPS, act, slope, R.kernel_chunks(inp["x"]), what)
    _assert_amax_word(fw["word"], fw["y"])
    bw = _backward(lib, "amax", inp, cfg, fw, act, slope)
    worst.update(R.check_backward(bw, inp, fw["y"], fw["save_mean"], fw["save_invstd"], act, slope, T, what))
    assert (bw["dweight"] is None) == (not cfg["pgrads"]) and (bw["dbias"] is None) == (not cfg["pgrads"])
    _assert_amax_word(bw["word"], bw["dx"])
    _note(worst, family, what)
    if spellings:
        _same_bits(fw, _forward(lib, "ex", inp, cfg, act, slope), FWD_OUT)
        _same_bits(fw, _forward(lib, "plain", inp, cfg, act, slope), FWD_OUT)
        _same_bits(bw, _backward(lib, "ex", inp, cfg, fw, act, slope), BWD_OUT)
        if not cfg["accumulate"]:
            _same_bits(bw, _backward(lib, "plain", inp, cfg, fw, act, slope), BWD_OUT)
    return fw, bw


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act,slope", ACTS)
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_every_element_at_every_geometry(i, act, slope):
    shape, geometry = SHAPES[i]
    assert R.bn_geometry(*shape) == geometry
    lib = sstem_native.load_library()
    inp = R.case_inputs(shape, CONFIGS[i], _gen(500 + i), device="cuda")
    _forward_backward_checked(lib, inp, CONFIGS[i], act, slope, "chunk_len %d" % geometry[0], "%s act %d" % (shape, act))


def test_configs_cover_every_nullable_argument_and_flag():
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in CONFIGS)
    assert has(affine=False) and has(running=False) and has(nbt=False) and has(nbt=True) and has(pgrads=False)
    assert has(momentum=0.0) and has(momentum=1.0) and has(momentum=0.1)
    assert has(pgrads=True, accumulate=1) and has(pgrads=True, accumulate=0)


# ---- conditioning -------------------------------------------------------------------------------------------------------------------------

def test_conditioning_large_mean_constant_channel_and_outlier_pivot():
    lib = sstem_native.load_library()
    inp = R.conditioning_inputs(_gen(31), device="cuda")
    assert R.bn_geometry(2, 3, 1100) == (1024, 2, 4)
    fw, _ = _forward_backward_checked(lib, inp, CONFIGS[0], ACT_LEAKY, 0.2, "conditioning", "1000 + randn / constant / outlier pivot", spellings=False)
    st = R.bn_stats_ref64(inp["x"], EPS, 0.1, None, None, R.kernel_chunks(inp["x"]))
    assert float(st["S_invstd"][0]) < 400.0                         # held to some hundreds of u from |x - pivot|, not to u * mean^2
    # the constant channel: every x - pivot is zero, the variance exactly 0
    assert float(fw["save_mean"][1]) == -3.25
    assert float(fw["save_invstd"][1]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))))


# ---- hand-made partials -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_partials", [1, 7, 300])
@pytest.mark.parametrize("i", [0, 1, 3, 4])
def test_hand_made_partials_of_any_partition(i, n_partials):
    """(count, mean, M2) triplets of an arbitrary partition -- unequal counts, empty runs that carry a finite mean, 1, 7 and 300 of them --
    formed in float64 and rounded to float32, with workspace = NULL: the same statistics and y bounds (the chunk term is now the
    rounding of the supplied triplets), and a workspace passed all the same is not touched."""
    shape, _ = SHAPES[i]
    lib = sstem_native.load_library()
    cfg = CONFIGS[i]
    inp = R.case_inputs(shape, cfg, _gen(600 + i), device="cuda")
    trip, table = R.partition_triplets(inp["x"], n_partials, seed=7 * n_partials + i)
    assert trip.shape == (shape[1], n_partials, 3) and (n_partials < 3 or bool((trip[..., 0] == 0).any()))
    for spelling in ("ex", "amax"):
        fw = _forward(lib, spelling, inp, cfg, ACT_RELU, 0.0, partials=trip, workspace=False)
        worst = R.check_forward(fw, inp, cfg["momentum"], EPS, ACT_RELU, 0.0, table, "%s, %d partials" % (shape, n_partials))
    _assert_amax_word(fw["word"], fw["y"])
    _note(worst, "hand-made partials", "%s, %d partials" % (shape, n_partials))
    _same_bits(fw, _forward(lib, "amax", inp, cfg, ACT_RELU, 0.0, partials=trip, workspace=True), FWD_OUT)


# ---- one launch ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act,slope", ACTS)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_one_launch_gives_the_two_launch_bits(i, act, slope, monkeypatch):
    shape, _ = SHAPES[i]
    lib = sstem_native.load_library()
    cfg = CONFIGS[i]
    inp = R.case_inputs(shape, cfg, _gen(700 + i), device="cuda")
    monkeypatch.setenv("SSTEM_BN_ONE_LAUNCH", "0")                 # read at every launch
    fw2 = _forward(lib, "amax", inp, cfg, act, slope)
    bw2 = _backward(lib, "amax", inp, cfg, fw2, act, slope)
    monkeypatch.setenv("SSTEM_BN_ONE_LAUNCH", "1")
    fw1 = _forward(lib, "amax", inp, cfg, act, slope)
    bw1 = _backward(lib, "amax", inp, cfg, fw2, act, slope)
    monkeypatch.delenv("SSTEM_BN_ONE_LAUNCH")
    _same_bits(fw1, fw2, FWD_OUT + ("word",))
    _same_bits(bw1, bw2, BWD_OUT + ("word",))


# ---- the mask fixture ---------------------------------------------------------------------------------------------------------------------

def mask_case(lib):
    """The fixture on the device, its bias aimed with the statistics a first launch of ``lib`` saved."""
    x, weight, dy, target = (t.cuda() for t in R.mask_fixture())
    assert R.bn_geometry(*R.MASK_SHAPE) == (1024, 2, 4) and bool((x * 8 == torch.round(x * 8)).all())
    inp = {"x": x, "dy": dy, "weight": weight, "bias": torch.zeros(8, device="cuda"), "running_mean": None, "running_var": None,
           "prior_dweight": None, "prior_dbias": None}
    cfg = dict(CONFIGS[0], running=False)
    first = _forward(lib, "ex", inp, cfg, ACT_NONE, 0.0)
    inp["bias"] = R.mask_bias(first["save_mean"], first["save_invstd"], weight, target)
    return inp, cfg, target


def mask_check(lib, act, slope):
    """Forward and backward on the fixture; the backward reference takes its mask from the launch's stored y.  One element whose mask
    the backward takes the other way misses the dx bound by orders of magnitude and shifts dbias by a whole dy."""
    inp, cfg, target = mask_case(lib)
    fw, bw = _forward_backward_checked(lib, inp, cfg, act, slope, "mask fixture", "mask fixture act %d" % act, spellings=False)
    at_target = inp["x"] == target[None, :, None]
    per_channel = at_target.sum(dim=(0, 2))
    assert int(per_channel.min()) >= 3
    if act == ACT_RELU:
        # the contract, said directly: where the forward stored 0, no gradient passes -- dx = k (-m_dz - xh m_dzx) within the bound
        ref = R.bn_backward_ref64(inp["dy"], inp["x"], fw["y"], fw["save_mean"], fw["save_invstd"], inp["weight"], act, slope, 4)
        cnt = float(R.MASK_SHAPE[0] * R.MASK_SHAPE[2])
        col = lambda t: t.to(torch.float64)[None, :, None]
        xh = (inp["x"].to(torch.float64) - col(fw["save_mean"])) * col(fw["save_invstd"])
        blocked = (col(inp["weight"]) * col(fw["save_invstd"])) * (-col(ref["dbias"]) / cnt - xh * col(ref["dweight"]) / cnt)
        zero = fw["y"] == 0
        print("elements holding the targeted value, per channel: %s; of them stored as 0: %s"
              % (per_channel.tolist(), (zero & at_target).sum(dim=(0, 2)).tolist()))
        assert_within_rounding(bw["dx"][zero], blocked[zero], ref["S_dx"][zero], R.N_DX, "dx where the forward stored 0")
    return fw, bw


@pytest.mark.parametrize("act,slope", ACTS[1:])
def test_mask_fixture_backward_takes_the_mask_of_the_stored_output(act, slope):
    mask_check(sstem_native.load_library(), act, slope)
