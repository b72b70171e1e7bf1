"""CPU-side checks of the flow colour code and the SFF image tail (include/sstem_display.h): the numpy restatement
tests/flow_color_ref.py against bytes recorded from the reference's own dense_flow and from PIL (tests/golden/flow_color.npz), the
wheel, the mutants the fixture has to catch, and the condition on the inputs that lets the GPU tests hold a device's bytes to the
reference although its atan2 need not have numpy's bits.  None of it needs a device."""
import os
import sys

import numpy as np
import pytest

import flow_color_ref as R
import sstem_native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_flow_color_golden as G  # noqa: E402

CASES = list(R.cases())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "flow_color.npz")))


@pytest.fixture(scope="module")
def flows():
    return R.cases()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.skipif(not G.reference_available(), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture(golden):
    fresh = G.generate()
    assert sorted(fresh) == sorted(golden)
    for k in golden:
        if k.endswith("_version"):
            continue
        a, b = np.asarray(fresh[k]), golden[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b), k


def test_inputs_follow_the_recipe(golden, flows):
    for name, flow in flows.items():
        assert flow.dtype == np.float32 and np.array_equal(_bits(flow), _bits(golden["flow_" + name])), name
        assert flow.shape == {"1x1": (1, 1, 2), "1x131": (1, 131, 2), "131x1": (131, 1, 2)}.get(name, (R.H0, R.W0, 2))
    batch = R.batch_case()
    assert np.array_equal(_bits(batch), _bits(golden["flow_batch"])) and batch.shape == (4, 2, R.H0, R.W0)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt((batch.astype(np.float64) ** 2).sum(1)).reshape(4, -1)
    assert np.allclose(np.nanmax(rad[:3], axis=1), [1e-3, 5.0, 4e6], rtol=1e-6) and np.isnan(rad[3]).sum() == 1
    # what the cases are there for
    assert float(R.max_radius(flows["zeros"])) == 0.0 and R.max_radius(flows["one_nan"]) == -1 and R.max_radius(flows["all_nan"]) == -1
    tiny = flows["tiny"]
    assert 0 < float(R.max_radius(tiny)) < 1e-18 and float((tiny[..., 0] * tiny[..., 0]).max()) < 1.2e-38     # the squares are subnormal
    assert np.isinf(flows["unknown"]).sum() == 1 and (np.abs(flows["unknown"]) > 1e7).sum() == 2
    assert np.array_equal(flows["integers"], np.rint(flows["integers"])) and np.abs(flows["integers"]).max() == 20
    knots = flows["knots"]
    assert np.signbit(knots[40, :, 1]).all() and not np.signbit(knots[3, :, 1]).any() and (knots[3, :, 1] == 0).all()
    assert (golden["rgb_zeros"] == 255).all() and (golden["rgb_all_nan"] == 0).all()
    assert (golden["rgb_unknown"][10, 11] == 0).all() and (golden["rgb_unknown"][50, 100] == 0).all() and (golden["rgb_one_nan"][33, 64] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(golden, flows, name):
    before = flows[name].copy()
    got = R.flow_to_image(flows[name])
    assert got.dtype == np.uint8 and np.array_equal(got, golden["rgb_" + name]), "%d bytes differ" % int((got != golden["rgb_" + name]).sum())
    assert np.array_equal(_bits(before), _bits(flows[name])), "the restatement wrote its argument"


def test_restatement_equals_the_reference_on_the_batch(golden):
    batch = R.batch_case()
    assert np.array_equal(R.flow_color_batch(batch), golden["rgb_batch"])
    for i in range(4):                                                       # and every image differs from its neighbours' normalisation
        alone = R.flow_to_image(np.ascontiguousarray(batch[i].transpose(1, 2, 0)))
        assert np.array_equal(alone, golden["rgb_batch"][i])


def test_wheel_equals_the_fixture_and_the_library_holds_the_same(golden):
    assert R.WHEEL.shape == (55, 3) and np.array_equal(R.WHEEL.astype(np.float64), golden["wheel"])
    lib = sstem_native.load_library()
    table = np.ctypeslib.as_array(lib.sstem_flow_color_wheel(), shape=(55, 3))
    assert np.array_equal(table, R.WHEEL)
    assert lib.sstem_flow_color_workspace_bytes(0) == 0 and lib.sstem_flow_color_workspace_bytes(5) == 5 * 512
    assert lib.sstem_flow_color_workspace_bytes(-1) == 0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_on_some_case(golden, flows, mutant):
    caught = []
    if mutant == "batch_max":
        if not np.array_equal(R.flow_color_batch(R.batch_case(), 0, mutant), golden["rgb_batch"]):
            caught.append("batch")
    else:
        for name, flow in flows.items():
            try:
                same = np.array_equal(R.flow_to_image(flow, 0, mutant), golden["rgb_" + name])
            except IndexError:                                               # k1 = 56 has no colour
                same = False
            if not same:
                caught.append(name)
    assert caught, "the fixture does not catch the mutant %r" % mutant


def _ambiguous(flow_hw2):
    lo, hi, _ = R.byte_range(flow_hw2)
    return int((lo != hi).sum()), lo.size, int((hi.astype(np.int64) - lo).max())


@pytest.mark.parametrize("name", CASES + ["batch0", "batch1", "batch2", "batch3"])
def test_few_bytes_depend_on_the_last_bits_of_the_angle(flows, name):
    """A condition on the inputs, not a tolerance: at most 1e-3 of a case's bytes may change anywhere within k steps of the angle, so
    the GPU test, which admits the range over those steps, holds all other bytes bit for bit."""
    if name.startswith("batch"):
        flow = np.ascontiguousarray(R.batch_case()[int(name[5:])].transpose(1, 2, 0))
    else:
        flow = flows[name]
    n, size, spread = _ambiguous(flow)
    print("%s: %d of %d bytes ambiguous within +-%d ulps, largest spread %d" % (name, n, size, R.ATAN2_ULPS, spread))
    assert n <= R.AMBIGUOUS_CAP * size, "%s: %d of %d" % (name, n, size)


def test_a_tiled_image_has_the_bytes_of_its_tile(flows):
    """What lets the GPU tests hold a million pixels to a reference of a few thousand."""
    small = flows["smooth_noise"]
    big, index = R.tiled(small, 150, 161)
    assert big.shape == (150, 161, 2) and index.max() == small.shape[0] * small.shape[1] - 1
    want = R.gather_range(R.byte_range(small), index, 150, 161)
    for got, w in zip(R.byte_range(big), want):
        assert np.array_equal(got, w)
    flow, index, base = R.grid_cap_case(4096 * 256)
    assert flow.shape == (1025, 1025, 2) and np.array_equal(flow.reshape(-1, 2)[:8710], flows[base].reshape(-1, 2))


def test_shift_ulps_moves_by_whole_steps_and_stays_inside_pi():
    x = np.array([-np.pi, -1.0, -0.0, 0.0, 1.0, np.pi])
    up, down = R.shift_ulps(x, 3), R.shift_ulps(x, -3)
    assert up[-1] == np.pi and down[0] == -np.pi and np.all(up >= x) and np.all(down <= x)
    assert up[1] == -1.0 + 3 * 2.0 ** -53 and down[4] == 1.0 - 3 * 2.0 ** -53 and up[4] == 1.0 + 3 * 2.0 ** -52
    assert np.array_equal(R.shift_ulps(x, 0), x)


# ---- the image tail ------------------------------------------------------------------------------------------------------------------
def test_luminance_equals_pil_and_is_the_identity_on_grey(golden):
    triples = golden["triples"]
    assert np.array_equal(triples, R.gray_triples())
    assert np.array_equal(R.luminance(triples), golden["triples_L"])
    assert np.array_equal(R.luminance(triples[:256]), np.arange(256, dtype=np.uint8))


def test_byte_conversion_equals_numpy_where_numpy_is_defined():
    x = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255), np.linspace(-3, 3, 1001, dtype=np.float32),
                        np.array([1.0, 2 / 255, np.nextafter(np.float32(2 / 255), np.float32(0))], dtype=np.float32)])
    v = x * np.float32(255)
    assert np.array_equal(R.to_u8(x), v.astype(np.int64).astype(np.uint8))       # truncation, then the low 8 bits
    assert R.to_u8(np.float32(256 / 255 + 1e-6)) == 0 and R.to_u8(np.float32(-1 / 255 - 1e-6)) == 255 and R.to_u8(np.float32(np.nan)) == 0


def test_stitch_is_the_reference_float_blend():
    rng = np.random.default_rng(3)
    warped = rng.random((2, 3, 9, 11), dtype=np.float32) * np.float32(0.02)      # luminances around the threshold of 2
    interp = rng.integers(0, 256, size=(2, 9, 11), dtype=np.uint8)
    _, rgb, stitch = R.sff_outputs(np.zeros((2, 9, 11), np.float32), warped, interp)
    L = R.luminance(rgb)
    assert (L < 2).any() and (L >= 2).any()
    mask = np.ones_like(L, dtype=np.float32)
    mask[L < 2] = 0
    assert np.array_equal(stitch, (interp * (1 - mask) + L * mask).astype(np.uint8))     # sff_scripts_fusion/inference.py:167-171
