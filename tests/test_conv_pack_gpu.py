"""The packed 3x3 weight layouts, pinned bit for bit: tests/golden/conv_pack_digests.json holds the SHA-256 of what
sstem_conv3x3_pack_weights_f32 wrote, per algorithm id and layer shape, at the commit before the pack kernels were folded into
csrc/conv_pack.h (tests/golden/make_conv_pack_golden.py wrote the file; it is not regenerated for a refactor).  Exact equality: a pack
kernel only rounds and moves weights, there is no sum whose order could differ."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def maker(golden_dir):
    spec = importlib.util.spec_from_file_location("make_conv_pack_golden", os.path.join(golden_dir, "make_conv_pack_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def packed(maker):
    return maker.generate()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "conv_pack_digests.json")) as f:
        return json.load(f)


def test_the_golden_covers_every_id_shape_and_call(maker, golden):
    want = {"%s/%dx%d/%s/%s" % (a, ci, co, call, side) for a in maker.ALGOS for ci, co in maker.cases()
            for call, sides in (("both", ("forward", "transposed")), ("forward", ("forward",)), ("transposed", ("transposed",)))
            for side in sides}
    assert len(maker.cases()) == 12 and len(maker.ALGOS) == 5
    assert set(golden) == want


def test_packed_bits_equal_the_golden(packed, golden):
    assert set(packed) == set(golden)
    wrong = [k for k in sorted(golden) if packed[k] != golden[k]]
    assert not wrong, "packed bits differ from the golden: %s" % wrong


def test_one_destination_alone_gives_the_same_bits_as_both(packed):
    for key, digest in packed.items():
        head, call, side = key.rsplit("/", 2)
        if call != "both":
            assert call == side
            assert digest == packed["%s/both/%s" % (head, side)], key
