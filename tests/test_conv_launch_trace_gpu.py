"""The launches hipnn.functional issues, route by route, against tests/golden/conv_launch_trace.json.

The golden was written by tests/golden/make_conv_launch_trace.py at the commit BEFORE the autograd layer of hipnn/functional.py
was taken apart (one gradient-delivery helper, _raw_conv as plan / workspace / launch): that change had to leave every launch where it
was -- same entry point, same integer and float arguments, same pointers given or left out, same stream, same order.  The file is
regenerated only where a route changes on purpose, never by a refactor of the Python layer.  Every case of the generator is compared,
and every logged argument of every launch."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_conv_launch_trace as gen  # noqa: E402

CASES = sorted(gen._cases())


@pytest.fixture(scope="module")
def traces(golden_dir):
    with open(os.path.join(golden_dir, "conv_launch_trace.json")) as f:
        want = json.load(f)
    return gen.generate(), want


def test_the_golden_holds_exactly_the_generators_cases(traces):
    got, want = traces
    assert sorted(got) == sorted(want) == CASES


@pytest.mark.parametrize("case", CASES)
def test_launch_trace_equals_the_pinned_one(case, traces):
    got, want = traces
    assert len(got[case]) > 0
    for i, (g, w) in enumerate(zip(got[case], want[case])):
        assert g == w, "%s, launch %d" % (case, i)
    assert len(got[case]) == len(want[case]), [r[0] for r in got[case]]
