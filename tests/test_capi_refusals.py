"""The C-ABI's refusals, pinned: tests/golden/capi_refusals.json holds what the library answered, at the commit before its entry
points were folded into shared bodies, to calls it refuses (status and the text of sstem_last_error(), one row per message and per
pair of checks violated together, values either side of every limit), to empty shapes and to its size / ``_supported`` queries.
A build must answer every row the same (tests/golden/make_capi_refusals.py wrote the file; it is not regenerated for a refactor).

The rows carry small integers where tensors go, so they are replayed in a child process that sees no device
(HIP_VISIBLE_DEVICES=-1): a call that wrongly passed validation ends as status 4 there, which fails the test, and launches nothing.
The child asks hipGetDeviceCount first and replays nothing if a device is visible after all."""
import os
import subprocess
import sys

import pytest


def test_recorded_refusals_replay(repo_root, golden_dir):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, os.path.join(repo_root, "tests", "capi_replay.py"), os.path.join(golden_dir, "capi_refusals.json")],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode == 77:
        pytest.skip("the child process sees a device despite HIP_VISIBLE_DEVICES=-1: nothing replayed")
    assert p.returncode == 0, p.stdout[-4000:]
    assert "replayed" in p.stdout and " 0 mismatches" in p.stdout, p.stdout[-4000:]
