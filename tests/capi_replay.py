"""Calls C-ABI entries with plain integers for pointers, for tests/golden/make_capi_refusals.py (which records the answers) and
tests/test_capi_refusals.py (which replays them in a child process: ``python tests/capi_replay.py FILE``).

Only ctypes is imported, no torch.  Nothing here may run where a device is visible: the pointer values of the rows are not memory.
``main`` asks hipGetDeviceCount first and replays nothing if it sees one (exit status 77)."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))

import sstem_native  # noqa: E402

HOST16 = "host16"     # the one host out-parameter of the C-ABI (sstem_conv3x3_pack_group_entry): sixteen int64 the call may write


def visible_devices():
    """hipGetDeviceCount of the HIP runtime the library itself loaded."""
    sstem_native.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    n = ctypes.c_int(0)
    rc = ctypes.CDLL(path).hipGetDeviceCount(ctypes.byref(n))
    return n.value if rc == 0 else 0


def call(lib, name, args):
    """-> [status, last-error text or None] of an int entry, else [value] (a query), with the sixteen words after a HOST16 call."""
    restype = sstem_native.C_ABI[name][0]
    buf = (ctypes.c_int64 * 16)(*([-1] * 16))
    rv = getattr(lib, name)(*[buf if a == HOST16 else a for a in args])
    if restype is ctypes.c_char_p:
        return [rv.decode()]
    if HOST16 in args:
        return [rv, list(buf)]
    if restype is ctypes.c_int and not name.endswith("_supported") and name not in ("sstem_version", "sstem_wgrad_deferred_count"):
        return [rv, lib.sstem_last_error().decode() if rv != 0 else None]
    return [rv]


def main(path):
    if visible_devices() > 0:
        print("SKIP: a device is visible")
        return 77
    lib = sstem_native.load_library()
    rows = []
    for name, e in json.load(open(path)).items():
        for want, calls in e["answers"]:
            for how in calls:
                if "base" in e:                 # the base call with the named arguments replaced, "pointers": every pointer argument
                    ptr = [t is ctypes.c_void_p and a != "stream" for a, t in zip(e["args"], sstem_native.C_ABI[name][1])]
                    how = [how.get(a, how["pointers"] if p and "pointers" in how else b) for a, b, p in zip(e["args"], e["base"], ptr)]
                rows.append((name, how, want))
    bad = 0
    for name, args, want in rows:
        got = call(lib, name, args)
        reached_hip = len(want) == 2 and not isinstance(want[1], list) and got[0] in (4, 5)
        if got != want or reached_hip:
            bad += 1
            print("MISMATCH %s%r\n  want %r\n  got  %r" % (name, tuple(args), want, got))
    print("replayed %d rows, %d mismatches" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
