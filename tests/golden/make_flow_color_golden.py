"""Generates tests/golden/flow_color.npz from the REFERENCE's utils/flow_display.py (sff_scripts_fusion), imported in place from the
reference tree with matplotlib's Agg backend (nothing is copied), and from PIL, on the CPU.  Recorded with NumPy 2.2.6 and Pillow
12.2.0; ``numpy_version`` and ``pil_version`` in the file say which.  Under NumPy 1.x the reference would run its second half in
float32 and the file would differ: the contract is the NumPy 2 path (include/sstem_display.h, deviation 2).

The file holds, for the cases of tests/flow_color_ref.py:
  ``flow_<case>`` float32 [H,W,2] and ``rgb_<case>`` uint8 [H,W,3]: the reference's own dense_flow on a COPY of the flow (it zeroes
      unknown pixels in its argument);
  ``flow_batch`` float32 [4,2,H,W] and ``rgb_batch`` uint8 [4,H,W,3]: dense_flow per image of the permuted batch;
  ``wheel`` float64 [55,3]: make_color_wheel();
  ``triples`` uint8 [n,3] and ``triples_L`` uint8 [n]: Image.fromarray(triples[None]).convert('L').

    python tests/golden/make_flow_color_golden.py [out.npz]
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import flow_color_ref as R  # noqa: E402

REFERENCE = os.environ.get("SSTEM_REFERENCE", "/root/reference")
FLOW_DISPLAY = os.path.join(REFERENCE, "sff_scripts_fusion", "utils", "flow_display.py")


def reference_available():
    return os.path.exists(FLOW_DISPLAY)


def _reference_module():
    import matplotlib
    matplotlib.use("Agg")                       # the reference imports pyplot at its top; nothing is drawn
    spec = importlib.util.spec_from_file_location("reference_flow_display", FLOW_DISPLAY)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def generate():
    import PIL
    from PIL import Image
    ref = _reference_module()
    out = {"numpy_version": np.array(np.__version__), "pil_version": np.array(PIL.__version__)}
    with np.errstate(all="ignore"):
        for name, flow in R.cases().items():
            out["flow_" + name] = flow
            rgb = ref.dense_flow(flow.copy())
            assert rgb.dtype == np.uint8 and rgb.shape == flow.shape[:2] + (3,)
            out["rgb_" + name] = rgb
        batch = R.batch_case()
        out["flow_batch"] = batch
        out["rgb_batch"] = np.stack([ref.dense_flow(np.ascontiguousarray(np.transpose(im, (1, 2, 0)))) for im in batch])
    out["wheel"] = ref.make_color_wheel()
    triples = R.gray_triples()
    out["triples"] = triples
    out["triples_L"] = np.asarray(Image.fromarray(triples[None]).convert("L"))[0].copy()
    assert out["triples_L"].shape == (len(triples),)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "flow_color.npz")
    data = generate()
    np.savez_compressed(path, **data)
    print("arrays:", len(data), "NumPy", data["numpy_version"], "PIL", data["pil_version"])
    print("wrote", path, os.path.getsize(path), "bytes")
