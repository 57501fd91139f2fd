"""Generate tests/golden/flow_colour.npz from the REFERENCE itself.

Runs only in the authoring container (it needs the reference's sources, found where make_golden.py finds them).  It
imports the reference's `utils/flowlib.py` by path - with an empty stand-in `png` module in `sys.modules` first: flowlib
imports one for its KITTI readers, which nothing here calls, and none is installed - and records `flow_to_image` of the
seven 32 x 48 flows of tests/render_cases.py together with the inputs.  Data only: nothing of the reference's source is
stored.

    python tests/golden/make_render_golden.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import REF  # noqa: E402
import render_cases as K  # noqa: E402


def load_ref_flowlib():
    sys.modules.setdefault("png", types.ModuleType("png"))
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("ref_flowlib", f"{REF}/utils/flowlib.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_ref_flowlib()
    out = {"cases": np.array(K.GOLDEN_CASES)}
    for name, flow in K.golden_flows().items():
        out[f"{name}_flow"] = flow
        # float64 of the fp32 values: the reference's arithmetic at full precision (it zeroes the unknown pixels of its
        # argument in place, hence a copy)
        img = ref.flow_to_image(flow.astype(np.float64))
        assert img.dtype == np.uint8 and img.shape == flow.shape[:2] + (3,)
        out[f"{name}_image"] = img
        print(name, flow.shape, "mean colour", img.reshape(-1, 3).mean(axis=0).round(2))
    np.savez_compressed(os.path.join(HERE, "flow_colour.npz"), **out)


if __name__ == "__main__":
    main()
