"""Generate tests/golden/ssim_reference.npz from the REFERENCE itself.

Runs only in the authoring container (it needs the reference's sources, found where make_golden.py finds them).  It
imports the reference's `utils/pytorch_ssim.py` by path, as make_golden.py imports `unet.py`, runs its
`ssim(pred, target, size_average=False)` and the `mse_error` of `utils/utils.py:110-111` (one line, restated here: that
module does not import without cv2) per sample on the four seeded recipes of tests/ssim_cases.py, each at one small
shape, and stores the recipes' parameters and the recorded numbers.  Nothing of the reference's source is stored.

    python tests/golden/make_ssim_golden.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import REF  # noqa: E402
import ssim_cases as K  # noqa: E402


def load_ref_ssim():
    spec = importlib.util.spec_from_file_location("ref_pytorch_ssim", f"{REF}/utils/pytorch_ssim.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_ref_ssim()
    mse = torch.nn.MSELoss()
    out = {"recipes": np.array([c[0] for c in K.FIXTURE_CASES]), "seeds": np.array([c[1] for c in K.FIXTURE_CASES], dtype=np.int64),
           "shapes": np.array([c[2] for c in K.FIXTURE_CASES], dtype=np.int64)}
    for recipe, seed, shape in K.FIXTURE_CASES:
        pred, target = K.inputs(recipe, seed, shape)
        with torch.no_grad():
            out[f"{recipe}_ssim"] = ref.ssim(pred, target, size_average=False).numpy()
            # the reference's loop calls its scoring function on a batch of one: per sample
            out[f"{recipe}_mse"] = np.array([float(mse(target[i:i + 1], pred[i:i + 1]) * 16 * 16) for i in range(shape[0])],
                                            dtype=np.float32)
        # a checksum of the inputs: the recipe must still produce the tensors the numbers were recorded on
        out[f"{recipe}_input_sum"] = np.array([pred.double().sum().item(), target.double().sum().item()])
        print(recipe, shape, "ssim", out[f"{recipe}_ssim"], "mse", out[f"{recipe}_mse"])
    np.savez(os.path.join(HERE, "ssim_reference.npz"), **out)


if __name__ == "__main__":
    main()
