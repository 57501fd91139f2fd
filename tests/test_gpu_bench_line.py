"""bench.py's plain run on the GPU: the JSON line holds the contract fields and nothing that takes runs of its own,
--steps is the number of timed steps, and --dump-outputs writes what the last timed forward returned (checked against
the CPU oracle on the same seeded clips)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

FULL_ONLY = ("parity_max_rel", "roofline", "kernels", "eval_e2e", "fp32_exact", "train", "train_wgrad_g11", "train_gan",
             "stress_memory", "cpu_baseline")


def test_plain_run_is_the_headline_and_dumps_the_timed_outputs(tmp_path):
    from ammcnet_aaai2021_amd import synthetic as S
    from oracle import ammc_oracle as O

    dump = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "AMMC_BENCH_SHARE_GPU")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
           "--batch", "2", "--size", "64", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "frames/s" and rec["higher_is_better"] is True and rec["metric"] and rec["dtype"]
    assert abs(rec["value"] - 2 / (rec["ms_per_step"] * 1e-3)) <= 0.02 * rec["value"]
    assert not [k for k in FULL_ONLY if k in rec], rec.keys()

    sd = S.make_twostream_state(n_embed=2000)
    rgb_x, op_x, _, _ = S.make_clips(2, 64, 64, tag="bench0")
    with torch.no_grad():
        rgb, op, (rd, od), (rq, oq) = O.twostream_forward(O.clone_state(sd), rgb_x, op_x, 2)
    want = {"rgb": rgb, "op": op, "rgb_diff": rd, "op_diff": od, "rgb_q": rq, "op_q": oq}
    assert sorted(os.listdir(dump)) == sorted(f"{n}.npy" for n in want)
    for name, w in want.items():
        got = np.load(dump / f"{name}.npy")
        assert got.dtype == np.float32 and got.size == w.numel(), name
        assert np.isfinite(got).all(), name
        if name in ("rgb", "op", "rgb_diff", "op_diff"):
            assert rel_err(got.reshape(tuple(w.shape)), w) <= 1e-4, name
