"""`run_train --bank_host_gb`: the joint stage fed from a two-tier clip bank (half of the set in pinned host memory, the
next iteration's clips prefetched on the bank's stream) trains as the all-device run does, and resumes as it does.  The
dataset recipe and the arguments are those of tests/test_gpu_run_train.py."""
import json
import os

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import run_train

pytestmark = pytest.mark.gpu
N_VIDEOS, N_FRAMES, H, W = 3, 12, 64, 96
TIERS = ("--bank_budget_gb", "0.0005", "--bank_host_gb", "0.01")      # the set is 0.98 MB at 64 x 64: about half fits


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from oracle.pipeline_oracle import write_flo
    root = tmp_path_factory.mktemp("train_set_tiered")
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:H, 0:W]
    for v in range(N_VIDEOS):
        dr, do = root / "rgb" / f"{v + 1:02d}", root / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        for i in range(N_FRAMES):                     # smooth moving pattern + noise: JPEG-like content
            base = 128 + 60 * np.sin((xx + 3 * i + 10 * v) / 9.0)[..., None] * np.cos(yy / 7.0)[..., None]
            img = np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(dr / f"{i:04d}.jpg", quality=90)
        for i in range(N_FRAMES - 1):
            write_flo(str(do / f"{i:04d}.flo"), rng.normal(0, 2, (H, W, 2)).astype(np.float32))
    return str(root / "rgb"), str(root / "op")


def _args(dataset, out, iterations, *extra):
    return ["--rgb_root", dataset[0], "--op_root", dataset[1], "--out", str(out), "--size", "64", "--batch", "4",
            "--iterations", str(iterations), "--save_every", "2", "--log_every", "1", "--flownet", "synthetic",
            "--workers", "4", *extra]


def _log(out):
    with open(os.path.join(out, "train_log.jsonl")) as fp:
        return [json.loads(ln) for ln in fp]


def _state(out, name):
    return {"G." + k: v for k, v in torch.load(os.path.join(out, "generator", name), map_location="cpu").items()} | \
           {"D." + k: v for k, v in torch.load(os.path.join(out, "discriminator", name), map_location="cpu").items()}


@pytest.fixture(scope="module")
def runs(dataset, tmp_path_factory):
    """device: all-device, 4 steps; tiered: two tiers, 4 steps; resumed: two tiers, 2 + 2 with --resume"""
    base = tmp_path_factory.mktemp("runs_tiered")
    out = {k: base / k for k in ("device", "tiered", "resumed")}
    run_train.main(_args(dataset, out["device"], 4))
    run_train.main(_args(dataset, out["tiered"], 4, *TIERS))
    run_train.main(_args(dataset, out["resumed"], 2, *TIERS))
    run_train.main(_args(dataset, out["resumed"], 4, *TIERS, "--resume"))
    return {k: str(v) for k, v in out.items()}


def test_start_record_shows_both_tiers_and_the_prefetch(runs):
    head = _log(runs["tiered"])[0]
    assert head["event"] == "start" and head["prefetch"] is True
    assert head["bank_device_GB"] > 0 and head["bank_host_GB"] > 0
    assert head["bank_device_GB"] <= 0.0005
    assert abs(head["bank_device_GB"] + head["bank_host_GB"] - 983040 / 1e9) < 2e-6       # 36 frames + 33 flows at 64 x 64
    heads = [r for r in _log(runs["resumed"]) if r.get("event") == "start"]
    assert len(heads) == 2 and all(h["prefetch"] is True and h["bank_host_GB"] > 0 for h in heads) and heads[1]["resumed"] is True
    dev = _log(runs["device"])[0]
    assert dev["prefetch"] is False and dev["bank_host_GB"] == 0 and dev["bank_device_GB"] > 0


def test_every_step_is_logged_with_finite_figures(runs):
    for k in ("tiered", "resumed"):
        log = _log(runs[k])
        steps = [r for r in log if "step" in r]
        assert [r["step"] for r in steps] == [1, 2, 3, 4], k
        assert log[-1]["event"] == "done" and log[-1]["skipped"] == 0
        for r in steps:
            for name in ("g_loss", "d_loss", "psnr_rgb", "psnr_op", "ms_per_iter", "data_host_ms_per_iter"):
                assert np.isfinite(r[name]), (k, name, r)


def test_tiered_and_resumed_runs_train_on_the_clips_of_the_all_device_run(runs):
    """the gathers are bit-identical and the sampler stream is consumed in the same order, so the first two iterations
    agree as closely as two identical runs do (rtol 1e-5, the criterion of
    tests/test_gpu_run_train.py::test_resume_ends_where_the_uninterrupted_run_ends: identical runs are not bitwise equal
    here); a wrong clip moves a loss by orders of magnitude more"""
    losses = {k: [(r["g_loss"], r["d_loss"]) for r in _log(runs[k]) if "step" in r] for k in runs}
    for k, v in losses.items():
        print(k, v)
    for k in ("tiered", "resumed"):
        assert np.allclose(losses[k][:2], losses["device"][:2], rtol=1e-5, atol=0), k
    assert np.allclose(losses["resumed"][:2], losses["tiered"][:2], rtol=1e-5, atol=0)
    final = {k: _state(runs[k], "step_000005.pth") for k in runs}
    ints = [k for k, v in final["device"].items() if not v.is_floating_point()]
    assert ints
    for name in ints:                                  # num_batches_tracked: the step count went on, resume included
        assert torch.equal(final["device"][name], final["tiered"][name]), name
        assert torch.equal(final["device"][name], final["resumed"][name]), name
