"""`python -m ammcnet_aaai2021_amd.run_train` end to end on a tiny JPEG + .flo set: checkpoints under the reference's
names that load strictly into the reference's models, a finite log, a first iteration equal to `train_step_gan` on the
same clips built by the evaluation pipeline, a 2 + 2 resume that ends where a 4-step run ends, and `run_test` reading
the trained generator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, pipeline as P, run_train
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_VIDEOS, N_FRAMES, H, W = 3, 12, 64, 96


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from oracle.pipeline_oracle import write_flo
    root = tmp_path_factory.mktemp("train_set")
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
    base = tmp_path_factory.mktemp("runs")
    out = {k: base / k for k in ("a", "b", "c")}
    run_train.main(_args(dataset, out["a"], 4))
    run_train.main(_args(dataset, out["b"], 4))
    run_train.main(_args(dataset, out["c"], 2))
    run_train.main(_args(dataset, out["c"], 4, "--resume"))
    return {k: str(v) for k, v in out.items()}


def test_checkpoints_carry_the_reference_names_and_load_strictly(runs):
    out = runs["a"]
    for sub in ("generator", "discriminator", "train_state"):
        assert sorted(os.listdir(os.path.join(out, sub))) == ["step_000003.pth", "step_000005.pth"], sub
    G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    G.load_state_dict(torch.load(os.path.join(out, "generator", "step_000005.pth"), map_location="cpu"), strict=True)
    D = A.PixelDiscriminator(3, [128, 256, 512, 512])
    D.load_state_dict(torch.load(os.path.join(out, "discriminator", "step_000005.pth"), map_location="cpu"), strict=True)
    st = torch.load(os.path.join(out, "train_state", "step_000005.pth"), map_location="cpu", weights_only=True)
    assert st["g_step"] == 4 and st["args"]["batch"] == 4 and set(st["sampler"]) >= {"keys", "pos"}


def test_log_lines_parse_and_losses_are_finite(runs):
    log = _log(runs["a"])
    head, steps, done = log[0], [r for r in log if "step" in r], log[-1]
    assert head["event"] == "start" and head["flow_term"].startswith("on") and head["sub_videos"] == N_VIDEOS
    assert head["rgb_frames"] == N_VIDEOS * N_FRAMES and head["op_frames"] == N_VIDEOS * (N_FRAMES - 1)
    assert [r["step"] for r in steps] == [1, 2, 3, 4] and done["event"] == "done" and done["skipped"] == 0
    for r in steps:
        for k in ("g_loss", "d_loss", "psnr_rgb", "psnr_op", "ms_per_iter", "data_host_ms_per_iter"):
            assert np.isfinite(r[k]), (k, r)
        assert r["lr_g"] == 2e-4 and r["lr_d"] == 2e-5 and r["skipped"] == 0


def test_first_iteration_equals_train_step_gan_on_pipeline_clips(dataset, runs, tmp_path):
    """the same draw, the same initial models; clips built by frames_to_device / flows_to_device instead of the bank"""
    a = run_train.parse(_args(dataset, tmp_path, 1))
    vids = P.list_subvideos(*dataset)
    sampler = P.ClipSampler([len(f) for f, _ in vids], [len(o) for _, o in vids], seed=a.seed)
    rv, rs, ov, os_ = sampler.draw(a.batch)
    rgb, op = [], []
    for i in range(a.batch):
        fr = np.stack([P.read_image(p) for p in vids[rv[i]][0][rs[i]:rs[i] + 5]])
        fl = np.stack([P.read_flo(p) for p in vids[ov[i]][1][os_[i]:os_[i] + 4]])
        rgb.append(P.frames_to_device(torch.from_numpy(fr).to(DEV), (64, 64)))
        op.append(P.flows_to_device(torch.from_numpy(fl).to(DEV), (64, 64)))
    G, D, F2 = run_train.build_models(a)
    G, D, flow_fn = run_train.to_device(G, D, F2, a, torch.device(DEV))
    opt_g, opt_d = Hn.adam(G.parameters(), lr=a.lr_g), Hn.adam(D.parameters(), lr=a.lr_d)
    gl, dl = Hn.train_step_gan(G, D, opt_g, opt_d, torch.stack(rgb), torch.stack(op), flow_fn, **run_train.lams_of(a))
    first = [r for r in _log(runs["a"]) if r.get("step") == 1][0]
    print("first iteration: run_train", first["g_loss"], first["d_loss"], "direct", float(gl), float(dl))
    assert abs(first["g_loss"] - float(gl)) <= 1e-5 * abs(float(gl))
    assert abs(first["d_loss"] - float(dl)) <= 1e-5 * abs(float(dl))


def test_resume_ends_where_the_uninterrupted_run_ends(runs):
    """Measured (MI355X): two identical 4-step runs are NOT bitwise equal - the split-fp16 training kernels reduce in a
    free order, and from the from-scratch init Adam turns the resulting last-bit noise of near-zero gradients (the
    BatchNorm shifts, early on) into whole +-lr steps, so single tensors of two identical runs differ by up to ~1e-1 of
    their (still tiny) magnitude.  What a resume must keep is what decides the trajectory: the clips of every iteration
    (sampler state), the weights and buffers, the Adam moments and the schedule.  So: the losses of iterations 3 and 4
    after a 2 + 2 resume equal the uninterrupted run's as closely as two identical runs agree (a wrong clip or lost
    moments moves them by orders of magnitude more), and every parameter lies within the lr-sized envelope those noise
    steps can open (a re-initialised or stale tensor does not)."""
    a, b, c = (_state(runs[k], "step_000005.pth") for k in "abc")
    la, lb, lc = ([(r["g_loss"], r["d_loss"]) for r in _log(runs[k]) if "step" in r] for k in "abc")
    assert len(la) == len(lb) == len(lc) == 4
    assert lc[:2] == la[:2] or np.allclose(lc[:2], la[:2], rtol=1e-5, atol=0)
    loss_ab = max(abs(x - y) / abs(x) for ra, rb in zip(la, lb) for x, y in zip(ra, rb))
    loss_ac = max(abs(x - y) / abs(x) for ra, rc in zip(la, lc) for x, y in zip(ra, rc))
    float_keys = [k for k in a if a[k].is_floating_point()]

    def spread(x, y):                         # absolute, in units of each network's learning rate
        return max(float((x[k].double() - y[k].double()).abs().max()) / (2e-4 if k[0] == "G" else 2e-5) for k in float_keys)
    ab, ac = spread(a, b), spread(a, c)
    print(f"identical 4-step runs: losses {loss_ab:.2e} apart, parameters {ab:.3f} lr apart; 2 + 2 resumed vs 4: losses "
          f"{loss_ac:.2e}, parameters {ac:.3f} lr")
    assert loss_ac <= max(4 * loss_ab, 1e-5)
    assert ac <= max(4 * ab, 24.0)            # a few +-lr noise steps per iteration, in both runs
    for k in a:
        if not a[k].is_floating_point():
            assert torch.equal(a[k], c[k]), k             # num_batches_tracked: the step count went on
    log_c = [r for r in _log(runs["c"]) if "step" in r]
    assert [r["step"] for r in log_c] == [1, 2, 3, 4]
    assert [r for r in _log(runs["c"]) if r.get("event") == "start"][1]["resumed"] is True


def test_run_test_scores_with_the_trained_generator(dataset, runs):
    ckpt = os.path.join(runs["a"], "generator", "step_000005.pth")
    r = subprocess.run([sys.executable, "-m", "ammcnet_aaai2021_amd.run_test", "--ckpt", ckpt, "--rgb_root", dataset[0],
                        "--op_root", dataset[1], "--size", "64"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["fps"] > 0 and line["videos"] == N_VIDEOS
