"""Deterministic training (`model.deterministic`, `run_train --deterministic`) at the 64 x 64 batch-2 fixtures' sizes:
with the switch on, equal runs end in equal BITS - every parameter, every buffer (BatchNorm statistics, step counters,
the EMA codebook), the gradients of the last step and the Adam state - for the generator step (`train_step`, three
iterations), the adversarial iteration (`train_step_gan`, two) and a single-stream stage (`train_step_single_gan`), with
the concurrency switches on and off (AMMC_TWO_STREAMS, AMMC_GAN_OVERLAP: same kernels on other HIP streams), under both
training precisions ("fp32" sends every layer through the fp32 form), and `run_train --deterministic` for 4 iterations
ends where 2 iterations + `--resume` for 2 more end.

With the switch on the gradients are those of the switch off within the run-to-run noise of the atomics - the gate of
tests/test_gpu_lanes.py (an expression there, not a name: 4 x the difference of two equal atomics runs + 1e-7 of the
tensor's magnitude), written out once in `_within_atomics_noise`.

Two equal runs do not prove determinism; the proof is in the code (no atomic, a fixed-order sum: DESIGN.md,
"Deterministic training").  These tests keep a later change from taking it away unnoticed."""
import json
import os

import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, run_train, synthetic as S, train as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW, BATCH = 64, 2
PRECISIONS = ["s16", "fp32"]


def _clips(tag):
    rgb_x, op_x, rgb_t, op_t = S.make_clips(BATCH, HW, HW, tag=tag)
    rgb = torch.cat([rgb_x.view(BATCH, 4, 3, HW, HW), rgb_t[:, None]], 1).to(DEV)
    op = torch.cat([op_x.view(BATCH, 3, 2, HW, HW), op_t[:, None]], 1).to(DEV)
    return rgb, op


def _generator(case, precision, det):
    if case == "joint":
        G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
        G.load_state_dict(S.make_twostream_state())
    else:
        G = A.get_unet_vq_topk_res(12, 3, 64, 256, 2)
        G.load_state_dict({k[4:]: v for k, v in S.make_twostream_state().items() if k.startswith("rgb.")})
    G = G.to(DEV).train()
    G.train_precision, G.deterministic = precision, det
    return G


def _discriminator(precision, det):
    D = A.PixelDiscriminator(3, [128, 256, 512, 512])
    D.load_state_dict(S.make_discriminator_state())
    D = D.to(DEV).train()
    D.precision, D.deterministic = precision, det
    return D


def _flow_fn(precision):
    F2 = A.FlowNet2SD()
    F2.load_state_dict(S.make_flownet2sd_state())
    F2 = F2.to(DEV).eval()
    F2.precision = precision
    return Hn.flownet_flow_fn(F2)


def _snapshot(**nets):
    """{name: cpu tensor} of everything a run leaves behind: state_dict (parameters and buffers), the gradients of the
    last step, the optimiser state"""
    torch.cuda.synchronize()
    out = {}
    for tag, (net, opt) in nets.items():
        for k, v in net.state_dict().items():
            out[f"{tag}.state.{k}"] = v.detach().cpu().clone()
        names = {p: n for n, p in net.named_parameters()}
        for p, n in names.items():
            assert p.grad is not None, n
            out[f"{tag}.grad.{n}"] = p.grad.detach().cpu().clone()
        for p, st in opt.state.items():
            for k, v in st.items():
                out[f"{tag}.adam.{names[p]}.{k}"] = torch.as_tensor(v).detach().cpu().clone()
    return out


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    worst = [(k, float((a[k].double() - b[k].double()).abs().max())) for k in bad[:6]]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, e.g. {worst}"
    assert all(bool(torch.isfinite(v.double()).all()) for v in a.values()), what


def _train_steps(precision, two_streams, monkeypatch, steps=3):
    monkeypatch.setattr(T, "TWO_STREAMS", two_streams)
    G = _generator("joint", precision, True)
    opt = Hn.adam(G.parameters(), lr=2e-4)
    rgb, op = _clips("det-train")
    losses = [Hn.train_step(G, opt, rgb, op).cpu() for _ in range(steps)]
    side = G._train_engine._last["ops"].side is not None
    assert G._train_engine._last["ops"].deterministic is True
    return _snapshot(G=(G, opt)) | {f"loss.{i}": v for i, v in enumerate(losses)}, side


@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_generator_steps_twice_and_on_one_stream(precision, monkeypatch):
    a, side_a = _train_steps(precision, True, monkeypatch)
    b, _ = _train_steps(precision, True, monkeypatch)
    c, side_c = _train_steps(precision, False, monkeypatch)
    assert side_a and not side_c                                     # the switch did switch
    assert any(k.startswith("G.adam.") and k.endswith("exp_avg_sq") for k in a)
    _assert_same_bits(a, b, "two equal runs")
    _assert_same_bits(a, c, "AMMC_TWO_STREAMS=1 against 0")


def _gan_steps(case, precision, overlap, det, monkeypatch, steps=2, lr=True):
    monkeypatch.setattr(Hn, "GAN_OVERLAP", overlap)
    G, D, flow_fn = _generator(case, precision, det), _discriminator(precision, det), _flow_fn(precision)
    if lr:
        opt_g, opt_d = Hn.adam(G.parameters(), lr=2e-4), Hn.adam(D.parameters(), lr=2e-5)
    else:                                                            # (lr 0: both steps run, one iteration's gradients stay comparable)
        opt_g, opt_d = torch.optim.SGD(G.parameters(), lr=0.0), torch.optim.SGD(D.parameters(), lr=0.0)
    rgb, op = _clips(f"det-gan-{case}")
    losses = {}
    for i in range(steps):
        if case == "joint":
            gl, dl = Hn.train_step_gan(G, D, opt_g, opt_d, rgb, op, flow_fn)
        else:
            gl, dl = Hn.train_step_single_gan(G, D, opt_g, opt_d, rgb, flow_fn)
        losses[f"g_loss.{i}"], losses[f"d_loss.{i}"] = gl.detach().cpu().clone(), dl.detach().cpu().clone()
    return _snapshot(G=(G, opt_g), D=(D, opt_d)) | losses


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_adversarial_iterations_twice_and_without_the_d_lane(precision, monkeypatch):
    a = _gan_steps("joint", precision, True, True, monkeypatch)
    b = _gan_steps("joint", precision, True, True, monkeypatch)
    c = _gan_steps("joint", precision, False, True, monkeypatch)
    assert any(k.startswith("D.adam.") for k in a) and any(k.startswith("D.grad.") for k in a)
    _assert_same_bits(a, b, "two equal runs")
    _assert_same_bits(a, c, "AMMC_GAN_OVERLAP=1 against 0")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_single_stream_stage_twice_and_without_the_d_lane(precision, monkeypatch):
    a = _gan_steps("rgb", precision, True, True, monkeypatch)
    b = _gan_steps("rgb", precision, True, True, monkeypatch)
    c = _gan_steps("rgb", precision, False, True, monkeypatch)
    _assert_same_bits(a, b, "two equal runs")
    _assert_same_bits(a, c, "AMMC_GAN_OVERLAP=1 against 0")


def _within_atomics_noise(got, ref, ref2) -> bool:
    """the gate of tests/test_gpu_lanes.py for gradients that end in fp32 atomics: `ref`, `ref2` = two equal atomics runs"""
    noise = float((ref - ref2).abs().max())
    return float((got - ref).abs().max()) <= max(4.0 * noise, 0.0) + 1e-7 * float(ref.abs().max())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gradients_with_the_switch_on_are_those_with_it_off_within_the_atomics_noise(precision, monkeypatch):
    on = _gan_steps("joint", precision, True, True, monkeypatch, steps=1, lr=False)
    off = _gan_steps("joint", precision, True, False, monkeypatch, steps=1, lr=False)
    off2 = _gan_steps("joint", precision, True, False, monkeypatch, steps=1, lr=False)
    grads = [k for k in off if ".grad." in k]
    assert len(grads) > 100
    for k in off:
        if ".grad." not in k:                                        # the forward, the losses, the buffers: the same kernels
            assert torch.equal(on[k], off[k]), k
    moved = [k for k in grads if not torch.equal(on[k], off[k])]
    worst = max((float((on[k] - off[k]).abs().max() / off[k].abs().max().clamp_min(1e-30)), k) for k in grads)
    print(f"{precision}: {len(moved)} of {len(grads)} gradients differ between deterministic and atomics, worst {worst[0]:.3e} ({worst[1]})")
    bad = [k for k in grads if not _within_atomics_noise(on[k], off[k], off2[k])]
    assert not bad, bad


# ---- run_train ---------------------------------------------------------------------------------------------------------------------
N_VIDEOS, N_FRAMES, H, W = 3, 12, 64, 96


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from oracle.pipeline_oracle import write_flo
    root = tmp_path_factory.mktemp("det_train_set")
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:H, 0:W]
    for v in range(N_VIDEOS):
        dr, do = root / "rgb" / f"{v + 1:02d}", root / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        for i in range(N_FRAMES):
            base = 128 + 60 * np.sin((xx + 3 * i + 10 * v) / 9.0)[..., None] * np.cos(yy / 7.0)[..., None]
            img = np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(dr / f"{i:04d}.jpg", quality=90)
        for i in range(N_FRAMES - 1):
            write_flo(str(do / f"{i:04d}.flo"), rng.normal(0, 2, (H, W, 2)).astype(np.float32))
    return str(root / "rgb"), str(root / "op")


def _args(dataset, out, iterations, *extra):
    return ["--rgb_root", dataset[0], "--op_root", dataset[1], "--out", str(out), "--size", "64", "--batch", "4",
            "--iterations", str(iterations), "--save_every", "2", "--log_every", "1", "--flownet", "synthetic",
            "--workers", "4", "--deterministic", *extra]


def _flat(obj, prefix=""):
    """a nested train state -> {path: leaf}"""
    if isinstance(obj, dict):
        out = {}
        for k, v in obj.items():
            out.update(_flat(v, f"{prefix}/{k}"))
        return out
    if isinstance(obj, (list, tuple)):
        out = {}
        for i, v in enumerate(obj):
            out.update(_flat(v, f"{prefix}/{i}"))
        return out
    return {prefix: obj}


def test_run_train_four_iterations_equal_two_plus_resume(dataset, tmp_path):
    full, parts = tmp_path / "full", tmp_path / "parts"
    run_train.main(_args(dataset, full, 4))
    run_train.main(_args(dataset, parts, 2))
    run_train.main(_args(dataset, parts, 4, "--resume"))
    name = "step_000005.pth"                                        # (`saver` of the reference: step + 1)
    for net in ("generator", "discriminator"):
        a = torch.load(os.path.join(full, net, name), map_location="cpu")
        b = torch.load(os.path.join(parts, net, name), map_location="cpu")
        assert sorted(a) == sorted(b)
        bad = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad, (net, len(bad), bad[:6])
    sa = torch.load(os.path.join(full, "train_state", name), map_location="cpu", weights_only=True)
    sb = torch.load(os.path.join(parts, "train_state", name), map_location="cpu", weights_only=True)
    assert sa["deterministic"] is True and sb["deterministic"] is True
    # `args` is the command line (iterations, --resume): it differs by construction; everything else is the run itself
    fa, fb = _flat({k: v for k, v in sa.items() if k != "args"}), _flat({k: v for k, v in sb.items() if k != "args"})
    assert sorted(fa) == sorted(fb)
    for k in fa:
        x, y = fa[k], fb[k]
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y), k
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), k
        else:
            assert x == y, (k, x, y)
    with open(os.path.join(parts, "train_log.jsonl")) as fp:
        log = [json.loads(ln) for ln in fp]
    heads = [r for r in log if r.get("event") == "start"]
    assert len(heads) == 2 and all(h["deterministic"] is True for h in heads) and heads[1]["resumed"] is True
    # the logged losses of iterations 3 and 4 are those of the uninterrupted run, digit for digit
    with open(os.path.join(full, "train_log.jsonl")) as fp:
        ref = {r["step"]: r for r in map(json.loads, fp) if "step" in r}
    for r in log:
        if "step" in r:
            assert (r["g_loss"], r["d_loss"]) == (ref[r["step"]]["g_loss"], ref[r["step"]]["d_loss"]), r["step"]
    # a run that was started deterministic is not resumed without the flag
    args = [a for a in _args(dataset, parts, 6, "--resume") if a != "--deterministic"]
    if not T.DETERMINISTIC:
        with pytest.raises(SystemExit, match="with --deterministic"):
            run_train.main(args)
