"""Host side of stage-1 training (`run_train --stage rgb|op`): the argument rules of each stage, the single-stream draw
rule (`pipeline.SingleClipSampler`) against a literal transcription of the reference's, the one-kind bank's listing and
budget, the single-stream losses, and the models each stage builds - whose two generator checkpoints must fill every
`rgb.*` / `op.*` key of the joint model through `load_pretrained_branches`.  The four training steps of `harness` run to
completion here as well, on toy CPU modules (the D lane is off on the CPU by construction): the schedule the two
adversarial steps share and the G-only tail of the other two, against plain autograd."""
import copy

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, harness, pipeline as P, run_train
from ammcnet_aaai2021_amd.unet import get_twostream, get_unet_vq_topk_res


def _parse(*argv):
    return run_train.parse(["--out", "o", "--iterations", "3", *argv])


def test_stage_argument_rules():
    a = _parse("--rgb_root", "r", "--op_root", "f")
    assert a.stage == "joint" and a.lam_adv_op == 0.0
    assert _parse("--stage", "rgb", "--rgb_root", "r").op_root is None
    assert _parse("--stage", "op", "--op_root", "f", "--lam_adv_op", "0.05").lam_adv_op == 0.05
    assert _parse("--stage", "rgb", "--rgb_root", "r", "--flownet", "synthetic").flownet == "synthetic"
    for bad in (["--rgb_root", "r"],                                       # joint needs both roots
                ["--op_root", "f"],
                ["--stage", "rgb"], ["--stage", "op"],
                ["--stage", "rgb", "--rgb_root", "r", "--op_root", "f"],   # a single stage reads one root only
                ["--stage", "op", "--op_root", "f", "--rgb_root", "r"],
                ["--stage", "rgb", "--rgb_root", "r", "--pretrain_rgb", "a", "--pretrain_op", "b"],
                ["--stage", "op", "--op_root", "f", "--pretrain_rgb", "a", "--pretrain_op", "b"],
                ["--stage", "rgb", "--rgb_root", "r", "--lam_adv_op", "0.1"],
                ["--rgb_root", "r", "--op_root", "f", "--lam_adv_op", "0.1"],
                ["--stage", "op", "--op_root", "f", "--lam_adv_op", "-1"],
                ["--stage", "op", "--op_root", "f", "--flownet", "synthetic"],
                ["--stage", "both", "--rgb_root", "r"]):
        with pytest.raises(SystemExit):
            _parse(*bad)


def test_stage_loss_weights():
    a = _parse("--stage", "rgb", "--rgb_root", "r", "--lam_gdl", "0.5")
    assert run_train.lams_of(a) == dict(lam_adv=0.05, lam_gdl=0.5, lam_flow=2.0, lam_lp=1.0, lam_latent=1.0)
    a = _parse("--stage", "op", "--op_root", "f", "--lam_adv_op", "0.2")
    assert run_train.lams_of(a) == dict(lam_lp_op=1.0, lam_adv_op=0.2, lam_latent=1.0)
    a = _parse("--rgb_root", "r", "--op_root", "f")
    assert run_train.lams_of(a) == harness.LAMS_ANOPRED


def reference_single_draws(lens, clip_len, batch, seed=2017):
    """literal transcription of clip_Train_DS.__getitem__ (two_stream_dataset.py:287-333): per sample the sub-video,
    then the start, from one RandomState"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(batch):
        vid = rng.randint(0, len(lens))
        start = rng.randint(0, lens[vid] - clip_len)
        out.append((vid, start))
    return np.array(out).T


@pytest.mark.parametrize("lens,clip", [([12, 12, 12], 5), ([6, 40, 9, 180, 7], 5), ([5, 39, 8, 179, 6], 4), ([31], 4)])
def test_single_sampler_follows_the_reference_draw_rule(lens, clip):
    s = P.SingleClipSampler(lens, clip, seed=2017)
    got = np.concatenate([np.stack(s.draw(b)) for b in (7, 1, 32)], axis=1)
    assert np.array_equal(got, reference_single_draws(lens, clip, 40))
    many = np.stack(P.SingleClipSampler(lens, clip, seed=5).draw(4000))
    top = np.asarray(lens)[many[0]] - clip - 1                 # the exclusive upper bound: never a video's last clip
    assert (many[1] >= 0).all() and (many[1] <= top).all()
    with pytest.raises(ValueError, match="op sub-videos \\[1\\]"):
        P.SingleClipSampler([9, 4], 4, what="op")


def test_single_sampler_state_round_trips_through_a_weights_only_load(tmp_path):
    s = P.SingleClipSampler([12, 30], 5, seed=3)
    s.draw(5)
    torch.save({"sampler": s.get_state()}, tmp_path / "st.pth")
    back = torch.load(tmp_path / "st.pth", map_location="cpu", weights_only=True)
    want = np.stack(s.draw(9))
    s2 = P.SingleClipSampler([12, 30], 5, seed=99)
    s2.set_state(back["sampler"])
    assert np.array_equal(np.stack(s2.draw(9)), want)


def _dummy_tree(root, lens, ext):
    for v, n in enumerate(lens):
        d = root / f"{v + 1:02d}"
        d.mkdir(parents=True)
        for i in range(n):
            (d / f"{i:04d}{ext}").write_bytes(b"not decoded")


def test_one_kind_listing_and_budget_count_that_kind_only(tmp_path, monkeypatch):
    _dummy_tree(tmp_path / "rgb", [180] * 4, ".jpg")
    _dummy_tree(tmp_path / "op", [179] * 4, ".flo")
    only_rgb = P.list_subvideos(str(tmp_path / "rgb"), None)
    only_op = P.list_subvideos(None, str(tmp_path / "op"))
    both = P.list_subvideos(str(tmp_path / "rgb"), str(tmp_path / "op"))
    assert [f for f, _ in only_rgb] == [f for f, _ in both] and all(o == [] for _, o in only_rgb)
    assert [o for _, o in only_op] == [o for _, o in both] and all(f == [] for f, _ in only_op)
    calls = []
    monkeypatch.setattr(P, "read_image", lambda p: calls.append(p))
    monkeypatch.setattr(P, "_read_flow_file", lambda p: calls.append(p))
    for rgb_root, op_root, n_rgb, n_op in ((str(tmp_path / "rgb"), None, 720, 0), (None, str(tmp_path / "op"), 0, 716)):
        need = P.bank_bytes(n_rgb, n_op, 256)
        with pytest.raises(_lib.AmmcHipError, match=f"{n_rgb} frames \\+ {n_op} flows .* need {need / 1e9:.2f} GB"):
            P.ClipBank(rgb_root, op_root, 256, "cuda:0", budget_gb=0.01)
    assert calls == []
    with pytest.raises(ValueError, match="needs rgb_root, op_root or both"):
        P.ClipBank(None, None, 256, "cuda:0")


def test_single_stream_losses_are_the_reference_sums():
    g = torch.Generator().manual_seed(4)
    pred, tgt = torch.randn(2, 3, 8, 8, generator=g), torch.randn(2, 3, 8, 8, generator=g)
    diff, d_gen = torch.rand(1, generator=g), torch.randn(2, 1, 5, 5, generator=g)
    fp, fg = torch.randn(2, 2, 8, 8, generator=g), torch.randn(2, 2, 8, 8, generator=g)
    lams = dict(lam_adv=0.3, lam_gdl=0.7, lam_flow=1.5, lam_lp=1.1, lam_latent=0.9)
    loss, t = harness.single_stream_loss("rgb", pred, tgt, diff, d_gen, fp, fg, **lams)
    want_int = torch.norm(pred - tgt, p=2, dim=1).mean()
    assert torch.allclose(t["int"], want_int) and torch.allclose(t["latent"], diff.sum())
    assert torch.allclose(t["adv"], ((d_gen - 1) ** 2 / 2).mean()) and torch.allclose(t["flow"], (fp - fg).abs().mean())
    assert torch.allclose(t["gdl"], harness.gradient_loss(pred, tgt))
    want = 0.3 * t["adv"] + 0.7 * t["gdl"] + 1.5 * t["flow"] + 1.1 * want_int + 0.9 * diff.sum()
    assert torch.allclose(loss, want, rtol=1e-6)
    po, to = pred[:, :2], tgt[:, :2]
    loss, t = harness.single_stream_loss("op", po, to, diff, d_gen, lam_lp_op=2.0, lam_adv_op=0.25, lam_latent=0.5)
    assert sorted(t) == ["adv", "int", "latent"]
    assert torch.allclose(loss, 2.0 * torch.norm(po - to, p=2, dim=1).mean() + 0.25 * t["adv"] + 0.5 * diff.sum())
    loss, t = harness.single_stream_loss("op", po, to, diff)
    assert sorted(t) == ["int", "latent"] and torch.allclose(loss, t["int"] + t["latent"])
    with pytest.raises(TypeError, match="lam_gdl"):
        harness.single_stream_loss("op", po, to, diff, lam_gdl=1.0)
    with pytest.raises(ValueError):
        harness.single_stream_loss("rgb", pred, tgt, diff)                  # the rgb stage always has its adversarial term


def test_steps_refuse_the_wrong_stream():
    G = torch.nn.Identity()
    with pytest.raises(ValueError):
        harness.train_step_single(G, None, torch.zeros(1, 5, 3, 8, 8))
    with pytest.raises(ValueError):
        harness.train_step_single(G, None, torch.zeros(1, 4, 2, 8, 8), lam_adv_op=0.1)
    with pytest.raises(ValueError):
        harness.train_step_single_gan(G, G, None, None, torch.zeros(1, 4, 2, 8, 8), flow_fn=lambda p, c: p)


def test_stage_models_are_the_single_stream_networks_and_fill_the_joint_model():
    a = _parse("--stage", "rgb", "--rgb_root", "r", "--n_embed", "32")
    Gr, Dr, F2 = run_train.build_models(a)
    assert F2 is None and Dr.net[0].weight.shape[1] == 3
    assert list(Gr.state_dict()) == list(get_unet_vq_topk_res(12, 3, 64, 32, 2).state_dict())
    b = _parse("--stage", "op", "--op_root", "f", "--n_embed", "32")
    Go, Do, _ = run_train.build_models(b)
    assert Do is None
    assert list(Go.state_dict()) == list(get_unet_vq_topk_res(6, 2, 64, 32, 2).state_dict())
    assert {k: v.shape for k, v in Go.state_dict().items()} == \
        {k: v.shape for k, v in get_unet_vq_topk_res(6, 2, 64, 32, 2).state_dict().items()}
    Do2 = run_train.build_models(_parse("--stage", "op", "--op_root", "f", "--lam_adv_op", "0.1"))[1]
    assert Do2 is not None and Do2.net[0].weight.shape[1] == 2
    # both stage-1 checkpoints fill every stream key of the joint model
    joint = get_twostream((12, 6), (3, 2), 64, 32, 2)
    sd_r = {k: (v + 1.0 if v.is_floating_point() else v + 7) for k, v in Gr.state_dict().items()}
    sd_o = {k: (v - 1.0 if v.is_floating_point() else v + 9) for k, v in Go.state_dict().items()}
    harness.load_pretrained_branches(joint, sd_r, sd_o)
    got = joint.state_dict()
    stream_keys = [k for k in got if k.startswith(("rgb.", "op."))]
    assert len(stream_keys) == len(sd_r) + len(sd_o)
    for k in stream_keys:
        src = sd_r if k.startswith("rgb.") else sd_o
        assert torch.equal(got[k], src[k.split(".", 1)[1]]), k


# ---- the training steps, run to completion on toy CPU modules ----------------------------------------------------------

class _ToyJoint(torch.nn.Module):
    """`twostream`'s calling convention: (rgb_in, op_in) -> (rgb, op, (rgb_diff, op_diff), extra)"""

    def __init__(self):
        super().__init__()
        self.rgb, self.op = torch.nn.Conv2d(12, 3, 3, padding=1), torch.nn.Conv2d(6, 2, 3, padding=1)

    def forward(self, rgb_in, op_in):
        r, o = torch.tanh(self.rgb(rgb_in)), torch.tanh(self.op(op_in))
        return r, o, ((r * r).mean().reshape(1), (o * o).mean().reshape(1)), None


class _ToySingle(torch.nn.Module):
    """`UNetMem_v7`'s calling convention: x -> (pred, diff, extra)"""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(4 * c if c == 3 else 3 * c, c, 3, padding=1)

    def forward(self, x):
        y = torch.tanh(self.conv(x))
        return y, (y * y).mean().reshape(1), None


class _ToyD(torch.nn.Module):
    """A conv discriminator that, like the HIP one, computes with a COPY of its filters taken at the forward: the G step
    differentiates through the filters of the `d_gen` forward while the live ones are updated in place before it.
    `fail_attached`: raise in the forward that is attached to the generator's graph (the `d_gen` forward)."""

    def __init__(self, c, fail_attached=False):
        super().__init__()
        self.a, self.b = torch.nn.Conv2d(c, 4, 3, padding=1), torch.nn.Conv2d(4, 1, 3, padding=1)
        self.fail_attached = fail_attached

    def forward(self, x):
        if self.fail_attached and x.requires_grad:
            raise RuntimeError("toy failure in the d_gen forward")
        h = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x, self.a.weight.clone(), self.a.bias.clone(), padding=1), 0.2)
        return torch.nn.functional.conv2d(h, self.b.weight.clone(), self.b.bias.clone(), padding=1)


def _toy_flow(prev, cur):
    return (cur - prev)[:, :2] * 0.5 + cur[:, 1:] * cur[:, :2]


def _clips(c, t, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, t, c, 8, 8, generator=g) * 2 - 1


LR_G, LR_D = 0.05, 0.1
JOINT_LAMS = dict(lam_adv=0.3, lam_gdl=0.7, lam_flow=1.5, lam_lp=1.1, lam_lp_op=0.8, lam_latent=0.9)
RGB_LAMS = dict(lam_adv=0.3, lam_gdl=0.7, lam_flow=1.5, lam_lp=1.1, lam_latent=0.9)


def _adversarial_case(kind, flow, **d_kw):
    """(run, reference): `run(G, D, opt_g, opt_d, outputs)` calls the entry point; `reference(G0, D0)` computes
    (g_loss, d_loss, prediction) with the operations of the schedule, in its order, on copies of the pre-step networks"""
    torch.manual_seed(11)
    flow_fn = _toy_flow if flow else None
    if kind == "joint":
        G, D = _ToyJoint(), _ToyD(3, **d_kw)
        rgb, op = _clips(3, 5, 1), _clips(2, 4, 2)
        rgb_in, op_in, target = rgb[:, :-1].reshape(2, 12, 8, 8), op[:, :-1].reshape(2, 6, 8, 8), rgb[:, -1]

        def run(G, D, opt_g, opt_d, outputs, rgb=rgb):
            return harness.train_step_gan(G, D, opt_g, opt_d, rgb, op, flow_fn, outputs=outputs, **JOINT_LAMS)

        def forward(G0):
            out = G0(rgb_in, op_in)
            return out[0], lambda d_gen, fp, fg: harness.generator_loss_full(out, target, op[:, -1], d_gen, fp, fg, **JOINT_LAMS)
        clips = rgb
    else:
        c, t, lams = (3, 5, RGB_LAMS) if kind == "rgb" else (2, 4, dict(lam_lp_op=1.2, lam_adv_op=0.25, lam_latent=0.5))
        G, D = _ToySingle(c), _ToyD(c, **d_kw)
        clips = _clips(c, t, 3)
        x, target = clips[:, :-1].reshape(2, -1, 8, 8), clips[:, -1]

        def run(G, D, opt_g, opt_d, outputs, clips=clips):
            return harness.train_step_single_gan(G, D, opt_g, opt_d, clips, flow_fn, outputs=outputs, **lams)

        def forward(G0):
            pred, diff, _ = G0(x)
            return pred, lambda d_gen, fp, fg: harness.single_stream_loss(kind, pred, target, diff, d_gen, fp, fg, **lams)[0]

    def reference(G0, D0):
        pred, g_loss_of = forward(G0)
        d_both = D0(torch.cat([target, pred.detach()]))                    # the ONE batched call of the D update
        d_loss = harness.discriminate_loss(d_both[:2], d_both[2:])
        fp = fg = None
        if flow:
            both = flow_fn(torch.cat([target, target]), torch.cat([pred.detach(), target]))
            fp, fg = both[:2], both[2:]
        return g_loss_of(D0(pred), fp, fg), d_loss, pred
    return G, D, clips, run, reference


def _params(m):
    return [p.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize("kind,flow", [("joint", True), ("joint", False), ("rgb", True), ("op", False)])
def test_adversarial_steps_run_the_shared_schedule(kind, flow):
    G, D, _, run, reference = _adversarial_case(kind, flow)
    G0, D0 = copy.deepcopy(G), copy.deepcopy(D)
    opt_g, opt_d = torch.optim.SGD(G.parameters(), lr=LR_G), torch.optim.SGD(D.parameters(), lr=LR_D)
    outputs = {}
    g_loss, d_loss = run(G, D, opt_g, opt_d, outputs)
    want_g, want_d, want_pred = reference(G0, D0)
    assert not g_loss.requires_grad and not d_loss.requires_grad
    assert torch.equal(g_loss, want_g.detach()) and torch.equal(d_loss, want_d.detach())
    # D: the gradient of discriminate_loss on the batched call; G: the gradient of the full loss through the D of BEFORE its step
    for p, w in zip(D.parameters(), torch.autograd.grad(want_d, list(D0.parameters()))):
        assert torch.equal(p.grad, w)
    g_grads = torch.autograd.grad(want_g, list(G0.parameters()))
    for p, w in zip(G.parameters(), g_grads):
        assert torch.equal(p.grad, w)
    through_stepped_d = torch.autograd.grad(reference(G0, D)[0], list(G0.parameters()))
    assert not all(torch.equal(a, b) for a, b in zip(g_grads, through_stepped_d))      # (the distinction is a real one)
    # both updates were taken, each with its own gradient
    for net, net0, lr in ((G, G0, LR_G), (D, D0, LR_D)):
        for p, p0 in zip(net.parameters(), net0.parameters()):
            assert p.requires_grad and not torch.equal(p, p0)
            assert torch.equal(p.detach(), torch.add(p0.detach(), p.grad, alpha=-lr))       # (SGD's own arithmetic)
    if kind == "joint":
        assert sorted(outputs) == ["op", "rgb"] and torch.equal(outputs["rgb"], want_pred.detach())
        assert outputs["op"].shape == (2, 2, 8, 8) and not outputs["rgb"].requires_grad and not outputs["op"].requires_grad
    else:
        assert sorted(outputs) == ["pred", "terms"] and torch.equal(outputs["pred"], want_pred.detach())
        want_terms = {"rgb": ["adv", "flow", "gdl", "int", "latent"], "op": ["adv", "int", "latent"]}[kind]
        assert sorted(outputs["terms"]) == want_terms and not any(v.requires_grad for v in outputs["terms"].values())


@pytest.mark.parametrize("kind", ["joint", "rgb"])
def test_adversarial_steps_restore_d_and_refuse_non_finite_losses(kind):
    # the d_gen forward raises: every D parameter is trainable again, nothing was updated
    G, D, _, run, _ = _adversarial_case(kind, True, fail_attached=True)
    g0, d0 = _params(G), _params(D)
    with pytest.raises(RuntimeError, match="toy failure"):
        run(G, D, torch.optim.SGD(G.parameters(), lr=LR_G), torch.optim.SGD(D.parameters(), lr=LR_D), None)
    assert all(p.requires_grad for p in D.parameters())
    assert all(torch.equal(p, q) for p, q in zip(list(G.parameters()) + list(D.parameters()), g0 + d0))
    # a non-finite loss: both updates are refused together
    G, D, clips, run, _ = _adversarial_case(kind, True)
    g0, d0 = _params(G), _params(D)
    bad = clips.clone()
    bad[0, -1, 0, 0, 0] = float("inf")
    outputs = {}
    with pytest.raises(FloatingPointError):
        run(G, D, torch.optim.SGD(G.parameters(), lr=LR_G), torch.optim.SGD(D.parameters(), lr=LR_D), outputs, bad)
    assert all(torch.equal(p, q) for p, q in zip(list(G.parameters()) + list(D.parameters()), g0 + d0))
    assert all(p.requires_grad for p in D.parameters())


@pytest.mark.parametrize("kind", ["joint", "op"])
def test_generator_only_steps_take_one_update_or_none(kind):
    torch.manual_seed(12)
    rgb, op = _clips(3, 5, 5), _clips(2, 4, 6)
    rgb_in, op_in = rgb[:, :-1].reshape(2, 12, 8, 8), op[:, :-1].reshape(2, 6, 8, 8)
    if kind == "joint":
        G, lams = _ToyJoint(), dict(lam_lp=1.1, lam_lp_op=0.8, lam_latent=0.9)

        def run(G, outputs, rgb=rgb, op=op):
            return harness.train_step(G, torch.optim.SGD(G.parameters(), lr=LR_G), rgb, op, **lams)

        def reference(G0):
            return harness.generator_loss(G0(rgb_in, op_in), rgb[:, -1], op[:, -1], **lams), None
    else:
        G, lams = _ToySingle(2), dict(lam_lp_op=1.2, lam_latent=0.5)

        def run(G, outputs, rgb=None, op=op):
            return harness.train_step_single(G, torch.optim.SGD(G.parameters(), lr=LR_G), op, outputs=outputs, **lams)

        def reference(G0):
            pred, diff, _ = G0(op_in)
            return harness.single_stream_loss("op", pred, op[:, -1], diff, **lams)[0], pred
    G0 = copy.deepcopy(G)
    outputs = {}
    loss = run(G, outputs)
    want, want_pred = reference(G0)
    assert not loss.requires_grad and torch.equal(loss, want.detach())
    for p, p0, w in zip(G.parameters(), G0.parameters(), torch.autograd.grad(want, list(G0.parameters()))):
        assert torch.equal(p.grad, w) and not torch.equal(p, p0)
        assert torch.equal(p.detach(), torch.add(p0.detach(), w, alpha=-LR_G))               # (SGD's own arithmetic)
    if kind == "op":
        assert sorted(outputs) == ["pred", "terms"] and sorted(outputs["terms"]) == ["int", "latent"]
        assert torch.equal(outputs["pred"], want_pred.detach()) and not outputs["pred"].requires_grad
    # a non-finite loss: no update
    before = _params(G)
    bad_rgb, bad_op = rgb.clone(), op.clone()
    bad_rgb[0, -1, 0, 0, 0] = bad_op[0, -1, 0, 0, 0] = float("nan")
    with pytest.raises(FloatingPointError):
        run(G, None, bad_rgb, bad_op)
    assert all(torch.equal(p, q) for p, q in zip(G.parameters(), before))
