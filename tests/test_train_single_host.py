"""Host side of stage-1 training (`run_train --stage rgb|op`): the argument rules of each stage, the single-stream draw
rule (`pipeline.SingleClipSampler`) against a literal transcription of the reference's, the one-kind bank's listing and
budget, the single-stream losses, and the models each stage builds - whose two generator checkpoints must fill every
`rgb.*` / `op.*` key of the joint model through `load_pretrained_branches`."""
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
