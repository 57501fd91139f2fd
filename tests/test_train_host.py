"""Host side of the training entry (run_train.py, pipeline.ClipSampler / ClipBank, csrc/clip_bank.hip): the reference's
draw rule, the bank's size estimate and budget refusal, the index validation, the train state and the argument checks
of the new C entry points - all decided before anything touches a GPU."""
import os

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, harness, pipeline as P, run_train


def reference_draws(rgb_lens, op_lens, batch, seed=2017, rgb_len=5, op_len=4):
    """literal transcription of TwoStream_Train_DS.__getitem__ (two_stream_dataset.py:467-468) over
    clip_Train_DS.__getitem__ (:289-292), num_workers=0: per sample the rgb (video, start), then the op (video, start)"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(batch):
        sub_vid = rng.randint(0, len(rgb_lens))
        cur_cid = rng.randint(0, rgb_lens[sub_vid] - rgb_len)
        op_vid = rng.randint(0, len(op_lens))
        op_cid = rng.randint(0, op_lens[op_vid] - op_len)
        out.append((sub_vid, cur_cid, op_vid, op_cid))
    return np.array(out).T


LAYOUTS = {
    "equal": ([12, 12, 12], [12, 12, 12]),
    "unequal": ([6, 40, 9, 180, 7], [5, 39, 8, 179, 6]),          # op folder one entry shorter than the rgb folder
    "one_video": ([31], [30]),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_sampler_follows_the_reference_draw_rule(layout):
    rgb_lens, op_lens = LAYOUTS[layout]
    s = P.ClipSampler(rgb_lens, op_lens, seed=2017)
    got = np.concatenate([np.stack(s.draw(b)) for b in (7, 1, 32)], axis=1)
    want = reference_draws(rgb_lens, op_lens, 40)
    assert np.array_equal(got, want)
    # starts stay in [0, len - clip - 1]: the exclusive upper bound never draws a video's last clip
    many = np.stack(P.ClipSampler(rgb_lens, op_lens, seed=5).draw(4000))
    for vids, starts, lens, clip in ((many[0], many[1], rgb_lens, 5), (many[2], many[3], op_lens, 4)):
        top = np.asarray(lens)[vids] - clip - 1
        assert (starts >= 0).all() and (starts <= top).all()
        if layout == "one_video":
            assert starts.max() == top.max() and starts.min() == 0


def test_sampler_refuses_videos_too_short_to_draw_from():
    with pytest.raises(ValueError, match="rgb sub-videos \\[1\\]"):
        P.ClipSampler([9, 5], [8, 8])
    with pytest.raises(ValueError, match="op sub-videos \\[0\\]"):
        P.ClipSampler([9, 9], [4, 8])


def test_train_state_round_trips_with_the_sampler_rng(tmp_path):
    s = P.ClipSampler([12, 30], [11, 29], seed=3)
    s.draw(5)
    p = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.Adam([p], lr=1e-3)
    p.grad = torch.full((3,), 0.5)
    opt.step()
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5)
    sched.step()
    sched.step()
    state = {"g_step": 7, "opt_g": opt.state_dict(), "sched_g": sched.state_dict(), "sampler": s.get_state(),
             "args": {"batch": 4, "milestones": [2]}}
    path = harness.save_checkpoint(state, str(tmp_path / "train_state"), 7)
    assert os.path.basename(path) == "step_000008.pth"                     # the reference's saver names: step + 1
    back = torch.load(path, map_location="cpu", weights_only=True)         # plain values and tensors only
    want = np.stack(s.draw(9))
    s2 = P.ClipSampler([12, 30], [11, 29], seed=99)
    s2.set_state(back["sampler"])
    assert np.array_equal(np.stack(s2.draw(9)), want)
    opt2 = torch.optim.Adam([torch.nn.Parameter(torch.ones(3))], lr=1e-3)
    opt2.load_state_dict(back["opt_g"])
    sched2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=[2], gamma=0.5)
    sched2.load_state_dict(back["sched_g"])
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == 5e-4
    assert torch.equal(opt2.state_dict()["state"][0]["exp_avg"], opt.state_dict()["state"][0]["exp_avg"])
    assert back["g_step"] == 7 and back["args"]["milestones"] == [2]


def write_flo(path, flow):
    h, w, _ = flow.shape
    with open(path, "wb") as f:
        np.array([202021.25], np.float32).tofile(f)
        np.array([w, h], np.int32).tofile(f)
        np.ascontiguousarray(flow, np.float32).tofile(f)


def test_flo_written_here_round_trips_through_read_flo(tmp_path):
    flow = np.random.default_rng(1).normal(0, 3, (7, 11, 2)).astype(np.float32)
    write_flo(tmp_path / "a.flo", flow)
    got = P.read_flo(str(tmp_path / "a.flo"))
    assert got.dtype == np.float32 and np.array_equal(got, flow)


def _dummy_tree(root, lens, ext):
    for v, n in enumerate(lens):
        d = root / f"{v + 1:02d}"
        d.mkdir(parents=True)
        for i in range(n):
            (d / f"{i:04d}{ext}").write_bytes(b"not decoded")


def test_bank_size_estimate_and_budget_refusal_before_any_decode(tmp_path, monkeypatch):
    _dummy_tree(tmp_path / "rgb", [180] * 16, ".jpg")
    _dummy_tree(tmp_path / "op", [179] * 16, ".flo")
    assert P.bank_bytes(16 * 180, 16 * 179, 256) == 16 * 180 * 3 * 65536 + 16 * 179 * 4 * 65536
    assert P.bank_bytes(10, 10, (96, 64)) == 10 * 3 * 64 * 96 + 10 * 4 * 64 * 96
    calls = []
    monkeypatch.setattr(P, "read_image", lambda p: calls.append(p))
    monkeypatch.setattr(P, "read_flo", lambda p: calls.append(p))
    monkeypatch.setattr(P, "_read_flow_file", lambda p: calls.append(p))
    need = P.bank_bytes(16 * 180, 16 * 179, 256)
    with pytest.raises(_lib.AmmcHipError, match=f"need {need / 1e9:.2f} GB.*budget of 1.00 GB"):
        P.ClipBank(str(tmp_path / "rgb"), str(tmp_path / "op"), 256, "cuda:0", budget_gb=1.0)
    assert calls == []
    with pytest.raises(_lib.AmmcHipError, match="no CPU pipeline"):
        P.ClipBank(str(tmp_path / "rgb"), str(tmp_path / "op"), 256, "cpu", budget_gb=100.0)
    assert calls == []


def test_index_validation_rejects_clips_that_cross_a_video():
    starts, counts = np.array([0, 12, 18]), np.array([12, 6, 9])        # videos [0, 12), [12, 18), [18, 27)
    ok = P.check_clip_indices("rgb", np.array([0, 7, 12, 13, 18, 22], np.int32), starts, counts, 5)
    assert ok.dtype == np.int64 and list(ok) == [0, 7, 12, 13, 18, 22]
    for bad in (8, 11, 14, 23, 27, -1, 1 << 40):                          # crosses 12 / 18 / the end, or outside the bank
        with pytest.raises(_lib.AmmcHipError, match="does not lie inside one sub-video"):
            P.check_clip_indices("rgb", np.array([0, bad]), starts, counts, 5)
    with pytest.raises(_lib.AmmcHipError, match="integers"):
        P.check_clip_indices("op", np.array([0.0]), starts, counts, 4)


def test_clip_bank_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    A = 0x100000                                                          # aligned, never dereferenced
    assert lib.ammc_frames_u8_resize_u8(None, 1, 8, 8, A, 4, 4, 0, None) == -1
    assert lib.ammc_frames_u8_resize_u8(A, 0, 8, 8, A, 4, 4, 0, None) == -1
    assert lib.ammc_frames_u8_resize_u8(A, 1, 8, -8, A, 4, 4, 0, None) == -1
    assert lib.ammc_flows_resize_c0(A, 1, 8, 8, None, 4, 4, None) == -1
    assert lib.ammc_flows_resize_c0(A, 1, 8, 8, A, 0, 4, None) == -1
    ok = [A, 100, A, 100, A, A, 32, 5, 4, 256, 256, A, A, None]

    def gather(**kw):
        a = list(ok)
        names = ["rgb", "n_rgb", "op", "n_op", "rf", "of", "b", "rl", "ol", "h", "w", "ro", "oo", "s"]
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.ammc_gather_clips(*a)
    for kw in (dict(rgb=None), dict(op=None), dict(rf=None), dict(of=None), dict(ro=None), dict(oo=None),
               dict(b=0), dict(rl=0), dict(ol=-1), dict(h=0), dict(n_rgb=4), dict(n_op=3),
               dict(h=3, w=5),                                              # h * w % 4 != 0
               dict(rgb=A + 2), dict(op=A + 4), dict(ro=A + 8), dict(oo=A + 4),   # alignment
               dict(b=4000)):                                               # 4000 * 19 planes > 65535
        assert gather(**kw) == -1, kw


def test_run_train_refuses_before_touching_data(tmp_path, monkeypatch):
    base = ["--rgb_root", str(tmp_path), "--op_root", str(tmp_path), "--out", str(tmp_path / "o"), "--iterations", "2"]
    with pytest.raises(SystemExit, match="multiple of 64"):
        run_train.main(base + ["--size", "100", "--flownet", "synthetic"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU per process"):
        run_train.main(base)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run_train.parse(base + ["--pretrain_rgb", "x.pth"])              # --pretrain_op missing
    a = run_train.parse(base)
    assert (a.batch, a.size, a.lr_g, a.lr_d, a.milestones, a.seed, a.log_every, a.save_every) == \
        (32, 256, 2e-4, 2e-5, [], 2017, 10, 1000)
    assert run_train.lams_of(a) == harness.LAMS_ANOPRED
    assert not (tmp_path / "o").exists()
