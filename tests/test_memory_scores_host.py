"""Host-side checks of the memory-score pass: the float64 reference on hand-made inputs, the C
entry's argument refusals, the near-tie cap of the shared cases, the `run_memory` parser and the frame assembly."""
import argparse

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, harness as Hn, parallel, run_memory, run_test

import memory_score_cases as K


def _hand_made(k=2, m=9, c=32, b=2, h=3, w=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((64, c), generator=g) / c ** 0.5, 0.1 * torch.randn((64,), generator=g),
            torch.randn((64, m), generator=g), torch.randn((b, h, w, c), generator=g), k)


def test_reference_a_position_moved_onto_a_slot():
    enc_w, enc_b, embed, x, k = _hand_made()
    ref = Hn.memory_scores_reference(enc_w, enc_b, embed, x, k)
    embed = embed.clone()
    embed[:, 6] = ref["z"][1, 2, 3].float()                       # slot 6 := the feature of one position (fp32-rounded)
    got = Hn.memory_scores_reference(enc_w, enc_b, embed, x, k)
    assert int(got["idx"][1, 2, 3, 0]) == 6
    assert float(got["map"][1, 2, 3]) < 1e-12 and float(got["map"][1, 2, 3]) >= 0.0
    assert tuple(got["map"].shape) == (2, 3, 4) and tuple(got["idx"].shape) == (2, 3, 4, 2) and got["idx"].dtype == torch.int32
    # the map is the direct squared distance to the nearest slot / d: the expanded form's minimum, up to float64 rounding
    assert torch.allclose(got["map"], got["dist"].min(-1).values / 64, rtol=0, atol=1e-12)
    z, e = got["z"], embed.double()
    s0 = int(got["idx"][0, 0, 0, 0])
    assert float(got["map"][0, 0, 0]) == pytest.approx(float(((e[:, s0] - z[0, 0, 0]) ** 2).sum() / 64), rel=1e-14)


def test_reference_k_order_ties_and_margin():
    enc_w, enc_b, embed, x, _ = _hand_made()
    embed = embed.clone()
    embed[:, 2] = embed[:, 7]                                      # an exact tie: slots 2 and 7
    ref = Hn.memory_scores_reference(enc_w, enc_b, embed, x, 3)
    d = ref["dist"]
    picked = torch.gather(d, -1, ref["idx"].long())
    assert bool((picked[..., 1:] >= picked[..., :-1]).all())       # nearest first
    assert torch.equal(picked[..., 0], d.min(-1).values)
    idx = ref["idx"]
    for r in range(2):                                              # equal distances: the lower slot first
        at = idx[..., r] == 7
        assert not bool((at & (idx[..., r + 1] == 2)).any())
        at = idx[..., r] == 2
        assert bool((idx[..., r + 1][at] == 7).all())
    assert tuple(ref["order"].shape) == (2, 3, 4, 4) and torch.equal(ref["order"][..., :3].to(torch.int32), idx)
    srt = torch.sort(d, -1).values[..., :4]
    assert torch.equal(ref["margin"], (srt[..., 1:] - srt[..., :-1]).min(-1).values)
    tied = (idx[..., :3] == 2).any(-1) & (idx[..., :3] == 7).any(-1)
    assert bool((ref["margin"][tied] == 0).all())
    one = Hn.memory_scores_reference(enc_w, enc_b, embed[:, :1], x, 1)          # a single slot: no gap to measure
    assert bool(torch.isinf(one["margin"]).all()) and bool((one["idx"] == 0).all())


def test_reference_commit_is_the_mean_and_worst_the_first_maximum():
    enc_w, enc_b, embed, x, k = _hand_made()
    x = x.clone()
    x[0, 2, 1] = x[0, 0, 3]                                        # two positions of identical content ...
    x[0, 0, 3] *= 40.0                                             # ... made the largest of their clip - and
    x[0, 2, 1] *= 40.0                                             # the same value at two places
    ref = Hn.memory_scores_reference(enc_w, enc_b, embed, x, k)
    assert torch.allclose(ref["commit"], ref["map"].mean(dim=(1, 2)), rtol=1e-15, atol=0)
    assert float(ref["map"][0, 0, 3]) == float(ref["map"][0, 2, 1]) == float(ref["worst"][0])
    assert int(ref["worst_idx"][0]) == 0 * 4 + 3 and ref["worst_idx"].dtype == torch.int32
    flat = ref["map"][1].reshape(-1)
    assert int(ref["worst_idx"][1]) == int(flat.argmax()) and float(ref["worst"][1]) == float(flat.max())
    z0 = ref["z"][0, 0, 0]
    near = embed.double()[:, int(ref["idx"][0, 0, 0, 0])]
    assert float(ref["scale"][0, 0, 0]) == pytest.approx(float(((z0 * z0).sum() + (near * near).sum()) / 64), rel=1e-14)


def test_entry_refuses_bad_arguments_without_a_device():
    """integer stand-ins for the pointers: every refusal is decided before anything touches the device.  Refusals only:
    a call that passed the checks would launch on these addresses"""
    lib = _lib.load()
    B, H, W, C, M = 2, 5, 7, 512, 256
    ok = dict(x=0x100000, xs=(H * W * C, W * C, C), b=B, h=H, w=W, c=C, enc_w=0x200000, enc_b=0x300000, e_dm=0x400000,
              e_md=0x500000, enorm=0x600000, d=64, m=M, k=2, map=0x700000, map_bs=H * W, idx=0x800000, commit=0x900000,
              worst=0xa00000, worst_idx=0xb00000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ammc_memory_scores_f32(a["x"], *a["xs"], a["b"], a["h"], a["w"], a["c"], a["enc_w"], a["enc_b"], a["e_dm"],
                                          a["e_md"], a["enorm"], a["d"], a["m"], a["k"], a["map"], a["map_bs"], a["idx"],
                                          a["commit"], a["worst"], a["worst_idx"], None)
    for name in ("x", "enc_w", "enc_b", "e_dm", "e_md", "enorm", "map", "commit", "worst", "worst_idx"):
        assert call(**{name: None}) == -1, name
        assert call(**{name: ok[name] + 2}) == -1, name                          # not 4-byte aligned
    assert call(idx=0x800002) == -1
    for name in ("b", "h", "w", "c", "d", "m", "k"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(xs=(H * W * C, W * C, C - 1)) == -1                              # pixel stride < c
    assert call(xs=(H * W * C, W * C - 1, C)) == -1                              # row stride < the row
    assert call(xs=(H * W * C - 1, W * C, C)) == -1                              # batch stride < the clip
    assert call(xs=(H * W * 600, W * 600 - 89, 600)) == -1                       # padded pixels: the row is (w - 1) * 600 + c
    assert call(map_bs=H * W - 1) == -1
    for d in (32, 63, 128):
        assert call(d=d) == -2, d
    for k in (3, 4):
        assert call(k=k) == -2, k
    for c in (16, 48, 500, 1056, 2048):
        assert call(c=c, xs=(H * W * c, W * c, c)) == -2, c
    assert call(m=1, k=2) == -2                                                  # m < k
    # bad AND unsupported: the bad argument decides
    assert call(d=128, x=None) == -1 and call(k=3, map_bs=0) == -1


@pytest.mark.parametrize("case,variant", K.all_variants(), ids=[K.name_of(c, v) for c, v in K.all_variants()])
def test_near_tie_cap(case, variant):
    """the share of positions whose ranking the GPU test may not compare exactly (margin <= 1e-4 |z|^2) is at
    most 3 % in every case - variant a's planted ties excepted: the float64 reference alone stays inside the cap, so
    the GPU test cannot hide a ranking bug behind exclusions"""
    ref = K.reference(case, variant)
    near = K.near_tie(ref)
    if variant == "a":
        planted = K.planted_tie(ref)
        assert bool(planted.any()) and bool((ref["margin"][planted] == 0).all())
        assert int((ref["idx"][..., 0] == K.TIE_COPIES[0]).sum()) >= 1              # what SEED_A was chosen for
        near = near & ~planted
    share = float(near.float().mean())
    print(f"{K.name_of(case, variant)}: near-tie share {100 * share:.3f} %")
    assert share <= 0.03


def test_cases_are_what_the_recipe_says():
    assert len(K.CASES) == 7 and len(K.all_variants()) == 13
    for case, variant in K.all_variants():
        b, h, w, c, m, k = case
        t = K.inputs(case, variant)
        assert tuple(t["x"].shape) == (b, h, w, c) and tuple(t["enc_w"].shape) == (64, c)
        assert tuple(t["enc_b"].shape) == (64,) and tuple(t["embed"].shape) == (64, m)
        assert all(v.dtype == torch.float32 for v in t.values())
    a = K.inputs(K.CASES[1], "a")["embed"]
    assert torch.equal(a[:, 3], a[:, 5]) and torch.equal(a[:, 20], a[:, 5])
    for case in K.PLANTED:
        ref, t = K.reference(case, "b"), K.inputs(case, "b")
        for s, (bb, y, xx) in zip(K.NEAR_SLOTS, K.near_rows(case)):
            assert int(ref["idx"][bb, y, xx, 0]) == s and float(ref["map"][bb, y, xx]) < 1e-13
            assert torch.equal(t["embed"][:, s], ref["z"][bb, y, xx].float())
        plain, big = K.inputs(case)["embed"], K.inputs(case, "c")["embed"]
        assert torch.equal(big[:, ::4], plain[:, ::4] * 1e5) and torch.equal(big[:, 1::4], plain[:, 1::4])


def _options(parser):
    return {a.dest: (tuple(a.option_strings), a.default, a.type, tuple(a.choices) if a.choices else None, a.nargs, a.const)
            for a in parser._actions if a.dest != "help"}


def test_run_memory_takes_every_option_of_run_test_unchanged(monkeypatch):
    """`run_memory` repeats run_test's model and data-source options (run_test builds its parser inside `main`): every
    one of them must exist in `run_memory` with the same flags, default, type and choices, and `run_memory` adds
    exactly its two"""
    class Got(Exception):
        pass

    def grab(self, args=None, namespace=None):
        raise Got(self)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(Got) as info:
        run_test.main([])
    monkeypatch.undo()
    theirs, ours = _options(info.value.args[0]), _options(run_memory.build_parser())
    assert len(theirs) >= 14
    for dest, spec in theirs.items():
        assert ours.get(dest) == spec, dest
    assert set(ours) - set(theirs) == {"maps_dir", "slots"}
    a = run_memory.build_parser().parse_args(["--synthetic"])
    assert a.maps_dir is None and a.slots is False                              # the maps folder is optional here
    a = run_memory.build_parser().parse_args(["--synthetic", "--maps_dir", "m", "--slots"])
    assert a.maps_dir == "m" and a.slots is True


def test_run_memory_refuses_more_than_one_rank(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_memory.main(["--synthetic", "--maps_dir", str(tmp_path / "maps")])
    assert "one GPU" in str(info.value.code) and "sharded map writing is not implemented" in str(info.value.code)
    assert not (tmp_path / "maps").exists() and capsys.readouterr().out == ""


@pytest.mark.parametrize("t", [7, 23])
def test_frame_assembly_of_per_clip_commit_arrays(t):
    """`assemble_localised` on the arrays of `memory_subvideo`: clip i fills frame i + len_clip - 1 of its stream, the head
    copies the first predicted frame, the flow stream's last frame copies the one before it"""
    rng = np.random.default_rng(t)
    h, w, k = 2, 3, 2
    for batches in (Hn.subvideo_batches(t), Hn.subvideo_batches(t, batch=3)):
        parts = []
        for s, e in batches:
            b = e - s
            part = {"rgb_comm": np.float32(rng.random()), "op_comm": np.float32(rng.random())}
            for st in ("rgb", "op"):
                part[f"{st}_clip_comm"] = rng.random(b, dtype=np.float32)
                part[f"{st}_commit_map"] = rng.random((b, h, w), dtype=np.float32)
                part[f"{st}_commit_worst_idx"] = rng.integers(0, h * w, b).astype(np.int32)
                part[f"{st}_slots"] = rng.integers(0, 256, (b, h, w, k)).astype(np.int32)
            parts.append(part)
        got = Hn.assemble_localised(t, batches, parts)
        want = Hn.assemble_records(t, batches, [dict(p, rgb_psnr=p["rgb_clip_comm"], op_psnr=p["op_clip_comm"]) for p in parts])
        assert np.array_equal(got["rgb_comm"], want["rgb_comm"]) and np.array_equal(got["op_comm"], want["op_comm"])
        assert np.array_equal(got["rgb_clip_comm"], want["rgb_psnr"]) and np.array_equal(got["op_clip_comm"], want["op_psnr"])
        for key, tail in (("clip_comm", ()), ("commit_map", (h, w)), ("commit_worst_idx", ()), ("slots", (h, w, k))):
            rgb = np.concatenate([p[f"rgb_{key}"] for p in parts])
            assert got[f"rgb_{key}"].shape == (t,) + tail and got[f"rgb_{key}"].dtype == rgb.dtype
            assert np.array_equal(got[f"rgb_{key}"][Hn.RGB_LEN_CLIP - 1:], rgb)
            for i in range(Hn.RGB_LEN_CLIP - 1):                                 # frames 0-3 copy frame 4
                assert np.array_equal(got[f"rgb_{key}"][i], rgb[0])
            op = np.concatenate([p[f"op_{key}"] for p in parts])
            assert np.array_equal(got[f"op_{key}"][Hn.OP_LEN_CLIP - 1:t - 1], op)
            for i in range(Hn.OP_LEN_CLIP - 1):                                  # frames 0-2 copy frame 3
                assert np.array_equal(got[f"op_{key}"][i], op[0])
            assert np.array_equal(got[f"op_{key}"][t - 1], op[-1])               # the last flow frame copies the one before
