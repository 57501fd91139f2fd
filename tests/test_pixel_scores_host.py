"""Pixel-level evaluation without a GPU: the equivalence the feature rests on - the criterion
as written against `roc_auc` of one number per frame -, the integer rank rule, the mask rules against their loop
forms, the argument checks of the C entry and of `ops.pixel_scores` (decided before any HIP call), the `run_pixel`
options and mask sources, and `pixel_level_auc` on records built by the numpy restatement (tests/pixel_cases.py)."""
import argparse
from fractions import Fraction
import math

import numpy as np
import pytest
import torch

import pixel_cases as PC
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, parallel, run_pixel, run_test


def _frame_numbers(maps, masks, num, den):
    ref = PC.batch_scores(maps, masks, num, den)
    ref["max_all"] = np.maximum(ref["max_in"], ref["max_out"])
    return ref


@pytest.mark.parametrize("frac", [(2, 5), (1, 1), (1, 4096), (3, 4)])
def test_criterion_as_written_equals_roc_auc_of_one_number_per_frame(frac):
    for maps, masks in PC.criterion_cases():
        ref = _frame_numbers(maps, masks, *frac)
        scores, labels = Hn.pixel_criterion_scores(ref["m"], ref["kth"], ref["max_all"])
        assert np.array_equal(labels, (masks.reshape(len(masks), -1) != 0).any(axis=1))
        assert 0 < labels.sum() < labels.size
        got = Hn.roc_auc(labels, scores, pos_label=1)
        want = PC.criterion_literal(maps, masks, *frac)
        assert abs(got - want) <= 1e-12, (frac, got, want)


def test_rank_rule_against_exact_rationals():
    for num, den in ((2, 5), (1, 1), (1, 4096), (1, 2), (3, 7), (4095, 4096), (5, 5)):
        for m in range(1, 51):
            k = PC.rank_k(m, num, den)
            assert k == math.ceil(Fraction(num * m, den)) and 1 <= k <= m
            # k is the least count that reaches the fraction
            assert Fraction(k, m) >= Fraction(num, den) and (k == 1 or Fraction(k - 1, m) < Fraction(num, den))
    assert [PC.rank_k(m, 2, 5) for m in (1, 2, 3, 5)] == [1, 1, 2, 2]


@pytest.mark.parametrize("src, size", [((240, 360), (64, 64)), ((60, 90), (64, 64)), ((7, 5), (7, 5)), ((5, 9), (13, 4)), ((1, 1), (3, 2))])
def test_resize_mask_is_the_nearest_rule(src, size):
    rng = np.random.default_rng(src[0] * 1000 + size[0])
    mask = (rng.random((3,) + src) < 0.3).astype(np.uint8) * rng.integers(1, 255, (3,) + src).astype(np.uint8)
    got = Hn.resize_mask(torch.from_numpy(mask), size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + size
    assert np.array_equal(got.numpy(), PC.resize_nearest(mask, *size))
    # the floating-point statement of the rule, where it is exact
    ys = [int(math.floor((y + 0.5) * src[0] / size[0])) for y in range(size[0])]
    assert ys == [((2 * y + 1) * src[0]) // (2 * size[0]) for y in range(size[0])]
    assert torch.equal(Hn.resize_mask(torch.from_numpy(mask) != 0, size), got != 0)


@pytest.mark.parametrize("hw, patch", [((64, 64), 16), ((27, 21), 8), ((5, 3), 8), ((33, 65), 32), ((16, 17), 16)])
def test_pool_mask_is_any_pixel_over_the_patch_grid(hw, patch):
    rng = np.random.default_rng(hw[0] * 100 + patch)
    mask = (rng.random((4,) + hw) < 0.01).astype(np.uint8) * 200
    mask[1] = 0
    mask[2, -1, -1] = 3                                                       # the ragged corner patch
    got = Hn.pool_mask(torch.from_numpy(mask), patch)
    want = PC.pool_any(mask, patch)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape == (4, -(-hw[0] // patch), -(-hw[1] // patch))
    assert np.array_equal(got.numpy(), want) and want[2, -1, -1] == 1 and not want[1].any()
    assert want.shape[1:] == (_lib.load().ammc_error_maps_patch_count(hw[0], 1, patch), _lib.load().ammc_error_maps_patch_count(1, hw[1], patch))


def test_entry_refuses_bad_arguments_without_a_device():
    """integer stand-ins for the pointers: every refusal is decided before anything touches the device.  Refusals only:
    a call that passed the checks would launch on these addresses"""
    lib = _lib.load()
    assert hasattr(lib, "ammc_pixel_scores_f32") and "ammc_pixel_scores_f32" in _lib.SIGNATURES
    H, W = 27, 21
    ok = dict(map=0x100000, map_bs=H * W, mask=0x200000, mask_bs=H * W, b=2, h=H, w=W, num=2, den=5, m=0x300000, kth=0x400000,
              max_in=0x500000, max_out=0x600000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ammc_pixel_scores_f32(a["map"], a["map_bs"], a["mask"], a["mask_bs"], a["b"], a["h"], a["w"], a["num"], a["den"],
                                         a["m"], a["kth"], a["max_in"], a["max_out"], None)
    for name in ("map", "mask", "m", "kth", "max_in", "max_out"):
        assert call(**{name: None}) == -1, name
    for name in ("b", "h", "w"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    big = dict(map_bs=1 << 25, mask_bs=1 << 25)
    assert call(h=4096, w=4097, **big) == -1 and call(h=1, w=(1 << 24) + 1, **big) == -1       # h * w > 2^24
    assert call(h=65536, w=65536, map_bs=1 << 40, mask_bs=1 << 40) == -1                      # ... and past 32 bits
    for num, den in ((0, 5), (-1, 5), (6, 5), (1, 4097), (4097, 4097), (1, 0)):
        assert call(num=num, den=den) == -1, (num, den)
    assert call(map_bs=H * W - 1) == -1 and call(mask_bs=H * W - 1) == -1 and call(map_bs=0) == -1
    assert call(map=0x100002) == -1 and call(kth=0x400001) == -1                              # not 4-byte aligned
    with pytest.raises(_lib.AmmcHipError):
        _lib.check(call(num=0), "pixel_scores")


def test_wrapper_refuses_before_loading_the_device():
    a, k = torch.zeros(2, 5, 7), torch.zeros(2, 5, 7, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ops.pixel_scores(a, k)                                                # CPU tensors
    for bad_map, bad_mask in ((a.double(), k), (a, k.int()), (a, k.float()), (a[0], k[0]), (a, k[:, :4]), (a[:1], k),
                              (a.unsqueeze(0), k.unsqueeze(0)), (a.numpy(), k)):
        with pytest.raises(ValueError):
            ops.pixel_scores(bad_map, bad_mask)
    for frac in ((0, 5), (6, 5), (1, 4097), (2,), "x", 3):
        with pytest.raises(ValueError):
            ops.pixel_scores(a, k, frac)
    # stride problems are refused before the device question is asked
    wide = torch.zeros(2, 5, 14)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixel_scores(wide[:, :, ::2], k)                                  # pixel stride 2
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixel_scores(a, torch.zeros(2, 7, 5, dtype=torch.uint8).transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixel_scores(torch.zeros(5 * 7 + 10).as_strided((2, 5, 7), (10, 7, 1)), k)        # batch stride < H * W


def _options(parser):
    return {a.dest: (tuple(a.option_strings), a.default, a.type, tuple(a.choices) if a.choices else None, a.nargs, a.const)
            for a in parser._actions if a.dest != "help"}


def test_run_pixel_takes_every_option_of_run_test_unchanged(monkeypatch):
    class Got(Exception):
        pass

    def grab(self, args=None, namespace=None):
        raise Got(self)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(Got) as info:
        run_test.main([])
    monkeypatch.undo()
    theirs, ours = _options(info.value.args[0]), _options(run_pixel.build_parser())
    assert len(theirs) >= 14
    for dest, spec in theirs.items():
        assert ours.get(dest) == spec, dest
    assert set(ours) - set(theirs) == {"patch", "frac", "normalise", "mask_root"}
    a = run_pixel.build_parser().parse_args(["--synthetic"])
    assert (a.patch, a.frac, a.normalise, a.mask_root) == (16, [2, 5], "none", None)
    a = run_pixel.build_parser().parse_args(["--synthetic", "--frac", "1", "2", "--patch", "8", "--normalise", "video"])
    assert (a.patch, a.frac, a.normalise) == (8, [1, 2], "video")
    for bad in (["--patch", "12"], ["--normalise", "frame"], ["--frac", "2"], ["--frac", "a", "b"]):
        with pytest.raises(SystemExit):
            run_pixel.build_parser().parse_args(["--synthetic"] + bad)


def test_run_pixel_refuses_more_than_one_rank_and_bad_fractions(monkeypatch, capsys):
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_pixel.main(["--synthetic"])
    assert "one GPU" in str(info.value.code) and capsys.readouterr().out == ""
    with pytest.raises(SystemExit) as info:
        run_pixel.main(["--synthetic", "--frac", "6", "5"])
    assert "--frac" in str(info.value.code)


def test_mask_root_subset_and_unknown_file_rules(tmp_path):
    root = tmp_path / "masks"
    root.mkdir()
    names = ["Test001", "Test002", "Test003"]
    np.save(root / "Test001.npy", np.ones((7, 4, 6), dtype=np.uint8))
    np.save(root / "Test003.npy", np.zeros((9, 4, 6), dtype=np.uint8))
    (root / "readme.txt").write_text("not a mask")
    got = run_pixel.masks_from_root(names, str(root))
    assert got[1] is None and got[0].shape == (7, 4, 6) and got[2].shape == (9, 4, 6) and got[0].all()
    np.save(root / "Test004.npy", np.zeros((3, 4, 6), dtype=np.uint8))          # matches no sub-video
    with pytest.raises(ValueError, match="Test004"):
        run_pixel.masks_from_root(names, str(root))


def test_synthetic_masks_are_deterministic_and_match_the_video_lengths():
    a, b = run_pixel.synthetic_masks(4, 12, 60, 90), run_pixel.synthetic_masks(4, 12, 60, 90)
    lens = [int(g.shape[0]) for g in run_test.synthetic_raw_sources(4, 12)[1]]
    assert [m.shape for m in a] == [(t, 60, 90) for t in lens] == [(12, 60, 90), (19, 60, 90), (26, 60, 90), (12, 60, 90)]
    flagged = total = 0
    for x, y in zip(a, b):
        assert x.dtype == np.uint8 and np.array_equal(x, y)
        for f in x:
            if f.any():                                                       # one rectangle: its bounding box is full
                ys, xs = np.nonzero(f.any(axis=1))[0], np.nonzero(f.any(axis=0))[0]
                assert f[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].all() and f.sum() == ys.size * xs.size
                flagged += 1
            total += 1
    assert 0 < flagged < total
    many = run_pixel.synthetic_masks(3, 200, 8, 8)
    share = np.mean([f.any() for m in many for f in m])
    assert 0.12 < share < 0.28                                                # "about a fifth"


def _records(maps_by_video, masks_by_video, frac=(2, 5)):
    """the result `evaluate_dataset_pixel` would give for these maps (pixel and patch map taken as one)"""
    rec = {"mask_videos": [], **{f"{g}_{k}": [] for g in ("pix", "patch") for k in ("m", "kth", "max_in", "max_out")}}
    for v, (maps, masks) in enumerate(zip(maps_by_video, masks_by_video)):
        if masks is None:
            for k in rec:
                if k != "mask_videos":
                    rec[k].append(None)
            continue
        rec["mask_videos"].append(v)
        ref = PC.batch_scores(maps, masks, *frac)
        for g in ("pix", "patch"):
            for k, val in ref.items():
                rec[f"{g}_{k}"].append(val)
    return rec


def test_pixel_level_auc_gives_none_with_a_note_for_an_empty_class():
    maps = PC.make_values("uniform", (10, 4, 4))
    for masks, word in ((np.zeros((10, 4, 4), np.uint8), "anomalous"), (np.ones((10, 4, 4), np.uint8), "normal")):
        out = Hn.pixel_level_auc(_records([maps], [masks]))
        assert out["auc_pixel"] is None and out["auc_pixel_patch"] is None and out["auc_frame_max"] is None
        assert word in out["note"] and out["n_anomalous"] + out["n_normal"] == 10 - Hn.DECIDABLE_IDX
    assert out["pointing"] == 1.0                                             # a full mask: nothing lies outside
    out = Hn.pixel_level_auc(_records([maps], [None]))
    assert out["auc_pixel"] is None and out["n_anomalous"] == out["n_normal"] == 0 and out["pointing"] is None
    with pytest.raises(ValueError):
        Hn.pixel_level_auc(_records([maps], [None]), normalise="frame")
    bad = maps.copy()
    bad[6, 0, 0] = np.inf
    mixed = np.zeros((10, 4, 4), np.uint8)
    mixed[5] = 1
    with pytest.raises(ValueError, match="finite"):
        Hn.pixel_level_auc(_records([bad], [mixed]))


def test_pixel_level_auc_is_the_criterion_and_video_normalisation_is_normalising_the_maps():
    cases = PC.criterion_cases()
    d = Hn.DECIDABLE_IDX
    vids = [(np.concatenate([m[:d], m]), np.concatenate([k[:d], k])) for m, k in cases[:3]]     # d frames to drop in front
    vids[1] = (vids[1][0] * np.float32(7.5), vids[1][1])                                       # videos on different scales
    maps_by_video, masks_by_video = [m for m, _ in vids] + [cases[3][0]], [k for _, k in vids] + [None]
    rec = _records(maps_by_video, masks_by_video)
    out = Hn.pixel_level_auc(rec)
    flat_maps = [f for m, _ in vids for f in m[d:]]
    flat_masks = [f for _, k in vids for f in k[d:]]
    want = PC.criterion_literal(flat_maps, flat_masks, 2, 5)
    assert abs(out["auc_pixel"] - want) <= 1e-12 and abs(out["auc_pixel_patch"] - want) <= 1e-12
    n_pos = sum(bool(f.any()) for f in flat_masks)
    assert (out["n_anomalous"], out["n_normal"]) == (n_pos, len(flat_masks) - n_pos)
    hits = [PC.kth_largest(a, k, 2, 5) for a, k in zip(flat_maps, flat_masks) if k.any()]
    assert out["pointing"] == np.mean([h[2] >= h[3] for h in hits])
    labels = np.array([bool(f.any()) for f in flat_masks])
    assert out["auc_frame_max"] == Hn.roc_auc(labels, np.array([f.max() for f in flat_maps], dtype=np.float64), pos_label=1)
    # "video": the same records against the criterion on maps divided by their video's largest (kept) value, in float64
    norm = Hn.pixel_level_auc(rec, normalise="video")
    scaled = [f for m, _ in vids for f in (m[d:].astype(np.float64) / m[d:].astype(np.float64).max())]
    want_n = PC.criterion_literal(scaled, flat_masks, 2, 5)
    assert abs(norm["auc_pixel"] - want_n) <= 1e-12 and norm["normalise"] == "video"
    rec_n = _records([m.astype(np.float64) / m[d:].astype(np.float64).max() for m in maps_by_video[:3]], masks_by_video[:3])
    plain = Hn.pixel_level_auc(rec_n)
    for key in ("auc_pixel", "auc_pixel_patch", "auc_frame_max", "pointing"):
        assert norm[key] == plain[key], key
    assert norm["auc_pixel"] != out["auc_pixel"]                              # the scales did matter
