"""Region-based evaluation without a GPU: the restatement of tests/region_cases.py against a
second labelling built differently (and scipy's where it imports), the match rule against exact rationals, the curve
area, the tracks and the thresholds of `harness`, the argument checks of the C entries and of `ops.label_regions` /
`ops.region_scores` (decided before any HIP call), and the `run_region` options."""
import argparse
from fractions import Fraction

import numpy as np
import pytest
import torch

import region_cases as RC
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, parallel, run_pixel, run_region, run_test


def _union_find_label(fg: np.ndarray, connectivity: int):
    """the second witness: union-find over ALL neighbour pairs, then numbering by the smallest member"""
    h, w = fg.shape
    parent = list(range(h * w))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    for y in range(h):
        for x in range(w):
            if not fg[y, x]:
                continue
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and fg[yy, xx]:
                    a, b = find(y * w + x), find(yy * w + xx)
                    parent[max(a, b)] = min(a, b)
    roots = sorted({find(i) for i in range(h * w) if fg.flat[i]})
    number = {r: k + 1 for k, r in enumerate(roots)}
    comp = np.zeros((h, w), dtype=np.int32)
    for i in range(h * w):
        if fg.flat[i]:
            comp.flat[i] = number[find(i)]
    return comp


@pytest.mark.parametrize("connectivity", [4, 8])
def test_flood_fill_agrees_with_union_find_and_scipy_on_every_case(connectivity):
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    pics = RC.pictures()
    pics["smooth_64"] = RC.smooth_maps(1, 64, 64, 6)[0] >= 0.5
    for name, fg in pics.items():
        comp, sizes = RC.flood_label(fg, connectivity)
        assert np.array_equal(comp, _union_find_label(fg, connectivity)), name
        assert sizes == np.bincount(comp.ravel(), minlength=len(sizes) + 1)[1:].tolist(), name
        if ndimage is not None:
            structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
            assert np.array_equal(comp, ndimage.label(fg, structure)[0]), name
    counts = {name: len(RC.flood_label(pics[name], connectivity)[1]) for name in pics}
    assert counts["checkerboard"] == (32 if connectivity == 4 else 1)
    assert counts["spiral"] == counts["serpentine"] == counts["u"] == counts["comb"] == counts["ring"] == counts["full"] == 1
    assert counts["diagonal_blobs"] == (2 if connectivity == 4 else 1) and counts["empty"] == 0
    assert counts["dots_32"] == 32 and counts["dots_33"] == 33
    assert pics["spiral"].sum() > 100                                          # a long arm, not a blob


def test_label_regions_restated_caps_at_32_and_drops_small_components():
    lab, count = RC.label_regions(RC.pictures()["dots_33"].astype(np.uint8))
    assert count == 33 and lab.max() == 32 and (lab > 0).sum() == 32 and lab[RC.pictures()["dots_33"]][-1] == 0
    mask = np.zeros((6, 9), np.uint8)
    mask[0, 0] = mask[2, 2:5] = mask[4:6, 7:9] = 7
    lab, count = RC.label_regions(mask, min_area=3)
    assert count == 2 and lab[0, 0] == 0 and lab[2, 3] == 1 and lab[5, 8] == 2
    lab, count = RC.label_regions(mask, min_area=1)
    assert count == 3 and lab[0, 0] == 1 and lab[2, 3] == 2 and lab[5, 8] == 3


def test_match_rule_against_exact_rationals():
    for num, den in ((1, 10), (1, 1), (1, 2), (3, 7), (1, 4096), (4095, 4096)):
        for c in (1, 2, 9, 10, 11, 64):
            for g in (1, 3, 10, 50):
                for inter in range(0, min(c, g) + 1):
                    iou = Fraction(inter, c + g - inter)
                    assert RC.matches(c, g, inter, num, den) == (iou >= Fraction(num, den)), (c, g, inter, num, den)
    assert RC.matches(10, 1, 1, 1, 10) and not RC.matches(11, 1, 1, 1, 10)
    big = 1 << 22                                                              # the largest sample: products past 32 bits
    assert RC.matches(big, big, big, 4096, 4096) and not RC.matches(big, big, big - 1, 4096, 4096)


def test_restated_scores_on_a_hand_made_sample():
    amap = np.zeros((6, 12), np.float32)
    amap[1, 1:11] = 1.0                                                       # a 10-pixel component over a 1-pixel region
    amap[4, 0:11] = 0.5                                                       # an 11-pixel component over another
    lab = np.zeros((6, 12), np.uint8)
    lab[1, 5], lab[4, 5] = 1, 2
    got = RC.scores(amap, lab, [1.0, 0.5, 2.0])
    assert got["n_px"].tolist() == [10, 21, 0] and got["n_comp"].tolist() == [1, 2, 0]
    assert got["n_fp"].tolist() == [0, 1, 0] and got["hit"].tolist() == [1, 1, 0]
    got = RC.scores(amap, lab, [0.5], min_area=11)
    assert got["n_comp"].tolist() == [1] and got["n_fp"].tolist() == [1] and got["hit"].tolist() == [0]


def test_region_curve_area_on_hand_made_curves():
    cases = {
        "non-monotone": ([0.0, 0.25, 0.5, 0.75], [0.25, 0.75, 0.5, 1.0]),
        "duplicate fprs": ([0.25, 0.25, 0.5, 0.5, 0.0], [0.25, 0.5, 0.75, 0.5, 0.125]),
        "below one": ([0.125, 0.25], [0.5, 1.0]),
        "crossing one": ([0.5, 1.5], [0.25, 0.75]),
        "all at zero": ([0.0, 0.0, 0.0], [0.25, 0.75, 0.5]),
        "exactly one": ([0.5, 1.0, 3.0], [0.5, 0.75, 1.0]),
        "all past one": ([2.0, 4.0], [0.5, 1.0]),
        "unsorted": ([0.75, 0.0, 0.5, 0.25], [1.0, 0.25, 0.5, 0.75]),
    }
    want = {"below one": Fraction(1, 8) * Fraction(1, 4) + Fraction(1, 8) * Fraction(3, 4) + Fraction(3, 4),
            "crossing one": Fraction(1, 2) * Fraction(1, 8) + Fraction(1, 2) * Fraction(3, 8),
            "all at zero": Fraction(3, 4), "all past one": Fraction(1, 2) * Fraction(1, 4)}
    for name, (fpr, rate) in cases.items():
        got = Hn.region_curve_area(fpr, rate)
        assert got == float(RC.curve_area(fpr, rate)), name
        if name in want:
            assert got == float(want[name]), name
        assert 0.0 <= got <= 1.0
    assert Hn.region_curve_area(*cases["non-monotone"]) == Hn.region_curve_area(*cases["unsorted"])
    assert Hn.region_curve_area([], []) == 0.0
    rng = np.random.default_rng(3)
    for _ in range(50):
        fpr, rate = rng.integers(0, 12, 9) / 8.0, rng.integers(0, 9, 9) / 8.0
        assert abs(Hn.region_curve_area(fpr, rate) - float(RC.curve_area(fpr, rate))) <= 1e-15       # (a cut at 1 may divide by 7 / 8)


def _frames(*rows):
    """label images 1 x w from strings: a digit is a region's label, '.' the background"""
    return np.array([[[0 if ch == "." else int(ch) for ch in row]] for row in rows], dtype=np.uint8)


def test_region_tracks_split_merge_and_gap():
    split = _frames("1111111.", "11...22.", "1....2..")
    merge = _frames("1...22..", "11111...")
    gap = _frames("11......", "........", "11......")
    apart = _frames("1..2....", "1..2....", "1......2")                      # the second region moves away: a new track
    for frames, want, n in ((split, [[0], [0, 0], [0, 0]], 1), (merge, [[0, 0], [0]], 1), (gap, [[0], [], [1]], 2),
                            (apart, [[0, 1], [0, 1], [0, 2]], 3)):
        got, count = Hn.region_tracks(frames)
        ref, ref_count = RC.tracks(frames)
        assert count == ref_count == n and [g.tolist() for g in got] == [r.tolist() for r in ref] == want
    rng = np.random.default_rng(5)
    for _ in range(5):
        masks = (rng.random((6, 9, 9)) < 0.3).astype(np.uint8)
        labs = np.stack([RC.label_regions(m)[0] for m in masks])
        got, count = Hn.region_tracks(labs)
        ref, ref_count = RC.tracks(labs)
        assert count == ref_count and [g.tolist() for g in got] == [r.tolist() for r in ref]
    assert Hn.region_tracks(np.zeros((0, 4, 4), np.uint8)) == ([], 0)


def test_region_thresholds_both_spacings():
    lin = Hn.region_thresholds(64)
    assert lin.dtype == np.float32 and lin.shape == (64,) and lin[-1] == 1.0 and lin[0] == np.float32(1 / 64)
    assert np.array_equal(lin, np.array([i / 64 for i in range(1, 65)], dtype=np.float64).astype(np.float32))
    lin7 = Hn.region_thresholds(7)
    assert np.array_equal(lin7, np.array([np.float32(i / 7) for i in range(1, 8)])) and (np.diff(lin7) > 0).all()
    log = Hn.region_thresholds(8, "log", 1e-3)
    assert np.array_equal(log, np.array([np.float32(np.power(np.float64(1e-3), (8 - i) / 8)) for i in range(1, 9)]))
    assert log[-1] == 1.0 and log[0] > 1e-3 and (np.diff(log) > 0).all() and (log > 0).all()
    assert Hn.region_thresholds(1).tolist() == [1.0] and Hn.region_thresholds(1, "log").tolist() == [1.0]
    for bad in ((0,), (4, "cubic"), (4, "log", 0.0), (4, "log", 1.0), (2.5,)):
        with pytest.raises(ValueError):
            Hn.region_thresholds(*bad)


def _auc_record(maps, masks, thresholds, **kw):
    """the result `evaluate_dataset_region` would give for one sub-video (pixel and patch map taken as one)"""
    labs = [RC.label_regions(m) for m in masks]
    ref = RC.batch_scores(maps, [l for l, _ in labs], thresholds, **kw)
    rec = {"mask_videos": [0]}
    for g in ("pix", "patch"):
        for key, val in ref.items():
            rec[f"{g}_{key}"] = [val]
        rec[f"{g}_gt_count"] = [np.array([c for _, c in labs], dtype=np.int32)]
        rec[f"{g}_labels"] = [np.stack([l for l, _ in labs])]
    return rec


def test_region_level_auc_against_the_definitions():
    d, t = Hn.DECIDABLE_IDX, 9
    maps = RC.smooth_maps(t, 12, 12, 3, seed=2)
    masks = RC.rectangles(t, 12, 12, 2, seed=4)
    masks[d + 1] = 0                                                          # a gap: the tracks end there
    thr = Hn.region_thresholds(6) * np.float32(maps.max())
    rec = _auc_record(maps, masks, thr)
    out = Hn.region_level_auc(rec, alpha=(1, 2))
    labs = rec["pix_labels"][0][d:]
    ids, n_tracks = RC.tracks(labs)
    n_gt = int(sum(int(l.max()) for l in labs))
    assert out["n_frames"] == t - d and out["n_gt_regions"] == n_gt > 0 and out["n_tracks"] == n_tracks >= 2
    assert out["track_note"] == Hn.REGION_TRACK_NOTE and "consecutive" in out["track_note"]
    hit, n_fp = rec["pix_hit"][0][d:], rec["pix_n_fp"][0][d:]
    for j in range(len(thr)):
        det = sum((int(hit[f, j]) >> r) & 1 for f in range(t - d) for r in range(int(labs[f].max())))
        assert out["curves"]["rbdr"][j] == det / n_gt and out["curves"]["fpr"][j] == n_fp[:, j].sum() / (t - d)
        good = 0
        for k in range(n_tracks):
            members = [(f, r) for f in range(t - d) for r in range(len(ids[f])) if ids[f][r] == k]
            good += 2 * sum((int(hit[f, j]) >> r) & 1 for f, r in members) >= len(members)
        assert out["curves"]["tbdr"][j] == good / n_tracks
    assert out["rbdc"] == Hn.region_curve_area(out["curves"]["fpr"], out["curves"]["rbdr"]) == out["rbdc_patch"]
    assert out["tbdc"] == Hn.region_curve_area(out["curves"]["fpr"], out["curves"]["tbdr"]) and 0 <= out["rbdc"] <= 1
    empty = Hn.region_level_auc(_auc_record(maps, np.zeros_like(masks), thr))
    assert empty["rbdc"] is None and empty["tbdc"] is None and empty["rbdc_patch"] is None and "ground-truth" in empty["note"]
    assert empty["n_gt_regions"] == 0 and empty["n_tracks"] == 0 and empty["n_frames"] == t - d
    none = Hn.region_level_auc({"mask_videos": []})
    assert none["rbdc"] is None and none["n_frames"] == 0
    bad = _auc_record(maps, masks, thr)
    bad["pix_n_comp"][0][d + 2, 1] = -1
    with pytest.raises(ValueError, match="labelling"):
        Hn.region_level_auc(bad)


def test_entries_refuse_bad_arguments_without_a_device():
    """integer stand-ins for the pointers: every refusal is decided before anything touches the device.  Refusals only:
    a call that passed the checks would launch on these addresses"""
    lib = _lib.load()
    for name in ("ammc_label_regions_u8", "ammc_region_scores_f32", "ammc_region_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    H, W, B, T = 27, 21, 2, 5
    n = H * W
    assert lib.ammc_region_workspace_bytes(B, T, H, W) == B * T * 3 * n * 4
    assert lib.ammc_region_workspace_bytes(16, 64, 256, 256) == 16 * 64 * 3 * 65536 * 4                # past 32 bits
    for bad in ((0, T, H, W), (B, 0, H, W), (B, T, 0, W), (B, T, H, -1), (1, 1, 2048, 2049), (1 << 16, 1 << 15, 1, 1)):
        assert lib.ammc_region_workspace_bytes(*bad) == -1, bad
    ok = dict(map=0x100000, map_bs=n, lab=0x200000, lab_bs=n, b=B, h=H, w=W, thr=0x300000, t=T, num=1, den=10, min_area=1, conn=8,
              n_px=0x400000, n_comp=0x500000, n_fp=0x600000, hit=0x700000, out_rs=T, ws=0x800000, ws_bytes=B * T * 3 * n * 4)

    def scores(**kw):
        a = dict(ok, **kw)
        return lib.ammc_region_scores_f32(a["map"], a["map_bs"], a["lab"], a["lab_bs"], a["b"], a["h"], a["w"], a["thr"], a["t"],
                                          a["num"], a["den"], a["min_area"], a["conn"], a["n_px"], a["n_comp"], a["n_fp"],
                                          a["hit"], a["out_rs"], a["ws"], a["ws_bytes"], None)
    for name in ("map", "lab", "thr", "n_px", "n_comp", "n_fp", "hit", "ws"):
        assert scores(**{name: None}) == -1, name
    for name in ("b", "h", "w", "t", "min_area"):
        assert scores(**{name: 0}) == -1 and scores(**{name: -3}) == -1, name
    for conn in (0, 6, 9, -8):
        assert scores(conn=conn) == -1, conn
    for num, den in ((0, 10), (-1, 10), (11, 10), (1, 4097), (1, 0)):
        assert scores(num=num, den=den) == -1, (num, den)
    assert scores(h=2048, w=2049, map_bs=1 << 23, lab_bs=1 << 23, ws_bytes=1 << 50) == -1             # h * w > 2^22
    assert scores(h=65536, w=65536, map_bs=1 << 40, lab_bs=1 << 40, ws_bytes=1 << 60) == -1           # ... and past 32 bits
    assert scores(map_bs=n - 1) == -1 and scores(lab_bs=n - 1) == -1 and scores(out_rs=T - 1) == -1 and scores(map_bs=0) == -1
    for name in ("map", "thr", "n_px", "n_comp", "n_fp", "hit", "ws"):
        assert scores(**{name: ok[name] + 2}) == -1, name                    # not 4-byte aligned
    assert scores(ws_bytes=ok["ws_bytes"] - 1) == -1 and scores(ws_bytes=0) == -1
    assert scores(b=1 << 16, t=1 << 15, h=1, w=1, map_bs=1, lab_bs=1, out_rs=1 << 15, ws_bytes=1 << 60) == -2     # the grid

    okl = dict(mask=0x100000, mask_bs=n, b=B, h=H, w=W, min_area=1, conn=8, lab=0x200000, lab_bs=n, count=0x300000, ws=0x400000,
               ws_bytes=B * 3 * n * 4)

    def label(**kw):
        a = dict(okl, **kw)
        return lib.ammc_label_regions_u8(a["mask"], a["mask_bs"], a["b"], a["h"], a["w"], a["min_area"], a["conn"], a["lab"],
                                         a["lab_bs"], a["count"], a["ws"], a["ws_bytes"], None)
    for name in ("mask", "lab", "count", "ws"):
        assert label(**{name: None}) == -1, name
    for name in ("b", "h", "w", "min_area"):
        assert label(**{name: 0}) == -1 and label(**{name: -1}) == -1, name
    assert label(conn=5) == -1 and label(mask_bs=n - 1) == -1 and label(lab_bs=n - 1) == -1
    assert label(count=0x300002) == -1 and label(ws=0x400001) == -1 and label(ws_bytes=okl["ws_bytes"] - 4) == -1
    assert label(h=2048, w=2049, mask_bs=1 << 23, lab_bs=1 << 23, ws_bytes=1 << 50) == -1
    with pytest.raises(_lib.AmmcHipError):
        _lib.check(scores(num=0), "region_scores")


def test_wrappers_refuse_before_loading_the_device():
    a, k, t = torch.zeros(2, 5, 7), torch.zeros(2, 5, 7, dtype=torch.uint8), torch.tensor([0.5, 1.0])
    with pytest.raises(ValueError, match="GPU"):
        ops.region_scores(a, k, t)                                            # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        ops.label_regions(k)
    for bad_map, bad_lab in ((a.double(), k), (a, k.int()), (a, k != 0), (a[0], k[0]), (a, k[:, :4]), (a[:1], k), (a.numpy(), k)):
        with pytest.raises(ValueError):
            ops.region_scores(bad_map, bad_lab, t)
    for bad_t in (t.double(), t.reshape(1, 2), torch.zeros(0), [0.5], torch.zeros(4)[::2]):
        with pytest.raises(ValueError):
            ops.region_scores(a, k, bad_t)
    for iou in ((0, 10), (11, 10), (1, 4097), (1,), "x", 3):
        with pytest.raises(ValueError):
            ops.region_scores(a, k, t, iou)
    for kw in (dict(min_area=0), dict(min_area=1.5), dict(connectivity=6), dict(connectivity="8")):
        with pytest.raises(ValueError):
            ops.region_scores(a, k, t, **kw)
        with pytest.raises(ValueError):
            ops.label_regions(k, **kw)
    for bad_mask in (k.float(), k[0], k.int(), k.numpy()):
        with pytest.raises(ValueError):
            ops.label_regions(bad_mask)
    wide = torch.zeros(2, 5, 14)
    with pytest.raises(ValueError, match="contiguous"):
        ops.region_scores(wide[:, :, ::2], k, t)                              # pixel stride 2
    with pytest.raises(ValueError, match="contiguous"):
        ops.region_scores(a, torch.zeros(2, 7, 5, dtype=torch.uint8).transpose(1, 2), t)
    with pytest.raises(ValueError, match="contiguous"):
        ops.label_regions(torch.zeros(5 * 7 + 10, dtype=torch.uint8).as_strided((2, 5, 7), (10, 7, 1)))   # batch stride < H * W


def _options(parser):
    return {a.dest: (tuple(a.option_strings), a.default, a.type, tuple(a.choices) if a.choices else None, a.nargs, a.const)
            for a in parser._actions if a.dest != "help"}


def test_run_region_takes_every_option_of_run_test_and_the_mask_source_of_run_pixel(monkeypatch):
    class Got(Exception):
        pass

    def grab(self, args=None, namespace=None):
        raise Got(self)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(Got) as info:
        run_test.main([])
    monkeypatch.undo()
    theirs, ours, pixel = _options(info.value.args[0]), _options(run_region.build_parser()), _options(run_pixel.build_parser())
    assert len(theirs) >= 14
    for dest, spec in theirs.items():
        assert ours.get(dest) == spec, dest
    assert ours["mask_root"] == pixel["mask_root"] and ours["patch"] == pixel["patch"]
    assert set(ours) - set(theirs) == {"patch", "iou", "alpha", "thresholds", "spacing", "log_floor", "normalise", "t_max",
                                       "min_area", "min_gt_area", "connectivity", "mask_root", "out"}
    a = run_region.build_parser().parse_args(["--synthetic"])
    assert (a.patch, a.iou, a.alpha, a.thresholds, a.spacing, a.normalise, a.t_max) == (16, [1, 10], [1, 10], 64, "linear", "video", None)
    assert (a.min_area, a.min_gt_area, a.connectivity, a.mask_root, a.out) == (1, 1, 8, None, None)
    for bad in (["--patch", "12"], ["--normalise", "frame"], ["--iou", "2"], ["--connectivity", "6"], ["--spacing", "cubic"]):
        with pytest.raises(SystemExit):
            run_region.build_parser().parse_args(["--synthetic"] + bad)


def test_run_region_refuses_bad_options_and_more_than_one_rank(monkeypatch, capsys):
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_region.main(["--synthetic"])
    assert "one GPU" in str(info.value.code) and capsys.readouterr().out == ""
    for argv, word in ((["--iou", "11", "10"], "--iou"), (["--alpha", "0", "10"], "--alpha"), (["--normalise", "none"], "--t_max"),
                       (["--thresholds", "0"], "--thresholds"), (["--spacing", "log", "--log_floor", "1.5"], "floor")):
        with pytest.raises(SystemExit) as info:
            run_region.main(["--synthetic"] + argv)
        assert word in str(info.value.code), argv


def test_synthetic_region_masks_are_deterministic_rectangles():
    a, b = run_region.synthetic_region_masks(4, 12, 60, 90), run_region.synthetic_region_masks(4, 12, 60, 90)
    assert [m.shape for m in a] == [(12, 60, 90), (19, 60, 90), (26, 60, 90), (12, 60, 90)]
    for x, y in zip(a, b):
        assert x.dtype == np.uint8 and np.array_equal(x, y)
    many = run_region.synthetic_region_masks(3, 200, 24, 24)
    counts = [RC.label_regions(f)[1] for m in many for f in m]
    share = np.mean([c > 0 for c in counts])
    assert 0.12 < share < 0.28 and set(counts) == {0, 1, 2, 3}                # "about a fifth", one to three regions
    # the pixel-level entry's masks are what they were
    assert not np.array_equal(run_pixel.synthetic_masks(1, 12, 24, 24)[0], run_region.synthetic_region_masks(1, 12, 24, 24)[0])
