"""The region-based pass on the device (csrc/region_scores.hip, `ops.label_regions`, `ops.region_scores`,
`harness.region_subvideo` / `evaluate_dataset_region` / `region_level_auc`, the `run_region` entry; DESIGN.md section
5.24) against the flood-fill restatement of tests/region_cases.py.  Every output is an integer: every comparison is
equality."""
import json

import numpy as np
import pytest
import torch

import region_cases as RC
import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_region, run_test, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("n_px", "n_comp", "n_fp", "hit")


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _labels(masks, min_area=1, connectivity=8):
    pairs = [RC.label_regions(m, min_area, connectivity) for m in masks]
    return np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.int32)


def _check_labels(masks, min_area, connectivity, what):
    got = ops.label_regions(_dev(masks), min_area, connectivity)
    want, count = _labels(masks, min_area, connectivity)
    assert got["labels"].dtype == torch.uint8 and got["count"].dtype == torch.int32
    assert np.array_equal(got["count"].cpu().numpy(), count), (what, got["count"].tolist(), count.tolist())
    assert np.array_equal(got["labels"].cpu().numpy(), want), what
    return got


def _check_scores(maps, labels, thr, what, **kw):
    iou = kw.pop("iou", (1, 10))
    got = ops.region_scores(_dev(maps), _dev(labels), _dev(np.asarray(thr, dtype=np.float32)), iou, **kw)
    want = RC.batch_scores(maps, labels, thr, num=iou[0], den=iou[1], **kw)
    for key in KEYS:
        assert got[key].dtype == torch.int32 and tuple(got[key].shape) == want[key].shape
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (what, key, got[key].tolist(), want[key].tolist())
    return got


def _bits(res):
    return torch.stack([res[k] for k in KEYS])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_every_picture_as_a_mask_and_as_a_map(connectivity):
    """the shapes at which labelling can go wrong: the picture's own components, then a smooth map and the picture's 0 / 1
    map against the picture's regions"""
    for name, pic in RC.pictures().items():
        h, w = pic.shape
        masks = np.stack([pic.astype(np.uint8) * 200, (~pic).astype(np.uint8)])
        for min_area in (1, 3):
            _check_labels(masks, min_area, connectivity, (name, min_area))
        labels, _ = _labels(masks, 1, connectivity)
        ones = np.stack([pic, pic]).astype(np.float32)
        _check_scores(ones, labels, [1.0, 0.5, 0.0, 2.0], (name, "0/1"), connectivity=connectivity)
        smooth = RC.smooth_maps(2, h, w, 3, seed=h * w)
        _check_scores(smooth, labels, [0.3, 0.5, 0.7], (name, "smooth"), connectivity=connectivity)
        _check_scores(smooth, labels, [0.5], (name, "min_area"), min_area=4, connectivity=connectivity, iou=(1, 4))


def test_values_and_thresholds():
    """>= at a stored value, -0.0 against +0.0, negatives, infinities and NaN (never detected, as a value and as a
    threshold); T = 1 and T = 65 with repeated and unsorted thresholds"""
    inf, nan = np.inf, np.nan
    kinds = np.array([0.0, -0.0, -1.0, inf, -inf, nan, 0.25, 1e-40, 0.75], dtype=np.float32)
    rng = np.random.default_rng(8)
    maps = kinds[rng.integers(0, len(kinds), (3, 5, 7))]
    masks = (rng.random((3, 5, 7)) < 0.3).astype(np.uint8)
    labels, _ = _labels(masks)
    thr = np.array([0.0, -0.0, 0.25, inf, -inf, nan, -1.0, 1e-40, 0.75, np.nextafter(np.float32(0.25), np.float32(1))], dtype=np.float32)
    got = _check_scores(maps, labels, thr, "values")
    n_px = got["n_px"].cpu().numpy()
    assert np.array_equal(n_px[:, 0], n_px[:, 1])                             # -0.0 and +0.0 are one threshold
    assert (n_px[:, 5] == 0).all()                                            # a NaN threshold detects nothing
    assert np.array_equal(n_px[:, 4], (~np.isnan(maps)).reshape(3, -1).sum(axis=1))       # -inf: everything but NaN
    assert np.array_equal(n_px[:, 3], (maps == inf).reshape(3, -1).sum(axis=1))
    assert np.array_equal(n_px[:, 2] - n_px[:, 9], (maps == 0.25).reshape(3, -1).sum(axis=1))          # >= includes equality
    _check_scores(maps, labels, [0.25], "T = 1")
    many = np.concatenate([thr, thr[::-1], rng.permutation(np.linspace(-1.5, 1.5, 45).astype(np.float32))])
    assert many.size == 65
    got = _check_scores(maps, labels, many, "T = 65")
    assert torch.equal(_bits(got)[:, :, :10], _bits(got)[:, :, 10:20].flip(-1))           # a repeated threshold repeats its column


def test_match_boundary():
    amap = np.zeros((1, 8, 12), np.float32)
    amap[0, 1, 1:11] = 1.0                                                    # a 10-pixel component ...
    amap[0, 4, 0:11] = 0.5                                                    # ... an 11-pixel one
    amap[0, 6:8, 0:2] = 0.5                                                   # and one far from every region
    lab = np.zeros((1, 8, 12), np.uint8)
    lab[0, 1, 5], lab[0, 4, 5] = 1, 2                                         # one-pixel regions
    got = _check_scores(amap, lab, [1.0, 0.5], "1 / 10")
    assert got["hit"].tolist() == [[1, 1]] and got["n_fp"].tolist() == [[0, 2]] and got["n_comp"].tolist() == [[1, 3]]
    got = _check_scores(amap, lab, [1.0, 0.5], "1 / 11", iou=(1, 11))
    assert got["hit"].tolist() == [[1, 3]] and got["n_fp"].tolist() == [[0, 1]]
    # one component matching two regions; two components matching one region
    amap = np.zeros((1, 6, 10), np.float32)
    amap[0, 1, 0:10] = 1.0
    amap[0, 4, 0:3] = amap[0, 4, 5:8] = 1.0
    lab = np.zeros((1, 6, 10), np.uint8)
    lab[0, 1, 0:4], lab[0, 1, 6:10], lab[0, 4, 0:8] = 1, 2, 3
    got = _check_scores(amap, lab, [1.0], "shared", iou=(3, 10))
    assert got["hit"].tolist() == [[7]] and got["n_fp"].tolist() == [[0]] and got["n_comp"].tolist() == [[3]]
    # min_area drops a component that would have matched: it detects nothing and is no false positive
    got = _check_scores(amap, lab, [1.0], "min_area", iou=(3, 10), min_area=4)
    assert got["hit"].tolist() == [[3]] and got["n_fp"].tolist() == [[0]] and got["n_comp"].tolist() == [[1]] and got["n_px"].tolist() == [[16]]


def test_ground_truth_region_counts():
    pics = RC.pictures()
    one = np.zeros((33, 31), bool)
    one[3:9, 4:20] = True
    masks = np.stack([pics["dots_32"], pics["dots_33"], one, np.zeros((33, 31), bool)]).astype(np.uint8)
    got = _check_labels(masks, 1, 8, "counts")
    assert got["count"].tolist() == [32, 33, 1, 0]
    lab = got["labels"].cpu().numpy()
    assert lab[0].max() == 32 and lab[1].max() == 32 and (lab[1] > 0).sum() == 32 and lab[1][pics["dots_33"]][-1] == 0
    smooth = RC.smooth_maps(4, 33, 31, 2, seed=9)
    res = _check_scores(smooth, lab, [0.2, 0.6], "up to 32 regions")
    own = _check_scores(masks.astype(np.float32), lab, [1.0], "every region by its own pixel")
    assert own["hit"][:, 0].tolist() == [-1, -1, 1, 0]                        # bit 31 is region 32's
    assert own["n_comp"][:, 0].tolist() == [32, 33, 1, 0] and own["n_fp"][:, 0].tolist() == [0, 1, 0, 0]
    # label values above 32 are background to the scores
    noisy = lab.copy()
    noisy[lab == 0] = np.random.default_rng(1).integers(33, 256, int((lab == 0).sum()))
    assert torch.equal(_bits(ops.region_scores(_dev(smooth), _dev(noisy), _dev(np.float32([0.2, 0.6])))), _bits(res))
    _check_scores(smooth, noisy, [0.2, 0.6], "labels above 32")


@pytest.fixture(scope="module")
def layout_case():
    b, h, w = 33, 17, 23
    maps, masks = RC.smooth_maps(b, h, w, 3, seed=12), RC.rectangles(b, h, w, 3, seed=13)
    labels, counts = _labels(masks)
    thr = np.float32([0.35, 0.5, 0.65])
    return maps, masks, labels, counts, thr, RC.batch_scores(maps, labels, thr)


@pytest.mark.parametrize("batch", [1, 2, 33])
def test_batches(layout_case, batch):
    maps, masks, labels, counts, thr, want = layout_case
    got = ops.region_scores(_dev(maps[:batch]), _dev(labels[:batch]), _dev(thr))
    for key in KEYS:
        assert np.array_equal(got[key].cpu().numpy(), want[key][:batch]), key
    lab = ops.label_regions(_dev(masks[:batch]))
    assert np.array_equal(lab["labels"].cpu().numpy(), labels[:batch]) and np.array_equal(lab["count"].cpu().numpy(), counts[:batch])


def test_layouts_give_the_same_bits(layout_case):
    """batch strides of their own, bases one float / one byte off, a bool mask, a chunked threshold list: the bits of the
    plain contiguous call"""
    maps, masks, labels, counts, thr, ref = layout_case
    b, (h, w) = 5, maps.shape[1:]
    n = h * w
    d_map, d_lab, d_mask, d_thr = _dev(maps[:b]), _dev(labels[:b]), _dev(masks[:b]), _dev(thr)
    want = _bits(ops.region_scores(d_map, d_lab, d_thr))
    assert np.array_equal(want.cpu().numpy(), np.stack([ref[k][:b] for k in KEYS]))

    def strided(t, pad, off):
        buf = torch.zeros(off + b * (n + pad) + 16, device=DEV, dtype=t.dtype)
        view = buf.as_strided((b, h, w), (n + pad, w, 1), off)
        view.copy_(t)
        return view
    for pad, off in ((4, 0), (3, 0), (0, 1), (8, 4), (5, 3)):
        assert torch.equal(_bits(ops.region_scores(strided(d_map, pad, off), d_lab, d_thr)), want), ("map", pad, off)
        assert torch.equal(_bits(ops.region_scores(d_map, strided(d_lab, pad, off), d_thr)), want), ("labels", pad, off)
        assert torch.equal(_bits(ops.region_scores(strided(d_map, pad, off), strided(d_lab, off, pad), d_thr)), want), ("both", pad, off)
        lab = ops.label_regions(strided(d_mask, pad, off), out={"labels": strided(torch.zeros_like(d_lab), off, pad)})
        assert torch.equal(lab["labels"], d_lab) and lab["count"].tolist() == counts[:b].tolist(), ("mask", pad, off)
    assert torch.equal(ops.label_regions(d_mask != 0)["labels"], d_lab)       # a bool mask
    off_thr = torch.zeros(4, device=DEV)
    off_thr[1:] = d_thr
    assert torch.equal(_bits(ops.region_scores(d_map, d_lab, off_thr[1:])), want)
    budget = ops.REGION_WORKSPACE_BUDGET
    try:                                                                      # one launch per threshold
        ops.REGION_WORKSPACE_BUDGET = 1
        assert torch.equal(_bits(ops.region_scores(d_map, d_lab, d_thr)), want)
    finally:
        ops.REGION_WORKSPACE_BUDGET = budget


def test_a_sample_scores_the_same_wherever_it_stands(layout_case):
    maps, masks, labels, counts, thr, ref = layout_case
    d_map, d_lab, d_mask, d_thr = _dev(maps), _dev(labels), _dev(masks), _dev(thr)
    alone = _bits(ops.region_scores(d_map[7:8], d_lab[7:8], d_thr))
    alone_lab = ops.label_regions(d_mask[7:8])["labels"]
    for pos in (0, 32):
        m2, l2, k2 = d_map.clone(), d_lab.clone(), d_mask.clone()
        m2[pos], l2[pos], k2[pos] = d_map[7], d_lab[7], d_mask[7]
        assert torch.equal(_bits(ops.region_scores(m2, l2, d_thr))[:, pos:pos + 1], alone), pos
        assert torch.equal(ops.label_regions(k2)["labels"][pos:pos + 1], alone_lab), pos
    one, two = ops.region_scores(d_map, d_lab, d_thr), ops.region_scores(d_map, d_lab, d_thr)
    assert torch.equal(_bits(one), _bits(two))


def test_out_views_are_written_in_place(layout_case):
    maps, masks, labels, counts, thr, ref = layout_case
    b, T = 6, len(thr)
    d_map, d_lab, d_mask, d_thr = _dev(maps[:b]), _dev(labels[:b]), _dev(masks[:b]), _dev(thr)
    base = ops.region_scores(d_map, d_lab, d_thr)
    flat = torch.full((4, b * T + 8), -5, device=DEV, dtype=torch.int32)
    out = {key: flat[i, 4:4 + b * T].view(b, T) for i, key in enumerate(KEYS)}
    got = ops.region_scores(d_map, d_lab, d_thr, out=out)
    for key in KEYS:
        assert got[key].data_ptr() == out[key].data_ptr() and torch.equal(got[key], base[key]), key
    assert bool((flat[:, :4] == -5).all()) and bool((flat[:, 4 + b * T:] == -5).all())      # nothing else written
    part = ops.region_scores(d_map, d_lab, d_thr, out={"hit": out["hit"]})
    assert part["hit"].data_ptr() == out["hit"].data_ptr() and torch.equal(part["n_fp"], base["n_fp"])
    for bad in ({"nope": out["hit"]}, {"hit": out["hit"].view(T, b)}, {"hit": torch.zeros((b, T), device=DEV)},
                {"hit": torch.zeros((b, 2 * T), device=DEV, dtype=torch.int32)[:, ::2]}):
        with pytest.raises(ValueError):
            ops.region_scores(d_map, d_lab, d_thr, out=bad)
    labels_out = torch.full((b + 2, 17, 23), 99, device=DEV, dtype=torch.uint8)
    count_out = torch.full((b + 2,), -5, device=DEV, dtype=torch.int32)
    lab = ops.label_regions(d_mask, out={"labels": labels_out[1:1 + b], "count": count_out[1:1 + b]})
    assert lab["labels"].data_ptr() == labels_out[1].data_ptr() and torch.equal(labels_out[1:1 + b], d_lab)
    assert count_out.tolist() == [-5] + counts[:b].tolist() + [-5] and bool((labels_out[0] == 99).all()) and bool((labels_out[-1] == 99).all())
    for bad in ({"labels": labels_out[:b].int()}, {"count": count_out[:b + 1]}, {"other": count_out[:b]}):
        with pytest.raises(ValueError):
            ops.label_regions(d_mask, out=bad)


def test_one_256x256_batch():
    """smooth random maps, 3 rectangles, 8 thresholds; 2 samples of the batch against the restatement"""
    b = 4
    maps, masks = RC.smooth_maps(b, 256, 256, 12, seed=3), RC.rectangles(b, 256, 256, 3, seed=4)
    thr = np.linspace(0.2, 0.9, 8).astype(np.float32)
    lab = ops.label_regions(_dev(masks))
    got = ops.region_scores(_dev(maps), lab["labels"], _dev(thr), (1, 10), 2)
    for i in (0, b - 1):
        want_lab, count = RC.label_regions(masks[i])
        assert int(lab["count"][i]) == count and np.array_equal(lab["labels"][i].cpu().numpy(), want_lab)
        want = RC.scores(maps[i], want_lab, thr, min_area=2)
        for key in KEYS:
            assert np.array_equal(got[key][i].cpu().numpy(), want[key]), (i, key)
        assert want["n_comp"].max() > 5
    assert int(got["n_comp"].min()) >= 0


@pytest.fixture(scope="module")
def model():
    m = A.get_twostream((12, 6), (3, 2), 64, 32, 2)
    m.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=32, k=2))
    m = m.to(DEV).eval()
    m.precision = "s16"
    return m


def test_evaluate_dataset_region_end_to_end(model):
    """2 sub-videos of 12 and 19 frames at 64 x 64 (the second longer than a batch, the first shorter), masks given at
    60 x 90, the first sub-video without one"""
    size, patch = 64, 16
    videos, _ = run_test.synthetic_dataset(2, 12, size)
    src = run_region.synthetic_region_masks(2, 12, 60, 90)
    src[1][8, 5:30, 10:50] = 1                                               # regions in consecutive frames: a track
    src[1][9, 8:28, 20:60] = 1
    values = Hn.region_thresholds(6)
    rec = Hn.evaluate_dataset_region(model, videos, [None, src[1]], "ped2", patch, values, device=DEV, keep_maps=True)
    assert rec["n_frames"] == [12, 19] and rec["mask_videos"] == [1]
    for key in ("rgb_img_pred_records", "rgb_fea_comm_records", "op_img_pred_records", "op_fea_comm_records"):
        assert [len(r) for r in rec[key]] == [12, 19] and all(np.isfinite(r).all() for r in rec[key]), key
    t, lc, d = 19, Hn.RGB_LEN_CLIP, Hn.DECIDABLE_IDX
    for key in ("pix_hit", "patch_n_fp", "pix_labels", "pixel_map", "mask"):
        assert rec[key][0] is None and rec[key][1] is not None, key
    mask = rec["mask"][1]
    assert np.array_equal(mask, Hn.resize_mask(torch.from_numpy(src[1]), (size, size)).numpy())
    pooled = Hn.pool_mask(torch.from_numpy(mask), patch).numpy()
    pix, pat = rec["pixel_map"][1], rec["patch_map"][1]
    assert pix.shape == (t, size, size) and pat.shape == (t, size // patch, size // patch) and pix.dtype == np.float32
    for g, maps, mk in (("pix", pix, mask), ("patch", pat, pooled)):
        thr = rec[f"{g}_thresholds"][1]
        assert np.array_equal(thr, values * np.float32(maps[lc - 1:].max())) and thr.dtype == np.float32     # one fp32 multiply
        labels, counts = _labels(mk)
        assert np.array_equal(rec[f"{g}_labels"][1][lc - 1:], labels[lc - 1:])
        assert np.array_equal(rec[f"{g}_gt_count"][1][lc - 1:], counts[lc - 1:]) and counts.max() >= 1
        frames = [lc - 1, 8, 9, t - 1] if g == "pix" else list(range(lc - 1, t))
        want = RC.batch_scores(maps[frames], labels[frames], thr)
        for key in KEYS:
            got = rec[f"{g}_{key}"][1]
            assert got.shape == (t, len(values)) and got.dtype == np.int32
            assert np.array_equal(got[frames], want[key]), (g, key)
            assert (got[:lc - 1] == got[lc - 1]).all(), (g, key)              # the head repeats frame len_clip - 1
    out = Hn.region_level_auc(rec)
    for key in ("rbdc", "tbdc", "rbdc_patch", "tbdc_patch"):
        assert 0.0 <= out[key] <= 1.0, key
    assert out["rbdc"] == Hn.region_curve_area(out["curves"]["fpr"], out["curves"]["rbdr"])
    assert out["tbdc_patch"] == Hn.region_curve_area(out["curves"]["fpr_patch"], out["curves"]["tbdr_patch"])
    assert out["n_frames"] == t - d and out["n_gt_regions"] == int(rec["pix_gt_count"][1][d:].sum()) > 0
    assert 1 <= out["n_tracks"] < out["n_gt_regions"] and out["track_note"] == Hn.REGION_TRACK_NOTE
    # the maps never come to the host unless asked for; "none" scales by t_max
    rec2 = Hn.evaluate_dataset_region(model, videos[1:], [src[1]], "ped2", patch, values, normalise="none", t_max=0.5, device=DEV)
    assert "pixel_map" not in rec2 and rec2["mask_videos"] == [0]
    assert np.array_equal(rec2["pix_thresholds"][0], values * np.float32(0.5))
    assert np.array_equal(rec2["pix_labels"][0], rec["pix_labels"][1])
    # a sub-video shorter than a batch
    rec3 = Hn.evaluate_dataset_region(model, videos[:1], [src[0]], "ped2", patch, values, connectivity=4, device=DEV, keep_maps=True)
    labels3, counts3 = _labels(Hn.pool_mask(torch.from_numpy(rec3["mask"][0]), patch).numpy(), 1, 4)
    want = RC.batch_scores(rec3["patch_map"][0][lc - 1:], labels3[lc - 1:], rec3["patch_thresholds"][0], connectivity=4)
    for key in KEYS:
        assert np.array_equal(rec3[f"patch_{key}"][0][lc - 1:], want[key]), key
    assert np.array_equal(rec3["patch_gt_count"][0][lc - 1:], counts3[lc - 1:]) and rec3["n_frames"] == [12]
    with pytest.raises(ValueError, match="frames"):
        Hn.evaluate_dataset_region(model, videos[:1], [src[1]], "ped2", patch, values, device=DEV)   # 19 masks for 12 frames
    with pytest.raises(ValueError, match="t_max"):
        Hn.evaluate_dataset_region(model, videos[:1], [src[0]], "ped2", patch, values, normalise="none", device=DEV)


def test_more_than_32_regions_raise_with_the_frame_and_a_hint(model):
    videos, _ = run_test.synthetic_dataset(1, 12, 64)
    mask = np.zeros((12, 64, 64), np.uint8)
    mask[7, ::4, ::8] = 1                                                     # 16 x 8 single pixels in frame 7
    with pytest.raises(ValueError, match=r"frame 7.*128 ground-truth regions.*--min_gt_area"):
        Hn.evaluate_dataset_region(model, videos, [mask], "ped2", 16, Hn.region_thresholds(2), device=DEV)
    rec = Hn.evaluate_dataset_region(model, videos, [mask], "ped2", 16, Hn.region_thresholds(2), min_gt_area=2, device=DEV)
    assert rec["pix_gt_count"][0].max() == 0 and rec["patch_gt_count"][0][7] == 1          # the pooled specks are one region


def test_run_region_entry(capsys, tmp_path):
    curves = tmp_path / "curves.npz"
    run_region.main(["--synthetic", "--videos", "2", "--frames", "12", "--size", "64", "--n_embed", "32", "--thresholds", "8",
                     "--out", str(curves)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for key in ("rbdc", "tbdc", "rbdc_patch", "tbdc_patch"):
        assert 0.0 <= line[key] <= 1.0, key
    assert line["fps"] > 0 and line["videos"] == 2 and line["predicted_frames"] == (12 - 4) + (19 - 4)
    assert line["iou"] == [1, 10] and line["alpha"] == [1, 10] and line["patch"] == 16 and line["thresholds"] == 8
    assert line["mask_videos"] == 2 and line["auc_note"] == "synthetic masks" and line["normalise"] == "video"
    assert line["n_frames"] == (12 - 4) + (19 - 4) and line["n_gt_regions"] >= line["n_tracks"] >= 1 and 0.0 <= line["auc"] <= 1.0
    assert "consecutive" in line["track_note"] and "curves" not in line and line["curves_file"] == str(curves)
    saved = np.load(curves)
    assert saved["fpr"].shape == saved["rbdr"].shape == saved["tbdr_patch"].shape == (8,) and saved["values"][-1] == 1.0
