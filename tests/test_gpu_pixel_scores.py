"""The pixel-level pass on the device (csrc/pixel_scores.hip, `ops.pixel_scores`, `harness.pixel_subvideo` /
`evaluate_dataset_pixel` / `pixel_level_auc`, the `run_pixel` entry) against the numpy
restatement of tests/pixel_cases.py.  The kernel does no floating-point arithmetic: its float outputs are stored map
values, so they are compared by VALUE EQUALITY with the restatement's (np.sort picks the same element up to the sign of
a zero), `m` exactly, and everything about the place in the batch, strides, alignment and repetition bit for bit."""
import json

import numpy as np
import pytest
import torch

import pixel_cases as PC
import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_pixel, run_test, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 7), (5, 3), (17, 23), (32, 32), (64, 64)]
FRACS = [(2, 5), (1, 1), (1, 4096)]
FLOATS = ("kth", "max_in", "max_out")


def _check(got, ref, what):
    """device dict against the restatement's arrays: m exactly, floats by value"""
    assert got["m"].dtype == torch.int32
    assert np.array_equal(got["m"].cpu().numpy(), ref["m"]), what
    for key in FLOATS:
        g = got[key].cpu().numpy()
        assert g.dtype == np.float32 and np.array_equal(g, ref[key]), (what, key, g, ref[key])
    assert np.array_equal(got["max_all"].cpu().numpy(), np.maximum(ref["max_in"], ref["max_out"])), what


def _bits(res):
    return torch.stack([res["m"]] + [res[k].view(torch.int32) for k in FLOATS])


def _stacked(shape, b=2):
    """every value kind x every mask kind at `shape`, b samples each, as one batch; with the reference per fraction"""
    combos = [(v, k) for v in PC.VALUE_KINDS for k in PC.MASK_KINDS]
    maps = np.concatenate([PC.case(v, k, (b,) + shape)[0] for v, k in combos])
    masks = np.concatenate([PC.case(v, k, (b,) + shape)[1] for v, k in combos])
    return combos, maps, masks


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_value_and_mask_kind(shape):
    combos, maps, masks = _stacked(shape)
    d_map, d_mask = torch.tensor(maps, device=DEV), torch.tensor(masks, device=DEV)
    for frac in FRACS:
        got = ops.pixel_scores(d_map, d_mask, frac)
        ref = {k: np.concatenate([PC.reference(v, mk, (2,) + shape, frac)[k] for v, mk in combos]) for k in ("m",) + FLOATS}
        _check(got, ref, (shape, frac))
        if frac == (1, 1):                                                    # the minimum over the mask
            has = ref["m"] > 0
            want = np.array([a[k != 0].min() if (k != 0).any() else -np.inf for a, k in zip(maps, masks)], dtype=np.float32)
            assert np.array_equal(got["kth"].cpu().numpy()[has], want[has])
        if frac == (1, 4096):                                                 # k = 1 while m <= 4096
            assert torch.equal(got["kth"], got["max_in"])
        # every float output is a stored value of its sample (or -inf for an empty set)
        for key in FLOATS:
            g = got[key].cpu().numpy()
            for i in range(len(maps)):
                assert g[i] in maps[i] or (g[i] == -np.inf and (ref["m"][i] == 0 or ref["m"][i] == maps[i].size)), (key, i)


def test_small_masks_take_the_expected_ranks():
    """m = 1, 2, 3, 5 at 2/5: k = 1, 1, 2, 2"""
    shape = (17, 23)
    for kind, k in (("m1", 1), ("m2", 1), ("m3", 2), ("m5", 2)):
        maps, masks = PC.case("uniform", kind, (2,) + shape)
        got = ops.pixel_scores(torch.tensor(maps, device=DEV), torch.tensor(masks, device=DEV))
        for i in range(2):
            inside = np.sort(maps[i][masks[i] != 0])[::-1]
            assert int(got["m"][i]) == inside.size == int(kind[1:]) and float(got["kth"][i]) == inside[k - 1]


@pytest.mark.parametrize("batch", [1, 2, 33])
@pytest.mark.parametrize("shape", [(17, 23), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batches(shape, batch):
    for values, masks in (("decimal", "p50"), ("uniform", "rect"), ("low_bits", "p05"), ("signs", "full"), ("range", "p50")):
        a, k = PC.case(values, masks, (batch,) + shape, 7)
        got = ops.pixel_scores(torch.tensor(a, device=DEV), torch.tensor(k, device=DEV))
        _check(got, PC.reference(values, masks, (batch,) + shape, (2, 5), 7), (values, masks))


def test_one_256x256_batch():
    for values, masks, frac in (("uniform", "p05", (2, 5)), ("decimal", "p50", (2, 5)), ("low_bits", "full", (1, 1)),
                                ("range", "rect", (2, 5)), ("equal", "full", (2, 5)), ("zeros", "empty", (2, 5)),
                                ("uniform", "p50", (1, 4096))):               # m > 4096: k = 8 or so, not the maximum
        a, k = PC.case(values, masks, (3, 256, 256), 3)
        got = ops.pixel_scores(torch.tensor(a, device=DEV), torch.tensor(k, device=DEV), frac)
        _check(got, PC.reference(values, masks, (3, 256, 256), frac, 3), (values, masks, frac))


@pytest.mark.parametrize("shape", [(17, 23), (32, 32), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_layouts_give_the_same_bits(shape):
    """batch strides of their own, a base one float / one byte off (the unaligned load paths), a bool mask: the bits of
    the plain contiguous call"""
    h, w = shape
    n, b = h * w, 5
    a, k = PC.case("decimal", "p50", (b,) + shape, 11)
    d_map, d_mask = torch.tensor(a, device=DEV), torch.tensor(k, device=DEV)
    base = ops.pixel_scores(d_map, d_mask)
    _check(base, PC.reference("decimal", "p50", (b,) + shape, (2, 5), 11), shape)
    want = _bits(base)

    def strided(t, pad, off):
        buf = torch.zeros(off + b * (n + pad) + 16, device=DEV, dtype=t.dtype)
        view = buf.as_strided((b, h, w), (n + pad, w, 1), off)
        view.copy_(t)
        return view
    for pad, off in ((4, 0), (3, 0), (0, 1), (8, 4), (5, 3)):
        assert torch.equal(_bits(ops.pixel_scores(strided(d_map, pad, off), d_mask)), want), ("map", pad, off)
        assert torch.equal(_bits(ops.pixel_scores(d_map, strided(d_mask, pad, off))), want), ("mask", pad, off)
        assert torch.equal(_bits(ops.pixel_scores(strided(d_map, pad, off), strided(d_mask, off, pad))), want), ("both", pad, off)
    assert torch.equal(_bits(ops.pixel_scores(d_map, d_mask != 0)), want)     # a bool mask
    assert torch.equal(_bits(ops.pixel_scores(d_map, strided(d_mask != 0, 3, 1))), want)
    assert torch.equal(_bits(ops.pixel_scores(d_map, d_mask)), want)          # the same launch again


@pytest.mark.parametrize("shape", [(17, 23), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_sample_scores_the_same_wherever_it_stands(shape):
    a, k = PC.case("decimal", "p50", (33,) + shape, 5)
    d_map, d_mask = torch.tensor(a, device=DEV), torch.tensor(k, device=DEV)
    alone = _bits(ops.pixel_scores(d_map[7:8], d_mask[7:8]))
    for pos in (0, 32):
        m2, k2 = d_map.clone(), d_mask.clone()
        m2[pos], k2[pos] = d_map[7], d_mask[7]
        assert torch.equal(_bits(ops.pixel_scores(m2, k2))[:, pos:pos + 1], alone), pos
    one, two = ops.pixel_scores(d_map, d_mask), ops.pixel_scores(d_map, d_mask)
    assert torch.equal(_bits(one), _bits(two))


def test_out_views_are_written_in_place():
    shape, b = (17, 23), 6
    a, k = PC.case("uniform", "p50", (b,) + shape, 2)
    d_map, d_mask = torch.tensor(a, device=DEV), torch.tensor(k, device=DEV)
    base = ops.pixel_scores(d_map, d_mask)
    flat = torch.full((4, 10), float("nan"), device=DEV)
    out = {"m": flat[0].view(torch.int32)[2:2 + b], "kth": flat[1, 2:2 + b], "max_in": flat[2, 2:2 + b], "max_out": flat[3, 2:2 + b]}
    got = ops.pixel_scores(d_map, d_mask, out=out)
    for key in out:
        assert got[key].data_ptr() == out[key].data_ptr() and torch.equal(got[key], base[key]), key
    assert torch.equal(flat[1:, 2:2 + b], torch.stack([base[key] for key in FLOATS]))
    assert bool(torch.isnan(flat[:, :2]).all()) and bool(torch.isnan(flat[:, 2 + b:]).all())        # nothing else written
    part = ops.pixel_scores(d_map, d_mask, out={"kth": out["kth"]})
    assert part["kth"].data_ptr() == out["kth"].data_ptr() and torch.equal(part["m"], base["m"])
    for bad in ({"nope": flat[0, :b]}, {"kth": flat[1, :b + 1]}, {"m": flat[0, :b]}, {"kth": flat[:, 0][:b]},
                {"kth": torch.zeros(b)}):
        with pytest.raises(ValueError):
            ops.pixel_scores(d_map, d_mask, out=bad)


@pytest.fixture(scope="module")
def model():
    m = A.get_twostream((12, 6), (3, 2), 64, 32, 2)
    m.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=32, k=2))
    m = m.to(DEV).eval()
    m.precision = "s16"
    return m


def test_evaluate_dataset_pixel_end_to_end(model):
    """2 sub-videos of 12 and 19 frames at 64 x 64, masks given at 60 x 90, the first sub-video without one"""
    size, patch, frac = 64, 16, (2, 5)
    videos, _ = run_test.synthetic_dataset(2, 12, size)
    src = run_pixel.synthetic_masks(2, 12, 60, 90)
    rec = Hn.evaluate_dataset_pixel(model, videos, [None, src[1]], "ped2", patch, frac, device=DEV, keep_maps=True)
    assert rec["n_frames"] == [12, 19] and rec["mask_videos"] == [1]
    for key in ("rgb_img_pred_records", "rgb_fea_comm_records", "op_img_pred_records", "op_fea_comm_records"):
        assert [len(r) for r in rec[key]] == [12, 19] and all(np.isfinite(r).all() for r in rec[key]), key
    names = [f"{g}_{k}" for g in ("pix", "patch") for k in ("m",) + FLOATS]
    for key in names + ["pixel_map", "patch_map", "mask"]:
        assert rec[key][0] is None and rec[key][1] is not None, key          # the sub-video without a mask: no pixel figure
    t, lc = 19, Hn.RGB_LEN_CLIP
    mask = rec["mask"][1]
    assert mask.shape == (t, size, size) and np.array_equal(mask, PC.resize_nearest(src[1], size, size))
    pooled = PC.pool_any(mask, patch)
    pix, pat = rec["pixel_map"][1], rec["patch_map"][1]
    assert pix.shape == (t, size, size) and pat.shape == (t, size // patch, size // patch) and pix.dtype == np.float32
    assert np.array_equal(pat.reshape(t, -1).max(axis=1), np.maximum(rec["patch_max_in"][1], rec["patch_max_out"][1]))
    for g, maps, mk in (("pix", pix, mask), ("patch", pat, pooled)):
        ref = PC.batch_scores(maps[lc - 1:], mk[lc - 1:], *frac)             # frame t's prediction meets mask[t]
        for key in ("m",) + FLOATS:
            got = rec[f"{g}_{key}"][1]
            assert got.shape == (t,) and got.dtype == ref[key].dtype
            assert np.array_equal(got[lc - 1:], ref[key]), (g, key)
            assert (got[:lc - 1] == got[lc - 1]).all(), (g, key)              # the head repeats frame len_clip - 1
        assert ref["m"].max() > 0 and ref["m"].min() == 0
    for i in range(lc - 1):
        assert np.array_equal(pix[i], pix[lc - 1])
    # the fixed-order PSNR record is the pixel pass's own: 10 log10(1 / mean of the pixel map) within fp32 rounding
    psnr = 10 * np.log10(1.0 / pix.astype(np.float64).reshape(t, -1).mean(axis=1))
    assert np.abs(psnr - rec["rgb_img_pred_records"][1]).max() <= 1e-3
    d = Hn.DECIDABLE_IDX
    for normalise in ("none", "video"):
        out = Hn.pixel_level_auc(rec, normalise)
        scale = 1.0 if normalise == "none" else float(pix[d:].max())
        pscale = 1.0 if normalise == "none" else float(pat[d:].max())
        assert abs(out["auc_pixel"] - PC.criterion_literal(pix[d:].astype(np.float64) / scale, mask[d:], *frac)) <= 1e-12
        assert abs(out["auc_pixel_patch"] - PC.criterion_literal(pat[d:].astype(np.float64) / pscale, pooled[d:], *frac)) <= 1e-12
        anom = mask[d:].reshape(t - d, -1).any(axis=1)
        assert (out["n_anomalous"], out["n_normal"]) == (int(anom.sum()), int((~anom).sum()))
        assert out["auc_frame_max"] == Hn.roc_auc(anom, pix[d:].reshape(t - d, -1).max(axis=1).astype(np.float64) / scale, pos_label=1)
        hit = [pix[f][mask[f] != 0].max() >= pix[f][mask[f] == 0].max() for f in range(d, t) if mask[f].any()]
        assert out["pointing"] == np.mean(hit)
    # the maps never come to the host unless asked for
    rec2 = Hn.evaluate_dataset_pixel(model, videos[1:], [src[1]], "ped2", patch, frac, device=DEV)
    assert "pixel_map" not in rec2 and rec2["mask_videos"] == [0]
    for g in ("pix", "patch"):
        assert np.array_equal(rec2[f"{g}_m"][0], rec[f"{g}_m"][1])             # (a function of the masks alone)
    with pytest.raises(ValueError, match="frames"):
        Hn.evaluate_dataset_pixel(model, videos[:1], [src[1]], "ped2", patch, frac, device=DEV)   # 19 masks for 12 frames


def test_run_pixel_entry(capsys):
    run_pixel.main(["--synthetic", "--videos", "2", "--frames", "12", "--size", "64", "--n_embed", "32"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for key in ("auc_pixel", "auc_pixel_patch", "auc_frame_max", "pointing"):
        assert 0.0 <= line[key] <= 1.0, key
    assert line["fps"] > 0 and line["videos"] == 2 and line["predicted_frames"] == (12 - 4) + (19 - 4)
    assert line["frac"] == [2, 5] and line["patch"] == 16 and line["mask_videos"] == 2 and line["auc_note"] == "synthetic masks"
    assert line["n_anomalous"] + line["n_normal"] == (12 - 4) + (19 - 4) and 0.0 <= line["auc"] <= 1.0
