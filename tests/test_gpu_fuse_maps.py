"""The fused localisation maps on the device (csrc/fuse_maps.hip, `ops.fuse_maps`, `harness.fused_subvideo` /
`evaluate_dataset_fused`, the `run_localise` entry).  The kernel against
`harness.fuse_maps_reference` within bounds derived from each case (tests/fuse_cases.py), its bit-level promises as
equalities, the pass against `evaluate_dataset_pixel` / `evaluate_dataset_region` and the restatements of
tests/pixel_cases.py and tests/region_cases.py."""
import functools
import json

import numpy as np
import pytest
import torch

import fuse_cases as FC
import pixel_cases as PC
import region_cases as RC
import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_localise, run_region, run_test, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pixel", "patch_mean", "frame_max")


@functools.lru_cache(maxsize=None)
def _case(h, w):
    src, coef = FC.make_sources(h, w, 4)
    return src, coef, FC.torch_sources(src, DEV), torch.tensor(coef, device=DEV)


@functools.lru_cache(maxsize=None)
def _reference(h, w, n_ch, radius):
    """computed once per case and shared (`pixel` does not depend on the patch size)"""
    src, coef, _, _ = _case(h, w)
    ref = Hn.fuse_maps_reference([torch.from_numpy(s) for s in src[:n_ch]], FC.CELLS[:n_ch], torch.from_numpy(coef[:n_ch]), radius, 8)
    return ref["pixel"].numpy()


def _run(h, w, n_ch, radius, patch, **kw):
    _, _, d_src, d_coef = _case(h, w)
    return ops.fuse_maps(d_src[:n_ch], FC.CELLS[:n_ch], d_coef[:n_ch].contiguous(), radius, patch, **kw)


def _bits(res):
    return [res[k].clone() for k in KEYS]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("h,w,n_ch", FC.kernel_cases())
def test_kernel_against_the_reference(h, w, n_ch):
    for radius in FC.RADII:
        want = _reference(h, w, n_ch, radius)
        for patch in FC.PATCHES:
            got = _run(h, w, n_ch, radius, patch)
            ph, pw = -(-h // patch), -(-w // patch)
            assert [tuple(got[k].shape) for k in KEYS] == [(FC.BATCH, h, w), (FC.BATCH, ph, pw), (FC.BATCH,)]
            assert all(got[k].dtype == torch.float32 for k in KEYS)
            pixel = got["pixel"].cpu().numpy()
            diff = np.abs(pixel.astype(np.float64) - want)
            bound = FC.pixel_bound(n_ch, radius)
            err = float((diff[want > 0] / want[want > 0]).max())
            print(f"{h}x{w} n_ch {n_ch} radius {radius} patch {patch}: pixel rel err {err:.3e} (bound {bound:.3e})")
            assert (diff <= bound * want).all(), (radius, patch, err, bound)
            own = FC.patch_means(pixel, patch)
            pdiff = np.abs(got["patch_mean"].cpu().numpy().astype(np.float64) - own)
            pbound = FC.patch_bound(h, w, patch)
            print(f"    patch_mean rel err {float((pdiff / own).max()):.3e} (bound {float(pbound.min()):.3e} .. {float(pbound.max()):.3e})")
            assert (pdiff <= pbound[None] * own).all(), (radius, patch)
            assert torch.equal(got["frame_max"].view(torch.int32), got["pixel"].amax(dim=(1, 2)).view(torch.int32)), (radius, patch)


@pytest.mark.parametrize("h,w", FC.FRAME_SIZES)
def test_one_channel_of_weight_one_without_a_window_is_the_source(h, w):
    _, _, d_src, _ = _case(h, w)
    one = torch.ones(1, device=DEV)
    for patch in FC.PATCHES:
        got = ops.fuse_maps(d_src[:1], (1,), one, 0, patch)
        assert torch.equal(got["pixel"].view(torch.int32), d_src[0].view(torch.int32)), patch
        assert torch.equal(got["frame_max"], d_src[0].amax(dim=(1, 2)))


@pytest.mark.parametrize("h,w", FC.FRAME_SIZES)
def test_a_sample_alone_gives_the_bits_it_has_in_the_batch(h, w):
    _, _, d_src, d_coef = _case(h, w)
    for n_ch, radius, patch in ((4, 4, 16), (4, 1, 8), (3, 0, 32), (1, 4, 8)):
        full = _bits(_run(h, w, n_ch, radius, patch))
        again = _bits(_run(h, w, n_ch, radius, patch))
        assert _same(full, again), (n_ch, radius, patch)                      # two runs, the same bits
        for b in range(FC.BATCH):
            alone = ops.fuse_maps([s[b:b + 1] for s in d_src[:n_ch]], FC.CELLS[:n_ch], d_coef[:n_ch].contiguous(), radius, patch)
            assert _same(_bits(alone), [x[b:b + 1] for x in full]), (n_ch, radius, patch, b)
        # ... and in another place of another batch
        order = [2, 0, 1]
        moved = ops.fuse_maps([s[order].contiguous() for s in d_src[:n_ch]], FC.CELLS[:n_ch], d_coef[:n_ch].contiguous(), radius, patch)
        assert _same(_bits(moved), [x[order] for x in full]), (n_ch, radius, patch)


@pytest.mark.parametrize("h,w", FC.FRAME_SIZES)
def test_out_views_and_strided_sources_give_the_same_bits(h, w):
    _, _, d_src, d_coef = _case(h, w)
    n_ch, radius, patch, B = 4, 2, 16, FC.BATCH
    ph, pw = -(-h // patch), -(-w // patch)
    want = _bits(_run(h, w, n_ch, radius, patch))

    def strided(shape, pad, off, fill=-7.0):
        n = shape[1] * shape[2]
        buf = torch.full((off + B * (n + pad) + 16,), fill, device=DEV)
        return buf, buf.as_strided(shape, (n + pad, shape[2], 1), off)
    for pad, off in ((4, 0), (3, 0), (0, 1), (8, 4), (5, 3), (h * w, 2)):
        pbuf, pview = strided((B, h, w), pad, off)
        mbuf, mview = strided((B, ph, pw), off, pad % 3)
        fbuf = torch.full((B + 2,), -7.0, device=DEV)
        got = _run(h, w, n_ch, radius, patch, out={"pixel": pview, "patch_mean": mview, "frame_max": fbuf[1:1 + B]})
        assert got["pixel"].data_ptr() == pview.data_ptr() and got["patch_mean"].data_ptr() == mview.data_ptr()
        assert _same(_bits(got), want), (pad, off)
        for buf, view in ((pbuf, pview), (mbuf, mview)):                      # nothing written beside the views
            keep = torch.ones_like(buf, dtype=torch.bool)
            keep.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
            assert bool((buf[keep] == -7.0).all()), (pad, off)
        assert fbuf[0] == -7.0 and fbuf[-1] == -7.0
        srcs = []
        for s in d_src[:n_ch]:
            _, v = strided(tuple(s.shape), pad, off)
            v.copy_(s)
            srcs.append(v)
        assert _same(_bits(ops.fuse_maps(srcs, FC.CELLS[:n_ch], d_coef[:n_ch].contiguous(), radius, patch)), want), ("sources", pad, off)
    part = _run(h, w, n_ch, radius, patch, out={"frame_max": torch.empty(B, device=DEV)})
    assert _same(_bits(part), want)
    for bad in ({"nope": want[0]}, {"pixel": want[0].double()}, {"pixel": torch.empty((B, h, w + 1), device=DEV)},
                {"frame_max": torch.empty(2 * B, device=DEV)[::2]}, {"pixel": torch.empty((B, h, w))}):
        with pytest.raises(ValueError):
            _run(h, w, n_ch, radius, patch, out=bad)


def test_ceil_grids_and_a_zero_coefficient():
    """a coarse grid of ceil(H / 8) x ceil(W / 8) cells (17 x 23: 3 x 3) reads cell (y // 8, x // 8) without clamping, and a
    coefficient of zero takes its channel out bit for bit"""
    h, w = 17, 23
    _, _, d_src, d_coef = _case(h, w)
    grid = S.hashed_uniform("fuse:ceil", (FC.BATCH, 3, 3), 0, 1).to(DEV)
    coef = torch.tensor([0.5, 2.0], device=DEV)
    got = ops.fuse_maps([d_src[0], grid], (1, 8), coef, 1, 8)
    ref = Hn.fuse_maps_reference([d_src[0].cpu(), grid.cpu()], (1, 8), coef.cpu(), 1, 8)
    assert bool(((got["pixel"].cpu().double() - ref["pixel"]).abs() <= FC.pixel_bound(2, 1) * ref["pixel"]).all())
    assert ref["raw"][0, 16, 22] == 0.5 * d_src[0][0, 16, 22].double().cpu() + 2.0 * grid[0, 2, 2].double().cpu()
    zero = ops.fuse_maps([d_src[0], grid], (1, 8), torch.tensor([1.0, 0.0], device=DEV), 2, 16)
    one = ops.fuse_maps([d_src[0]], (1,), torch.ones(1, device=DEV), 2, 16)
    assert _same(_bits(zero), _bits(one))


def test_a_workspace_per_stream_one_for_cuda_and_cuda0_and_no_overlapping_out_samples():
    """`ops._workspace` under `fuse_maps`, `label_regions` and `region_scores`: two streams, two
    buffers each; tensors made under torch.device("cuda") and under "cuda:0" on one stream share one; the results are those
    of the default stream.  And the rule `error_maps` gained: `out` samples that overlap are refused."""
    B, h, w = 2, 17, 23
    g = torch.Generator().manual_seed(23)
    maps, mask = torch.rand((B, h, w), generator=g), torch.rand((B, h, w), generator=g) > 0.7
    values = torch.tensor([0.25, 0.5, 0.75])
    rkeys = ("n_px", "n_comp", "n_fp", "hit")

    def run(dev):
        mp = maps.to(dev)
        fused = ops.fuse_maps([mp], (1,), torch.ones(1, device=dev), 1, 8)
        labels = ops.label_regions(mask.to(dev))["labels"]
        scores = ops.region_scores(fused["pixel"], labels, values.to(dev))
        return [fused[k] for k in KEYS] + [labels] + [scores[k] for k in rkeys]
    base = run(DEV)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    idx = torch.device(DEV).index
    got, used = [], []
    for stream, dev in ((s1, DEV), (s2, torch.device("cuda")), (s1, torch.device("cuda")), (s2, DEV)):
        with torch.cuda.stream(stream):
            got.append(run(dev))
        used.append([ops._workspaces[(name, idx, stream.cuda_stream)].data_ptr() for name in ("fuse", "region")])
    torch.cuda.synchronize()
    assert int(base[-4].sum()) > 0 and int(base[3].max()) > 0                 # something was scored against some region
    for res in got:
        assert all(torch.equal(a, b) for a, b in zip(res, base))
    assert used[0] == used[2] and used[1] == used[3]                           # "cuda" and "cuda:0" on one stream: one workspace
    assert all(a != b for a, b in zip(used[0], used[1]))                       # two streams: two
    assert {k[1] for k in ops._workspaces} == {idx}                            # keyed by the device's index, never by its spelling
    pred, target = torch.rand((B, 3, h, w), generator=g).to(DEV), torch.rand((B, 3, h, w), generator=g).to(DEV)
    overlapping = torch.empty(h * w + 10, device=DEV).as_strided((B, h, w), (10, w, 1))
    with pytest.raises(ValueError, match="batch stride"):
        ops.error_maps(pred, target, 8, True, {"pixel": overlapping})
    apart = torch.empty(2 * h * w + 10, device=DEV).as_strided((B, h, w), (h * w + 10, w, 1))
    want = ops.error_maps(pred, target, 8, True)
    assert torch.equal(ops.error_maps(pred, target, 8, True, {"pixel": apart})["pixel"], want["pixel"])


# ---- the pass ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    m = A.get_twostream((12, 6), (3, 2), 64, 32, 2)
    m.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=32, k=2))
    m = m.to(DEV).eval()
    m.precision = "s16"
    return m


@pytest.fixture(scope="module")
def data():
    """2 sub-videos of 12 and 19 frames at 64 x 64 (the second longer than a batch), masks given at 60 x 90"""
    videos, _ = run_test.synthetic_dataset(2, 12, 64)
    src = run_region.synthetic_region_masks(2, 12, 60, 90)
    src[1][8, 5:30, 10:50] = 1                                               # regions in consecutive frames: a track
    src[1][9, 8:28, 20:60] = 1
    return videos, src


PIX = tuple(f"pix_{k}" for k in ("m", "kth", "max_in", "max_out"))
REG = tuple(f"pix_{k}" for k in ("n_px", "n_comp", "n_fp", "hit", "gt_count", "labels", "thresholds"))
RECORDS = ("rgb_img_pred_records", "rgb_fea_comm_records", "op_img_pred_records", "op_fea_comm_records")


def test_the_rgb_channel_alone_is_the_pixel_and_the_region_pass(model, data):
    """weights (1, 0, 0, 0), radius 0, normalise "none", scales 1: the fused map IS the rgb error map, so the pixel figures
    are `evaluate_dataset_pixel`'s and the region figures `evaluate_dataset_region`'s, bit for bit; the sub-video without
    a mask is left out of every setting"""
    videos, src = data
    masks = [None, src[1]]
    values = Hn.region_thresholds(6)
    kw = dict(radius=0, patch=16, thresholds=values, normalise="none", scales=(1, 1, 1, 1), device=DEV)
    rec = Hn.evaluate_dataset_fused(model, videos, masks, [(1, 0, 0, 0), (1, 0, 0, 0)], "ped2", **kw)
    assert rec["weights"] == [[1.0, 0.0, 0.0, 0.0]] * 2 and len(rec["settings"]) == 2
    pix = Hn.evaluate_dataset_pixel(model, videos, masks, "ped2", 16, (2, 5), device=DEV)
    reg = Hn.evaluate_dataset_region(model, videos, masks, "ped2", 16, values, device=DEV)
    for one in rec["settings"]:
        assert one["n_frames"] == [12, 19] and one["mask_videos"] == [1] and one["dataset"] == "ped2"
        assert set(pix) <= set(one) and set(reg) <= set(one)                  # every key of both results
        for key in PIX + REG + ("frame_max",):
            assert one[key][0] is None and one[key][1] is not None, key      # the None mask: left out
        for key in PIX:
            assert one[key][1].dtype == pix[key][1].dtype and np.array_equal(one[key][1], pix[key][1]), key
        for key in REG:
            assert one[key][1].dtype == reg[key][1].dtype and np.array_equal(one[key][1], reg[key][1]), key
        for key in RECORDS:
            # (the fixed-order PSNR of `ops.error_maps` repeats bit for bit; the other three come from the forward's own
            # epilogue sums, whose float atomics fix no order: two forwards agree to rounding)
            same = np.array_equal if key == "rgb_img_pred_records" else functools.partial(np.allclose, rtol=1e-5, atol=0)
            assert all(same(a, b) for a, b in zip(one[key], pix[key])), key
            assert one[key] is rec["settings"][0][key]                        # the record lists are shared
        got, want = Hn.pixel_level_auc(one), Hn.pixel_level_auc(pix)        # (the patch maps differ: a mean of means)
        for key in ("auc_pixel", "auc_frame_max", "pointing", "n_anomalous", "n_normal"):
            assert got[key] == want[key], key
        got, want = Hn.region_level_auc(one), Hn.region_level_auc(reg)
        assert (got["rbdc"], got["tbdc"]) == (want["rbdc"], want["tbdc"])
    assert rec["coef"][0] is None and np.array_equal(rec["coef"][1], np.float32([[1, 0, 0, 0]] * 2))
    # thresholds times t_max, as `region_subvideo` takes them with normalise="none"
    rec2 = Hn.evaluate_dataset_fused(model, videos[1:], masks[1:], [(1, 0, 0, 0)], "ped2", t_max=0.5, **kw)
    reg2 = Hn.evaluate_dataset_region(model, videos[1:], masks[1:], "ped2", 16, values, normalise="none", t_max=0.5, device=DEV)
    assert "pixel_map" not in rec2["settings"][0] and "channel_maps" not in rec2
    for key in REG:
        assert np.array_equal(rec2["settings"][0][key][0], reg2[key][0]), key
    assert np.array_equal(rec2["settings"][0]["pix_thresholds"][0], values * np.float32(0.5))
    # without the region criterion; a refused budget names the size
    rec3 = Hn.evaluate_dataset_fused(model, videos[1:], masks[1:], [(1, 0, 0, 0)], "ped2", region=False, **kw)
    assert "pix_hit" not in rec3["settings"][0] and np.array_equal(rec3["settings"][0]["pix_kth"][0], pix["pix_kth"][1])
    with pytest.raises(ValueError, match=r"\d+ bytes \(\d+\.\d MiB\)"):
        Hn.evaluate_dataset_fused(model, videos[1:], masks[1:], [(1, 0, 0, 0)], "ped2", budget=1 << 16, **kw)
    with pytest.raises(ValueError, match="frames"):
        Hn.evaluate_dataset_fused(model, videos[:1], [src[1]], [(1, 0, 0, 0)], "ped2", **kw)         # 19 masks for 12 frames


def test_kept_maps_follow_the_definitions_and_the_figures_follow_the_maps(model, data):
    videos, src = data
    weights = [(1, 0, 0, 0), (1, 1, 0, 0), (1, 2, 0.5, 0.25)]
    values, radius, patch, size = Hn.region_thresholds(6), 2, 16, 64
    rec = Hn.evaluate_dataset_fused(model, videos[1:], [src[1]], weights, "ped2", radius, patch, thresholds=values, device=DEV,
                                    keep_maps=True)
    t, lc = 19, Hn.RGB_LEN_CLIP
    chans = rec["channel_maps"][0]
    assert tuple(chans) == Hn.FUSE_CHANNELS
    assert [chans[n].shape for n in Hn.FUSE_CHANNELS] == [(t, size, size)] * 2 + [(t, size // 8, size // 8)] * 2
    assert all(c.dtype == np.float32 and np.isfinite(c).all() and c.min() >= 0 and c.max() > 0 for c in chans.values())
    maxima = np.float32([chans[n][lc - 1:].max() for n in Hn.FUSE_CHANNELS])
    assert np.array_equal(rec["channel_max"][0], maxima)
    mask = rec["settings"][0]["mask"][0]
    assert np.array_equal(mask, Hn.resize_mask(torch.from_numpy(src[1]), (size, size)).numpy())
    pooled = PC.pool_any(mask, patch)
    srcs = [torch.from_numpy(chans[n][lc - 1:]) for n in Hn.FUSE_CHANNELS]
    truth = {}
    for g, mk in (("pix", mask), ("patch", pooled)):
        pairs = [RC.label_regions(m) for m in mk]
        truth[g] = np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.int32)
    differ = []
    for gi, (wv, one) in enumerate(zip(weights, rec["settings"])):
        coef = FC.coefficients(wv, maxima, "video")
        assert np.array_equal(rec["coef"][0][gi], coef), gi
        pix, pat = one["pixel_map"][0], one["patch_map"][0]
        assert pix.shape == (t, size, size) and pat.shape == (t, size // patch, size // patch) and pix.dtype == np.float32
        ref = Hn.fuse_maps_reference(srcs, Hn.FUSE_CELLS, torch.from_numpy(coef), radius, patch)["pixel"].numpy()
        diff = np.abs(pix[lc - 1:].astype(np.float64) - ref)
        print(f"setting {gi}: fused pixel rel err {float((diff[ref > 0] / ref[ref > 0]).max()):.3e} (bound {FC.pixel_bound(4, radius):.3e})")
        assert (diff <= FC.pixel_bound(4, radius) * ref).all(), gi
        own = FC.patch_means(pix[lc - 1:], patch)
        assert (np.abs(pat[lc - 1:].astype(np.float64) - own) <= FC.patch_bound(size, size, patch)[None] * own).all(), gi
        assert np.array_equal(one["frame_max"][0], pix.reshape(t, -1).max(axis=1)), gi
        for g, maps, mk in (("pix", pix, mask), ("patch", pat, pooled)):
            want = PC.batch_scores(maps, mk, 2, 5)
            for key in ("m", "kth", "max_in", "max_out"):
                got = one[f"{g}_{key}"][0]
                assert got.dtype == want[key].dtype and np.array_equal(got[lc - 1:], want[key][lc - 1:]), (gi, g, key)
                assert (got[:lc - 1] == got[lc - 1]).all(), (gi, g, key)     # the head repeats frame len_clip - 1
            thr = one[f"{g}_thresholds"][0]
            assert thr.dtype == np.float32 and np.array_equal(thr, values * np.float32(maps[lc - 1:].max())), (gi, g)
            labels, counts = truth[g]
            assert np.array_equal(one[f"{g}_labels"][0][lc - 1:], labels[lc - 1:])
            assert np.array_equal(one[f"{g}_gt_count"][0][lc - 1:], counts[lc - 1:]) and counts.max() >= 1
            frames = [lc - 1, 8, 9, t - 1] if g == "pix" else list(range(lc - 1, t))
            rwant = RC.batch_scores(maps[frames], labels[frames], thr)
            for key in ("n_px", "n_comp", "n_fp", "hit"):
                got = one[f"{g}_{key}"][0]
                assert got.shape == (t, len(values)) and got.dtype == np.int32
                assert np.array_equal(got[frames], rwant[key]), (gi, g, key)
        fig, reg = Hn.pixel_level_auc(one), Hn.region_level_auc(one)
        scores, labels = Hn.pixel_criterion_scores(one["pix_m"][0][Hn.DECIDABLE_IDX:], one["pix_kth"][0][Hn.DECIDABLE_IDX:],
                                                   np.maximum(one["pix_max_in"][0], one["pix_max_out"][0])[Hn.DECIDABLE_IDX:])
        assert fig["auc_pixel"] == Hn.roc_auc(labels, scores, pos_label=1)
        assert all(0.0 <= reg[k] <= 1.0 for k in ("rbdc", "tbdc", "rbdc_patch", "tbdc_patch"))
        differ.append(pix)
    assert not np.array_equal(differ[0], differ[1]) and not np.array_equal(differ[1], differ[2])      # the weights matter


def test_run_localise_entry(capsys, tmp_path):
    out = tmp_path / "figures.npz"
    run_localise.main(["--synthetic", "--videos", "2", "--frames", "12", "--size", "64", "--n_embed", "32", "--thresholds", "8",
                       "--weights", "1,0,0,0;1,1,0,0;1,1,1,1", "--out", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["fps"] > 0 and line["videos"] == 2 and line["predicted_frames"] == (12 - 4) + (19 - 4) and 0.0 <= line["auc"] <= 1.0
    assert [s["weights"] for s in line["settings"]] == [[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]]
    for s in line["settings"]:
        assert set(s) == {"weights"} | set(run_localise.FIGURES)
        assert all(0.0 <= s[key] <= 1.0 for key in run_localise.FIGURES), s
    top = max(s["auc_pixel"] for s in line["settings"])
    first = next(i for i, s in enumerate(line["settings"]) if s["auc_pixel"] == top)
    assert line["best"]["index"] == first and line["best"]["weights"] == line["settings"][first]["weights"]
    assert line["radius"] == 2 and line["normalise"] == "video" and "consecutive" in line["track_note"]
    assert line["mask_videos"] == 2 and line["auc_note"] == "synthetic masks" and line["figures_file"] == str(out)
    saved = np.load(out)
    assert saved["weights"].shape == (3, 4) and saved["auc_pixel"].shape == (3,) and saved["rbdr_2"].shape == (8,)
    run_localise.main(["--synthetic", "--videos", "1", "--frames", "12", "--size", "64", "--n_embed", "32", "--no_region",
                       "--weights", "1,1", "--radius", "0", "--normalise", "none", "--scales", "1,4"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(line["settings"]) == 1 and "rbdc" not in line["settings"][0] and line["track_note"] is None and line["scales"] == [1.0, 4.0]
    assert line["channels"] == ["rgb_err", "op_err"] and line["region"] is False
