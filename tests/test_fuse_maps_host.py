"""The fused localisation maps without a device: `harness.fuse_maps_reference` and
`harness.fuse_coefficients` against the loop restatements of tests/fuse_cases.py, the argument checks of `ops.fuse_maps`,
the C entry's refusals, the options of `run_localise`, and a constructed example in which fusing the channels changes the
pixel-level verdict."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import fuse_cases as FC
import pixel_cases as PC
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, parallel, run_localise, run_pixel, run_test


@pytest.mark.parametrize("h,w", [(8, 8), (17, 23), (40, 72)])
def test_reference_equals_the_loop_restatement(h, w):
    src, coef = FC.make_sources(h, w, 4)
    for n_ch, radius, patch in ((1, 0, 8), (2, 1, 16), (3, 4, 32), (4, 4, 8), (4, 2, 16)):
        want = FC.fuse_loops(src[:n_ch], FC.CELLS[:n_ch], coef[:n_ch], radius, patch, h, w)
        got = Hn.fuse_maps_reference([torch.from_numpy(s) for s in src[:n_ch]], FC.CELLS[:n_ch], torch.from_numpy(coef[:n_ch]),
                                     radius, patch)
        for key in ("raw", "pixel", "patch_mean", "frame_max"):
            assert got[key].dtype == torch.float64 and tuple(got[key].shape) == want[key].shape, key
            np.testing.assert_allclose(got[key].numpy(), want[key], rtol=1e-13, atol=0, err_msg=f"{key} {n_ch} {radius} {patch}")


def test_reference_clamps_the_coarse_grid_and_normalises_by_the_count():
    """17 x 23 in cells of 8: rows 16 and columns 16..22 read the LAST cell; a constant map stays constant up to the edge"""
    one = torch.ones(1, 17, 23)
    grid = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]])
    got = Hn.fuse_maps_reference([one, grid], (1, 8), [0.0, 1.0], 0, 8)
    raw = got["raw"][0]
    assert raw[0, 0] == 1 and raw[7, 15] == 2 and raw[8, 7] == 3 and raw[16, 22] == 4 and raw[16, 0] == 3 and raw[0, 22] == 2
    flat = Hn.fuse_maps_reference([3.0 * one], (1,), [1.0], 4, 16)
    assert torch.equal(flat["pixel"], 3.0 * one.double()) and torch.equal(flat["patch_mean"], torch.full((1, 2, 2), 3.0, dtype=torch.float64))


def test_fuse_coefficients_equal_their_fp32_restatement():
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(1, 5))
        w = rng.random(n).astype(np.float32) * 3
        mx = (rng.random(n).astype(np.float32) * np.float32(1e-3)) ** 2
        mx[rng.random(n) < 0.3] = 0.0                                         # a channel that is zero everywhere
        sc = rng.random(n).astype(np.float32) * 100
        got = Hn.fuse_coefficients(w.tolist(), torch.from_numpy(mx), "video")
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), FC.coefficients(w, mx, "video"))
        assert (got.numpy()[mx == 0] == 0).all() and np.isfinite(got.numpy()).all()
        assert np.array_equal(Hn.fuse_coefficients(torch.from_numpy(w), torch.from_numpy(mx), "video").numpy(), got.numpy())
        assert np.array_equal(Hn.fuse_coefficients(w, None, "none", sc).numpy(), FC.coefficients(w, None, "none", sc))
        assert np.array_equal(Hn.fuse_coefficients(w, torch.from_numpy(mx), "none").numpy(), w)
    assert Hn.fuse_coefficients([1, 2], torch.tensor([0.0, 4.0])).tolist() == [0.0, 0.5]
    for bad in (dict(weights=[1, 2], maxima=None), dict(weights=[1, 2], maxima=torch.ones(3)),
                dict(weights=[1, 2], maxima=None, normalise="none", scales=[1.0]), dict(weights=[1], maxima=torch.ones(1), normalise="frame")):
        with pytest.raises(ValueError):
            Hn.fuse_coefficients(**bad)


def test_fusion_weights_are_checked():
    assert Hn.check_fusion_weights([[1, 0, 0, 0]]) == [[1.0, 0.0, 0.0, 0.0]]
    assert Hn.check_fusion_weights([(1, 0), (0.5, 2)]) == [[1.0, 0.0], [0.5, 2.0]]
    for bad in ([], [[1, 1, 1, 1, 1]], [[1, -1]], [[0, 0, 0]], [[1, 0]] * 9, [[1, 0], [1]], [[float("nan"), 1]], [["x"]], 3, [1, 0, 0, 0]):
        with pytest.raises(ValueError):
            Hn.check_fusion_weights(bad)
    assert Hn.FUSE_CHANNELS == ("rgb_err", "op_err", "rgb_commit", "op_commit") and Hn.FUSE_CELLS == (1, 1, 8, 8)


def test_wrapper_refuses_before_loading_the_device():
    a, g, cf = torch.zeros(2, 16, 24), torch.zeros(2, 2, 3), torch.ones(2)
    with pytest.raises(ValueError, match="GPU"):
        ops.fuse_maps([a, g], (1, 8), cf)                                     # CPU tensors
    for srcs, cells in (([], ()), ([a] * 5, (1,) * 5), ([a.double()], (1,)), ([a[0]], (1,)), ([a.numpy()], (1,)), ([a, g], (1,)),
                        ([a, g], (1, 0)), ([a, g], (1, "x")), ([a, g], (1, 4)), ([a, g[:1]], (1, 8)), ([a, torch.zeros(2, 3, 3)], (1, 8)),
                        ([a, torch.zeros(2, 2, 5)], (1, 8)), (a, (1,))):
        with pytest.raises(ValueError):
            ops.fuse_maps(srcs, cells, torch.ones(max(1, len(cells))))
    with pytest.raises(ValueError, match="contiguous"):
        ops.fuse_maps([torch.zeros(2, 16, 48)[:, :, ::2], g], (1, 8), cf)     # pixel stride 2
    with pytest.raises(ValueError, match="contiguous"):
        ops.fuse_maps([torch.zeros(16 * 24 + 10).as_strided((2, 16, 24), (10, 24, 1)), g], (1, 8), cf)     # batch stride < a sample
    for coef in (torch.ones(3), torch.ones(2).double(), torch.ones(4)[::2], [1.0, 1.0], torch.ones(1, 2)):
        with pytest.raises(ValueError, match="coef"):
            ops.fuse_maps([a, g], (1, 8), coef)
    for radius in (-1, 9, 1.0, "2", True):
        with pytest.raises(ValueError, match="radius"):
            ops.fuse_maps([a, g], (1, 8), cf, radius)
    for patch in (0, 4, 12, 64):
        with pytest.raises(ValueError, match="patch"):
            ops.fuse_maps([a, g], (1, 8), cf, 0, patch)
    for out in ({"nope": a}, {"pixel": torch.zeros(2, 16, 25)}, {"pixel": a.double()}, {"patch_mean": torch.zeros(2, 1, 1)},
                {"frame_max": torch.zeros(3)}, {"frame_max": torch.zeros(4)[::2]}, {"pixel": torch.zeros(2, 16, 48)[:, :, ::2]}):
        with pytest.raises(ValueError, match="out"):
            ops.fuse_maps([a, g], (1, 8), cf, 0, 16, out)
    assert ops.FUSE_MAX_CHANNELS == 4 and ops.FUSE_MAX_RADIUS == 8 and ops.FUSE_TILE == (32, 64)


def test_entry_refuses_bad_arguments_without_a_device():
    """integer stand-ins for the device pointers: every refusal is decided before anything touches the device.  Refusals
    only: a call that passed the checks would launch on these addresses"""
    lib = _lib.load()
    assert hasattr(lib, "ammc_fuse_maps_f32") and "ammc_fuse_maps_f32" in _lib.SIGNATURES
    assert lib.ammc_abi_version() == _lib.ABI_VERSION == 42
    H, W, B = 17, 23, 2
    ok = dict(src=[0x100000, 0x200000, 0x300000], bs=[H * W, H * W, 4], gh=[H, H, 2], gw=[W, W, 2], cell=[1, 1, 8], coef=0x400000,
              b=B, h=H, w=W, radius=2, patch=16, pixel=0x500000, px_bs=H * W, pm=0x600000, pm_bs=4, fmax=0x700000, ws=0x800000)

    def call(**kw):
        a = dict(ok, **kw)
        n = len(a["src"])
        arrays = [(ctypes.c_void_p * max(n, 1))(*a["src"]), (ctypes.c_int64 * max(n, 1))(*a["bs"]), (ctypes.c_int32 * max(n, 1))(*a["gh"]),
                  (ctypes.c_int32 * max(n, 1))(*a["gw"]), (ctypes.c_int32 * max(n, 1))(*a["cell"])]
        return lib.ammc_fuse_maps_f32(*(ctypes.addressof(x) for x in arrays), a.get("n_ch", n), a["coef"], a["b"], a["h"], a["w"],
                                      a["radius"], a["patch"], a["pixel"], a["px_bs"], a["pm"], a["pm_bs"], a["fmax"], a["ws"], None)
    for name in ("coef", "pixel", "pm", "fmax", "ws"):
        assert call(**{name: None}) == -1, name
        assert call(**{name: ok[name] + 2}) == -1, name                      # not 4-byte aligned
    assert call(src=[0x100000, None, 0x300000]) == -1 and call(src=[0x100002, 0x200000, 0x300000]) == -1
    assert call(n_ch=0) == -1 and call(n_ch=5) == -1
    for name in ("b", "h", "w"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(radius=-1) == -1 and call(radius=9) == -1
    for patch in (0, 4, 12, 64):
        assert call(patch=patch) == -1, patch
    assert call(cell=[1, 0, 8]) == -1 and call(cell=[1, 1, 4]) == -1         # a 2 x 2 grid is not 17 x 23 in cells of 4
    assert call(gh=[H, H, 4]) == -1 and call(gw=[W, W, 1]) == -1 and call(gh=[H, H - 1, 2]) == -1 and call(gh=[H, H, 0]) == -1
    assert call(bs=[H * W - 1, H * W, 4]) == -1 and call(bs=[H * W, H * W, 3]) == -1
    assert call(px_bs=H * W - 1) == -1 and call(pm_bs=3) == -1
    assert call(h=1 << 15, w=(1 << 13) + 1, gh=[1 << 15] * 2 + [1 << 12], gw=[(1 << 13) + 1] * 2 + [1 << 10], bs=[1 << 40] * 3,
                px_bs=1 << 40, pm_bs=1 << 40) == -2                          # h * w > 2^28
    with pytest.raises(_lib.AmmcHipError):
        _lib.check(call(radius=9), "fuse_maps")


def _options(parser):
    return {a.dest: (tuple(a.option_strings), a.default, a.type, tuple(a.choices) if a.choices else None, a.nargs, a.const)
            for a in parser._actions if a.dest != "help"}


def test_run_localise_takes_every_option_of_run_test_and_the_mask_source_of_run_pixel(monkeypatch):
    class Got(Exception):
        pass

    def grab(self, args=None, namespace=None):
        raise Got(self)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(Got) as info:
        run_test.main([])
    monkeypatch.undo()
    theirs, ours, pixel = _options(info.value.args[0]), _options(run_localise.build_parser()), _options(run_pixel.build_parser())
    for dest, spec in theirs.items():
        assert ours.get(dest) == spec, dest
    assert ours["mask_root"] == pixel["mask_root"] and ours["patch"] == pixel["patch"] and ours["frac"] == pixel["frac"]
    assert set(ours) - set(theirs) == {"weights", "radius", "normalise", "scales", "patch", "frac", "no_region", "thresholds", "spacing",
                                       "iou", "alpha", "min_area", "min_gt_area", "connectivity", "mask_root", "out"}
    a = run_localise.build_parser().parse_args(["--synthetic"])
    assert (a.weights, a.radius, a.normalise, a.scales, a.no_region) == ("1,0,0,0;1,1,0,0;1,1,1,1", 2, "video", None, False)
    assert run_localise.parse_weights(a.weights) == [[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]]


def test_run_localise_refuses_bad_options_and_more_than_one_rank(monkeypatch, capsys):
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_localise.main(["--synthetic"])
    assert "one GPU" in str(info.value.code) and capsys.readouterr().out == ""
    for argv, word in ((["--weights", "1,1,1,1,1"], "--weights"),                       # 5 weights
                       (["--weights", "1,-1,0,0"], "--weights"),                        # a negative weight
                       (["--weights", "1,0,0,0;0,0,0,0"], "zeros"),                     # a setting of all zeros
                       (["--weights", ";".join(["1,0,0,0"] * 9)], "settings"),          # 9 settings
                       (["--radius", "9"], "--radius"), (["--radius", "-1"], "--radius"),
                       (["--weights", "1,x"], "--weights"), (["--weights", "1,0;1"], "--weights"),
                       (["--scales", "1,1,1,1"], "--normalise none"), (["--normalise", "none", "--scales", "1,1"], "--scales"),
                       (["--frac", "3", "2"], "--frac"), (["--iou", "11", "10"], "--iou"), (["--thresholds", "0"], "--thresholds")):
        with pytest.raises(SystemExit) as info:
            run_localise.main(["--synthetic"] + argv)
        assert word in str(info.value.code), argv
    for bad in (["--patch", "12"], ["--normalise", "frame"], ["--connectivity", "6"], ["--spacing", "cubic"]):
        with pytest.raises(SystemExit):
            run_localise.build_parser().parse_args(["--synthetic"] + bad)


def test_fusion_changes_the_pixel_level_verdict():
    """12 frames of 16 x 24, six with a ground-truth rectangle.  The rgb error peaks OUTSIDE the mask - and highest in the
    normal frames - while the flow error and both commit maps peak inside it: on the rgb channel alone the criterion ranks
    the normal frames above the anomalous ones, on the fused map it separates them"""
    t, h, w = 12, 16, 24
    rng = np.random.default_rng(11)
    masks = np.zeros((t, h, w), np.uint8)
    chans = [0.05 * rng.random((t, h, w)).astype(np.float32) for _ in range(2)] + [0.05 * rng.random((t, 2, 3)).astype(np.float32) for _ in range(2)]
    for f in range(t):
        if f % 2 == 0:                                                        # anomalous: the region fills coarse cell (1, 1)
            masks[f, 8:16, 8:16] = 1
            chans[0][f, 1:4, 18:22] += 0.5                                    # the rgb error looks elsewhere
            chans[1][f, 8:16, 8:16] += 1.0
            chans[2][f, 1, 1] += 1.0
            chans[3][f, 1, 1] += 1.0
        else:
            chans[0][f, 2:5, 2:6] += 1.0                                      # a normal frame with a large rgb error
    maxima = [float(c.max()) for c in chans]
    auc = {}
    for weights in ((1, 0, 0, 0), (1, 1, 1, 1)):
        coef = Hn.fuse_coefficients(weights, torch.tensor(maxima), "video")
        assert np.array_equal(coef.numpy(), FC.coefficients(weights, maxima, "video"))
        fused = Hn.fuse_maps_reference([torch.from_numpy(c) for c in chans], Hn.FUSE_CELLS, coef, 1, 8)["pixel"].numpy()
        s = PC.batch_scores(fused, masks, 2, 5)
        scores, labels = Hn.pixel_criterion_scores(s["m"], s["kth"], np.maximum(s["max_in"], s["max_out"]))
        auc[weights] = Hn.roc_auc(labels, scores, pos_label=1)
        assert auc[weights] == pytest.approx(PC.criterion_literal(fused, masks, 2, 5))
        pointing = (s["max_in"] >= s["max_out"])[s["m"] > 0].mean()
        assert pointing == (0.0 if weights == (1, 0, 0, 0) else 1.0)
    assert auc[(1, 0, 0, 0)] == 0.0 and auc[(1, 1, 1, 1)] == 1.0
