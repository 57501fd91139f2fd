"""Anomaly localisation without a GPU: the float64 reference of the error maps on planted inputs, the argument checks
of the two C entries (decided before any HIP call), the frame assembly of `localise_subvideo` against
`assemble_records`, and the options of the `run_maps` entry."""
import argparse

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, harness as Hn, parallel, run_maps, run_test


def test_reference_one_wrong_pixel_gives_one_patch():
    g = torch.Generator().manual_seed(3)
    target = torch.rand(2, 3, 27, 21, generator=g) * 2 - 1
    pred = target.clone()
    pred[1, 2, 19, 9] += 0.5                                   # patch (2, 1) of sample 1 at patch 8: pw = 3 -> index 7
    ref = Hn.error_maps_reference(pred, target, 8)
    assert ref["patch_sum"].shape == (2, 4, 3) and ref["pixel"].shape == (2, 27, 21)
    assert ref["patch_sum"].dtype == torch.float64
    nz = ref["patch_sum"].nonzero().tolist()
    assert nz == [[1, 2, 1]]
    e2 = float(((target[1, 2, 19, 9].double() - pred[1, 2, 19, 9].double()) * 0.5) ** 2)
    assert abs(float(ref["patch_sum"][1, 2, 1]) - e2) <= 1e-15
    assert abs(float(ref["pixel"][1, 19, 9]) - e2 / 3) <= 1e-15 and int((ref["pixel"] != 0).sum()) == 1
    assert int(ref["worst_idx"][1]) == 7 and float(ref["worst"][1]) == float(ref["patch_mean"][1, 2, 1])
    assert int(ref["worst_idx"][0]) == 0 and float(ref["worst"][0]) == 0.0       # all equal: the lowest index
    assert float(ref["frame_sq"][0]) == 0.0 and abs(float(ref["frame_sq"][1]) - e2) <= 1e-15


def test_reference_ragged_patches_divide_by_the_true_count():
    pred = torch.zeros(1, 3, 27, 21)
    target = torch.ones(1, 3, 27, 21)                          # e^2 = 0.25 everywhere: every patch MEAN is 0.25
    ref = Hn.error_maps_reference(pred, target, 8)
    assert torch.equal(ref["patch_mean"], torch.full((1, 4, 3), 0.25, dtype=torch.float64))
    rows, cols = [8, 8, 8, 3], [8, 8, 5]
    want = torch.tensor([[0.25 * 3 * r * c for c in cols] for r in rows], dtype=torch.float64)
    assert torch.equal(ref["patch_sum"][0], want)
    assert int(ref["worst_idx"][0]) == 0


def test_reference_psnr_is_psnr_per_sample():
    g = torch.Generator().manual_seed(5)
    pred = torch.tanh(torch.randn(3, 3, 27, 21, generator=g)).double()
    target = (torch.rand(3, 3, 27, 21, generator=g) * 2 - 1).double()
    for patch in (8, 16, 32):
        ref = Hn.error_maps_reference(pred, target, patch)
        assert float((ref["psnr"] - Hn.psnr_per_sample(pred, target)).abs().max()) <= 1e-12


def test_patch_count():
    lib = _lib.load()
    assert lib.ammc_error_maps_patch_count(27, 21, 8) == 12
    assert lib.ammc_error_maps_patch_count(256, 256, 16) == 256
    for bad in ((0, 21, 8), (27, -1, 8), (27, 21, 0), (27, 21, 12), (27, 21, 64)):
        assert lib.ammc_error_maps_patch_count(*bad) == 0, bad


def test_entry_refuses_bad_arguments_without_a_device():
    """integer stand-ins for the pointers: every refusal is decided before anything touches the device.  Refusals only:
    a call that passed the checks would launch on these addresses"""
    lib = _lib.load()
    B, C, H, W = 2, 3, 27, 21
    ok = dict(pred=0x100000, ps=(C * H * W, H * W, W), target=0x200000, ts=(C * H * W, H * W, W), b=B, c=C, h=H, w=W, patch=8,
              patch_sum=0x300000, ps_bs=12, patch_mean=0x400000, pixel=0x500000, px_bs=H * W, frame_sq=0x600000,
              worst=0x700000, worst_idx=0x800000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ammc_error_maps_f32(a["pred"], *a["ps"], a["target"], *a["ts"], a["b"], a["c"], a["h"], a["w"], a["patch"],
                                       a["patch_sum"], a["ps_bs"], a["patch_mean"], a["pixel"], a["px_bs"], a["frame_sq"],
                                       a["worst"], a["worst_idx"], None)
    for name in ("pred", "target", "patch_sum", "patch_mean", "frame_sq", "worst", "worst_idx"):
        assert call(**{name: None}) == -1, name
    for name in ("b", "c", "h", "w"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    for key in ("ps", "ts"):
        assert call(**{key: (C * H * W, H * W, W - 1)}) == -1                    # row stride < w
        assert call(**{key: (C * H * W, H * W - 1, W)}) == -1                    # channel stride < the plane
        assert call(**{key: (C * H * W - 1, H * W, W)}) == -1                    # batch stride < the sample
        assert call(**{key: (C * H * 32, H * 32 - 12, 32)}) == -1                # padded rows: the plane is (h - 1) * 32 + w
    assert call(ps_bs=11) == -1                                                  # < ph * pw
    assert call(px_bs=H * W - 1) == -1
    assert call(pred=0x100002) == -1                                             # not 4-byte aligned
    assert call(c=5, ps=(5 * H * W, H * W, W), ts=(5 * H * W, H * W, W)) == -2
    for patch in (0, 4, 12, 64):
        assert call(patch=patch) == -2, patch
    # a frame wider than 65535 column chunks of the grid (64 quads of 4 pixels at patch 8, 32 at patch 16 / 32)
    for patch, w in ((8, 4 * 64 * 65535), (16, 4 * 32 * 65535)):
        wide = dict(b=1, c=1, h=1, patch=patch, ps_bs=w, px_bs=w + 4)
        assert call(w=w + 1, ps=(w + 1, w + 1, w + 1), ts=(w + 1, w + 1, w + 1), **wide) == -2


@pytest.mark.parametrize("t", [7, 20])
def test_frame_assembly_fills_as_assemble_records(t):
    batches = Hn.subvideo_batches(t)
    assert batches == ([(0, 3)] if t == 7 else [(0, 16)])
    rng = np.random.default_rng(t)
    ph, pw = 2, 3
    for batches in (batches, Hn.subvideo_batches(t, batch=2)):                  # several batches, the last one short
        parts, scores = [], []
        for s, e in batches:
            b = e - s
            sc = {"rgb_psnr": rng.random(b, dtype=np.float32), "op_psnr": rng.random(b, dtype=np.float32),
                  "rgb_comm": np.float32(rng.random()), "op_comm": np.float32(rng.random())}
            scores.append(sc)
            parts.append(dict(sc, rgb_patch=rng.random((b, ph, pw), dtype=np.float32),
                              op_patch=rng.random((b, ph, pw), dtype=np.float32),
                              rgb_worst_idx=rng.integers(0, 6, b).astype(np.int32),
                              op_worst_idx=rng.integers(0, 6, b).astype(np.int32)))
        want = Hn.assemble_records(t, batches, scores)
        got = Hn.assemble_localised(t, batches, parts)
        for key in want:
            assert got[key].shape == (t,) and np.array_equal(got[key], want[key]), key
        assert got["rgb_patch"].shape == (t, ph, pw) and got["rgb_worst_idx"].dtype == np.int32
        clip = np.concatenate([p["rgb_patch"] for p in parts])
        assert np.array_equal(got["rgb_patch"][Hn.RGB_LEN_CLIP - 1:], clip)
        for i in range(Hn.RGB_LEN_CLIP - 1):                                     # the head copies frame len_clip - 1
            assert np.array_equal(got["rgb_patch"][i], clip[0])
        clip = np.concatenate([p["op_patch"] for p in parts])
        assert np.array_equal(got["op_patch"][Hn.OP_LEN_CLIP - 1:t - 1], clip)
        assert np.array_equal(got["op_patch"][t - 1], clip[-1]) and np.array_equal(got["op_patch"][0], clip[0])
        idx = np.concatenate([p["op_worst_idx"] for p in parts])
        assert got["op_worst_idx"][t - 1] == idx[-1] and got["op_worst_idx"][1] == idx[0]


def test_run_maps_parser_patch_values():
    p = run_maps.build_parser()
    a = p.parse_args(["--synthetic", "--maps_dir", "m"])
    assert a.maps_dir == "m" and a.patch == 16 and a.pixel_maps is False
    for v in (8, 16, 32):
        a = p.parse_args(["--synthetic", "--maps_dir", "m", "--patch", str(v), "--pixel_maps"])
        assert a.patch == v and a.maps_dir == "m" and a.pixel_maps is True
    for v in ("4", "12", "64", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["--synthetic", "--maps_dir", "m", "--patch", v])
    with pytest.raises(SystemExit):
        p.parse_args(["--synthetic"])                          # the maps folder is what the entry is for


def _options(parser):
    return {a.dest: (tuple(a.option_strings), a.default, a.type, tuple(a.choices) if a.choices else None, a.nargs, a.const)
            for a in parser._actions if a.dest != "help"}


def test_run_maps_takes_every_option_of_run_test_unchanged(monkeypatch):
    """`run_maps` repeats run_test's model and data-source options (run_test builds its parser inside `main`): every
    one of them must exist in `run_maps` with the same flags, default, type and choices - the two cannot drift apart
    unnoticed - and `run_maps` adds exactly its three"""
    class Got(Exception):
        pass

    def grab(self, args=None, namespace=None):
        raise Got(self)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(Got) as info:
        run_test.main([])
    monkeypatch.undo()
    theirs, ours = _options(info.value.args[0]), _options(run_maps.build_parser())
    assert len(theirs) >= 14
    for dest, spec in theirs.items():
        assert ours.get(dest) == spec, dest
    assert set(ours) - set(theirs) == {"maps_dir", "patch", "pixel_maps"}


def test_run_maps_refuses_more_than_one_rank(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_maps.main(["--synthetic", "--maps_dir", str(tmp_path / "maps")])
    assert "one GPU" in str(info.value.code)
    assert not (tmp_path / "maps").exists() and capsys.readouterr().out == ""
