"""The SSIM / MSE pass (csrc/ssim.hip, `ops.ssim`, `harness.quality_subvideo`, the `run_quality` entry; DESIGN.md section
5.19) against `harness.ssim_reference` in float64 on the same tensors (tests/ssim_cases.py: four seeded recipes).

Gates (u = 2^-24).
  map, ssim_c, ssim   per case and quantity: the kernel's largest absolute error is at most 2 x the larger of the two fp32
                      witnesses' errors on that quantity and case, plus 4 u.  The witnesses are the reference's own
                      arithmetic (`ssim_reference(dtype=float32)`: the 2-D window through conv2d) and a separable fp32
                      restatement (tests/ssim_cases.py).  The `2 x envelope of fp32 witnesses` rule is tests/truth.py's: a
                      third summation order has independent rounding of the same size and the cancellation in
                      G(x^2) - mu^2 amplifies all three alike; 4 u covers the last roundings of a value of magnitude <= 1.
  sq                  a sum of non-negative terms: (depth + 3) u RELATIVE.  A term d^2 carries 3 u (the difference, twice
                      in the square, and the product's rounding).  The longest chain of dependent fp32 adds behind a
                      term is 2 (the thread's 4 rows, pairwise) + (c - 1) (the channels) + 6 (the xor tree over the 64
                      lanes) + 3 (the 4 waves in order) = c + 10; the tile partials are added in double (nothing visible
                      in fp32) and the total is rounded to fp32 once: depth = c + 11, i.e. (c + 14) u <= 1.1e-6.
What the header defines exactly (ssim from the returned ssim_c, psnr and mse from the returned sq, 1.0 where the window
sees pred == target) and everything about the ORDER of the additions (place in the batch, strides, alignment, map or
not, `out=` views, repeated launches, streams) is compared bit for bit.

Measured on an MI355X (largest over the cases of a recipe; kernel error / envelope of the two witnesses):
  recipe    map                   ssim_c                ssim
  random    3.8e-07 / 5.0e-07     1.1e-08 / 1.9e-08     5.0e-09 / 1.2e-08
  close     2.9e-06 / 1.4e-05     1.1e-07 / 1.4e-07     5.2e-08 / 1.2e-07
  smooth    2.4e-06 / 7.0e-06     1.0e-07 / 3.8e-07     5.8e-08 / 1.8e-07
  planted   1.7e-06 / 2.3e-06     3.6e-08 / 4.0e-08     1.2e-08 / 3.8e-08
  the largest error / gate of any case and quantity: 0.42;  sq: at most 9.6e-08 relative (gate 9.5e-07 at c = 2)."""
import functools
import json

import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_quality, run_test, synthetic as S

import ssim_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = ops.SSIM_TILE
U = 2.0 ** -24
SHAPES = [(1, 2, 5, 7), (1, 3, 8, 8), (3, 3, 27, 21), (2, 1, T, T), (2, 3, T + 1, T + 1), (5, 3, 40, 72), (2, 2, 64, 96),
          (1, 4, 16, 16)]
CASES = [(r, 2000 + 10 * i + j, s) for i, s in enumerate(SHAPES) for j, r in enumerate(K.RECIPES)
         if r != "planted" or (s[2] >= K.PLANT and s[3] >= K.PLANT)]
ORDER_CASES = [c for c in CASES if c[0] == "random"]
KEYS = ("ssim", "ssim_c", "sq", "mse", "psnr", "map")
nan = float("nan")


def _id(case):
    return f"{case[0]}-{'x'.join(map(str, case[2]))}"


@functools.lru_cache(maxsize=None)
def _dev(case):
    return tuple(t.to(DEV) for t in K.inputs(*case))


def _equal(a, b, keys=KEYS):
    for k in keys:
        if k in a and k in b:
            assert torch.equal(a[k], b[k]), k


def test_the_cases_cover_every_recipe_and_shape():
    assert {c[0] for c in CASES} == set(K.RECIPES) and {c[2] for c in CASES} == set(SHAPES)
    assert sum(c[0] == "planted" for c in CASES) >= 3 and ops.SSIM_TILE == A._lib.load().ammc_ssim_tile()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_against_fp64(case):
    pred, target = _dev(case)
    ref = K.reference(*case)
    w32, sep = K.witnesses(*case)
    got = ops.ssim(pred, target, map=True)
    b, c, h, w = case[2]
    assert got["ssim"].shape == (b,) and got["ssim_c"].shape == (b, c) and got["sq"].shape == (b,) and got["map"].shape == (b, h, w)
    for q in ("map", "ssim_c", "ssim"):
        truth = ref[q]
        err = float((got[q].double().cpu() - truth).abs().max())
        env = max(float((w32[q].double() - truth).abs().max()), float((sep[q].double() - truth).abs().max()))
        gate = 2 * env + 4 * U
        print(f"{_id(case)} {q}: kernel error {err:.3e}, witnesses' envelope {env:.3e}, gate {gate:.3e}")
        assert err <= gate, (q, err, env)
    rel = float(((got["sq"].double().cpu() - ref["sq"]).abs() / ref["sq"]).max())
    gate = (c + 11 + 3) * U
    print(f"{_id(case)} sq: relative error {rel:.3e}, gate {gate:.3e}")
    assert rel <= gate
    if case[0] == "planted":
        # numerator and denominator are the same bits wherever the whole window sees pred == target
        y, x = K.plant_origin(h, w)
        inner = got["map"][0, y + 11:y + K.PLANT - 11, x + 11:x + K.PLANT - 11]
        assert inner.numel() == 4 and bool((inner == 1.0).all())
        assert int((got["map"] == 1.0).sum()) >= (K.PLANT - 10) ** 2           # (5 pixels from the border are enough)


def _ssim_by_definition(ssim_c):
    v = ssim_c.cpu().numpy()
    out = np.empty(v.shape[0], dtype=np.float32)
    for b in range(v.shape[0]):
        s = np.float64(v[b, 0])
        for ch in range(1, v.shape[1]):
            s = s + np.float64(v[b, ch])
        out[b] = np.float32(s / np.float64(v.shape[1]))
    return torch.from_numpy(out)


@pytest.mark.parametrize("case", ORDER_CASES, ids=_id)
def test_exact_contracts_recomputed_from_the_returned_values(case):
    pred, target = _dev(case)
    got = ops.ssim(pred, target)
    assert "map" not in got
    assert torch.equal(got["ssim"].cpu(), _ssim_by_definition(got["ssim_c"]))
    n = float(case[2][1] * case[2][2] * case[2][3])
    assert torch.equal(got["mse"], 256.0 * got["sq"] / n)
    assert torch.equal(got["psnr"], 10.0 * torch.log10(4.0 * n / got["sq"]))
    # the frame PSNR of the scoring loop, from the fixed-order sum: 4 ulp of a value below 64 dB on top of sq's gate
    want = Hn.psnr_per_sample(pred.double(), target.double())
    assert float((got["psnr"].double() - want).abs().max()) <= 10 * np.log10(1 + 18 * U) + 4 * 2.0 ** -23 * 64


def _in_buffer(t, pad_b, pad_c, pad_h, pad_w, offset=0):
    """`t` [B,C,H,W] as a view inside a larger NaN-filled buffer (padded batch / channel / row strides, base `offset` floats in)"""
    b, c, h, w = t.shape
    n = (b + pad_b) * (c + pad_c) * (h + pad_h) * (w + pad_w)
    flat = torch.full((n + offset,), nan, device=t.device)
    v = flat[offset:].view(b + pad_b, c + pad_c, h + pad_h, w + pad_w)[:b, :c, :h, :w]
    v.copy_(t)
    return v


@pytest.mark.parametrize("case", ORDER_CASES, ids=_id)
def test_order_does_not_depend_on_batch_strides_alignment_or_map(case):
    pred, target = _dev(case)
    shape = case[2]
    base = ops.ssim(pred, target, map=True)
    _equal(base, ops.ssim(pred, target, map=True))                                       # two launches in a row
    _equal(base, ops.ssim(pred, target, map=False))                                      # without the map
    g = torch.Generator().manual_seed(11)
    for i in {0, shape[0] - 1}:                                                          # alone / at every place of a batch of 3
        alone = ops.ssim(pred[i:i + 1], target[i:i + 1], map=True)
        for pos in range(3):
            p3 = torch.tanh(torch.randn(3, *shape[1:], generator=g)).to(DEV)
            t3 = (torch.rand(3, *shape[1:], generator=g) * 2 - 1).to(DEV)
            p3[pos], t3[pos] = pred[i], target[i]
            three = ops.ssim(p3, t3, map=True)
            for k in KEYS:
                assert torch.equal(alone[k][0], three[k][pos]), (k, i, pos)
                assert torch.equal(alone[k][0], base[k][i]), (k, i)
    # views inside NaN-filled buffers: a channel-sliced tensor, row-padded tensors (rows w + 3 and w + 4 floats apart: one of
    # the two keeps every row 16-byte aligned, the other does not), padded batch strides, a base one float off 16 bytes
    for pads, off in (((1, 1, 2, 4), 0), ((1, 1, 2, 3), 0), ((0, 0, 0, 0), 1), ((2, 0, 1, 8), 1), ((0, 2, 0, 0), 0)):
        pv, tv = _in_buffer(pred, *pads, offset=off), _in_buffer(target, *pads, offset=(off + 2) % 4 if off else 0)
        assert pv.data_ptr() % 16 == 4 * off
        _equal(base, ops.ssim(pv, tv, map=True))
        _equal(base, ops.ssim(pv, target, map=True))                                     # mixed: one operand strided only
    # the targets of a batch are a slice of a longer sub-video: the same batch stride, another base
    longer = torch.full((shape[0] + 3,) + shape[1:], nan, device=DEV)
    longer[2:2 + shape[0]] = target
    _equal(base, ops.ssim(pred, longer[2:2 + shape[0]], map=True))


@pytest.mark.parametrize("case", ORDER_CASES, ids=_id)
def test_out_views_and_nothing_outside_them_is_written(case):
    pred, target = _dev(case)
    b, c, h, w = case[2]
    base = ops.ssim(pred, target, map=True)
    mbuf = torch.full((b + 2, h * w + 5), nan, device=DEV)
    bufs = {"ssim": torch.full((b + 2,), nan, device=DEV), "sq": torch.full((b + 2,), nan, device=DEV),
            "ssim_c": torch.full((b + 2, c), nan, device=DEV)}
    out = {k: v[1:b + 1] for k, v in bufs.items()}
    out["map"] = mbuf[1:b + 1, :h * w].unflatten(1, (h, w))                              # a batch stride of h w + 5
    got = ops.ssim(pred, target, map=True, out=out)
    _equal(base, got)
    for k in ("ssim", "sq", "ssim_c", "map"):
        assert got[k].data_ptr() == out[k].data_ptr()
    for k, v in bufs.items():
        assert bool(torch.isnan(v[[0, b + 1]]).all()) and not bool(torch.isnan(v[1:b + 1]).any()), k
    assert not bool(torch.isnan(mbuf[1:b + 1, :h * w]).any())
    assert bool(torch.isnan(mbuf[[0, b + 1]]).all()) and bool(torch.isnan(mbuf[:, h * w:]).all())
    mbuf.fill_(nan)                                                                      # without a map no map buffer is touched
    no_map = ops.ssim(pred, target, out={k: v for k, v in out.items() if k != "map"})
    assert "map" not in no_map and bool(torch.isnan(mbuf).all())
    _equal(base, no_map)
    with pytest.raises(ValueError, match="contiguous"):
        ops.ssim(pred, target, map=True, out={"map": torch.empty(b, h, 2 * w, device=DEV)[..., ::2]})
    with pytest.raises(ValueError, match="must be"):
        ops.ssim(pred, target, out={"ssim": torch.empty(b + 1, device=DEV)})


def test_two_streams_each_with_its_own_workspace():
    a, b = ORDER_CASES[-3], ORDER_CASES[-2]                                              # several tiles each
    base_a, base_b = ops.ssim(*_dev(a), map=True), ops.ssim(*_dev(b), map=True)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    got_a, got_b = [], []
    for _ in range(3):
        with torch.cuda.stream(s1):
            got_a.append(ops.ssim(*_dev(a), map=True))
        with torch.cuda.stream(s2):
            got_b.append(ops.ssim(*_dev(b), map=True))
    torch.cuda.synchronize()
    for g in got_a:
        _equal(base_a, g)
    for g in got_b:
        _equal(base_b, g)
    idx = torch.device(DEV).index
    w1, w2 = ops._workspaces[("ssim", idx, s1.cuda_stream)], ops._workspaces[("ssim", idx, s2.cuda_stream)]
    assert w1.data_ptr() != w2.data_ptr()


def test_nan_in_one_sample_reaches_that_sample_only():
    case = next(c for c in ORDER_CASES if c[2] == (5, 3, 40, 72))
    pred, target = (t.clone() for t in _dev(case))
    base = ops.ssim(pred, target, map=True)
    pred[2, 1, 17, 40] = nan
    got = ops.ssim(pred, target, map=True)
    for k in ("ssim", "sq", "mse", "psnr"):
        assert bool(torch.isnan(got[k][2])), k
    assert bool(torch.isnan(got["ssim_c"][2, 1])) and not bool(torch.isnan(got["ssim_c"][2, [0, 2]]).any())
    hit = torch.isnan(got["map"][2])
    assert int(hit.sum()) == 11 * 11 and bool(hit[12:23, 35:46].all())
    others = [0, 1, 3, 4]
    for k in KEYS:
        assert torch.equal(got[k][others], base[k][others]), k
    inf = ops.ssim(torch.full_like(pred, float("inf")), target)                          # non-finite inputs propagate
    assert not bool(torch.isfinite(inf["ssim"]).any()) and not bool(torch.isfinite(inf["sq"]).any())


def test_unsupported_channel_count_is_an_error():
    x = torch.zeros(1, 5, 16, 16, device=DEV)
    with pytest.raises(A._lib.AmmcHipError):
        ops.ssim(x, x)


@pytest.fixture(scope="module")
def model():
    m = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    m.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=256, k=2))
    m = m.to(DEV).eval()
    m.precision = "s16"
    return m


def test_quality_subvideo(model):
    t, size = Hn.RGB_LEN_CLIP + 20, 64
    (rgb, op), = run_test.synthetic_dataset(1, t, size)[0]
    rgb, op = rgb.to(DEV), op.to(DEV)
    preds = []
    rec = Hn.quality_subvideo(model, rgb, op, maps=True, predictions=preds)
    assert [(p[0], p[1]) for p in preds] == [(0, 16), (16, 21)]                          # two batches, the second one partial
    keys = {f"{st}_{k}" for st in ("rgb", "op") for k in ("ssim", "mse", "psnr", "comm", "ssim_map")}
    assert set(rec) == keys
    for st in ("rgb", "op"):
        lc = Hn.RGB_LEN_CLIP if st == "rgb" else Hn.OP_LEN_CLIP
        assert rec[f"{st}_ssim_map"].shape == (t, size, size) and rec[f"{st}_ssim_map"].dtype == np.float32
        for k in ("ssim", "mse", "psnr", "comm", "ssim_map"):
            a = rec[f"{st}_{k}"]
            assert a.shape[0] == t and np.isfinite(a).all(), (st, k)
            for i in range(lc - 1):
                assert np.array_equal(a[i], a[lc - 1]), (st, k, i)
    for k in ("ssim", "mse", "psnr", "comm", "ssim_map"):
        assert np.array_equal(rec[f"op_{k}"][t - 1], rec[f"op_{k}"][t - 2]), k
    assert np.abs(rec["rgb_ssim"]).max() <= 1.0 + 1e-6
    for s, e, rgb_pred, op_pred, fused in preds:
        for st, pred, frames, lc, fz in (("rgb", rgb_pred, rgb, Hn.RGB_LEN_CLIP, fused[0]), ("op", op_pred, op, Hn.OP_LEN_CLIP, fused[1])):
            tgt = frames[s + lc - 1:e + lc - 1]
            sl = slice(s + lc - 1, e + lc - 1)
            # the frames as scored, through `ops.ssim` again: the same bits
            one = ops.ssim(pred, tgt, map=True)
            for k, key in (("ssim", "ssim"), ("mse", "mse"), ("psnr", "psnr"), ("ssim_map", "map")):
                assert np.array_equal(rec[f"{st}_{k}"][sl], one[key].cpu().numpy()), (st, k)
            if st == "rgb":
                # the output layer's epilogue adds at most 256 tile sums in an arbitrary fp32 order: 255 u = 6.6e-5 dB
                d = float((torch.from_numpy(rec["rgb_psnr"][sl]).double() - fz.double().cpu()).abs().max())
                print(f"rgb_psnr vs the epilogue's: {d:.3e} dB")
                assert d <= 1e-4


def test_evaluate_dataset_quality_fills(model):
    videos, _ = run_test.synthetic_dataset(2, 12, 64)
    rec = Hn.evaluate_dataset_quality(model, videos, "ped2", device=DEV)
    assert rec["n_frames"] == [12, 19] and rec["map_files"] == [] and rec["dataset"] == "ped2"
    for key in ("rgb_img_pred_records", "rgb_fea_comm_records", "op_img_pred_records", "op_fea_comm_records",
                "rgb_ssim_records", "op_ssim_records", "rgb_mse_records", "op_mse_records"):
        assert len(rec[key]) == 2
        lc = Hn.RGB_LEN_CLIP if key.startswith("rgb_") else Hn.OP_LEN_CLIP
        for a, t in zip(rec[key], (12, 19)):
            assert a.shape == (t,) and a.dtype == np.float32 and np.isfinite(a).all(), key
            assert (a[:lc - 1] == a[lc - 1]).all(), key                                  # `assemble_records`' head fill
            if key.startswith("op_"):
                assert a[t - 1] == a[t - 2], key                                         # and the flow stream's last frame
    # mse and psnr are two functions of one sum
    for m, p in zip(rec["rgb_mse_records"], rec["rgb_img_pred_records"]):
        assert np.allclose(10 * np.log10(1024.0 / m.astype(np.float64)), p, rtol=0, atol=1e-4)


def test_run_quality_entry(tmp_path, capsys):
    """`run_quality` = run_test's options + --maps_dir / --ssim_maps; run_test itself prints what it printed"""
    argv = ["--synthetic", "--videos", "2", "--frames", "24", "--size", "64"]
    maps = tmp_path / "maps"
    run_quality.main(argv + ["--maps_dir", str(maps), "--ssim_maps"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["maps"] == {"dir": str(maps), "files": 2, "ssim_maps": True}
    for k in ("auc", "auc_ssim", "auc_mse"):
        assert 0.0 <= line[k] <= 1.0, k
    assert -1.0 <= line["mean_ssim_rgb"] <= 1.0 and -1.0 <= line["mean_ssim_op"] <= 1.0
    assert line["videos"] == 2 and line["predicted_frames"] == (24 - 4) + (31 - 4)
    files = sorted(p.name for p in maps.iterdir())
    assert files == ["0000.npz", "0001.npz"]
    want = {f"{st}_{k}" for st in ("rgb", "op") for k in ("ssim", "mse", "psnr", "comm", "ssim_map")}
    for name, t in zip(files, (24, 31)):
        z = np.load(maps / name)
        assert set(z.files) == want
        assert z["rgb_ssim_map"].shape == (t, 64, 64) and z["op_ssim_map"].shape == (t, 64, 64)
        for k in want - {"rgb_ssim_map", "op_ssim_map"}:
            assert z[k].shape == (t,) and z[k].dtype == np.float32, k
    run_quality.main(argv)                                                               # no folder: the scores alone
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "maps" not in line and "auc_ssim" in line and "mean_ssim_rgb" in line
    run_test.main(argv)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "auc" in line and "auc_ssim" not in line and "mean_ssim_rgb" not in line
