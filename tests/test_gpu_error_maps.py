"""The error-map pass (csrc/error_maps.hip, `ops.error_maps`, `harness.localise_subvideo`, the `run_maps` entry)
against `harness.error_maps_reference` (float64, plain torch) on the same tensors.

Gates (u = 2^-24, all RELATIVE to the float64 value, entry by entry):
  patch_sum, patch_mean  1e-5.  Every term is non-negative, so a sum in any order is within (depth + 3) u of the exact
                         one; the kernel's longest chain of dependent adds is 20, i.e. 1.4e-6.
  pixel                  1e-6: one difference, three squares, two adds, one divide - 7 roundings, 4.2e-7.
  psnr                   10 log10(1 + 1e-5) dB (the gate on the sums; the second level of frame_sq runs in double) plus
                         4 ulp of a value below 64 dB for the fp32 quotient and logarithm: 7.4e-5 dB.
What the header defines exactly (frame_sq from the returned patch_sum, worst, worst_idx) and everything about the
ORDER of the additions (place in the batch, strides, alignment, pixel map or not) is compared bit for bit."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_maps, run_test, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 3, 8, 8, 8), (3, 3, 27, 21, 8), (2, 2, 64, 64, 16), (5, 3, 40, 72, 32), (2, 3, 64, 96, 8), (1, 4, 16, 16, 16)]
SUM_GATE, PIXEL_GATE = 1e-5, 1e-6
PSNR_GATE = 10 * math.log10(1 + SUM_GATE) + 4 * 2.0 ** -23 * 64
KEYS = ("patch_sum", "patch_mean", "frame_sq", "worst", "worst_idx", "psnr")
nan = float("nan")


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(pred, target) on the CPU: tanh of seeded normals, uniform [-1, 1]; where a frame has more than one patch,
    patch (0, 0) of sample 0 is predicted exactly"""
    b, c, h, w, patch = shape
    g = torch.Generator().manual_seed(1000 + h * w + c)
    pred = torch.tanh(torch.randn(b, c, h, w, generator=g))
    target = torch.rand(b, c, h, w, generator=g) * 2 - 1
    if _planted(shape):
        pred[0, :, :patch, :patch] = target[0, :, :patch, :patch]
    return pred, target


def _planted(shape):
    return shape[2] > shape[4] or shape[3] > shape[4]


@functools.lru_cache(maxsize=None)
def _reference(shape):
    pred, target = _inputs(shape)
    return Hn.error_maps_reference(pred, target, shape[4])


def _dev(shape):
    return tuple(t.to(DEV) for t in _inputs(shape))


def _rel_ok(got, ref, gate, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    worst = float((err / ref.abs().clamp_min(1e-300)).max())
    print(f"{what}: max relative error {worst:.3e} (gate {gate:.1e})")
    assert bool((err <= gate * ref.abs()).all()), (what, worst)


def _equal(a, b, keys=KEYS + ("pixel",)):
    for k in keys:
        if k in a and k in b:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parity_against_fp64(shape):
    pred, target = _dev(shape)
    ref = _reference(shape)
    got = ops.error_maps(pred, target, shape[4], pixel=True)
    b, c, h, w, patch = shape
    ph, pw = -(-h // patch), -(-w // patch)
    assert got["patch_sum"].shape == (b, ph, pw) and got["pixel"].shape == (b, h, w) and got["worst_idx"].dtype == torch.int32
    _rel_ok(got["patch_sum"], ref["patch_sum"], SUM_GATE, "patch_sum")
    _rel_ok(got["patch_mean"], ref["patch_mean"], SUM_GATE, "patch_mean")
    _rel_ok(got["pixel"], ref["pixel"], PIXEL_GATE, "pixel")
    _rel_ok(got["frame_sq"], ref["frame_sq"], SUM_GATE, "frame_sq")
    d = float((got["psnr"].double().cpu() - ref["psnr"]).abs().max())
    print(f"psnr: max |difference| {d:.3e} dB (gate {PSNR_GATE:.2e})")
    assert d <= PSNR_GATE
    # a patch predicted exactly is exactly 0 (and nothing else is)
    if _planted(shape):
        assert float(got["patch_sum"][0, 0, 0]) == 0.0 and float(got["patch_mean"][0, 0, 0]) == 0.0
        assert bool((got["pixel"][0, :patch, :patch] == 0).all())
    assert int((got["patch_sum"] == 0).sum()) == int(_planted(shape))
    assert torch.equal(got["worst_idx"].cpu(), ref["worst_idx"])            # (no near-ties in these inputs)


def _frame_sq_by_definition(patch_sum):
    ps = patch_sum.cpu().numpy()
    out = np.empty(ps.shape[0], dtype=np.float32)
    for b in range(ps.shape[0]):
        total = np.float64(0.0)
        for i in range(ps.shape[1]):
            row = np.float64(0.0)
            for j in range(ps.shape[2]):
                row = row + np.float64(ps[b, i, j])
            total = total + row
        out[b] = np.float32(total)
    return torch.from_numpy(out)


def _check_contracts(got):
    assert torch.equal(got["frame_sq"].cpu(), _frame_sq_by_definition(got["patch_sum"]))
    flat = got["patch_mean"].flatten(1)
    assert torch.equal(got["worst"], flat.amax(dim=1))
    first = (flat == got["worst"][:, None]).int().argmax(dim=1).to(torch.int32)
    assert torch.equal(got["worst_idx"], first)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_contracts_recomputed_from_the_returned_maps(shape):
    pred, target = _dev(shape)
    _check_contracts(ops.error_maps(pred, target, shape[4]))


@pytest.mark.parametrize("shape,a,b", [((2, 3, 64, 96, 8), (1, 2), (5, 9)), ((2, 2, 64, 64, 16), (0, 3), (2, 0)),
                                       ((5, 3, 40, 72, 32), (0, 1), (0, 0))], ids=str)
def test_worst_idx_is_the_lowest_among_equal_patches(shape, a, b):
    """two patches of identical content, the largest of their frame: a real tie - and the same bits at two places"""
    pred, target = (t.clone() for t in _inputs(shape))
    patch = shape[4]
    g = torch.Generator().manual_seed(7)
    c = shape[1]
    t_blk = 0.9 + 0.1 * torch.rand(c, patch, patch, generator=g)
    p_blk = -0.9 - 0.1 * torch.rand(c, patch, patch, generator=g)
    for (i, j) in (a, b):
        target[1, :, i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] = t_blk
        pred[1, :, i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] = p_blk
    got = ops.error_maps(pred.to(DEV), target.to(DEV), patch)
    pw = got["patch_mean"].shape[2]
    pm = got["patch_mean"][1]
    assert float(pm[a]) == float(pm[b]) and float(got["patch_sum"][1][a]) == float(got["patch_sum"][1][b])
    assert float(got["worst"][1]) == float(pm[a]) and float(pm[a]) > 0.8
    assert int(got["worst_idx"][1]) == min(a[0] * pw + a[1], b[0] * pw + b[1])
    _check_contracts(got)


def _in_buffer(t, pad_b, pad_c, pad_h, pad_w, offset=0):
    """`t` [B,C,H,W] as a view inside a larger NaN-filled buffer (padded batch / channel / row strides, base `offset` floats in)"""
    b, c, h, w = t.shape
    n = (b + pad_b) * (c + pad_c) * (h + pad_h) * (w + pad_w)
    flat = torch.full((n + offset,), nan, device=t.device)
    v = flat[offset:].view(b + pad_b, c + pad_c, h + pad_h, w + pad_w)[:b, :c, :h, :w]
    v.copy_(t)
    return v


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_order_does_not_depend_on_batch_strides_alignment_or_pixel(shape):
    pred, target = _dev(shape)
    patch = shape[4]
    base = ops.error_maps(pred, target, patch, pixel=True)
    _equal(base, ops.error_maps(pred, target, patch, pixel=True))                        # the same launch twice
    _equal(base, ops.error_maps(pred, target, patch, pixel=False))                       # without the pixel map
    for i in {0, shape[0] - 1}:                                                          # alone / at position 3 of a batch of 5
        alone = ops.error_maps(pred[i:i + 1], target[i:i + 1], patch, pixel=True)
        g = torch.Generator().manual_seed(11)
        p5 = torch.tanh(torch.randn(5, *shape[1:4], generator=g)).to(DEV)
        t5 = (torch.rand(5, *shape[1:4], generator=g) * 2 - 1).to(DEV)
        p5[3], t5[3] = pred[i], target[i]
        five = ops.error_maps(p5, t5, patch, pixel=True)
        for k in KEYS + ("pixel",):
            assert torch.equal(alone[k][0], five[k][3]), (k, i)
            assert torch.equal(alone[k][0], base[k][i]), (k, i)
    # views inside NaN-filled buffers: padded batch / channel / row strides (rows w + 3 and w + 4 floats apart: one of the
    # two keeps every row 16-byte aligned, the other does not) and a base one float off a 16-byte boundary
    for pads, off in (((1, 1, 2, 4), 0), ((1, 1, 2, 3), 0), ((0, 0, 0, 0), 1), ((2, 0, 1, 8), 1)):
        pv, tv = _in_buffer(pred, *pads, offset=off), _in_buffer(target, *pads, offset=(off + 2) % 4 if off else 0)
        assert pv.data_ptr() % 16 == 4 * off
        _equal(base, ops.error_maps(pv, tv, patch, pixel=True))
        _equal(base, ops.error_maps(pv, target, patch, pixel=True))                      # mixed: one operand strided only


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_nothing_outside_the_outputs_is_written(shape):
    pred, target = _dev(shape)
    b, c, h, w, patch = shape
    ph, pw = -(-h // patch), -(-w // patch)
    base = ops.error_maps(pred, target, patch, pixel=True)

    def holder(inner, pad):
        buf = torch.full((b + 2, inner + pad), nan, device=DEV)
        return buf, buf[1:b + 1, :inner]
    bufs, out = {}, {}
    for k, inner, shp in (("patch_sum", ph * pw, (ph, pw)), ("patch_mean", ph * pw, (ph, pw)), ("pixel", h * w, (h, w))):
        bufs[k], v = holder(inner, 5)
        out[k] = v.unflatten(1, shp)
    for k in ("frame_sq", "worst"):
        bufs[k] = torch.full((b + 2,), nan, device=DEV)
        out[k] = bufs[k][1:b + 1]
    bufs["worst_idx"] = torch.full((b + 2,), -7, device=DEV, dtype=torch.int32)
    out["worst_idx"] = bufs["worst_idx"][1:b + 1]
    got = ops.error_maps(pred, target, patch, pixel=True, out=out)
    _equal(base, got)
    for k in ("patch_sum", "patch_mean", "pixel"):
        inner = out[k][0].numel()
        assert got[k].data_ptr() == out[k].data_ptr()
        assert not bool(torch.isnan(bufs[k][1:b + 1, :inner]).any())
        assert bool(torch.isnan(bufs[k][0]).all()) and bool(torch.isnan(bufs[k][b + 1]).all())
        assert bool(torch.isnan(bufs[k][:, inner:]).all())
    for k in ("frame_sq", "worst"):
        assert bool(torch.isnan(bufs[k][[0, b + 1]]).all()) and not bool(torch.isnan(bufs[k][1:b + 1]).any())
    assert bufs["worst_idx"][[0, b + 1]].tolist() == [-7, -7]
    # without a pixel map no pixel buffer is touched
    bufs["pixel"].fill_(nan)
    no_px = ops.error_maps(pred, target, patch, pixel=False, out={k: v for k, v in out.items() if k != "pixel"})
    assert "pixel" not in no_px and bool(torch.isnan(bufs["pixel"]).all())
    _equal(base, no_px)


@pytest.fixture(scope="module")
def model():
    m = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    m.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=256, k=2))
    m = m.to(DEV).eval()
    m.precision = "s16"
    return m


def test_localise_subvideo(model):
    t, size, patch = 11, 64, 16
    (rgb, op), = run_test.synthetic_dataset(1, t, size)[0]
    rgb, op = rgb.to(DEV), op.to(DEV)
    preds = []
    rec = Hn.localise_subvideo(model, rgb, op, patch=patch, pixel=True, batch=4, predictions=preds)
    assert [(p[0], p[1]) for p in preds] == [(0, 4), (4, 7)]
    ph = pw = size // patch
    for st in ("rgb", "op"):
        assert rec[f"{st}_patch"].shape == (t, ph, pw) and rec[f"{st}_pixel"].shape == (t, size, size)
        for k in ("psnr", "worst", "worst_idx", "comm"):
            assert rec[f"{st}_{k}"].shape == (t,), (st, k)
        assert rec[f"{st}_worst_idx"].dtype == np.int32 and rec[f"{st}_patch"].dtype == np.float32
        lc = Hn.RGB_LEN_CLIP if st == "rgb" else Hn.OP_LEN_CLIP
        for k in ("patch", "pixel", "psnr", "worst", "worst_idx", "comm"):
            a = rec[f"{st}_{k}"]
            for i in range(lc - 1):
                assert np.array_equal(a[i], a[lc - 1]), (st, k, i)
    for k in ("patch", "pixel", "psnr", "worst", "worst_idx", "comm"):
        assert np.array_equal(rec[f"op_{k}"][t - 1], rec[f"op_{k}"][t - 2]), k
    assert np.isfinite(rec["rgb_psnr"]).all() and np.isfinite(rec["op_psnr"]).all()
    for s, e, rgb_pred, op_pred, fused in preds:
        for st, pred, frames, lc, fz in (("rgb", rgb_pred, rgb, Hn.RGB_LEN_CLIP, fused[0]), ("op", op_pred, op, Hn.OP_LEN_CLIP, fused[1])):
            tgt = frames[s + lc - 1:e + lc - 1]
            sl = slice(s + lc - 1, e + lc - 1)
            ref = Hn.error_maps_reference(pred, tgt, patch)
            _rel_ok(torch.from_numpy(rec[f"{st}_patch"][sl]), ref["patch_mean"], SUM_GATE, f"{st}_patch")
            _rel_ok(torch.from_numpy(rec[f"{st}_pixel"][sl]), ref["pixel"], PIXEL_GATE, f"{st}_pixel")
            _rel_ok(torch.from_numpy(rec[f"{st}_worst"][sl]), ref["worst"], SUM_GATE, f"{st}_worst")
            psnr = torch.from_numpy(rec[f"{st}_psnr"][sl]).double()
            d = float((psnr - ref["psnr"].cpu()).abs().max())
            print(f"{st}_psnr vs float64: {d:.3e} dB")
            assert d <= PSNR_GATE
            # the output layer's epilogue adds at most 256 tile sums in an arbitrary fp32 order: 255 u = 6.6e-5 dB
            d = float((psnr - fz.double().cpu()).abs().max())
            print(f"{st}_psnr vs the epilogue's: {d:.3e} dB")
            assert d <= 1e-4
            # the scoring kernels on the same forward outputs: the same bits, call after call
            one, two = ops.error_maps(pred, tgt, patch, pixel=True), ops.error_maps(pred, tgt, patch, pixel=True)
            _equal(one, two)
            for k, key in (("patch", "patch_mean"), ("pixel", "pixel"), ("psnr", "psnr"), ("worst", "worst"), ("worst_idx", "worst_idx")):
                assert np.array_equal(rec[f"{st}_{k}"][sl], one[key].cpu().numpy()), (st, k)


def test_run_maps_entry(tmp_path, capsys):
    """`run_maps` = run_test's options + --maps_dir / --patch / --pixel_maps; run_test itself prints what it printed"""
    argv = ["--synthetic", "--videos", "2", "--frames", "12", "--size", "64"]
    maps = tmp_path / "maps"
    run_maps.main(argv + ["--maps_dir", str(maps), "--patch", "16"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["maps"] == {"dir": str(maps), "patch": 16, "files": 2, "pixel": False}
    assert 0.0 <= line["auc"] <= 1.0 and 0.0 <= line["auc_patch"] <= 1.0
    assert line["videos"] == 2 and line["predicted_frames"] == (12 - 4) + (19 - 4)
    files = sorted(p.name for p in maps.iterdir())
    assert files == ["0000.npz", "0001.npz"]
    for name, t in zip(files, (12, 19)):
        z = np.load(maps / name)
        want = {f"{st}_{k}" for st in ("rgb", "op") for k in ("patch", "psnr", "worst", "worst_idx", "comm")}
        assert set(z.files) == want
        assert z["rgb_patch"].shape == (t, 4, 4) and z["op_patch"].shape == (t, 4, 4)
        for k in want - {"rgb_patch", "op_patch"}:
            assert z[k].shape == (t,), k
        assert np.array_equal(z["rgb_worst"], z["rgb_patch"].reshape(t, -1).max(axis=1))
    run_test.main(argv)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "auc" in line and "maps" not in line and "auc_patch" not in line
