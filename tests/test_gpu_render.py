"""The render pass (csrc/render.hip, `ops.render_panels` / `ops.flow_to_rgb` / `ops.render_stats`,
`harness.render_subvideo`, the `run_panels` entry) against `harness.render_reference` (plain numpy: fp32 for the colour
code, float64 for the frame and heat tiles), against the reference's own `flow_to_image` (tests/golden/flow_colour.npz)
and against itself (strides, alignment, batching, tile subsets).

Tolerance.  Frame tiles and the four maxima are exact.  A flow or heat tile value may differ
from the witness by ONE grey level: the device's atan2f and numpy's differ by a few ulp, and the heat tiles are fp32
against float64, which moves a `floor` only where its argument lies within about 1e-3 of an integer.  The share of such
values, pooled over the shapes below, was measured on an MI355X (FLOW_SHARE / HEAT_SHARE); the tests gate at four times
the measured shares."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_maps, run_panels, run_test, synthetic as S
import render_cases as K
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"

# measured shares of values one grey level off the witness (none was further off), pooled over K.DEVICE_SHAPES
FLOW_SHARE = 0.0                 # op_target, op_pred: 0 of 451518 values, and 0 of 32235 against the fixture
HEAT_SHARE = 223 / 451518        # rgb_heat, op_heat: 4.9e-4 (all of them in rgb_heat: the flow pair's test errors are tiny)
GATE = 4.0

FRAME_TILES, FLOW_TILES, HEAT_TILES = ("rgb_target", "rgb_pred"), ("op_target", "op_pred"), ("rgb_heat", "op_heat")


@functools.lru_cache(maxsize=None)
def dev_inputs(shape):
    return tuple(t.to(DEV) for t in K.inputs(shape))


@functools.lru_cache(maxsize=None)
def dev_panels(shape, flow_norm="target"):
    """the default 2 x 3 panels of a case, as a host array (shared, read-only)"""
    return ops.render_panels(*dev_inputs(shape), flow_scale=K.FLOW_SCALE, flow_norm=flow_norm).cpu().numpy()


def tile_of(panels: np.ndarray, name: str, shape) -> np.ndarray:
    _, h, w = shape
    i = Hn.RENDER_TILES.index(name)
    r, c = divmod(i, 3)
    return panels[:, r * h:(r + 1) * h, c * w:(c + 1) * w]


def off_by(a: np.ndarray, b: np.ndarray):
    """(largest difference, values that differ, values)"""
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return int(d.max()) if d.size else 0, int((d != 0).sum()), int(d.size)


@pytest.mark.parametrize("shape", K.DEVICE_SHAPES)
def test_panels_against_the_reference(shape):
    ref = K.reference(shape)
    got = dev_panels(shape)
    assert got.shape == ref["panels"].shape and got.dtype == np.uint8
    stats = ops.render_stats(*dev_inputs(shape), flow_scale=K.FLOW_SCALE).cpu().numpy()
    assert np.array_equal(stats.view(np.uint32), ref["stats"].view(np.uint32))           # the maxima: bit for bit
    for name in FRAME_TILES:
        assert np.array_equal(tile_of(got, name, shape), ref[name]), name                # frame tiles: exact
    for name in FLOW_TILES + HEAT_TILES:
        worst, n, total = off_by(tile_of(got, name, shape), ref[name])
        print(f"{shape} {name}: {n} of {total} values differ, by at most {worst}")
        assert worst <= 1, name


def test_share_of_values_one_level_off():
    """pooled over the shapes: at most four times the measured share (the docstring of this module)"""
    for kind, names, measured in (("flow", FLOW_TILES, FLOW_SHARE), ("heat", HEAT_TILES, HEAT_SHARE)):
        n = total = 0
        for shape in K.DEVICE_SHAPES:
            for name in names:
                _, d, t = off_by(tile_of(dev_panels(shape), name, shape), K.reference(shape)[name])
                n, total = n + d, total + t
        print(f"{kind} tiles: {n} of {total} values one level off: share {n / total:.3e} (measured {measured:.3e})")
        assert n / total <= GATE * measured, kind


def test_colour_code_against_flow_to_image():
    """the device's colour code against the reference's own output, with the host test's compare rule and exclusion cap;
    `render_reference` equals the fixture exactly on those pixels, so the device is held to what it is held to against
    `render_reference`: one grey level, the flow tiles' share"""
    g = np.load(os.path.join(GOLDEN, "flow_colour.npz"))
    flows = np.ascontiguousarray(np.stack([g[f"{name}_flow"].transpose(2, 0, 1) for name in K.GOLDEN_CASES]))
    got = ops.flow_to_rgb(torch.from_numpy(flows).to(DEV)).cpu().numpy()
    n = total = 0
    for i, name in enumerate(K.GOLDEN_CASES):
        r = Hn.flow_colour_reference(flows[i:i + 1])
        cmp = K.compared(r["raw"][0], r["max_rad"][0]) | ~r["known"][0]
        assert int((~cmp).sum()) <= K.MAX_EXCLUDED, name
        worst, d, t = off_by(got[i][cmp], g[f"{name}_image"][cmp])
        print(f"{name}: {d} of {t} compared values differ, by at most {worst}; {int((~cmp).sum())} pixels left out")
        assert worst <= 1, name
        assert (got[i][~cmp].max(axis=-1) >= 254).all(), name           # the pixels at the maximum: inside, not dimmed
        n, total = n + d, total + t
    assert (got[K.GOLDEN_CASES.index("zeros")] == 255).all()
    for y, x in K.UNKNOWN_AT:
        assert got[K.GOLDEN_CASES.index("unknown")][y, x].tolist() == [0, 0, 0]
    print(f"golden: {n} of {total} values one level off: share {n / total:.3e}")
    assert n / total <= GATE * FLOW_SHARE


def test_stats_are_the_maxima_on_every_launch():
    shape = (17, 16, 16)
    ins = dev_inputs(shape)
    want = K.reference(shape)["stats"]
    first = ops.render_stats(*ins, flow_scale=K.FLOW_SCALE)
    assert np.array_equal(first.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # equal to amax of the fp32 quantities, restated here with numpy (IEEE: correctly rounded sqrt and division; torch's
    # vectorised CPU sqrt is not)
    rp, rt, fp, ft = (t.numpy() for t in K.inputs(shape))
    with np.errstate(invalid="ignore"):
        ok = (np.abs(ft) <= np.float32(1e7)).all(axis=1)                # False for a NaN
        u, v = np.where(ok, ft[:, 0], np.float32(0)), np.where(ok, ft[:, 1], np.float32(0))
    got = first.cpu().numpy()
    assert np.array_equal(got[:, 0], np.sqrt(u * u + v * v).max(axis=(1, 2)))
    d = np.float32(0.5) * (rt - rp)
    acc = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert acc.dtype == np.float32 and np.array_equal(got[:, 2], (acc / np.float32(3)).max(axis=(1, 2)))
    for fill in (0.0, 3.0e38, float("nan"), -1.0):                     # whatever the buffer held before
        out = torch.full((shape[0], 4), fill, device=DEV)
        assert ops.render_stats(*ins, flow_scale=K.FLOW_SCALE, out=out) is out
        assert torch.equal(out.view(torch.int32), first.view(torch.int32))
    big = (16, 64, 64)                                                 # more than one workgroup per sample
    a = ops.render_stats(*dev_inputs(big), flow_scale=K.FLOW_SCALE)
    b = ops.render_stats(*dev_inputs(big), flow_scale=K.FLOW_SCALE)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(a.cpu().numpy().view(np.uint32), K.reference(big)["stats"].view(np.uint32))


def strided(t: torch.Tensor, pad: int, offset: int = 0) -> torch.Tensor:
    """the same values as a view with a batch stride of a sample + `pad` floats, `offset` floats into its buffer"""
    b = t.shape[0]
    n = t[0].numel()
    buf = torch.full((offset + b * (n + pad),), 7.0, device=t.device, dtype=t.dtype)
    v = buf[offset:].view(b, n + pad)[:, :n].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("shape", ((16, 64, 64), (3, 21, 27)))
def test_strides_alignment_tiles_and_out_slots(shape):
    b, h, w = shape
    ins = dev_inputs(shape)
    want = torch.from_numpy(dev_panels(shape)).to(DEV)
    # batch strides: whole quads (the 16-byte path stays) and odd (scalar loads), and a base 4 bytes off a quad
    for pad, offset in ((8, 0), (3, 0), (0, 1), (5, 3)):
        views = [strided(t, pad, offset) for t in ins]
        assert not views[0].is_contiguous() or (pad == 0)
        assert torch.equal(ops.render_panels(*views, flow_scale=K.FLOW_SCALE), want), (pad, offset)
        assert torch.equal(ops.render_stats(*views, flow_scale=K.FLOW_SCALE).view(torch.int32),
                           ops.render_stats(*ins, flow_scale=K.FLOW_SCALE).view(torch.int32))
    # out=: the rows of a larger buffer, dword-aligned and not
    for lead, pad in ((0, 16), (1, 5)):
        per = want[0].numel()
        buf = torch.full((lead + b * (per + pad),), 9, device=DEV, dtype=torch.uint8)
        out = buf[lead:].view(b, per + pad)[:, :per].view(want.shape)
        assert ops.render_panels(*ins, flow_scale=K.FLOW_SCALE, out=out) is out
        assert torch.equal(out, want)
        assert (buf[lead:].view(b, per + pad)[:, per:] == 9).all() and (buf[:lead] == 9).all()      # nothing beyond a panel
    # a subset, reordered: every tile equals its place in the full panel
    for tiles in (("op_heat", "rgb_pred", "op_target"), (("rgb_heat",), ("op_pred",)), ("rgb_target",),
                  (("op_pred", "rgb_heat"), ("op_target", "rgb_target"))):
        rows = Hn.panel_layout(tiles)
        got = ops.render_panels(*ins, tiles=tiles, flow_scale=K.FLOW_SCALE).cpu().numpy()
        assert got.shape == (b, len(rows) * h, len(rows[0]) * w, 3)
        for r, row in enumerate(rows):
            for c, name in enumerate(row):
                assert np.array_equal(got[:, r * h:(r + 1) * h, c * w:(c + 1) * w], tile_of(want.cpu().numpy(), name, shape)), (tiles, name)


@pytest.mark.parametrize("shape", ((3, 21, 27), (17, 16, 16)))
def test_a_sample_alone_equals_the_sample_in_its_batch(shape):
    ins = dev_inputs(shape)
    want = dev_panels(shape)
    for i in range(shape[0]):
        alone = ops.render_panels(*(t[i:i + 1] for t in ins), flow_scale=K.FLOW_SCALE).cpu().numpy()
        assert np.array_equal(alone[0], want[i]), i
    tail = ops.render_panels(*(t[1:] for t in ins), flow_scale=K.FLOW_SCALE).cpu().numpy()     # at another place in a batch
    assert np.array_equal(tail, want[1:])


def test_flow_norm_each_is_flow_to_rgb_and_supplied_values_apply():
    shape = (3, 21, 27)
    b, h, w = shape
    rp, rt, fp, ft = dev_inputs(shape)
    each = ops.render_panels(rp, rt, fp, ft, tiles=("op_target", "op_pred"), flow_scale=(2.0, 3.0), flow_norm="each")
    assert torch.equal(each[:, :, :w], ops.flow_to_rgb(ft, scale=(2.0, 3.0)))
    assert torch.equal(each[:, :, w:], ops.flow_to_rgb(fp, scale=(2.0, 3.0)))
    # "target": the predicted flow by the target's maximum = the stand-alone entry with that radius supplied
    stats = ops.render_stats(rp, rt, fp, ft, flow_scale=K.FLOW_SCALE)
    assert torch.equal(torch.from_numpy(tile_of(dev_panels(shape), "op_pred", shape)).to(DEV),
                       ops.flow_to_rgb(fp, max_rad=stats[:, 0].contiguous()))
    # a supplied radius below the data: the pixels beyond it are dimmed by a quarter, the others are as before at that radius
    half = (stats[:, 1] * 0.5).contiguous()
    got = ops.flow_to_rgb(fp, max_rad=half).cpu().numpy()
    ref = Hn.flow_colour_reference(K.inputs(shape)[2], max_rad=half.cpu())
    assert off_by(got, ref["rgb"])[0] <= 1
    outside = ~ref["inside"] & ref["known"]
    assert outside.sum() > 50 and (got[outside].max(axis=-1) <= 191).all() and (got[outside].max(axis=-1) >= 190).all()
    out = torch.empty((b, h, w, 3), device=DEV, dtype=torch.uint8)
    assert ops.flow_to_rgb(fp, max_rad=half, out=out) is out and np.array_equal(out.cpu().numpy(), got)
    # fixed heat maxima: against the witness with the same values, and one tensor = the pair of it
    hm = torch.full((b,), 0.01, device=DEV)
    fixed = ops.render_panels(rp, rt, fp, ft, tiles=("rgb_heat", "op_heat"), heat_max=hm, alpha=0.35).cpu().numpy()
    pair = ops.render_panels(rp, rt, fp, ft, tiles=("rgb_heat", "op_heat"), heat_max=(hm, hm), alpha=0.35).cpu().numpy()
    assert np.array_equal(fixed, pair)
    want = Hn.render_reference(*K.inputs(shape), tiles=("rgb_heat", "op_heat"), heat_max=hm.cpu(), alpha=0.35)["panels"]
    assert off_by(fixed, want)[0] <= 1
    assert not np.array_equal(fixed, np.concatenate([tile_of(dev_panels(shape), n, shape) for n in ("rgb_heat", "op_heat")], axis=2))


# ---- end to end: harness.render_subvideo and the run_panels entry ------------------------------------------------

ARGV = ["--synthetic", "--videos", "2", "--frames", "12", "--size", "64"]


@functools.lru_cache(maxsize=None)
def model_and_videos():
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=256, k=2))
    model = model.to(DEV).eval()
    model.precision = "s16"
    videos, _ = run_test.synthetic_dataset(2, 12, 64)
    return model, [(rgb.to(DEV).contiguous(), op.to(DEV).contiguous()) for rgb, op in videos]


def test_render_subvideo_against_the_ops_on_the_same_predictions():
    """frame order and indexing, `select`, and the panels themselves: `localise_subvideo`'s `predictions=` hook hands
    over what the same clips predicted"""
    model, videos = model_and_videos()
    rgb, op = videos[1]                                                # 19 frames: 15 clips, one batch
    t, _, h, w = rgb.shape
    stats = {}
    got = list(Hn.render_subvideo(model, rgb, op, batch=4, stats=stats))          # four batches, the last one short
    assert [f for f, _ in got] == list(range(Hn.RGB_LEN_CLIP - 1, t))
    assert stats["render_batches"] == 4 and stats["copies"] == 4 + stats["rerun_batches"] and stats["render_ms"] > 0
    preds = []
    Hn.localise_subvideo(model, rgb, op, batch=4, predictions=preds)
    for s, e, rgb_out, op_out, _ in preds:
        want = ops.render_panels(rgb_out, rgb[s + 4:e + 4], op_out, op[s + 3:e + 3], flow_scale=(float(h), float(w))).cpu().numpy()
        for i in range(s, e):
            assert got[i][1].shape == (2 * h, 3 * w, 3) and np.array_equal(got[i][1], want[i - s]), i
    some = list(Hn.render_subvideo(model, rgb, op, select=[17, 5, 9, 9], batch=4, tiles=("rgb_pred", "op_pred")))
    assert [f for f, _ in some] == [5, 9, 17]
    for f, panel in some:
        assert np.array_equal(panel[:, :w], got[f - 4][1][:h, w:2 * w]) and np.array_equal(panel[:, w:], got[f - 4][1][h:, w:2 * w])
    with pytest.raises(ValueError):
        list(Hn.render_subvideo(model, rgb, op, select=[3]))


def test_run_panels_entry_writes_what_render_subvideo_yields(tmp_path, capsys):
    from PIL import Image
    out = tmp_path / "panels"
    run_panels.main(ARGV + ["--panels_dir", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    model, videos = model_and_videos()
    n = sum(rgb.shape[0] - 4 for rgb, _ in videos)
    assert line["panels_written"] == n == line["predicted_frames"] and line["gpus"] == 1 and 0.0 <= line["auc"] <= 1.0
    assert line["render_ms_per_batch"] > 0 and line["write_s"] > 0 and line["fps"] > 0 and line["fps_no_writers"] >= line["fps"]
    for v, (rgb, op) in enumerate(videos):
        names = sorted(os.listdir(out / f"{v:04d}"))
        assert names == [f"{f:06d}.png" for f in range(4, rgb.shape[0])]
        for f, panel in Hn.render_subvideo(model, rgb, op):
            assert np.array_equal(np.asarray(Image.open(out / f"{v:04d}" / f"{f:06d}.png")), panel), (v, f)


def test_run_panels_top_k_and_records_are_run_maps(tmp_path, capsys):
    out, maps = tmp_path / "top", tmp_path / "maps"
    run_panels.main(ARGV + ["--panels_dir", str(out), "--top", "3", "--format", "npy", "--tiles", "rgb_heat"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    run_maps.main(ARGV + ["--maps_dir", str(maps)])
    theirs = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["auc"] == theirs["auc"] and line["panels_written"] == 6
    model, videos = model_and_videos()
    rec = Hn.evaluate_dataset_panels(model, videos, top=3)
    for v in range(2):
        z = np.load(maps / f"{v:04d}.npz")
        worst = Hn.select_frames(z["rgb_psnr"], top=3)
        assert sorted(os.listdir(out / f"{v:04d}")) == [f"{f:06d}.npy" for f in worst]
        assert len(worst) == 3 and set(np.argsort(z["rgb_psnr"][4:], kind="stable")[:3] + 4) == set(worst)
        assert np.load(out / f"{v:04d}" / f"{worst[0]:06d}.npy").shape == (64, 64, 3)
        for key, name in (("rgb_img_pred_records", "rgb_psnr"), ("rgb_fea_comm_records", "rgb_comm"),
                          ("op_img_pred_records", "op_psnr"), ("op_fea_comm_records", "op_comm")):
            assert np.array_equal(rec[key][v], z[name]), (v, key)
        assert rec["panel_frames"][v] == worst
