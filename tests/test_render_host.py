"""CPU-side checks of the render pass: `harness.render_reference` - the witness of
tests/test_gpu_render.py - against the reference's own `flow_to_image` (tests/golden/flow_colour.npz) and against
hand-computed values, the panel layout, the argument checks of the C entries and of the ops (decided without a GPU), the
writer pool and `run_panels`' options."""
import os
import threading
import time

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, parallel, run_maps, run_panels
import render_cases as K
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "flow_colour.npz"))


def test_fixture_holds_the_cases_of_render_cases(golden):
    assert tuple(golden["cases"]) == K.GOLDEN_CASES
    for name, flow in K.golden_flows().items():
        assert golden[f"{name}_flow"].shape == K.GOLDEN_HW + (2,) and golden[f"{name}_image"].shape == K.GOLDEN_HW + (3,)
        assert np.array_equal(golden[f"{name}_flow"], flow, equal_nan=True), name
    assert (golden["zeros_image"] == 255).all()                      # no flow: white


def test_colour_wheel_is_the_published_one():
    w = np.round(Hn.colour_wheel().astype(np.float64) * 255).astype(int)
    assert w.shape == (55, 3)
    assert w[0].tolist() == [255, 0, 0] and w[14].tolist() == [255, 238, 0] and w[15].tolist() == [255, 255, 0]
    assert w[21].tolist() == [0, 255, 0] and w[25].tolist() == [0, 255, 255] and w[36].tolist() == [0, 0, 255]
    assert w[49].tolist() == [255, 0, 255] and w[54].tolist() == [255, 0, 43]
    assert (w.max(axis=1) == 255).all()                              # every entry has a channel at full value


@pytest.mark.parametrize("name", K.GOLDEN_CASES)
def test_reference_colour_code_equals_flow_to_image(golden, name):
    """exactly, on every compared pixel; at most MAX_EXCLUDED pixels (those that attain the largest radius) are left out,
    and those are drawn inside (at full saturation, not dimmed by a quarter)"""
    flow, img = golden[f"{name}_flow"], golden[f"{name}_image"]
    r = Hn.flow_colour_reference(torch.from_numpy(flow.transpose(2, 0, 1).copy())[None])
    cmp = K.compared(r["raw"][0], r["max_rad"][0]) | ~r["known"][0]
    assert int((~cmp).sum()) <= K.MAX_EXCLUDED
    assert np.array_equal(r["rgb"][0][cmp], img[cmp])
    assert r["inside"][0][~cmp].all()
    assert (r["rgb"][0][~cmp].max(axis=-1) >= 254).all()             # the wheel's own colour: a channel at full value
    if name == "unknown":
        for y, x in K.UNKNOWN_AT:
            assert r["rgb"][0][y, x].tolist() == [0, 0, 0] and not r["known"][0][y, x]
        assert r["max_rad"][0] < 100.0                               # the unknown pixels did not enter the maximum


def test_supplied_radius_dims_the_pixels_beyond_it_and_scale_applies():
    flow = torch.zeros(1, 2, 1, 4)
    flow[0, 0] = torch.tensor([[1.0, 2.0, 4.0, -4.0]])               # along +x / -x: a = +/-1 or 0 on the wheel
    own = Hn.flow_colour_reference(flow)["rgb"][0, 0]
    half = Hn.flow_colour_reference(flow, max_rad=torch.tensor([2.0]))
    assert half["inside"][0, 0].tolist() == [True, True, False, False]
    # u = 4 (a = atan2(-0, -4) / pi = -1 -> wheel[1] = red... of -u): the saturated colour, then dimmed by a quarter
    full = Hn.flow_colour_reference(flow[..., 2:], max_rad=torch.tensor([4.0]))["rgb"][0, 0]
    assert np.array_equal(half["rgb"][0, 0, 2:], np.floor(full.astype(np.float64) * 0.75).astype(np.uint8))
    assert np.array_equal(own[2:], full)
    scaled = Hn.flow_colour_reference(flow / 8.0, scale=(8.0, 1.0))["rgb"][0, 0]
    assert np.array_equal(scaled, own)


def test_frame_tile_on_hand_computed_values():
    x = np.array([-1.0, 1.0, 0.0, 1.5, -2.0, -1.0 + 1.0 / 127.5, 0.5, float("nan")], dtype=np.float32)
    got = Hn.frame_tile_reference(np.broadcast_to(x[None, None, None, :], (1, 3, 1, 8)).copy())
    assert got.shape == (1, 1, 8, 3)
    # (0.5 + 1) * 127.5 + 0.5 = 191.75
    assert got[0, 0, :, 0].tolist() == [0, 255, 128, 255, 0, 1, 191, 0]


def test_heat_tile_on_hand_computed_values():
    e = np.array([[[0.0, 0.5, 1.0, 2.0, 0.25]]])
    hot = Hn.heat_tile_reference(e, np.array([1.0]), 77.0, 1.0)[0, 0]
    # t = 0: (0, 0, .5); t = .5: (.5, 1, .5); t = 1 (and beyond): (.5, 0, 0); t = .25: (0, .5, 1);  floor(255 c + .5)
    assert hot.tolist() == [[0, 0, 128], [128, 255, 128], [128, 0, 0], [128, 0, 0], [0, 128, 255]]
    assert (Hn.heat_tile_reference(e, np.array([1.0]), 77.0, 0.0) == 77).all()          # alpha 0: the grey alone
    assert Hn.heat_tile_reference(e, np.array([0.0]), 77.0, 1.0)[0, 0].tolist() == [[0, 0, 128]] * 5      # heat_max 0: t = 0
    # alpha .5 over grey 100 at t = .5: .5 * 100 + .5 * 255 * (.5, 1, .5) + .5 = (114.25, 178, 114.25)
    assert Hn.heat_tile_reference(e, np.array([1.0]), 100.0, 0.5)[0, 0, 1].tolist() == [114, 178, 114]


def test_reference_stats_tiles_and_layout():
    shape = (3, 21, 27)
    rp, rt, fp, ft = K.inputs(shape)
    ref = K.reference(shape)
    b, h, w = shape
    assert ref["panels"].shape == (b, 2 * h, 3 * w, 3) and ref["panels"].dtype == np.uint8
    for r, row in enumerate(Hn.RENDER_DEFAULT_TILES):
        for c, name in enumerate(row):
            assert np.array_equal(ref["panels"][:, r * h:(r + 1) * h, c * w:(c + 1) * w], ref[name]), name
    st = ref["stats"]
    assert st.dtype == np.float32 and st.shape == (b, 4) and np.isfinite(st).all()
    assert st[0, 2] == 0 and st[0, 3] == 0                           # sample 0: pred == target
    assert st[b - 1, 0] == 0 and (ref["op_target"][b - 1] == 255).all()               # the zero flow: white
    grey = ref["rgb_target"][:1].astype(np.float64).sum(axis=3) / 3.0
    assert np.array_equal(ref["rgb_heat"][0], Hn.heat_tile_reference(np.zeros((1, h, w)), np.ones(1), grey, 0.6)[0])     # t = 0
    assert st[:, 0].max() < 10.0                                     # planted 1e9 / -3e8 / NaN stayed out of the maxima
    s = b // 2
    assert ref["op_target"][s, h // 2, w // 3].tolist() == [0, 0, 0] and ref["op_pred"][s, h - 1, 0].tolist() == [0, 0, 0]
    # a subset, reordered, in one row and as a column
    sub = Hn.render_reference(rp, rt, fp, ft, tiles=("op_heat", "rgb_pred"), flow_scale=K.FLOW_SCALE)
    assert sub["panels"].shape == (b, h, 2 * w, 3)
    assert np.array_equal(sub["panels"][:, :, :w], ref["op_heat"]) and np.array_equal(sub["panels"][:, :, w:], ref["rgb_pred"])
    col = Hn.render_reference(rp, rt, fp, ft, tiles=(("op_pred",), ("op_target",)), flow_scale=K.FLOW_SCALE)
    assert np.array_equal(col["panels"][:, :h], ref["op_pred"]) and np.array_equal(col["panels"][:, h:], ref["op_target"])
    # "each": the predicted flow by its own maximum = the stand-alone colour code
    each = K.reference(shape, "each")
    assert np.array_equal(each["op_pred"], Hn.flow_colour_reference(fp, K.FLOW_SCALE)["rgb"])
    assert np.array_equal(each["op_target"], ref["op_target"])
    for bad in ((), ("rgb_pred", "rgb_pred"), ("rgb",), (("rgb_pred", "op_pred"), ("rgb_heat",))):
        with pytest.raises(ValueError):
            Hn.panel_layout(bad)
    with pytest.raises(ValueError):
        Hn.panel_layout(Hn.RENDER_TILES + ("rgb_pred",))


def test_c_entries_reject_bad_arguments_without_a_gpu():
    """argument errors are status codes decided before any HIP call (fake, aligned, never dereferenced addresses)"""
    import ctypes as C
    lib = _lib.load()
    P = 0x100000
    n = 8 * 8
    ins = [P, 3 * n, 2 * P, 3 * n, 3 * P, 2 * n, 4 * P, 2 * n]

    def stats(ins=ins, b=2, h=8, w=8, su=1.0, sv=1.0, out=5 * P):
        return lib.ammc_render_stats_f32(*ins, b, h, w, su, sv, out, None)
    assert stats(out=None) == -1 and stats(out=5 * P + 2) == -1
    assert stats(b=0) == -1 and stats(h=0) == -1 and stats(w=-1) == -1
    assert stats(su=float("inf")) == -1 and stats(sv=float("nan")) == -1
    assert stats(ins=[None, 0] * 4) == -1                                   # nothing to read
    assert stats(ins=[None, 0] + ins[2:]) == -1                             # the frame pair: both or neither
    assert stats(ins=[P + 2] + ins[1:]) == -1                               # a float pointer off its alignment
    assert stats(ins=ins[:5] + [2 * n - 1] + ins[6:]) == -1                 # a batch stride below a sample
    assert stats(b=65536) == -2 and stats(h=1 << 15, w=1 << 14, b=1) == -2

    def panels(ins=ins, b=2, h=8, w=8, su=1.0, sv=1.0, tiles=(0, 1, 2, 3, 4, 5), rows=2, cols=3, st=5 * P, each=0, mr=None,
               hr=None, ho=None, alpha=0.6, out=6 * P, out_bs=6 * n * 3):
        arr = (C.c_int32 * max(len(tiles), 1))(*tiles) if tiles is not None else None
        return lib.ammc_render_panels_u8(*ins, b, h, w, su, sv, arr, rows, cols, st, each, mr, hr, ho, alpha, out, out_bs, None)
    assert panels(tiles=None) == -1 and panels(out=None) == -1
    assert panels(rows=0) == -1 and panels(rows=3, cols=3) == -1 and panels(rows=7, cols=1) == -1
    assert panels(tiles=(0, 1, 2, 3, 4, 6)) == -1 and panels(tiles=(0, 1, 2, 3, 4, 4)) == -1 and panels(tiles=(0, -1), rows=1, cols=2) == -1
    assert panels(alpha=1.5) == -1 and panels(alpha=-0.1) == -1 and panels(alpha=float("nan")) == -1 and panels(each=2) == -1
    assert panels(st=None) == -1                                            # a normalisation nobody supplies
    assert panels(ins=[None, 0] + ins[2:]) == -1                            # rgb_heat / rgb_pred read rgb_pred
    assert panels(tiles=(3,), rows=1, cols=1, st=None, ins=[None, 0] * 3 + ins[6:]) == -1      # op_target by its own maximum: stats
    assert panels(out_bs=6 * n * 3 - 1) == -1 and panels(mr=P + 1) == -1 and panels(b=0) == -1 and panels(b=70000) == -2

    def colour(flow=P, bs=2 * n, b=2, h=8, w=8, su=1.0, sv=1.0, mr=None, ws=2 * P, out=3 * P, out_bs=n * 3):
        return lib.ammc_flow_colour_u8(flow, bs, b, h, w, su, sv, mr, ws, out, out_bs, None)
    assert colour(flow=None) == -1 and colour(out=None) == -1 and colour(ws=None) == -1 and colour(ws=2 * P + 1) == -1
    assert colour(bs=2 * n - 1) == -1 and colour(out_bs=n * 3 - 1) == -1 and colour(h=0) == -1 and colour(su=float("inf")) == -1
    assert colour(b=65536) == -2


def test_ops_argument_checks_come_before_any_hip_call():
    b, h, w = 2, 8, 12
    rp, rt = torch.zeros(b, 3, h, w), torch.zeros(b, 3, h, w)
    fp, ft = torch.zeros(b, 2, h, w), torch.zeros(b, 2, h, w)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.render_panels(rp, rt, fp, ft)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.flow_to_rgb(ft)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.render_stats(rp, rt, fp, ft)
    for bad in (dict(rgb_pred=rp[:, :2]), dict(rgb_target=rt.double()), dict(op_pred=fp[:1]), dict(op_target=ft[..., :8]),
                dict(op_target=ft.transpose(2, 3).contiguous().transpose(2, 3)), dict(rgb_pred=rp[0])):
        args = dict(rgb_pred=rp, rgb_target=rt, op_pred=fp, op_target=ft)
        args.update(bad)
        with pytest.raises(ValueError, match="render_panels"):
            ops.render_panels(**args)
    for kw, why in ((dict(tiles=("rgb_pred", "nope")), "unknown tile"), (dict(tiles=("rgb_pred", "rgb_pred")), "at most once"),
                    (dict(alpha=1.2), "alpha"), (dict(alpha="x"), "alpha"), (dict(flow_norm="frame"), "flow_norm"),
                    (dict(flow_norm=torch.ones(3)), "flow_norm"), (dict(heat_max="each"), "heat_max"),
                    (dict(heat_max=torch.ones(b).double()), "heat_max"), (dict(heat_max=(torch.ones(b),)), "heat_max"),
                    (dict(flow_scale=(1.0,)), "scale"), (dict(flow_scale=(float("inf"), 1.0)), "scale"),
                    (dict(out=torch.zeros(b, 2 * h, 3 * w, 3)), "out must be"),
                    (dict(out=torch.zeros(b, h, w, 3, dtype=torch.uint8)), "out must be")):
        with pytest.raises(ValueError, match=why):
            ops.render_panels(rp, rt, fp, ft, **kw)
    for kw in (dict(scale=(1.0, 2.0, 3.0)), dict(max_rad=torch.ones(b + 1)), dict(out=torch.zeros(b, h, w, 3))):
        with pytest.raises(ValueError, match="flow_to_rgb"):
            ops.flow_to_rgb(ft, **kw)
    with pytest.raises(ValueError, match="flow_to_rgb"):
        ops.flow_to_rgb(rt)


def test_writer_pool_keeps_the_order_and_bounds_the_queue():
    pool = Hn.OrderedWriterPool(workers=3)
    running, peak, lock = [0], [0], threading.Lock()

    def job(i):
        with lock:
            running[0] += 1
            peak[0] = max(peak[0], running[0])
        time.sleep(0.002 * ((7 * i) % 5))                            # later jobs finish before earlier ones
        with lock:
            running[0] -= 1
        return i
    for i in range(40):
        pool.submit(job, i)
    assert pool.close() == list(range(40))
    assert 1 <= peak[0] <= 3 and pool.busy_s > 0
    assert Hn.OrderedWriterPool(workers=64).workers == 16
    with pytest.raises(ValueError):
        Hn.OrderedWriterPool(workers=0)


def test_writer_pool_propagates_the_first_error():
    def job(i):
        if i == 5:
            raise OSError(f"disk full at {i}")
        return i
    pool = Hn.OrderedWriterPool(workers=2)
    with pytest.raises(OSError, match="disk full at 5"):
        for i in range(200):
            pool.submit(job, i)
        pool.close()
    pool = Hn.OrderedWriterPool(workers=2)
    for i in range(6):
        pool.submit(job, i)
    with pytest.raises(OSError, match="disk full at 5"):
        pool.close()


def test_write_panel_round_trips(tmp_path):
    from PIL import Image
    panel = (np.arange(6 * 10 * 3) % 251).astype(np.uint8).reshape(6, 10, 3)
    p = Hn.write_panel(str(tmp_path / "a.png"), panel, "png")
    assert np.array_equal(np.asarray(Image.open(p)), panel)
    p = Hn.write_panel(str(tmp_path / "a.npy"), panel, "npy")
    assert np.array_equal(np.load(p), panel)
    with pytest.raises(ValueError):
        Hn.write_panel(str(tmp_path / "a.jpg"), panel, "jpg")


def test_select_frames():
    psnr = np.array([9, 9, 9, 9, 30.0, 20.0, 25.0, 20.0, 40.0, 10.0], dtype=np.float32)
    assert Hn.select_frames(psnr) == [4, 5, 6, 7, 8, 9]
    assert Hn.select_frames(psnr, every=2) == [4, 6, 8]
    assert Hn.select_frames(psnr, top=3) == [5, 7, 9]                # 10, 20, 20: the earlier of equal frames first
    assert Hn.select_frames(psnr, top=2) == [5, 9]
    assert Hn.select_frames(psnr, every=2, top=1) == [6] and Hn.select_frames(psnr, top=100) == [4, 5, 6, 7, 8, 9]
    with pytest.raises(ValueError):
        Hn.select_frames(psnr, every=0)


def test_run_panels_options_and_refusals(monkeypatch, capsys):
    a = run_panels.parse_options(["--synthetic", "--panels_dir", "x"])
    assert a.tiles == [list(r) for r in Hn.RENDER_DEFAULT_TILES] and a.flow_norm == "target" and a.heat_max == "frame"
    assert (a.alpha, a.every, a.top, a.workers, a.format) == (0.6, 1, None, 8, "png")
    a = run_panels.parse_options(["--synthetic", "--panels_dir", "x", "--tiles", "rgb_pred,op_pred/rgb_heat,op_heat", "--flow_norm",
                                  "2.5", "--heat_max", "0.05", "--alpha", "1", "--every", "3", "--top", "4", "--workers", "99",
                                  "--format", "npy"])
    assert a.tiles == [["rgb_pred", "op_pred"], ["rgb_heat", "op_heat"]] and a.flow_norm == 2.5 and a.heat_max == 0.05
    assert (a.alpha, a.every, a.top, a.workers, a.format) == (1.0, 3, 4, 16, "npy")
    assert run_panels.parse_options(["--synthetic", "--panels_dir", "x", "--flow_norm", "each"]).flow_norm == "each"
    for bad in (["--tiles", "rgb_pred,flow"], ["--tiles", "rgb_pred,rgb_pred"], ["--tiles", "rgb_pred,op_pred/rgb_heat"], ["--tiles", ""],
                ["--flow_norm", "frame"], ["--flow_norm", "-1"], ["--heat_max", "each"], ["--heat_max", "0"], ["--heat_max", "nan"],
                ["--alpha", "1.5"], ["--every", "0"], ["--top", "0"], ["--workers", "0"], ["--format", "jpg"]):
        with pytest.raises(SystemExit):
            run_panels.parse_options(["--synthetic", "--panels_dir", "x"] + bad)
    with pytest.raises(SystemExit):
        run_panels.parse_options(["--synthetic"])                    # --panels_dir is required
    with pytest.raises(SystemExit) as info:
        run_panels.parse_options(["--panels_dir", "x"])
    assert "--synthetic" in str(info.value.code)
    capsys.readouterr()
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_panels.main(["--synthetic", "--panels_dir", "x"])
    assert "one GPU" in str(info.value.code) and capsys.readouterr().out == ""
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (0, 1, torch.device("cpu")))
    with pytest.raises(SystemExit) as info:
        run_panels.main(["--synthetic", "--panels_dir", "x"])
    assert "needs a GPU" in str(info.value.code)


def test_run_panels_takes_every_option_of_run_maps_but_its_own():
    theirs = {a.dest for a in run_maps.build_parser()._actions}
    ours = {a.dest for a in run_panels.build_parser()._actions}
    assert theirs - {"maps_dir", "patch", "pixel_maps"} <= ours
