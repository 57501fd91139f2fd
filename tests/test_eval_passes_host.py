"""The pass driver of the evaluation harness (`harness._run_pass`) and the entries' scaffold
(`_entry`) on the CPU: a stub model with the evaluation forward's signature stands in for the HIP model, so the frame
assembly, the S16 range-guard re-run, the int32 sections, the scratch sections and the `predictions` hook run without a
device.  Every value is a small integer held in fp32: sums are exact in any order and `np.array_equal` applies."""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _entry, harness as Hn, parallel
from ammcnet_aaai2021_amd import run_fusion, run_maps, run_memory, run_panels, run_pixel, run_quality, run_test

SHIFT = 4096.0          # what the stub's exact run adds to everything it returns
NAN_BITS = 2143289345   # 0x7fc00001: a NaN when read as fp32


def make_frames(t: int):
    """8 x 8 frames whose values say which frame they are: small integers, different per frame, channel and pixel"""
    px = torch.arange(64, dtype=torch.float32).reshape(8, 8) % 5
    rgb = torch.stack([torch.stack([px + f + c for c in range(3)]) for f in range(t)])
    op = torch.stack([torch.stack([px + 2 * f + 7 * c for c in range(2)]) for f in range(t - 1)])
    return rgb.contiguous(), op.contiguous()


class StubModel(torch.nn.Module):
    """`forward_scored` of the HIP model on the CPU: everything it returns is a sum of its inputs, shifted by SHIFT when
    `exact`; `calls` logs (first clip, exact); `last_overflow` is set for the batches whose first clip is in `overflow`
    unless the run is exact"""

    def __init__(self, overflow=()):
        super().__init__()
        self.overflow, self.calls = set(overflow), []

    def forward_scored(self, rgb_in, op_in, rgb_t, op_t, defer_guard=False, exact=False):
        assert defer_guard and not torch.is_grad_enabled()
        s = int(rgb_t[0, 0, 0, 0]) - (Hn.RGB_LEN_CLIP - 1)                    # pixel (0, 0) of channel 0 holds the frame index
        self.calls.append((s, bool(exact)))
        shift = SHIFT if exact else 0.0
        self.last_overflow = torch.tensor([0.0 if exact or s not in self.overflow else 1.0])
        rgb_out, op_out = rgb_t + rgb_in[:, :3] + shift, op_t + op_in[:, :2] + shift
        diffs = (rgb_in.sum() + shift, op_in.sum() + shift)
        return (rgb_out, op_out, diffs, None), rgb_in.sum(dim=(1, 2, 3)) + shift, op_t.sum(dim=(1, 2, 3)) + shift


SECTIONS = [("rgb_score", ()), ("op_vec", (2, 3)), ("rgb_count", ()), ("op_room", (3,))]


def run_driver(t, batch, overflow=(), predictions=None, sections=SECTIONS, scratch=("op_room",), seen=None):
    model = StubModel(overflow)
    rgb, op = make_frames(t)
    batches = Hn._checked_batches(None, rgb, op, batch)

    def on_batch(slots, s, e, k, fwd):
        if seen is not None:
            seen.append(slots)
        slots.view("rgb_score")[s:e] = fwd.fused[0]
        slots.view("op_vec")[s:e] = fwd.op_pred[:, :, 0, :3]
        slots.view("rgb_count")[s:e] = (NAN_BITS + torch.arange(s, e, dtype=torch.int32)) * (1 - 2 * (torch.arange(s, e, dtype=torch.int32) % 2))
        slots.view("op_room")[s:e] = 1.0
    rec = Hn._run_pass(model, rgb, op, batches, sections, ("rgb_count",), on_batch, predictions, scratch=scratch)
    return model, batches, rec


def expected(t, batch, exact_batches=()):
    """the records frame by frame, from the frames alone: frame f >= lc - 1 takes clip f - (lc - 1), the first lc - 1
    frames copy frame lc - 1, the flow stream's last frame copies the one before"""
    rgb, op = (x.numpy() for x in make_frames(t))
    n_clip = t - 4
    ends = [min(s + batch, n_clip) for s in range(0, n_clip, batch)]

    def shift(c):
        return np.float32(SHIFT if c // batch in exact_batches else 0.0)
    out = {"rgb_score": np.empty(t, np.float32), "op_vec": np.empty((t, 2, 3), np.float32), "rgb_count": np.empty(t, np.int32),
           "rgb_comm": np.empty(t, np.float32), "op_comm": np.empty(t, np.float32)}
    for f in range(t):
        c = max(f, 4) - 4                                                      # the rgb stream: lc = 5
        s, e = c // batch * batch, ends[c // batch]
        out["rgb_score"][f] = rgb[c:c + 4].sum() + shift(c)
        out["rgb_count"][f] = (NAN_BITS + c) * (1 - 2 * (c % 2))
        out["rgb_comm"][f] = sum(rgb[i:i + 4].sum() for i in range(s, e)) + shift(c)
        c = min(max(f, 3), t - 2) - 3                                          # the flow stream: lc = 4
        s, e = c // batch * batch, ends[c // batch]
        out["op_vec"][f] = op[c + 3][:, 0, :3] + op[c][:, 0, :3] + shift(c)
        out["op_comm"][f] = sum(op[i:i + 3].sum() for i in range(s, e)) + shift(c)
    return out


def assert_records(rec, want):
    assert set(rec) == set(want)
    for key, w in want.items():
        assert rec[key].dtype == w.dtype and rec[key].shape == w.shape, key
        assert np.array_equal(rec[key].view(np.int32), w.view(np.int32)), key     # bit for bit (the int32 section holds NaN patterns)


@pytest.mark.parametrize("t,batch", [(11, 4), (5, 16), (21, 16)])
def test_driver_assembles_the_frames_of_every_batch(t, batch):
    model, batches, rec = run_driver(t, batch)
    assert batches == Hn.subvideo_batches(t, batch) and model.calls == [(s, False) for s, _ in batches]
    assert_records(rec, expected(t, batch))
    assert not hasattr(model, "s16_fallbacks")


def test_driver_reruns_only_the_flagged_batch_exactly():
    preds = []
    model, batches, rec = run_driver(15, 4, overflow=(4,), predictions=preds)
    assert batches == [(0, 4), (4, 8), (8, 11)]
    assert model.calls == [(0, False), (4, False), (8, False), (4, True)]
    assert model.s16_fallbacks == 1
    assert_records(rec, expected(15, 4, exact_batches=(1,)))
    plain = expected(15, 4)
    assert np.array_equal(rec["rgb_score"][:8], plain["rgb_score"][:8]) and np.array_equal(rec["rgb_score"][12:], plain["rgb_score"][12:])
    assert np.array_equal(rec["rgb_score"][8:12], plain["rgb_score"][8:12] + np.float32(SHIFT))
    # the hook: one tuple per batch in batch order, the flagged batch's from its exact run
    rgb, op = make_frames(15)
    assert [(s, e) for s, e, *_ in preds] == batches
    for k, (s, e, rgb_pred, op_pred, fused) in enumerate(preds):
        shift = SHIFT if k == 1 else 0.0
        assert torch.equal(rgb_pred, rgb[s + 4:e + 4] + rgb[s:e] + shift) and torch.equal(op_pred, op[s + 3:e + 3] + op[s:e] + shift)
        assert len(fused) == 2 and torch.equal(fused[1], op[s + 3:e + 3].sum(dim=(1, 2, 3)) + shift)


def test_driver_without_a_flag_runs_every_batch_once():
    model, batches, rec = run_driver(15, 4)
    assert model.calls == [(0, False), (4, False), (8, False)] and not hasattr(model, "s16_fallbacks")
    assert_records(rec, expected(15, 4))


def test_driver_reruns_every_flagged_batch_in_batch_order():
    model, batches, rec = run_driver(15, 4, overflow=(0, 4, 8))
    assert model.calls == [(0, False), (4, False), (8, False), (0, True), (4, True), (8, True)]
    assert model.s16_fallbacks == 3
    assert_records(rec, expected(15, 4, exact_batches=(0, 1, 2)))
    model.overflow = set()                                      # a model counts across sub-videos: nothing is added without a flag
    rgb, op = make_frames(9)
    Hn._run_pass(model, rgb, op, Hn._checked_batches(None, rgb, op, 4), [("rgb_x", ())], (), lambda *a: None)
    assert model.s16_fallbacks == 3


def test_int32_sections_come_back_bit_for_bit_and_sections_are_aligned():
    seen = []
    _, _, rec = run_driver(11, 4, seen=seen)
    assert rec["rgb_count"].dtype == np.int32
    clips = np.r_[[0] * 4, np.arange(7)]
    assert np.array_equal(rec["rgb_count"], (NAN_BITS + clips) * (1 - 2 * (clips % 2)))
    assert np.isnan(rec["rgb_count"][::2].view(np.float32)).all() and (rec["rgb_count"][5::2] < 0).all()
    layout = seen[0].layout                                                    # 7 clips: rows of 1, 6, 1 and 3 elements
    assert list(layout) == ["rgb_score", "op_vec", "rgb_count", "op_room", "comm", "flag"]
    assert [off for off, _ in layout.values()] == [0, 8, 52, 60, 84, 88]
    assert all(off % 4 == 0 for off, _ in layout.values()) and seen[0].flat.numel() == 92


def test_scratch_sections_are_not_returned():
    _, _, rec = run_driver(11, 4)
    assert "op_room" not in rec and set(rec) == {"rgb_score", "op_vec", "rgb_count", "rgb_comm", "op_comm"}
    _, _, rec = run_driver(11, 4, scratch=())
    assert rec["op_room"].shape == (11, 3) and (rec["op_room"] == 1.0).all()


def test_sub_video_checks():
    rgb, op = make_frames(4)
    with pytest.raises(ValueError, match="at least 5 frames"):
        Hn._checked_batches(None, rgb, op, 4)
    rgb, op = make_frames(11)
    for bad in (op[:-1], torch.cat([op, op[:1]])):
        with pytest.raises(ValueError, match="T-1 flows"):
            Hn._checked_batches(None, rgb, bad, 4)
    assert Hn._checked_batches(None, rgb, op, 4) == [(0, 4), (4, 7)]


def test_public_passes_refuse_cpu_tensors():
    rgb, op = make_frames(11)
    model = StubModel()
    calls = {"localise_subvideo": lambda: Hn.localise_subvideo(model, rgb, op),
             "memory_subvideo": lambda: Hn.memory_subvideo(model, rgb, op),
             "quality_subvideo": lambda: Hn.quality_subvideo(model, rgb, op),
             "pixel_subvideo": lambda: Hn.pixel_subvideo(model, rgb, op, torch.zeros((11, 8, 8), dtype=torch.uint8)),
             "render_subvideo": lambda: next(Hn.render_subvideo(model, rgb, op))}
    for name, call in calls.items():
        with pytest.raises(ValueError) as info:
            call()
        assert str(info.value) == f"{name} reads a sub-video resident on the GPU (contiguous tensors): move it there first"
    assert model.calls == []


# ---- the entries' scaffold --------------------------------------------------------------------------------------------

DATASETS = ("avenue", "ped2", "shanghaitech")
# (option strings, default, choices, required), in the parser's order
COMMON = [(("--dataset_name",), "ped2", DATASETS, False), (("--ckpt",), None, None, False), (("--data",), None, None, False),
          (("--synthetic",), False, None, False), (("--raw",), False, None, False), (("--rgb_root",), None, None, False),
          (("--op_root",), None, None, False), (("--videos",), 4, None, False), (("--frames",), 60, None, False),
          (("--size",), 256, None, False), (("--precision",), "s16", ("fp32", "s16"), False), (("--embed_dim",), 64, None, False),
          (("--n_embed",), 256, None, False), (("--k",), 2, None, False)]
QUALITY = [(("--maps_dir",), None, None, False), (("--ssim_maps",), False, None, False)]
OPTIONS = {
    run_test: COMMON,
    run_maps: [(("--maps_dir",), None, None, True), (("--patch",), 16, (8, 16, 32), False), (("--pixel_maps",), False, None, False)] + COMMON,
    run_memory: [(("--maps_dir",), None, None, False), (("--slots",), False, None, False)] + COMMON,
    run_quality: QUALITY + COMMON,
    run_pixel: [(("--patch",), 16, (8, 16, 32), False), (("--frac",), [2, 5], None, False),
                (("--normalise",), "none", ("none", "video"), False), (("--mask_root",), None, None, False)] + COMMON,
    run_fusion: QUALITY + COMMON + [(("--records",), None, None, False), (("--save_records",), None, None, False),
                                    (("--channels",), "rgb_img_pred,rgb_fea_comm", None, False), (("--step",), None, None, False),
                                    (("--out",), None, None, False)],
    run_panels: [(("--panels_dir",), None, None, True), (("--format",), "png", ("png", "npy"), False),
                 (("--tiles",), "rgb_target,rgb_pred,rgb_heat/op_target,op_pred,op_heat", None, False),
                 (("--flow_norm",), "target", None, False), (("--heat_max",), "frame", None, False), (("--alpha",), 0.6, None, False),
                 (("--every",), 1, None, False), (("--top",), None, None, False), (("--workers",), 8, None, False)] + COMMON,
}


@pytest.mark.parametrize("entry", list(OPTIONS), ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_entry_options_are_what_they_were(entry):
    got = [(tuple(a.option_strings), a.default, tuple(a.choices) if a.choices is not None else None, bool(a.required))
           for a in entry.build_parser()._actions if a.dest != "help"]
    assert got == OPTIONS[entry]


def test_load_sources_synthetic_and_none():
    a = run_test.build_parser().parse_args(["--synthetic", "--videos", "2", "--frames", "12", "--size", "16"])
    sources, gt, streamed = _entry.load_sources(a)
    assert not streamed and len(sources) == 2 and len(gt) == 2
    assert [tuple(rgb.shape) for rgb, _ in sources] == [(12, 3, 16, 16), (19, 3, 16, 16)]
    assert [tuple(op.shape) for _, op in sources] == [(11, 2, 16, 16), (18, 2, 16, 16)]
    assert [g.shape for g in gt] == [(12,), (19,)] and all(set(np.unique(g)) <= {0, 1} for g in gt)
    assert run_test.synthetic_dataset is _entry.synthetic_dataset and run_test.synthetic_raw_sources is _entry.synthetic_raw_sources
    a = run_test.build_parser().parse_args(["--synthetic", "--raw", "--videos", "2", "--frames", "12"])
    sources, gt, streamed = _entry.load_sources(a)
    assert streamed and len(sources) == 2 and [g.shape for g in gt] == [(12,), (19,)]
    for argv in ([], ["--rgb_root", "x"], ["--raw"]):
        with pytest.raises(SystemExit) as info:
            _entry.load_sources(run_test.build_parser().parse_args(argv))
        assert info.value.code == "give --data, --rgb_root/--op_root or --synthetic"
    with pytest.raises(SystemExit) as info:
        _entry.load_sources(run_test.build_parser().parse_args([]), "--records, --data, --rgb_root/--op_root or --synthetic")
    assert info.value.code == "give --records, --data, --rgb_root/--op_root or --synthetic"


def test_device_exits_keep_their_words(monkeypatch):
    phrases = {"run_maps": ": sharded map writing is not implemented", "run_memory": ": sharded map writing is not implemented",
               "run_quality": ": sharded map writing is not implemented",
               "run_pixel": ": sharded pixel-level evaluation is not implemented",
               "run_panels": ": sharded picture writing is not implemented", "run_fusion": ""}
    argv = {"run_maps": ["--maps_dir", "x"], "run_panels": ["--panels_dir", "x"]}
    for entry in (run_maps, run_memory, run_quality, run_pixel, run_panels, run_fusion):
        name = entry.__name__.rsplit(".", 1)[-1]
        monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (1, 2, torch.device("cpu")))
        with pytest.raises(SystemExit) as info:
            entry.main(["--synthetic"] + argv.get(name, []))
        assert info.value.code == f"{name} runs on one GPU{phrases[name]} (start a single process)"
        monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (0, 1, torch.device("cpu")))
        with pytest.raises(SystemExit) as info:
            entry.main(["--synthetic"] + argv.get(name, []))
        assert info.value.code == f"{name} needs a GPU: the HIP path has no CPU fallback"
    with pytest.raises(SystemExit) as info:
        run_test.main(["--synthetic"])
    assert info.value.code == "run_test needs a GPU: the HIP path has no CPU fallback"


def test_base_report_fields_rounding_and_order():
    a = run_test.build_parser().parse_args(["--synthetic", "--dataset_name", "avenue", "--precision", "fp32"])
    model = types.SimpleNamespace(s16_fallbacks=3)
    out = _entry.base_report(a, model, [12, 19], 0.123456)
    assert list(out.items()) == [("dataset", "avenue"), ("videos", 2), ("predicted_frames", 23), ("gpus", 1), ("total_time_s", 0.123),
                                 ("fps", round(23 / 0.123456, 2)), ("precision", "fp32"), ("s16_fallbacks", 3)]
    st = types.SimpleNamespace(host_seconds=1.23456, bytes_uploaded=3 * 2**20 + 2**19)
    out = _entry.base_report(a, object(), [12], 2.0, st, "quality", gpus=8)
    assert list(out.items())[3:] == [("gpus", 8), ("total_time_s", 2.0), ("fps", 4.0), ("precision", "fp32"), ("s16_fallbacks", 0),
                                     ("host_read_s", 1.235), ("uploaded_MB", 3.5),
                                     ("staging", "streamed: overlapped with the quality loop (total_time_s covers it)")]
