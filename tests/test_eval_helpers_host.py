"""The helpers the evaluation ops and the mask-aware passes share, on the CPU: the `out=` table of
`ops` (`_slots`, `_bs`), the one slot class of the harness (`_Slots`), the mask path (`_frame_mask`, `_checked_mask`) and
the entries' mask sources (`_entry.load_masks`).  Nothing here loads the HIP library."""
import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _entry, harness as Hn, ops, run_pixel

CPU = torch.device("cpu")
NAN_BITS = 0x7fc00001        # a NaN with a payload when read as fp32


# ---- ops._slots ---------------------------------------------------------------------------------------------------------

WANT = {"map": ((2, 3, 5), torch.float32), "count": ((2,), torch.int32), "table": ((2, 4), torch.int32)}


def _strided(shape, strides, n):
    return torch.zeros(n).as_strided(shape, strides)


def test_absent_slots_are_allocated_and_given_ones_returned():
    res, bs = ops._slots("op", None, CPU, 2, WANT, ("map",))
    assert list(res) == list(WANT) and bs == {"map": 15}
    for key, (shape, dtype) in WANT.items():
        assert tuple(res[key].shape) == shape and res[key].dtype == dtype and res[key].device == CPU and res[key].is_contiguous()
    mine = {"count": torch.zeros(2, dtype=torch.int32), "map": torch.zeros(2, 3, 5)}
    res, bs = ops._slots("op", mine, CPU, 2, WANT, ("map",))
    assert res["count"] is mine["count"] and res["map"] is mine["map"] and tuple(res["table"].shape) == (2, 4)
    assert list(res) == list(WANT) and list(mine) == ["count", "map"]          # `want`'s order; the caller's dict is left alone
    assert ops._slots("op", {}, CPU, 2, WANT, ("map",))[1] == {"map": 15}


@pytest.mark.parametrize("out,words", [
    ({"nope": torch.zeros(2)}, "no slot"),                                      # an unknown key
    ({"map": torch.zeros(2, 3, 6)}, "must be"),                                 # a wrong shape
    ({"map": torch.zeros(2, 3, 5, dtype=torch.float64)}, "must be"),            # a wrong dtype
    ({"count": torch.zeros(2)}, "must be"),
    ({"map": torch.zeros(2, 3, 5, device="meta")}, "must be"),                  # another device
    ({"map": np.zeros((2, 3, 5), np.float32)}, "must be"),                      # not a tensor
    ({"count": torch.zeros(4, dtype=torch.int32)[::2]}, "contiguous"),          # a 1-D slot with stride 2
    ({"table": torch.zeros(2, 8, dtype=torch.int32)[:, :4]}, "contiguous"),     # the kernel takes no stride for it
    ({"map": torch.zeros(2, 3, 10)[:, :, ::2]}, "contiguous"),                  # a sample with non-contiguous rows
    ({"map": torch.zeros(2, 6, 5)[:, ::2]}, "contiguous"),
    ({"map": _strided((2, 3, 5), (10, 5, 1), 25)}, "batch stride"),             # samples that overlap
    ({"map": _strided((2, 3, 5), (0, 5, 1), 15)}, "batch stride"),
])
def test_bad_slots_are_refused(out, words):
    with pytest.raises(ValueError, match=words) as info:
        ops._slots("some_op", out, CPU, 2, WANT, ("map",))
    assert str(info.value).startswith("some_op: ")


def test_batch_strides_are_reported_in_elements():
    wide = _strided((2, 3, 5), (40, 5, 1), 80)
    res, bs = ops._slots("op", {"map": wide}, CPU, 2, WANT, ("map",))
    assert res["map"] is wide and bs == {"map": 40}
    exact = _strided((2, 3, 5), (15, 5, 1), 30)
    assert ops._slots("op", {"map": exact}, CPU, 2, WANT, ("map",))[1] == {"map": 15}
    # one sample: torch may give its dimension any stride - the sample's size stands in for a smaller one
    want1 = {"map": ((1, 3, 5), torch.float32)}
    one = _strided((1, 3, 5), (1, 5, 1), 15)
    assert one.stride(0) == 1 and one.is_contiguous()
    assert ops._slots("op", {"map": one}, CPU, 1, want1, ("map",))[1] == {"map": 15}
    assert ops._slots("op", {"map": _strided((1, 3, 5), (64, 5, 1), 15)}, CPU, 1, want1, ("map",))[1] == {"map": 64}
    assert ops._bs(one, 15) == 15 and ops._bs(wide, 15) == 40 and ops._bs(wide[:1], 15) == 40
    # a [1] slot of any stride is contiguous
    ops._slots("op", {"count": torch.zeros(4, dtype=torch.int32)[::2][:1]}, CPU, 1, {"count": ((1,), torch.int32)})


def test_pair_parse():
    assert ops._pair("op", "frac", (2, 5), 4096) == (2, 5) and ops._pair("op", "iou", [1, 1], 1) == (1, 1)
    for bad in ((0, 5), (6, 5), (1, 4097), (1,), (1, 2, 3), 3, ("a", 1), None):
        with pytest.raises(ValueError, match="op: "):
            ops._pair("op", "frac", bad, 4096)


# ---- harness._Slots -----------------------------------------------------------------------------------------------------

SECTIONS = [("scalar", (), torch.float32), ("ints", (2, 3), torch.int32), ("odd", (5,), torch.uint8),
            ("bytes", (4, 7), torch.uint8), ("none", (0,), torch.float32)]


def test_sections_are_aligned_and_sized():
    slots = Hn._Slots(SECTIONS, CPU)
    assert list(slots.layout) == [name for name, _, _ in SECTIONS]
    # words: 1, 6, 2 (5 bytes), 7 (28 bytes), 0 - each section starts at the next multiple of four
    assert [off for off, _ in slots.layout.values()] == [0, 4, 12, 16, 24]
    assert all(off % 4 == 0 for off, _ in slots.layout.values())
    assert slots.flat.numel() == 24 and slots.flat.dtype == torch.int32 and not slots.flat.any()
    for name, shape, dtype in SECTIONS:
        v = slots.view(name)
        assert tuple(v.shape) == shape and v.dtype == dtype, name
        assert v.numel() == 0 or v.data_ptr() == slots.flat.data_ptr() + 4 * slots.layout[name][0], name
    assert Hn._Slots([], CPU).flat.numel() == 0


def test_device_and_host_views_agree_bit_for_bit():
    slots = Hn._Slots(SECTIONS, CPU)
    slots.view("scalar").fill_(-0.0)
    slots.view("ints").copy_(torch.tensor([[NAN_BITS, -NAN_BITS, 1], [-1, 2 ** 31 - 1, -2 ** 31]], dtype=torch.int32))
    slots.view("odd").copy_(torch.tensor([1, 2, 3, 4, 255], dtype=torch.uint8))
    slots.view("bytes").copy_((torch.arange(28) * 9 % 256).to(torch.uint8).reshape(4, 7))
    host = slots.flat.clone().numpy()                                          # the one copy
    for name, shape, dtype in SECTIONS:
        h = slots.view(name, host)
        assert h.shape == shape and h.dtype == Hn._SLOT_DTYPES[dtype], name
        assert np.array_equal(h.reshape(-1).view(np.uint8), slots.view(name).reshape(-1).view(torch.uint8).numpy()), name
    assert slots.view("ints", host)[0, 0] == NAN_BITS and np.isnan(slots.view("ints", host).view(np.float32)[0, 0])
    assert np.signbit(slots.view("scalar", host)) and slots.view("scalar", host) == 0.0
    # an fp32 section carries the pattern too: words are reinterpreted, never converted
    slots.view("scalar").view(torch.int32).fill_(NAN_BITS)
    assert slots.view("scalar", slots.flat.numpy()).view(np.int32) == NAN_BITS


@pytest.mark.parametrize("name", [name for name, shape, _ in SECTIONS if shape != (0,)])
def test_writing_one_section_leaves_the_others_zero(name):
    slots = Hn._Slots(SECTIONS, CPU)
    v = slots.view(name)
    (v.view(torch.int32) if v.dtype == torch.float32 else v).fill_(255 if v.dtype == torch.uint8 else -1)   # every bit of every byte
    off, (shape, dtype) = slots.layout[name]
    nbytes = int(np.prod(shape)) * (1 if dtype == torch.uint8 else 4)
    raw = slots.flat.numpy().view(np.uint8)
    assert raw[4 * off:4 * off + nbytes].all()
    raw[4 * off:4 * off + nbytes] = 0
    assert not raw.any()                                                       # the padding of the odd section included
    for other, _, _ in SECTIONS:
        assert other == name or not slots.view(other).any(), other


# ---- the mask path --------------------------------------------------------------------------------------------------------

def _mask():
    g = np.random.default_rng(7)
    return (g.random((6, 5, 9)) > 0.6).astype(np.uint8)


FRAMES = torch.zeros(6, 3, 8, 8)


@pytest.mark.parametrize("dtype", [np.bool_, np.uint8, np.int64, np.float64])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_frame_mask_is_resize_mask_of_the_uint8_mask(dtype, as_tensor):
    base = _mask()
    want = Hn.resize_mask(torch.from_numpy(base), (8, 8))
    given = (base * (1 if dtype in (np.bool_, np.uint8) else 3)).astype(dtype)   # nonzero becomes 1
    if dtype == np.float64:
        given = given * 0.25
    got = Hn._frame_mask("who", [None, torch.from_numpy(given) if as_tensor else given], 1, FRAMES)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (6, 8, 8) and got.is_contiguous() and got.device == FRAMES.device
    assert torch.equal(got, want) and 0 < int(got.sum()) < got.numel()
    assert torch.equal(Hn._checked_mask("who", got, 6, 8, 8, CPU), want)


def test_frame_mask_refusals_and_none():
    base = _mask()
    assert Hn._frame_mask("who", [None, base], 0, FRAMES) is None
    with pytest.raises(ValueError, match=r"who: mask 0 is \(5, 5, 9\), its sub-video has 6 frames"):
        Hn._frame_mask("who", [base[:5]], 0, FRAMES)
    with pytest.raises(ValueError, match="its sub-video has 6 frames"):
        Hn._frame_mask("who", [base[0]], 0, FRAMES)
    with pytest.raises(ValueError, match=r"who: 1 masks for more than 1 sub-videos \(None marks one without\)"):
        Hn._frame_mask("who", [base], 1, FRAMES)


def test_checked_mask():
    m = Hn.resize_mask(torch.from_numpy(_mask()), (8, 8)).contiguous()         # [6, 8, 8] uint8
    assert Hn._checked_mask("who", m, 6, 8, 8, CPU) is m
    as_bool = m != 0
    viewed = Hn._checked_mask("who", as_bool, 6, 8, 8, CPU)
    assert viewed.dtype == torch.uint8 and viewed.data_ptr() == as_bool.data_ptr() and torch.equal(viewed, m)   # the same memory
    wide = torch.zeros(6, 8, 16, dtype=torch.uint8)[:, :, ::2]
    assert Hn._checked_mask("who", wide, 6, 8, 8, CPU).is_contiguous()
    for bad in (m[:5], m[:, :7], m.to(torch.int64), m.float(), m[0], torch.zeros((6, 8, 8), dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match=r"who: mask must be uint8 \(6, 8, 8\) on cpu, got "):
            Hn._checked_mask("who", bad, 6, 8, 8, CPU)


def test_masked_dataset_loop_with_a_stub_pass():
    """`_evaluate_masked` around a pass that returns what it was given: the zero mask of a sub-video without one, the
    lists by key, `mask_videos`, and `mask` under `keep_maps` alone"""
    videos = [(torch.zeros(6, 3, 8, 8), torch.zeros(5, 2, 8, 8)), (torch.zeros(7, 3, 8, 8), torch.zeros(6, 2, 8, 8))]
    seen = []

    def subvideo(v, rgb, op, dm, keep):
        seen.append((v, keep, dm.clone()))
        t = rgb.shape[0]
        return {"rgb_psnr": np.full(t, v), "rgb_comm": np.zeros(t), "op_psnr": np.zeros(t), "op_comm": np.zeros(t), "x": np.full(t, 10 + v)}

    model = torch.nn.Linear(1, 1)
    for keep in (False, True):
        seen.clear()
        keys = ["x"] + (["mask"] if keep else [])
        out = Hn._evaluate_masked("who", model, videos, [_mask(), None], "name", keys, subvideo, keep, CPU)
        assert list(out) == ["dataset", "rgb_img_pred_records", "rgb_fea_comm_records", "op_img_pred_records", "op_fea_comm_records",
                             "n_frames", "mask_videos"] + keys
        assert out["n_frames"] == [6, 7] and out["mask_videos"] == [0] and out["x"][1] is None and (out["x"][0] == 10).all()
        assert [len(r) for r in out["rgb_img_pred_records"]] == [6, 7]           # the frame records of both
        assert [(v, k) for v, k, _ in seen] == [(0, keep), (1, False)]
        assert torch.equal(seen[0][2], Hn.resize_mask(torch.from_numpy(_mask()), (8, 8)))
        assert tuple(seen[1][2].shape) == (7, 8, 8) and seen[1][2].dtype == torch.uint8 and not seen[1][2].any()
        if keep:
            assert out["mask"][1] is None and np.array_equal(out["mask"][0], seen[0][2].numpy())
    with pytest.raises(ValueError, match="who: 1 masks for more than 1 sub-videos"):
        Hn._evaluate_masked("who", model, videos, [None], "name", ["x"], subvideo, False, CPU)


def test_frames_of_repeats_the_first_clip():
    a = np.arange(6, dtype=np.int32).reshape(3, 2)
    assert np.array_equal(Hn._frames_of(a), np.array([[0, 1]] * 5 + [[2, 3], [4, 5]])) and Hn._frames_of(a).dtype == np.int32


# ---- _entry.load_masks ----------------------------------------------------------------------------------------------------

def _args(*argv):
    return run_pixel.build_parser().parse_args(list(argv))


def _fail(*a, **k):
    raise AssertionError("the synthetic masks were asked for")


def test_load_masks_from_the_blob():
    a = _args("--data", "blob.pt")
    with pytest.raises(SystemExit) as info:
        _entry.load_masks(a, [0, 1], {"videos": [0, 1]}, _fail)
    assert info.value.code == "--data: the blob has no 'masks' list (one [T,h,w] array or None per sub-video)"
    with pytest.raises(SystemExit) as info:
        _entry.load_masks(a, [0, 1], {"masks": [None]}, _fail)
    assert info.value.code == "1 masks for 2 sub-videos"
    masks = [None, np.zeros((5, 2, 2), np.uint8)]
    assert _entry.load_masks(a, [0, 1], {"masks": masks}, _fail) is masks


def test_load_masks_from_a_folder(tmp_path):
    rgb, root = tmp_path / "rgb", tmp_path / "masks"
    for name in ("b", "a"):
        (rgb / name).mkdir(parents=True)
    root.mkdir()
    np.save(root / "b.npy", np.ones((5, 2, 3), np.uint8))
    (root / "notes.txt").write_text("not a mask")
    a = _args("--rgb_root", str(rgb), "--op_root", str(rgb), "--mask_root", str(root))
    got = _entry.load_masks(a, [0, 1], {}, _fail)
    assert got[0] is None and got[1].shape == (5, 2, 3)                        # in the sorted order of the folders
    with pytest.raises(SystemExit) as info:
        _entry.load_masks(a, [0, 1, 2], {}, _fail)
    assert info.value.code == "2 masks for 3 sub-videos"
    np.save(root / "c.npy", np.ones((5, 2, 3), np.uint8))
    with pytest.raises(SystemExit) as info:
        _entry.load_masks(a, [0, 1], {}, _fail)
    assert info.value.code == f"--mask_root {root}: ['c.npy'] match no sub-video folder (2 folders)"
    assert run_pixel.masks_from_root is _entry.masks_from_root


def test_load_masks_synthetic_default():
    calls = []

    def fake(*args):
        calls.append(args)
        return ["m"] * args[0]
    assert _entry.load_masks(_args("--synthetic", "--videos", "3", "--frames", "12", "--size", "32"), [0] * 3, {}, fake) == ["m"] * 3
    assert _entry.load_masks(_args("--synthetic", "--raw", "--videos", "2"), [0] * 2, {}, fake) == ["m"] * 2
    assert calls == [(3, 12, 32, 32), (2, 60, 240, 360)]
    with pytest.raises(SystemExit) as info:
        _entry.load_masks(_args("--synthetic", "--videos", "2"), [0] * 3, {}, fake)
    assert info.value.code == "2 masks for 3 sub-videos"
    got = _entry.load_masks(_args("--synthetic", "--videos", "2", "--frames", "9", "--size", "8"), [0] * 2, {}, run_pixel.synthetic_masks)
    assert [m.shape for m in got] == [(9, 8, 8), (16, 8, 8)]
