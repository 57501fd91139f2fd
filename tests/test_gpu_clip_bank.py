"""The training clip bank (csrc/clip_bank.hip, pipeline.ClipBank): fill + gather bit-identical to
oracle/pipeline_oracle.py's loaders and to `frames_to_device` / `flows_to_device` on the same frames, at the
geometries of test_gpu_pipeline.py."""
import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, pipeline as P
from oracle import pipeline_oracle as PO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB_LENS, OP_LENS = (7, 6), (6, 5)                     # two sub-videos; the op folders one entry shorter


def _tree(root, h, w, seed, png):
    """frames as .npy (or lossless PNG) and flows as .flo; returns the decoded arrays per sub-video"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    vids = []
    for v, (nr, no) in enumerate(zip(RGB_LENS, OP_LENS)):
        dr, do = root / "rgb" / f"{v + 1:02d}", root / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        fr = rng.integers(0, 256, (nr, h, w, 3), dtype=np.uint8)
        fl = rng.normal(0, 3, (no, h, w, 2)).astype(np.float32)
        for i in range(nr):
            if png:
                Image.fromarray(fr[i]).save(dr / f"{i:04d}.png")
            else:
                np.save(dr / f"{i:04d}.npy", fr[i])
        for i in range(no):
            PO.write_flo(str(do / f"{i:04d}.flo"), fl[i])
        vids.append((fr, fl))
    return vids


@pytest.mark.parametrize("h,w,oh,ow", [(240, 360, 256, 256), (360, 640, 256, 256), (480, 856, 256, 256),
                                        (158, 238, 256, 256), (3, 5, 8, 8)])
def test_bank_gather_is_bit_identical_to_the_loaders(tmp_path, h, w, oh, ow):
    vids = _tree(tmp_path, h, w, h * 1000 + w, png=(h == 240))
    bank = P.ClipBank(str(tmp_path / "rgb"), str(tmp_path / "op"), (ow, oh), DEV, workers=4, budget_gb=4.0)
    assert bank.rgb.dtype == torch.uint8 and tuple(bank.rgb.shape) == (sum(RGB_LENS), 3, oh, ow)
    assert tuple(bank.op.shape) == (sum(OP_LENS), oh, ow) and bank.fill_seconds > 0
    # every video's first and last start the sampler can draw, and the last clip the bank holds (never drawn)
    rgb_pairs = [(v, s) for v, n in enumerate(RGB_LENS) for s in sorted({0, n - 6, n - 5})]
    op_pairs = [(v, s) for v, n in enumerate(OP_LENS) for s in sorted({0, n - 5, n - 4})]
    b = max(len(rgb_pairs), len(op_pairs))
    rgb_pairs = (rgb_pairs * b)[:b]
    op_pairs = (op_pairs * b)[:b]
    rv, rs = np.array(rgb_pairs).T
    ov, os_ = np.array(op_pairs).T
    rf, of = bank.global_index(rv, rs, ov, os_)
    rgb, op = bank.gather(rf, of)
    torch.cuda.synchronize()
    assert tuple(rgb.shape) == (b, 5, 3, oh, ow) and tuple(op.shape) == (b, 4, 2, oh, ow)
    rgb, op = rgb.cpu().numpy(), op.cpu().numpy()
    for i in range(b):
        fr, _ = vids[rv[i]]
        _, fl = vids[ov[i]]
        want_rgb = np.stack([PO.load_frame(fr[rs[i] + t], (ow, oh)) for t in range(5)])
        want_op = np.stack([PO.load_op(fl[os_[i] + t].copy(), (ow, oh)) for t in range(4)])
        assert np.array_equal(rgb[i], want_rgb), i
        assert np.array_equal(op[i], want_op), i
    # the same frames through the evaluation pipeline's kernels
    for v, (fr, fl) in enumerate(vids):
        ev_rgb = P.frames_to_device(torch.from_numpy(fr).to(DEV), (ow, oh))
        ev_op = P.flows_to_device(torch.from_numpy(fl).to(DEV), (ow, oh))
        g_rgb, g_op = bank.gather(bank.rgb_start[v] + np.arange(RGB_LENS[v] - 4), bank.op_start[v] + np.zeros(RGB_LENS[v] - 4, np.int64))
        for s in range(RGB_LENS[v] - 4):
            assert torch.equal(g_rgb[s], ev_rgb[s:s + 5])
        g_rgb, g_op = bank.gather(bank.rgb_start[v] + np.zeros(OP_LENS[v] - 3, np.int64), bank.op_start[v] + np.arange(OP_LENS[v] - 3))
        for s in range(OP_LENS[v] - 3):
            assert torch.equal(g_op[s], ev_op[s:s + 4])


def test_sub_videos_of_different_source_sizes_share_one_bank(tmp_path):
    """`_fill` resizes every sub-video from its own source size: 12 x 16 and 9 x 21 into one 8 x 8 bank, each gathered
    clip bit-identical to the loaders on its own frames"""
    rng = np.random.default_rng(53)
    vids = []
    for v, (h, w) in enumerate(((12, 16), (9, 21))):
        dr, do = tmp_path / "rgb" / f"{v + 1:02d}", tmp_path / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        fr = rng.integers(0, 256, (RGB_LENS[v], h, w, 3), dtype=np.uint8)
        fl = rng.normal(0, 3, (OP_LENS[v], h, w, 2)).astype(np.float32)
        for i in range(RGB_LENS[v]):
            np.save(dr / f"{i:04d}.npy", fr[i])
        for i in range(OP_LENS[v]):
            PO.write_flo(str(do / f"{i:04d}.flo"), fl[i])
        vids.append((fr, fl))
    bank = P.ClipBank(str(tmp_path / "rgb"), str(tmp_path / "op"), 8, DEV, workers=2, budget_gb=4.0)
    assert tuple(bank.rgb.shape) == (sum(RGB_LENS), 3, 8, 8) and tuple(bank.op.shape) == (sum(OP_LENS), 8, 8)
    # every clip either video holds
    pairs = [(v, s, min(s, OP_LENS[v] - 4)) for v in range(2) for s in range(RGB_LENS[v] - 4)]
    rv, rs, os_ = np.array(pairs).T
    rf, of = bank.global_index(rv, rs, rv, os_)
    rgb, op = bank.gather(rf, of)
    torch.cuda.synchronize()
    rgb, op = rgb.cpu().numpy(), op.cpu().numpy()
    for i, (v, s, so) in enumerate(pairs):
        fr, fl = vids[v]
        assert np.array_equal(rgb[i], np.stack([PO.load_frame(fr[s + t], (8, 8)) for t in range(5)])), (v, s)
        assert np.array_equal(op[i], np.stack([PO.load_op(fl[so + t].copy(), (8, 8)) for t in range(4)])), (v, so)


def test_gather_refuses_bad_indices_before_the_launch(tmp_path):
    _tree(tmp_path, 12, 16, 3, png=False)
    bank = P.ClipBank(str(tmp_path / "rgb"), str(tmp_path / "op"), 16, DEV, workers=2)
    for rf, of in (([3], [0]),                    # rgb clip 3..7 crosses from video 1 into video 2
                   ([0], [3]),                    # op clip 3..6 crosses (video 1 holds 6 flows: 0..5)
                   ([sum(RGB_LENS) - 4], [0]), ([-1], [0]), ([0, 1], [0])):
        with pytest.raises(_lib.AmmcHipError):
            bank.gather(np.array(rf), np.array(of))
    rgb, op = bank.gather(np.array([2, 8]), np.array([2, 7]))             # the last clips of each video
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(op).all())
