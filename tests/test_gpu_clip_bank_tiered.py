"""The two-tier clip bank on the GPU (csrc/clip_bank.hip `ammc_gather_clips_tiered`, `pipeline.ClipBank` with a host
budget, `ClipBank.prefetch`): gathers from a bank split between device memory and pinned host memory are bit-identical
to the all-device gathers wherever the split lies, a pageable host pointer never reaches the kernel, and a prefetched
batch equals a plain one."""
import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, pipeline as P
from oracle import pipeline_oracle as PO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_RGB, N_OP, RGB_LEN, OP_LEN = 11, 9, 5, 4
SIZES = [(8, 8), (6, 10), (16, 24)]                    # h * w = 64 (16-pixel loads), 60 (the 4-pixel path), 384
SPLITS = [(0, 0), (3, 7), (11, 9), (6, 0)]             # (rgb, op) frames in the device tier
# every start a bank of 11 / 9 frames has: frame 0, n - len, every clip that straddles any of the splits (rgb 6: starts
# 2..5, all 4; op 7: starts 4, 5; rgb 3: 0..2), clips wholly in each tier - and one -1 per kind, in different samples
RGB_FIRST = np.array([0, 1, 2, 3, 4, 5, 6, -1, 6], np.int32)
OP_FIRST = np.array([0, 1, 2, 3, 4, 5, -1, 0, 5], np.int32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _banks(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    rgb = torch.randint(0, 256, (N_RGB, 3, h, w), dtype=torch.uint8, generator=g)
    op = torch.randn(N_OP, h, w, generator=g) * 3
    return rgb, op


def _pinned_slice(t, offset):
    """a copy of `t` in pinned memory, `offset` bytes into its allocation (the entry must map an interior pointer)"""
    raw = torch.empty(t.numel() * t.element_size() + offset, dtype=torch.uint8, pin_memory=True)
    out = raw[offset:].view(t.dtype).view(t.shape)
    out.copy_(t)
    return out


def _ptr(t):
    """the address of a tensor (NULL for None or an empty one); an int is an address already"""
    if isinstance(t, int):
        return t
    return t.data_ptr() if t is not None and t.numel() else None


def _tiered(tiers, firsts, h, w, outs):
    """tiers: {kind: (dev tensor, host tensor, n_dev, n)}; a kind absent from `firsts` is passed as NULLs"""
    args = []
    for kind in ("rgb", "op"):
        dev, host, n_dev, n = tiers[kind] if kind in firsts else (None, None, 0, 0)
        args += [_ptr(dev), _ptr(host), n_dev, n]
    b = len(next(iter(firsts.values())))
    s = torch.cuda.current_stream().cuda_stream
    return _lib.load().ammc_gather_clips_tiered(*args, _ptr(firsts.get("rgb")), _ptr(firsts.get("op")), b, RGB_LEN, OP_LEN,
                                                h, w, _ptr(outs.get("rgb")), _ptr(outs.get("op")), s)


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def reference(request):
    """per size: the banks, the device index rows and the all-device gathers (two-kind and one-kind), computed once"""
    h, w = request.param
    lib = _lib.load()
    rgb, op = _banks(h, w)
    d_rgb, d_op = rgb.to(DEV), op.to(DEV)
    rf, of = torch.from_numpy(RGB_FIRST).to(DEV), torch.from_numpy(OP_FIRST).to(DEV)
    b = len(RGB_FIRST)
    want_rgb = torch.full((b, RGB_LEN, 3, h, w), 5.0, device=DEV)
    want_op = torch.full((b, OP_LEN, 2, h, w), 5.0, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ammc_gather_clips(d_rgb.data_ptr(), N_RGB, d_op.data_ptr(), N_OP, rf.data_ptr(), of.data_ptr(), b, RGB_LEN,
                                     OP_LEN, h, w, want_rgb.data_ptr(), want_op.data_ptr(), s))
    one_rgb, one_op = torch.full_like(want_rgb, 6.0), torch.full_like(want_op, 6.0)
    _lib.check(lib.ammc_gather_clips_one(d_rgb.data_ptr(), N_RGB, 0, rf.data_ptr(), b, RGB_LEN, h, w, one_rgb.data_ptr(), s))
    _lib.check(lib.ammc_gather_clips_one(d_op.data_ptr(), N_OP, 1, of.data_ptr(), b, OP_LEN, h, w, one_op.data_ptr(), s))
    torch.cuda.synchronize()
    # the reference itself: NaN rows exactly where the index is -1, finite everywhere else
    for want, first in ((want_rgb, RGB_FIRST), (want_op, OP_FIRST)):
        for i, f in enumerate(first):
            assert bool(torch.isnan(want[i]).all()) if f < 0 else bool(torch.isfinite(want[i]).all())
    return dict(h=h, w=w, rgb=rgb, op=op, d_rgb=d_rgb, d_op=d_op, rf=rf, of=of, want_rgb=want_rgb, want_op=want_op,
                one_rgb=one_rgb, one_op=one_op)


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: f"split{s[0]}-{s[1]}")
def test_tiered_gather_is_bit_identical_to_the_all_device_gather(reference, split):
    r = reference
    h, w, b = r["h"], r["w"], len(RGB_FIRST)
    sr, so = split
    tiers = {"rgb": (r["d_rgb"][:sr].contiguous(), _pinned_slice(r["rgb"][sr:], 64), sr, N_RGB),
             "op": (r["d_op"][:so].contiguous(), _pinned_slice(r["op"][so:], 0), so, N_OP)}
    got_rgb = torch.full((b, RGB_LEN, 3, h, w), 7.0, device=DEV)
    got_op = torch.full((b, OP_LEN, 2, h, w), 7.0, device=DEV)
    _lib.check(_tiered(tiers, {"rgb": r["rf"], "op": r["of"]}, h, w, {"rgb": got_rgb, "op": got_op}), "tiered")
    torch.cuda.synchronize()
    assert torch.equal(_bits(got_rgb), _bits(r["want_rgb"]))
    assert torch.equal(_bits(got_op), _bits(r["want_op"]))
    ok_rgb, ok_op = RGB_FIRST >= 0, OP_FIRST >= 0
    assert torch.equal(got_rgb[ok_rgb], r["want_rgb"][ok_rgb]) and torch.equal(got_op[ok_op], r["want_op"][ok_op])
    assert bool(torch.isnan(got_rgb[~ok_rgb]).all()) and bool(torch.isnan(got_op[~ok_op]).all())
    # the single-kind form: the other kind's `first` NULL, its arguments not read
    only_rgb, only_op = torch.full_like(got_rgb, 8.0), torch.full_like(got_op, 8.0)
    _lib.check(_tiered(tiers, {"rgb": r["rf"]}, h, w, {"rgb": only_rgb}), "tiered rgb")
    _lib.check(_tiered(tiers, {"op": r["of"]}, h, w, {"op": only_op}), "tiered op")
    torch.cuda.synchronize()
    assert torch.equal(_bits(only_rgb), _bits(r["one_rgb"])) and torch.equal(_bits(only_op), _bits(r["one_op"]))


def test_a_pageable_host_tier_is_refused_and_nothing_is_launched(reference):
    """the host tier as a pageable numpy pointer: AMMC_EINVAL before the launch, the output untouched.  Every index lies
    in the device tier on purpose: even a launch that slipped through would not read the pageable memory."""
    r = reference
    h, w = r["h"], r["w"]
    sr, so = 6, 5
    page_rgb = np.zeros((N_RGB - sr) * 3 * h * w + 16, np.uint8)
    page_op = np.zeros((N_OP - so) * h * w + 4, np.float32)
    a_rgb = page_rgb.ctypes.data + (-page_rgb.ctypes.data) % 16            # 16-byte aligned: only the kind of memory is wrong
    a_op = page_op.ctypes.data + (-page_op.ctypes.data) % 16
    rf = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)             # clips 0..4, 1..5 of a 6-frame device tier
    of = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)             # clips of a 5-flow device tier
    got_rgb = torch.full((3, RGB_LEN, 3, h, w), 7.0, device=DEV)
    got_op = torch.full((3, OP_LEN, 2, h, w), 7.0, device=DEV)
    pinned_rgb, pinned_op = _pinned_slice(r["rgb"][sr:], 0), _pinned_slice(r["op"][so:], 0)
    d_rgb, d_op = r["d_rgb"][:sr].contiguous(), r["d_op"][:so].contiguous()
    for tiers in ({"rgb": (d_rgb, a_rgb, sr, N_RGB), "op": (d_op, pinned_op, so, N_OP)},
                  {"rgb": (d_rgb, pinned_rgb, sr, N_RGB), "op": (d_op, a_op, so, N_OP)}):
        assert _tiered(tiers, {"rgb": rf, "op": of}, h, w, {"rgb": got_rgb, "op": got_op}) == -1      # AMMC_EINVAL
        torch.cuda.synchronize()
        assert bool((got_rgb == 7.0).all()) and bool((got_op == 7.0).all())
    # the same call with both tiers pinned goes through (the refusal above was about the memory, nothing else)
    _lib.check(_tiered({"rgb": (d_rgb, pinned_rgb, sr, N_RGB), "op": (d_op, pinned_op, so, N_OP)}, {"rgb": rf, "op": of}, h, w,
                       {"rgb": got_rgb, "op": got_op}), "tiered")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got_rgb).all()) and not bool((got_rgb == 7.0).all())
    del page_rgb, page_op


# ---- pipeline.ClipBank -------------------------------------------------------------------------------------------------

RGB_LENS, OP_LENS = (7, 6), (6, 5)                     # two sub-videos, as tests/test_gpu_clip_bank.py


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """frames as .npy / lossless PNG, flows as .flo, 12 x 16 at the source"""
    from PIL import Image
    root = tmp_path_factory.mktemp("tiered_set")
    rng = np.random.default_rng(29)
    for v, (nr, no) in enumerate(zip(RGB_LENS, OP_LENS)):
        dr, do = root / "rgb" / f"{v + 1:02d}", root / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        for i in range(nr):
            fr = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
            if v == 0:
                Image.fromarray(fr).save(dr / f"{i:04d}.png")
            else:
                np.save(dr / f"{i:04d}.npy", fr)
        for i in range(no):
            PO.write_flo(str(do / f"{i:04d}.flo"), rng.normal(0, 3, (12, 16, 2)).astype(np.float32))
    return str(root / "rgb"), str(root / "op")


# every clip the banks hold, as global first frames (video 1 starts at frame 7 / flow 6)
ALL_RGB = np.array([0, 1, 2, 7, 8, 2])
ALL_OP = np.array([0, 1, 2, 6, 7, 0])


def _roots(tree, kinds):
    return (tree[0] if "rgb" in kinds else None, tree[1] if "op" in kinds else None)


def _first(kinds, rgb, op):
    return tuple(x for k, x in (("rgb", rgb), ("op", op)) if k in kinds)


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("size", [16, (10, 6)], ids=["16x16", "10x6"])
@pytest.mark.parametrize("kinds", [("rgb", "op"), ("rgb",), ("op",)], ids=["joint", "rgb", "op"])
def test_bank_with_a_host_tier_gathers_what_the_all_device_bank_gathers(tree, kinds, size):
    roots = _roots(tree, kinds)
    full = P.ClipBank(*roots, size, DEV, workers=2, budget_gb=4.0)
    assert full.host_nbytes == 0 and full.device_nbytes == full.nbytes
    assert (full.n_rgb_dev, full.n_op_dev) == (full.n_rgb, full.n_op)
    budget_gb = 0.45 * full.nbytes / 1e9               # about half of the set: the split falls inside sub-video 0
    bank = P.ClipBank(*roots, size, DEV, workers=2, budget_gb=budget_gb, host_budget_gb=0.001)
    assert 0 < bank.device_nbytes <= budget_gb * 1e9 and bank.host_nbytes > 0
    assert bank.device_nbytes + bank.host_nbytes == bank.nbytes == full.nbytes
    w, h = P._size_wh(size)
    assert bank.device_nbytes == bank.n_rgb_dev * 3 * h * w + bank.n_op_dev * 4 * h * w
    for kind, n_dev, n, host in (("rgb", bank.n_rgb_dev, bank.n_rgb, bank.rgb_host), ("op", bank.n_op_dev, bank.n_op, bank.op_host)):
        if kind in kinds:
            assert 0 < n_dev < n and host.is_pinned() and host.shape[0] == n - n_dev
    # the split lies inside sub-video 0 of each kind (7 frames / 6 flows): that sub-video was filled across it
    if "rgb" in kinds:
        assert bank.n_rgb_dev < RGB_LENS[0]
    if "op" in kinds:
        assert bank.n_op_dev < OP_LENS[0]
    first = _first(kinds, ALL_RGB, ALL_OP)
    got, want = bank.gather(*first), full.gather(*first)
    torch.cuda.synchronize()
    assert _same(got, want)
    # what has not changed: the same small budget WITHOUT a host budget is refused as before (passes on the parent too)
    with pytest.raises(_lib.AmmcHipError, match="of device memory, more than the budget of"):
        P.ClipBank(*roots, size, DEV, workers=2, budget_gb=budget_gb)
    with pytest.raises(_lib.AmmcHipError, match="host budget"):
        P.ClipBank(*roots, size, DEV, workers=2, budget_gb=budget_gb, host_budget_gb=1e-7)
    with pytest.raises(_lib.AmmcHipError):             # indices stay global and validated: a clip across two sub-videos
        bank.gather(*_first(kinds, np.array([3]), np.array([3])))


@pytest.mark.parametrize("tiered", [True, False], ids=["tiered", "all-device"])
@pytest.mark.parametrize("kinds", [("rgb", "op"), ("op",)], ids=["joint", "op"])
def test_prefetched_batches_equal_plain_gathers(tree, kinds, tiered):
    roots = _roots(tree, kinds)
    ref = P.ClipBank(*roots, 16, DEV, workers=2, budget_gb=4.0)
    bank = P.ClipBank(*roots, 16, DEV, workers=2, budget_gb=0.45 * ref.nbytes / 1e9, host_budget_gb=0.001) if tiered else \
        P.ClipBank(*roots, 16, DEV, workers=2, budget_gb=4.0)
    assert (bank.host_nbytes > 0) == tiered
    rng = np.random.default_rng(5)
    rounds = [_first(kinds, rng.choice(ALL_RGB, 4), rng.choice(ALL_OP, 4)) for _ in range(7)]
    want = [ref.gather(*f) for f in rounds]
    want = [w if isinstance(w, tuple) else (w,) for w in want]
    sums = [sum(t.double().sum() for t in w) for w in want]
    clips = bank.gather(*rounds[0])
    for i in range(6):
        bank.prefetch(*rounds[i + 1])
        cur = clips if isinstance(clips, tuple) else (clips,)
        used = sum(t.double().sum() for t in cur)      # the consumer of clips_i: kernels on the current stream
        nxt = bank.gather(*rounds[i + 1])
        assert _same(cur, want[i]) and bool(used == sums[i]), i
        assert _same(nxt, want[i + 1]), i
        clips = nxt
    # a gather with other indices than the prefetched ones drops the prefetch and is still right; so is the next one
    bank.prefetch(*rounds[0])
    assert _same(bank.gather(*rounds[3]), want[3])
    assert _same(bank.gather(*rounds[0]), want[0])
    with pytest.raises(_lib.AmmcHipError):             # prefetch validates like gather
        bank.prefetch(*_first(kinds, np.array([3]), np.array([3])))
    torch.cuda.synchronize()
