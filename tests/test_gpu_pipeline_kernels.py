"""The input-pipeline and clip-bank kernels in isolation (csrc/pipeline.hip, csrc/clip_bank.hip, csrc/resize_common.h)
over the table of tests/pipeline_cases.py; the host half is tests/test_pipeline_cases_host.py.

Resize entries (`ammc_frames_u8_to_f32`, `ammc_flows_to_f32`, `ammc_frames_u8_resize_u8`, `ammc_flows_resize_c0`): every
geometry x pattern (x bgr for the frames) x alignment variant, bit-identical to oracle/pipeline_oracle.py (floats
compared as int32), guards around every source and destination untouched, a second launch the same bits, the bank form
plus the numpy normalise | (c0, c0 / w) equal to the float form, and the answers known by hand.

Gather entries (`ammc_gather_clips`, `ammc_gather_clips_one`, `ammc_gather_clips_tiered`): every plane size of
`GATHER_SIZES` against the numpy restatement of the clips (never against another kernel), the tiered form at every split
and with the host tier at both offsets of its pinned allocation, jointly and with one kind's `first` NULL.  Outputs are
pre-filled with the sentinel: a pixel the kernel forgot is a failure.

Offsets beyond 2^31: one rgb bank of 10930 frames (2.15 GB), filled by `ammc_frames_u8_resize_u8` and gathered from at
both ends, all-device and split between the tiers.  It is the only large allocation of the file.  Offsets that large in
the float outputs of the resize entries would need an output of 8 GiB and are out of scope here."""
import numpy as np
import pytest
import torch

import pipeline_cases as K
from ammcnet_aaai2021_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
geoms = pytest.mark.parametrize("g", K.GEOMS, ids=K.geom_id)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """`count` elements of `dtype` (torch.uint8 | torch.int32) inside a flat device buffer: `pad` bytes of `fill`, `off`
    elements more of it (the allocation is 256-byte aligned: `off` is the body's distance from a 16-byte boundary), the
    body - filled with `fill` as well - and `pad` bytes of `fill` behind it"""

    def __init__(self, count, dtype=torch.uint8, off=0, fill=K.BYTE, pad=K.GUARD):
        size = 4 if dtype == torch.int32 else 1
        self.lo, self.count, self.fill = pad // size + off, count, fill
        self.flat = torch.full((self.lo + count + pad // size,), fill, dtype=dtype, device=DEV)
        self.body = self.flat[self.lo:self.lo + count]
        self.ptr = self.flat.data_ptr() + self.lo * size
        assert self.flat.data_ptr() % 256 == 0

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        a = a.view(np.int32 if self.flat.dtype == torch.int32 else np.uint8).reshape(-1)
        assert a.size == self.count
        self.body.copy_(torch.from_numpy(a))
        return self

    def get(self, dtype, shape):
        return self.body.cpu().numpy().view(dtype).reshape(shape)

    def intact(self) -> bool:
        return bool((self.flat[:self.lo] == self.fill).all()) and bool((self.flat[self.lo + self.count:] == self.fill).all())


def f32dst(count, off=0, pad=K.GUARD):
    return Buf(count, torch.int32, off, K.SENT, pad)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run_frames(fr, g, bgr=0, src_off=0, dst_off=0, guard=K.BYTE, twice=False):
    """both frame entries on uint8 [n][h][w][3] -> (float32 [n][3][oh][ow], uint8 [n][3][oh][ow]); asserts the guards"""
    lib, s = _lib.load(), _stream()
    n, h, w = fr.shape[:3]
    oh, ow = g[2:]
    src = Buf(fr.size, off=src_off, fill=guard).put(fr)
    d32, d8 = f32dst(n * 3 * oh * ow, dst_off), Buf(n * 3 * oh * ow, off=dst_off)
    assert src.ptr % 2 == src_off and d32.ptr % 16 == 4 * dst_off and d8.ptr % 2 == dst_off
    for _ in range(2 if twice else 1):
        _lib.check(lib.ammc_frames_u8_to_f32(src.ptr, n, h, w, d32.ptr, oh, ow, bgr, s), "frames_u8_to_f32")
        _lib.check(lib.ammc_frames_u8_resize_u8(src.ptr, n, h, w, d8.ptr, oh, ow, bgr, s), "frames_u8_resize_u8")
    torch.cuda.synchronize()
    assert src.intact() and d32.intact() and d8.intact(), "a guard was written"
    assert np.array_equal(src.get(np.uint8, fr.shape), fr), "the source was written"
    return d32.get(np.float32, (n, 3, oh, ow)), d8.get(np.uint8, (n, 3, oh, ow))


def run_flows(fl, g, src_off=0, dst_off=0, twice=False):
    """both flow entries on float32 [n][h][w][2] -> (float32 [n][2][oh][ow], c0 float32 [n][oh][ow]); asserts the guards"""
    lib, s = _lib.load(), _stream()
    n, h, w = fl.shape[:3]
    oh, ow = g[2:]
    src = Buf(fl.size * 4, off=4 * src_off).put(fl)
    d2, d1 = f32dst(n * 2 * oh * ow, dst_off), f32dst(n * oh * ow, dst_off)
    assert src.ptr % 16 == 4 * src_off and d2.ptr % 16 == 4 * dst_off and d1.ptr % 16 == 4 * dst_off
    for _ in range(2 if twice else 1):
        _lib.check(lib.ammc_flows_to_f32(src.ptr, n, h, w, d2.ptr, oh, ow, s), "flows_to_f32")
        _lib.check(lib.ammc_flows_resize_c0(src.ptr, n, h, w, d1.ptr, oh, ow, s), "flows_resize_c0")
    torch.cuda.synchronize()
    assert src.intact() and d2.intact() and d1.intact(), "a guard was written"
    assert np.array_equal(bits(src.get(np.float32, fl.shape)), bits(fl)), "the source was written"
    return d2.get(np.float32, (n, 2, oh, ow)), d1.get(np.float32, (n, oh, ow))


# ---- the resize entries ------------------------------------------------------------------------------------------------
@geoms
def test_frame_entries_are_bit_identical_to_the_oracle(g):
    for p in K.FRAME_PATTERNS:
        fr = K.frames(g, p)
        want8, want32 = K.want_frames_u8(fr, g), K.want_frames_f32(fr, g)
        for a in K.alignments(g):
            so, do = K.ALIGNMENTS[a]
            for bgr in (0, 1):                              # the same bytes read as BGR: the planes come out reversed
                got32, got8 = run_frames(fr, g, bgr, so, do, K.source_guard(p))
                w32, w8 = (want32[:, ::-1], want8[:, ::-1]) if bgr else (want32, want8)
                assert np.array_equal(bits(got32), bits(w32)), (p, a, bgr, "ammc_frames_u8_to_f32")
                assert np.array_equal(got8, w8), (p, a, bgr, "ammc_frames_u8_resize_u8")
                # the bank form + the numpy normalise is the float form
                assert np.array_equal(bits(K.normalize(got8)), bits(got32)), (p, a, bgr)
        again32, again8 = run_frames(fr, g, 0, twice=True, guard=K.source_guard(p))
        assert np.array_equal(bits(again32), bits(want32)) and np.array_equal(again8, want8), (p, "second launch")


@geoms
def test_flow_entries_are_bit_identical_to_the_oracle(g):
    ow = g[3]
    for p in K.FLOW_PATTERNS:
        fl = K.flows(g, p)
        want = K.want_flows_f32(fl, g)
        for a in K.alignments(g):
            so, do = K.ALIGNMENTS[a]
            got, c0 = run_flows(fl, g, so, do)
            assert np.array_equal(bits(got), bits(want)), (p, a, "ammc_flows_to_f32")
            assert np.array_equal(bits(c0), bits(want[:, 0])), (p, a, "ammc_flows_resize_c0")
            # the bank form + (c0, c0 / w) is the float form
            assert np.array_equal(bits(np.stack([c0, c0 / np.float32(ow)], 1)), bits(got)), (p, a)
        again, c0 = run_flows(fl, g, twice=True)
        assert np.array_equal(bits(again), bits(want)) and np.array_equal(bits(c0), bits(want[:, 0])), (p, "second launch")


def test_answers_known_by_hand_hold_for_the_kernels():
    rng = np.random.default_rng(3)
    for g in ((8, 8, 8, 8), (256, 256, 256, 256)):                                                # identity
        fr, fl = K.frames(g, "rand"), K.flows(g, "rand")
        got32, got8 = run_frames(fr, g)
        assert np.array_equal(got8, fr.transpose(0, 3, 1, 2))
        assert np.array_equal(bits(got32), bits(K.normalize(fr.transpose(0, 3, 1, 2))))
        got, c0 = run_flows(fl, g)
        assert np.array_equal(bits(c0), bits(fl[..., 0] / np.float32(g[2]))) and np.array_equal(bits(got[:, 0]), bits(c0))
    for g in K.GEOMS:                                                                             # constants stay constants
        for p, v, around in (("zero", 0, K.BYTE), ("full", 255, 0)):
            got32, got8 = run_frames(K.frames(g, p), g, guard=K.source_guard(p))
            m = K.mid(g)
            assert (got8[m] == v).all() and (np.delete(got8, m, 0) == around).all(), (g, p)
            assert (got32[m] == (-1.0 if v == 0 else 1.0)).all(), (g, p)
    g = (1, 1, 4, 4)                                                                              # a 1 x 1 source
    fr = rng.integers(0, 256, (3, 1, 1, 3), dtype=np.uint8)
    got32, got8 = run_frames(fr, g)
    assert np.array_equal(got8, np.broadcast_to(fr.transpose(0, 3, 1, 2), (3, 3, 4, 4)))
    fl = rng.normal(0, 3, (3, 1, 1, 2)).astype(np.float32)
    got, c0 = run_flows(fl, g)
    assert np.array_equal(bits(c0), bits(np.broadcast_to(fl[..., 0] / np.float32(4), (3, 4, 4))))
    for g in ((16, 24, 8, 12), (32, 32, 8, 8)):                                                   # the mean of the middle neighbours,
        ramp = K.hramp(g[0], g[1])[None]                                                          # .5 rounding up
        want = K.hramp_mean(g).transpose(2, 0, 1)[None]
        for bgr in (0, 1):
            got32, got8 = run_frames(ramp, g, bgr)
            assert np.array_equal(got8, want[:, ::-1] if bgr else want), (g, bgr)
            assert np.array_equal(bits(got32), bits(K.normalize(got8)))
    g = (16, 24, 8, 12)                                                                           # the flows' ramp: exact in float32
    got, c0 = run_flows(K.flows(g, "ramp"), g)
    want = (np.arange(12, dtype=np.float32) + np.float32(0.25) - 3) / np.float32(8)
    assert np.array_equal(bits(c0[0]), bits(np.tile(want, (8, 1))))
    assert np.array_equal(bits(got[0, 1]), bits(np.tile(want / np.float32(12), (8, 1))))


# ---- the gather entries ------------------------------------------------------------------------------------------------
class Clips:
    """the sentinel-filled, guarded outputs of one gather and their comparison with the numpy reference, on the device"""

    def __init__(self, ref):
        self.ref = ref
        b, h, w = len(K.RGB_FIRST), ref["h"], ref["w"]
        self.rgb = f32dst(b * K.RGB_LEN * 3 * h * w, pad=K.GUARD_OUT)
        self.op = f32dst(b * K.OP_LEN * 2 * h * w, pad=K.GUARD_OUT)
        assert self.rgb.ptr % 16 == 0 and self.op.ptr % 16 == 0

    def untouched(self, kind) -> bool:
        buf = self.rgb if kind == "rgb" else self.op
        return bool((buf.flat == K.SENT).all())

    def same(self, kind) -> bool:
        """`pipeline_cases.same_clips` (bit for bit where the reference is a number; a refused row NaN and no pixel of it
        still the pre-fill); the guards intact"""
        buf = self.rgb if kind == "rgb" else self.op
        return buf.intact() and K.same_clips(buf.body, self.ref["want_" + kind], self.ref["nan_" + kind])


@pytest.fixture(scope="module", params=K.GATHER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def ref(request):
    """per plane size: the banks (host, and guarded on the device: the rgb bank 4 bytes off a 16-byte boundary, which is
    all its entry asks for), the device index rows and the numpy reference clips as int32 bits on the device"""
    h, w = request.param
    rgb, op = K.gather_banks(h, w)
    want_rgb = K.gather_rgb_ref(rgb, K.RGB_FIRST, K.RGB_LEN)
    want_op = K.gather_op_ref(op, K.OP_FIRST, K.OP_LEN)
    b = len(K.RGB_FIRST)
    r = dict(h=h, w=w, rgb=rgb, op=op, d_rgb=Buf(rgb.size, off=4).put(rgb), d_op=Buf(op.size * 4).put(op),
             rf=torch.from_numpy(K.RGB_FIRST).to(DEV), of=torch.from_numpy(K.OP_FIRST).to(DEV),
             want_rgb=torch.from_numpy(bits(want_rgb).reshape(b, -1)).to(DEV), want_op=torch.from_numpy(bits(want_op).reshape(b, -1)).to(DEV),
             nan_rgb=torch.from_numpy(K.RGB_FIRST < 0).to(DEV), nan_op=torch.from_numpy(K.OP_FIRST < 0).to(DEV))
    assert np.isnan(want_rgb[K.RGB_FIRST < 0]).all() and np.isfinite(want_rgb[K.RGB_FIRST >= 0]).all()
    assert np.isnan(want_op[K.OP_FIRST < 0]).all() and np.isfinite(want_op[K.OP_FIRST >= 0]).all()
    assert r["d_rgb"].ptr % 16 == 4 and r["d_op"].ptr % 16 == 0
    return r


def _banks_intact(r) -> bool:
    return (r["d_rgb"].intact() and r["d_op"].intact() and np.array_equal(r["d_rgb"].get(np.uint8, r["rgb"].shape), r["rgb"])
            and np.array_equal(bits(r["d_op"].get(np.float32, r["op"].shape)), bits(r["op"])))


def test_plain_gather_equals_the_numpy_reference(ref):
    lib, s, r = _lib.load(), _stream(), ref
    b = len(K.RGB_FIRST)
    out = Clips(r)
    for launch in range(2):
        _lib.check(lib.ammc_gather_clips(r["d_rgb"].ptr, K.N_RGB, r["d_op"].ptr, K.N_OP, r["rf"].data_ptr(), r["of"].data_ptr(), b,
                                         K.RGB_LEN, K.OP_LEN, r["h"], r["w"], out.rgb.ptr, out.op.ptr, s), "gather_clips")
        torch.cuda.synchronize()
        assert out.same("rgb") and out.same("op"), launch
    assert _banks_intact(r)


def test_one_kind_gather_equals_the_numpy_reference(ref):
    lib, s, r = _lib.load(), _stream(), ref
    b = len(K.RGB_FIRST)
    out = Clips(r)
    for launch in range(2):
        _lib.check(lib.ammc_gather_clips_one(r["d_rgb"].ptr, K.N_RGB, 0, r["rf"].data_ptr(), b, K.RGB_LEN, r["h"], r["w"], out.rgb.ptr, s),
                   "gather_clips_one rgb")
        torch.cuda.synchronize()
        assert out.same("rgb") and out.untouched("op"), launch
    for launch in range(2):
        _lib.check(lib.ammc_gather_clips_one(r["d_op"].ptr, K.N_OP, 1, r["of"].data_ptr(), b, K.OP_LEN, r["h"], r["w"], out.op.ptr, s),
                   "gather_clips_one op")
        torch.cuda.synchronize()
        assert out.same("rgb") and out.same("op"), launch
    assert _banks_intact(r)


class Pinned:
    """a copy of the numpy array `a` in pinned memory, `offset` bytes into its allocation, 4 KiB of 0xA5 behind it"""

    def __init__(self, a, offset):
        n = a.nbytes
        self.raw = torch.full((offset + n + K.GUARD,), K.BYTE, dtype=torch.uint8).pin_memory()
        self.lo, self.n = offset, n
        self.raw[offset:offset + n].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
        self.ptr = (self.raw.data_ptr() + offset) if n else None
        self.want = self.raw.clone()

    def intact(self) -> bool:
        return bool(torch.equal(self.raw, self.want))


def _tiered(lib, tiers, firsts, outs, h, w, rgb_len=K.RGB_LEN, op_len=K.OP_LEN):
    """tiers: {kind: (device address | None, host address | None, n_dev, n)}; a kind absent from `firsts` is passed as NULLs"""
    args = []
    for kind in ("rgb", "op"):
        args += list(tiers[kind]) if kind in firsts else [None, None, 0, 0]
    b = len(next(iter(firsts.values())))
    ptr = lambda d, k: d[k].data_ptr() if k in d and hasattr(d[k], "data_ptr") else d.get(k)
    return lib.ammc_gather_clips_tiered(*args, ptr(firsts, "rgb"), ptr(firsts, "op"), b, rgb_len, op_len, h, w,
                                        outs.get("rgb"), outs.get("op"), _stream())


@pytest.mark.parametrize("split", K.SPLITS, ids=lambda s: f"split{s[0]}-{s[1]}")
def test_tiered_gather_equals_the_numpy_reference(ref, split):
    lib, r = _lib.load(), ref
    h, w = r["h"], r["w"]
    sr, so = split
    # the device tiers: the leading frames in guarded buffers of their own (NULL for an empty tier)
    dev_rgb = Buf(sr * 3 * h * w, off=4).put(r["rgb"][:sr]) if sr else None
    dev_op = Buf(so * h * w * 4).put(r["op"][:so]) if so else None
    for offset in K.PINNED_OFFSETS:
        host_rgb, host_op = Pinned(r["rgb"][sr:], offset), Pinned(r["op"][so:], offset)
        tiers = {"rgb": (dev_rgb.ptr if sr else None, host_rgb.ptr, sr, K.N_RGB), "op": (dev_op.ptr if so else None, host_op.ptr, so, K.N_OP)}
        firsts = {"rgb": r["rf"], "op": r["of"]}
        out = Clips(r)
        for launch in range(2):
            _lib.check(_tiered(lib, tiers, firsts, {"rgb": out.rgb.ptr, "op": out.op.ptr}, h, w), "tiered")
            torch.cuda.synchronize()
            assert out.same("rgb") and out.same("op"), (offset, launch)
        # one kind's `first` NULL: its arguments are not read, its output not written
        only = Clips(r)
        _lib.check(_tiered(lib, tiers, {"rgb": r["rf"]}, {"rgb": only.rgb.ptr}, h, w), "tiered rgb")
        torch.cuda.synchronize()
        assert only.same("rgb") and only.untouched("op"), offset
        only = Clips(r)
        _lib.check(_tiered(lib, tiers, {"op": r["of"]}, {"op": only.op.ptr}, h, w), "tiered op")
        torch.cuda.synchronize()
        assert only.same("op") and only.untouched("rgb"), offset
        assert host_rgb.intact() and host_op.intact(), offset
    assert (dev_rgb is None or dev_rgb.intact()) and (dev_op is None or dev_op.intact())


# ---- offsets beyond 2^31 -----------------------------------------------------------------------------------------------
BIG_N, BIG_H, BIG_W = 10930, 256, 256                     # 10930 x 3 x 65536 = 2,148,925,440 bytes; 2^31 lies in frame 10922
BIG_SPLIT = 10924
BIG_FIRST = np.array([0, 10921, BIG_N - K.RGB_LEN], np.int32)       # the first clip, one across 2^31 (and the split), the last
BIG_OP_FIRST = np.array([0, 5, -1], np.int32)


def _colour(f):
    """the colour of frame f of the large bank: it encodes the frame number"""
    f = np.asarray(f, np.int64)
    return np.stack([f % 256, (f // 256) % 256, (f * 7 + 3) % 251], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def big():
    lib, s = _lib.load(), _stream()
    size, frame = BIG_N * 3 * BIG_H * BIG_W, 3 * BIG_H * BIG_W
    assert size > 2 ** 31 and (int(BIG_FIRST[1]) + 2) * frame > 2 ** 31 > int(BIG_FIRST[1]) * frame and BIG_SPLIT * frame > 2 ** 31
    flat = torch.empty(K.GUARD + size + K.GUARD, dtype=torch.uint8, device=DEV)                  # not zero-filled
    flat[:K.GUARD] = K.BYTE
    flat[-K.GUARD:] = K.BYTE
    bank = flat[K.GUARD:K.GUARD + size].view(BIG_N, 3, BIG_H, BIG_W)
    src = Buf(BIG_N * 3).put(_colour(np.arange(BIG_N)))                                          # 10930 frames of 1 x 1 x 3
    _lib.check(lib.ammc_frames_u8_resize_u8(src.ptr, BIG_N, 1, 1, bank.data_ptr(), BIG_H, BIG_W, 0, s), "frames_u8_resize_u8")
    torch.cuda.synchronize()
    assert src.intact()
    assert bool((flat[:K.GUARD] == K.BYTE).all()) and bool((flat[-K.GUARD:] == K.BYTE).all())
    _, op = K.gather_banks(BIG_H, BIG_W)
    b = len(BIG_FIRST)
    # the reference clips from the colours (the test below checks that the bank holds them)
    small = lambda f0, n: np.broadcast_to(_colour(np.arange(f0, f0 + n))[:, :, None, None], (n, 3, BIG_H, BIG_W))
    want_rgb = np.concatenate([K.gather_rgb_ref(small(0, 5), [0], K.RGB_LEN),
                               K.gather_rgb_ref(small(10921, 9), [0, 4], K.RGB_LEN)])
    want_op = K.gather_op_ref(op, BIG_OP_FIRST, K.OP_LEN)
    return dict(h=BIG_H, w=BIG_W, flat=flat, bank=bank, op=op, d_op=Buf(op.size * 4).put(op),
                rf=torch.from_numpy(BIG_FIRST).to(DEV), of=torch.from_numpy(BIG_OP_FIRST).to(DEV),
                want_rgb=torch.from_numpy(bits(want_rgb).reshape(b, -1)).to(DEV), want_op=torch.from_numpy(bits(want_op).reshape(b, -1)).to(DEV),
                nan_rgb=torch.from_numpy(BIG_FIRST < 0).to(DEV), nan_op=torch.from_numpy(BIG_OP_FIRST < 0).to(DEV))


class BigClips(Clips):
    def __init__(self, ref):
        self.ref = ref
        b, hw = len(BIG_FIRST), BIG_H * BIG_W
        self.rgb = f32dst(b * K.RGB_LEN * 3 * hw, pad=K.GUARD_OUT)
        self.op = f32dst(b * K.OP_LEN * 2 * hw, pad=K.GUARD_OUT)


def test_bank_beyond_2_gib_is_filled_where_it_should_be(big):
    bank = big["bank"]
    for f0, n in ((0, 5), (BIG_N - 9, 9)):                                                        # the first and the last three among them
        got = bank[f0:f0 + n].cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(_colour(np.arange(f0, f0 + n))[:, :, None, None], got.shape)), f0
    # every frame's first and last pixel of every plane: no frame landed on another one's place
    ends = bank.view(BIG_N, 3, -1)[:, :, [0, -1]].cpu().numpy()
    assert np.array_equal(ends, np.broadcast_to(_colour(np.arange(BIG_N))[:, :, None], ends.shape))


def test_gathers_beyond_2_gib_equal_the_numpy_reference(big):
    lib, s, r = _lib.load(), _stream(), big
    b = len(BIG_FIRST)
    out = BigClips(r)
    _lib.check(lib.ammc_gather_clips(r["bank"].data_ptr(), BIG_N, r["d_op"].ptr, K.N_OP, r["rf"].data_ptr(), r["of"].data_ptr(), b,
                                     K.RGB_LEN, K.OP_LEN, BIG_H, BIG_W, out.rgb.ptr, out.op.ptr, s), "gather_clips")
    torch.cuda.synchronize()
    assert out.same("rgb") and out.same("op")
    one = BigClips(r)
    _lib.check(lib.ammc_gather_clips_one(r["bank"].data_ptr(), BIG_N, 0, r["rf"].data_ptr(), b, K.RGB_LEN, BIG_H, BIG_W, one.rgb.ptr, s),
               "gather_clips_one")
    torch.cuda.synchronize()
    assert one.same("rgb") and one.untouched("op")


def test_tiered_gather_beyond_2_gib_equals_the_numpy_reference(big):
    """the same bank split at frame 10924: the device tier ends beyond 2^31 bytes, the host tier holds the last 6 frames"""
    lib, r = _lib.load(), big
    host = Pinned(r["bank"][BIG_SPLIT:].cpu().numpy(), 0)
    assert host.n == 6 * 3 * BIG_H * BIG_W
    tiers = {"rgb": (r["bank"].data_ptr(), host.ptr, BIG_SPLIT, BIG_N), "op": (r["d_op"].ptr, None, K.N_OP, K.N_OP)}
    out = BigClips(r)
    _lib.check(_tiered(lib, tiers, {"rgb": r["rf"], "op": r["of"]}, {"rgb": out.rgb.ptr, "op": out.op.ptr}, BIG_H, BIG_W), "tiered")
    torch.cuda.synchronize()
    assert out.same("rgb") and out.same("op") and host.intact()
    only = BigClips(r)
    _lib.check(_tiered(lib, tiers, {"rgb": r["rf"]}, {"rgb": only.rgb.ptr}, BIG_H, BIG_W), "tiered rgb")
    torch.cuda.synchronize()
    assert only.same("rgb") and only.untouched("op")
