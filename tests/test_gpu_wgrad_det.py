"""The deterministic forms of the implicit-GEMM weight-gradient kernels on the device: `ammc_conv_wgrad_s16_det`
(wgrad_s16_kernel: ntaps 4 / 16 / 9) and `ammc_conv_wgrad_f32_det` (wgrad_f32_kernel: ntaps 1 / 9 / 16 / 4), each case
against the fp64 weight gradient of the reference operator and against the atomics entry on the same operands.

Shapes: the smallest at which the split logic can go wrong, and the conditions are ASSERTED through the `_det_variant`
label, not hoped for: k >= 3 slabs (the order of the sum matters), k >= 9 (the reduce kernel's unrolled body), a ragged last split (chunks not a multiple of the
chunks per split), a pixel count that is no multiple of the 32-pixel chunk, one split (k == 1: stored straight into dw,
no workspace), n = 32 / 64 / 128, stride 1 and 2, with and without `g_inv_scale`.

Gates, taken from where the atomics form of the same descriptor is held to them:
  S16   max|got - want| / max|want| <= wgrad_cases.GATE (3e-6; operands, geometry and reference of tests/wgrad_cases.py)
  fp32  e <= FACTOR x the error of torch's fp32 autograd on the CPU (tests/test_gpu_wgrad_f32.py: 3 x the witness)
and the deterministic result is within the same gate of the atomics entry's.

Every launch: dw [n][kpad] and the slab workspace are pre-filled with NaN between 4-KB canaries - dw comes back finite
(nothing needs zeroing, every element is written), no canary changes (nothing outside dw[n][kpad] and
slabs[0 .. slab_floats) is written), what the atomics form leaves exactly zero is exactly zero; dw EQUALS the slabs added
one after the other in fp32 (slab 0 + slab 1 + ..., the documented order); a second launch into fresh buffers and a
launch on a second HIP stream beside an unrelated kernel give the same bits.  Two equal runs do not prove determinism -
the proof is that the path has no atomic and a fixed-order sum ("Deterministic training") - these guard
against a regression."""
import ctypes as C

import pytest
import torch

import wgrad_cases as W
from test_gpu_wgrad_f32 import FACTOR, _nhwc, _strides, _truth
from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd._lib import AmmcWgradDesc

pytestmark = pytest.mark.gpu
DEV = W.DEV

_c = lambda name, kind, B, H, W_, n, cin, **kw: W.Case("det-" + name, kind, B, H, W_, n, cin, W.IM2COL, **kw)
# expect: what the label must say about the splits - "k>=3", "k==1", "ragged" (chunks % chunks-per-split), "m%32"
S16_CASES = [
    (_c("convt-k4-ragged-n64", "convt", 2, 23, 21, 64, 32, a_step=2, scaled="a", gmag=1e-3), ("k>=3", "ragged", "m%32")),
    (_c("convt-k4-n128-unscaled", "convt", 2, 24, 20, 128, 64, a_step=2, scaled=""), ("k>=3",)),
    (_c("c4-s2-k4-n64-cin8of3", "conv4", 2, 23, 21, 64, 8, cin_true=3, a_step=2, gmag=1e-6), ("k>=3", "ragged", "m%32")),
    (_c("c4-s1-k4-n32of1-cin64", "conv4", 1, 25, 31, 32, 64, cout=1, a_step=1, gmag=3e-4), ("k>=3", "ragged", "m%32")),
    (_c("c4-s2-k1-n64", "conv4", 1, 6, 5, 64, 64, a_step=2, a_odd=1, scaled=""), ("k==1", "m%32")),
    (_c("c3-k3-n64-cin32", "conv3", 2, 15, 21, 64, 32, gmag=1e-2), ("k>=3", "ragged", "m%32")),
    (_c("c3-k4-n160-cin16of12-slice", "conv3", 2, 23, 21, 160, 16, cin_true=12, gmag=1e-5, geom="slice"), ("k>=3", "ragged")),
    (_c("c3-k1-n32of3", "conv3", 1, 9, 7, 32, 32, cout=3, scaled=""), ("k==1", "m%32")),
    # more than eight slabs: the reduce kernel's unrolled body (eight loads in flight) and its tail
    (_c("c4-s2-k13-n64-cin8of3", "conv4", 2, 40, 39, 64, 8, cin_true=3, a_step=2, gmag=1e-4), ("k>=9", "ragged", "m%32")),
]
# name, kind, B, H, W (pixel space of g), (n, true rows), (cin, true channels), a_step, expectations
F32_CASES = [
    ("1x1-k4-enc-n32of24-cin64", "conv1", 2, 23, 21, (32, 24), (64, 64), 1, ("k>=3", "ragged", "m%32")),
    ("1x1-k4-dec-n128-cin32", "conv1", 2, 24, 20, (128, 128), (32, 32), 1, ("k>=3",)),
    ("3x3-k4-n128-cin16of12", "conv3", 2, 23, 21, (128, 128), (16, 12), 1, ("k>=3", "ragged", "m%32")),
    ("3x3-k1-outc-n32of3", "conv3", 1, 9, 7, (32, 3), (64, 64), 1, ("k==1", "m%32")),
    ("4x4-s2-k4-n64-cin8of3", "conv4", 2, 23, 21, (64, 64), (8, 3), 2, ("k>=3", "ragged", "m%32")),
    ("4x4-s1-k3-n64-cin32", "conv4", 2, 15, 21, (64, 64), (32, 32), 1, ("k>=3", "ragged", "m%32")),
    ("convt-k4-n64-co32", "convt", 2, 23, 21, (64, 64), (32, 32), 2, ("k>=3", "ragged", "m%32")),
    ("1x1-k13-n32-cin64", "conv1", 2, 40, 39, (32, 32), (64, 64), 1, ("k>=9", "ragged", "m%32")),
]


def _ptr(t, off=0):
    return t.data_ptr() + 4 * off


def _bits(t):
    return t.contiguous().view(torch.int32)


def _label(form, d):
    buf = C.create_string_buffer(96)
    rc = getattr(_lib.load(), f"ammc_conv_wgrad_{form}_det_variant")(C.byref(d), buf, 96)
    assert rc == 0, rc
    name, k = buf.value.decode().rsplit("+det", 1)
    return name, int(k)


def _check_splits(form, d, expect):
    """the conditions the case was chosen for, read from the library's own answer"""
    lib = _lib.load()
    name, k = _label(form, d)
    kpad = (d.ntaps * d.cin + 31) // 32 * 32
    need = int(getattr(lib, f"ammc_conv_wgrad_{form}_det_floats")(C.byref(d)))
    assert need == (k * d.n * kpad if k > 1 else 0), (name, k, need)
    M = d.batch * d.height * d.width
    nchunks = -(-M // 32)
    per = -(-nchunks // k)
    assert (k - 1) * per < nchunks <= k * per                   # k splits of `per` chunks, the last one not empty
    for e in expect:
        ok = {"k>=3": k >= 3, "k>=9": k >= 9, "k==1": k == 1, "ragged": nchunks % per != 0, "m%32": M % 32 != 0}[e]
        assert ok, (e, name, k, M, nchunks, per)
    return k, need, kpad


def _busy(stream):
    """an unrelated kernel on `stream`: a long elementwise pass over 256 MB"""
    with torch.cuda.stream(stream):
        x = torch.ones(64 << 20, device=DEV)
        for _ in range(4):
            x.mul_(1.0000001)
    return x


def _launches(launch):
    """three launches into fresh NaN-filled guarded buffers: on the current stream twice, and on a second stream while the
    first runs an unrelated kernel.  Returns [(dw Guarded, slabs Guarded | None)] x 3, synchronised."""
    outs = [launch(torch.cuda.current_stream().cuda_stream) for _ in range(2)]
    torch.cuda.synchronize()
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(main)
    keep = _busy(main)
    with torch.cuda.stream(side):
        outs.append(launch(side.cuda_stream))
    torch.cuda.synchronize()
    del keep
    return outs


def _check_slabs_and_bits(outs, k, n, kpad):
    dw0, slabs0 = outs[0]
    packed = dw0.t.view(n, kpad)
    assert bool(torch.isfinite(packed).all()), "an element of dw was not written (NaN pre-fill), or an unwritten slab element was read"
    for dw, slabs in outs:
        assert dw.pads_intact(), "written outside dw[n][kpad]"
        assert slabs is None or slabs.pads_intact(), "written outside slabs[0 .. slab_floats)"
    if k > 1:
        sl = slabs0.t.view(k, n, kpad)
        assert bool(torch.isfinite(sl).all()), "a slab element was not written"
        acc = torch.zeros(n, kpad, device=DEV)
        for s in range(k):                                      # slab 0 + slab 1 + ... in that order, fp32
            acc = acc + sl[s]
        assert torch.equal(acc, packed), "dw is not the in-order fp32 sum of the slabs"
    assert torch.equal(_bits(outs[1][0].t), _bits(dw0.t)), "a second launch into fresh buffers gives other bits"
    assert torch.equal(_bits(outs[2][0].t), _bits(dw0.t)), "a launch on a second stream beside another kernel gives other bits"
    return packed


def _check_zero_padding(packed, n, n_true, cin, c_true, ntaps, kpad, convt, pad_cols_zero):
    if not convt:
        if n_true < n:
            assert float(packed[n_true:].abs().max()) == 0.0, "rows cout .. n"
        if c_true < cin:
            assert float(packed[:, :ntaps * cin].view(n, ntaps, cin)[:, :, c_true:].abs().max()) == 0.0, "channels beyond the true ones"
    if pad_cols_zero and kpad > ntaps * cin:
        assert float(packed[:, ntaps * cin:].abs().max()) == 0.0, "columns ntaps * cin .. kpad"


# ---- S16 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,expect", S16_CASES, ids=[c.name for c, _ in S16_CASES])
def test_wgrad_s16_det_vs_fp64_and_the_atomics_entry(case, expect):
    c, lib = case, _lib.load()
    o = W.host_ops(c)
    keep = []
    gc, _, g_inv = W._operand(c, "g", o.g, c.scaled == "g", keep)
    ac, _, a_inv = W._operand(c, "a", o.a, c.scaled == "a", keep)
    inv = g_inv if g_inv is not None else a_inv
    assert (inv is None) == c.inv_null
    inv_p = _ptr(inv) if inv is not None else None
    zeros = W.Guarded(128, fill=0)
    mk = lambda dw: W.desc(c, g=_ptr(gc.t), a=_ptr(ac.t), dw=_ptr(dw.t), zeros=_ptr(zeros.t))
    d0 = mk(zeros)
    assert W.variant(d0) == (0, W.IM2COL) or W.current_switch()   # the atomics entry ends in the same kernel
    k, need, kpad = _check_splits("s16", d0, expect)
    assert kpad == c.kpad and _label("s16", d0)[0] == "wgrad_s16"

    def launch(stream):
        dw = W.Guarded(c.n * kpad)                              # NaN: no zeroing is needed
        slabs = W.Guarded(need) if need else None
        rc = lib.ammc_conv_wgrad_s16_det(C.byref(mk(dw)), inv_p, _ptr(slabs.t) if slabs else None, need, stream)
        assert rc == 0, rc
        return dw, slabs
    torch.cuda.synchronize()
    outs = _launches(launch)
    packed = _check_slabs_and_bits(outs, k, c.n, kpad)
    assert all(x.pads_intact() for x in (gc, ac, zeros))
    _check_zero_padding(packed, c.n, c.rows, c.cin, c.chans, c.ntaps, kpad, c.kind == "convt", True)

    s = torch.cuda.current_stream().cuda_stream

    def unpack(p):
        out = torch.full(W.wshape(c), float("nan"), device=DEV)
        if c.kind == "convt":
            _lib.check(lib.ammc_unpack_convt_wgrad_f32(_ptr(p), c.n, c.cin, _ptr(out), s), "unpack_convt")
        else:
            _lib.check(lib.ammc_unpack_conv_wgrad_f32(_ptr(p), c.rows, c.chans, W.wshape(c)[2], c.cin, _ptr(out), s), "unpack")
        return out.cpu()
    dwz = W.Guarded(c.n * kpad, fill=0)
    _lib.check(lib.ammc_conv_wgrad_s16(C.byref(mk(dwz)), inv_p, s), "atomics entry")
    torch.cuda.synchronize()
    got, atom = unpack(outs[0][0].t), unpack(dwz.t)
    want = W.reference(c, o=o)
    scale = float(want.abs().max())
    e_det, e_atom = W.rel_err(got, want), W.rel_err(atom, want)
    d_at = float((got.double() - atom.double()).abs().max()) / scale
    print(f"wgrad_s16_det {c.name} [+det{k}]: e_det {e_det:.3e} e_atomics {e_atom:.3e} det vs atomics {d_at:.3e} (gate {W.GATE:.0e})")
    assert bool(torch.isfinite(got).all()) and e_det <= W.GATE, e_det
    assert d_at <= W.GATE, d_at
    del keep


# ---- fp32 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,B,H,W_,nn,cc,a_step,expect", F32_CASES, ids=[c[0] for c in F32_CASES])
def test_wgrad_f32_det_vs_fp64_and_the_atomics_entry(name, kind, B, H, W_, nn, cc, a_step, expect):
    lib = _lib.load()
    (n, n_true), (cin, c_true) = nn, cc
    tag = "wgdet-" + name
    ntaps = {"conv3": 9, "conv1": 1, "conv4": 16, "convt": 4}[kind]
    g = S.hashed_uniform(tag + "g", (B, n_true, H, W_))
    if kind in ("conv3", "conv1"):
        a = S.hashed_uniform(tag + "a", (B, c_true, H, W_))
        abuf, a_corner, ks = _nhwc(a, cin, 1 if kind == "conv3" else 0), 0, (3 if kind == "conv3" else 1)
    elif kind == "conv4":
        ah, aw = (H - 1, W_ - 1) if a_step == 1 else (2 * H - 2, 2 * W_ - 2)
        a = S.hashed_uniform(tag + "a", (B, c_true, ah, aw))
        abuf, a_corner, ks = _nhwc(a, cin, 2), 0, 4
    else:
        a = S.hashed_uniform(tag + "a", (B, c_true, 2 * H, 2 * W_))
        abuf = _nhwc(a, cin, 1)
        a_corner, ks = _strides(abuf)[1] + _strides(abuf)[2], 2
    wshape = (n_true, c_true, ks, ks)
    gbuf = _nhwc(g, n, 1)
    zeros = W.Guarded(128, fill=0)

    def mk(dw):
        d = AmmcWgradDesc()
        d.g, d.a, d.dw, d.zeros = _ptr(gbuf, _strides(gbuf)[1] + _strides(gbuf)[2]), _ptr(abuf, a_corner), _ptr(dw.t), _ptr(zeros.t)
        d.batch, d.height, d.width, d.n, d.cin, d.ntaps, d.a_step = B, H, W_, n, cin, ntaps, a_step
        d.g_bs, d.g_rs, d.g_ps = _strides(gbuf)
        d.a_bs, d.a_rs, d.a_ps = _strides(abuf)
        return d
    k, need, kpad = _check_splits("f32", mk(zeros), expect)

    def launch(stream):
        dw = W.Guarded(n * kpad)
        slabs = W.Guarded(need) if need else None
        rc = lib.ammc_conv_wgrad_f32_det(C.byref(mk(dw)), _ptr(slabs.t) if slabs else None, need, stream)
        assert rc == 0, rc
        return dw, slabs
    torch.cuda.synchronize()
    outs = _launches(launch)
    packed = _check_slabs_and_bits(outs, k, n, kpad)
    assert zeros.pads_intact()
    _check_zero_padding(packed, n, n_true, cin, c_true, ntaps, kpad, kind == "convt", False)

    s = torch.cuda.current_stream().cuda_stream

    def unpack(p):
        out = torch.empty(wshape, device=DEV)
        if kind == "convt":
            _lib.check(lib.ammc_unpack_convt_wgrad_f32(_ptr(p), n_true, c_true, _ptr(out), s), "unpack_convt")
        else:
            _lib.check(lib.ammc_unpack_conv_wgrad_f32(_ptr(p), n_true, c_true, ks, cin, _ptr(out), s), "unpack")
        return out.cpu()
    dwz = W.Guarded(n * kpad, fill=0)
    _lib.check(lib.ammc_conv_wgrad_f32(C.byref(mk(dwz)), s), "atomics entry")
    torch.cuda.synchronize()
    got, atom = unpack(outs[0][0].t), unpack(dwz.t)
    want = _truth(kind, g, a, wshape, a_step, torch.float64)
    wit = _truth(kind, g, a, wshape, a_step, torch.float32)
    scale = float(want.abs().max())
    e_det = float((got.double() - want).abs().max()) / scale
    e_atom = float((atom.double() - want).abs().max()) / scale
    e_wit = float((wit.double() - want).abs().max()) / scale
    d_at = float((got.double() - atom.double()).abs().max()) / scale
    print(f"wgrad_f32_det {name} [+det{k}]: e_det {e_det:.3e} e_atomics {e_atom:.3e} e_witness {e_wit:.3e} det vs atomics {d_at:.3e}")
    assert e_det <= FACTOR * e_wit, (e_det, e_wit)
    assert d_at <= FACTOR * e_wit, (d_at, e_wit)


def test_the_cases_cover_what_they_are_there_for():
    s16 = [c for c, _ in S16_CASES]
    assert {c.ntaps for c in s16} == {4, 16, 9} and {c.a_step for c in s16} == {1, 2}
    assert {32, 64, 128} <= {c.n for c in s16} and any(c.inv_null for c in s16) and any(not c.inv_null for c in s16)
    assert {e for _, es in S16_CASES for e in es} == {"k>=3", "k>=9", "k==1", "ragged", "m%32"}
    assert {{"conv1": 1, "conv3": 9, "conv4": 16, "convt": 4}[c[1]] for c in F32_CASES} >= {1, 9, 16}
    assert {c[7] for c in F32_CASES} == {1, 2} and {32, 64, 128} <= {c[5][0] for c in F32_CASES}
    assert {e for c in F32_CASES for e in c[8]} == {"k>=3", "k>=9", "k==1", "ragged", "m%32"}
