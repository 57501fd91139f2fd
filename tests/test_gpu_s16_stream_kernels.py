"""The streaming kernels that write or read S16 images on the training path, and the S16 encoder / decoder entry points,
each alone through ctypes against the fp64 references of tests/stream_refs.py and the numpy restatement of the encoding
in tests/s16_codec.py (csrc/train_kernels.hip, conv_gemm_s16.hip, flownet.hip, layout_pool.hip; shapes and inputs:
tests/s16_stream_cases.py, tests/stream_cases.py).  The machinery is that of tests/test_gpu_stream_kernels.py: "grid"
inputs must give the reference rounded to fp32, "cont" inputs are held per element to a bound derived from the kernel
(u = 2^-24, times 2; `RATIO` lines, AMMC_STREAM_RATIOS), every output is a view inside a sentinel-filled buffer.

The exactness rule of the S16 outputs: where a kernel can also store its fp32 value (y32, dc32) the twin must be
`encode` of that stored value (times the power-of-two factor), bit for bit, and the same bits without the fp32 output;
where it cannot (`ammc_split_scaled_strided_f32`, `ammc_split_rows_scaled_f32`, `ammc_lrelu_s16`) every fp32 operation
of the kernel is a single correctly rounded one and the expected bits are the numpy float32 emulation.

`ammc_reduce_partials_seg_f32`: the columns from `max_from` on are combined by a maximum that starts from 0, so they
are non-negative by contract (max |g|, max |xhat| rows); the test keeps to that.

AMMC_ROW_KERNELS=0 (the one-item forms of the two apply passes) runs in one child process
(`test_one_item_forms_in_a_child_process`): the parent hands it a SHA-256 of every output of every apply case and the
child asserts, besides its own parity, that the one-item form's bits are the row form's."""
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd.engine import Act, _ptr

import s16_codec as Q
import s16_stream_cases as C
import stream_cases as K
import stream_refs as R
from test_gpu_stream_kernels import (DEV, EINVAL, EUNSUP, SENT, U, _bits, _bounded, _chain, _dev, _exact, _in_act, _out_act,
                                     _partial, _partial_ok, _reduce, _s, _sent, _untouched)

pytestmark = pytest.mark.gpu
N_INV = 1024                                   # what train.py passes
SWITCH = "AMMC_ROW_KERNELS"
DIGEST_ENV = "AMMC_S16_STREAM_DIGESTS"         # the child reads the row forms' digests from the file this names
ROWS_ON = SWITCH not in os.environ or os.environ[SWITCH].strip() not in ("0", "")
DIGESTS = {}
BYTE_SENT = 0xA5


# ---- helpers ---------------------------------------------------------------------------------------------------------

def _np32(t):
    return t.detach().float().cpu().contiguous().numpy()


def _act_words(a: Act):
    return a.buf.view(torch.int32)[:, 1:1 + a.H, 1:1 + a.W, a.c_off:a.c_off + a.c].cpu().contiguous().numpy()


def _same_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ; (index, got, want): "
                             f"{[(tuple(i), hex(int(got[tuple(i)]) & 0xFFFFFFFF), hex(int(want[tuple(i)]) & 0xFFFFFFFF)) for i in idx]}")


def _twin_is(a: Act, t32, what):
    """the S16 view `a` holds `encode` of the fp32 values t32 [B, H, W, c]"""
    _same_words(_act_words(a), Q.words(np.asarray(t32, dtype=np.float32)), what)


def _twin_in(t, ctot=None, c_off=0):
    """the fp32 NHWC tensor t, encoded on the HOST, as a channel slice of a ctot-wide S16 buffer with a one-pixel halo; the
    rest of the buffer holds the encoding of a large finite value"""
    b, h, w, c = t.shape
    full = torch.full((b, h + 2, w + 2, ctot or c), 1.0e4)
    full[:, 1:-1, 1:-1, c_off:c_off + c] = t
    buf = torch.from_numpy(Q.words(full.numpy())).to(DEV).view(torch.float32)
    return Act(buf, b, h, w, c, c_off, 1)


def _slots(*values):
    """256 amax slots (fp32 bit patterns), the given ones scattered over them, behind them a sentinel tail"""
    t = torch.zeros(256 + 8, dtype=torch.int32)
    t[256:] = SENT
    for i, v in enumerate(values):
        t[(37 + 101 * i) % 256] = Q.f32_bits(v)
    return t.to(DEV)


def _slot_max(slots):
    assert bool((slots[256:] == SENT).all()), "a write behind the 256 slots"
    return int(slots[:256].max())


def _inv():
    return _sent(N_INV + 32)


def _inv_ok(inv, f, what):
    want = torch.full((N_INV,), 1.0 / f)
    assert float(want[0]) * f == 1.0
    _bits(inv[:N_INV], want, f"{what}: inv_scale[0..{N_INV})")
    assert bool((inv.view(torch.int32)[N_INV:] == SENT).all()), f"{what}: inv_scale written behind n_inv"


def _idx_buf(n):
    return torch.full((n + 64,), BYTE_SENT, dtype=torch.uint8, device=DEV)


def _same_buf(a, b, what):
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what


def _digest(key, *tensors):
    """SHA-256 of the outputs of an apply case; inside the child: the one-item form's bits against the row form's"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    DIGESTS[key] = h.hexdigest()
    if os.environ.get(DIGEST_ENV):
        with open(os.environ[DIGEST_ENV]) as fp:
            ref = json.load(fp)
        assert key in ref, key
        assert ref[key] == DIGESTS[key], f"{key}: the one-item form's bits differ from the row form's"


def _takes_rows(lib, c, ps_a, ps_b, ps_c, w):
    """which form the entry points take, asserted through the library's own predicate"""
    got = lib.ammc_bn_bwd_unpool_supported(c, ps_a, ps_b, ps_c, w)
    assert got == int(C.rows_form(c) and ROWS_ON), (c, got)
    return bool(got)


def _amb(x, scale, shift, relu):
    """1 where pre = x scale + shift lies within its own rounding error of zero (the mask may fall either way)"""
    xd, sc, sh = x.double(), scale.double(), shift.double()
    if not relu:
        return torch.zeros_like(xd)
    return ((xd * sc + sh).abs() <= 2 * U * ((xd * sc).abs() + sh.abs())).double()


# ---- the apply pass of a BatchNorm unit: y = act(x scale + shift) + res ----------------------------------------------------

def _ssa_bound(x, scale, shift, res):
    """t = x scale + shift: the product and the sum (one rounding if contracted), the residual's addition: k = 3 over the
    sum of the magnitudes; ReLU is monotone and 1-Lipschitz: it adds nothing"""
    return 3 * U * ((x.double() * scale.double()).abs() + shift.double().abs() + (res.double().abs() if res is not None else 0.0))


@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_scale_shift_act_f32_and_s16(shape, kind):
    lib = _lib.load()
    b, h, w, c = shape
    x, scale, shift, res = C.ssa_case(kind, shape)
    X, RS = _in_act(x, c + 8, 4), _in_act(res, c, 0)                    # a slice of a wider buffer / a dense tensor
    sc_d, sh_d = _dev(scale, shift)
    for relu in (0, 1):
        for use_res in (0, 1):
            what = f"{shape} {kind} relu={relu} res={use_res}"
            r_args = (RS.pix0(), *RS.strides) if use_res else (None, 0, 0, 0)

            def run(with32):
                y16, y32 = _out_act(b, h, w, c, c + 8, 8), (_out_act(b, h, w, c, c + 8, 8) if with32 else None)
                _lib.check(lib.ammc_scale_shift_act_s16_f32(X.pix0(), *X.strides, _ptr(sc_d), _ptr(sh_d), *r_args, y32.pix0() if with32 else None,
                                                            y16.pix0(), *y16.strides, relu, b, h, w, c, _s()), "scale_shift_act_s16")
                _untouched(y16)
                if with32:
                    _untouched(y32)
                return y16, y32

            _takes_rows(lib, c, X.ps, RS.ps if use_res else 0, c + 8, w)
            y16, y32 = run(1)
            z16, _ = run(0)
            t16, t32 = run(1)
            _same_buf(y16.buf, z16.buf, f"{what}: the twin without the fp32 output")
            _same_buf(y16.buf, t16.buf, f"{what}: a second launch (twin)")
            _same_buf(y32.buf, t32.buf, f"{what}: a second launch (y32)")
            F = _out_act(b, h, w, c, c + 4, 0)
            _lib.check(lib.ammc_scale_shift_act_f32(X.pix0(), *X.strides, _ptr(sc_d), _ptr(sh_d), *r_args, F.pix0(), *F.strides, relu,
                                                    b, h, w, c, _s()), "scale_shift_act")
            _untouched(F)
            _bits(F.interior(), y32.interior(), f"{what}: the fp32 kernel against the S16 kernel's y32")
            _twin_is(y16, _np32(y32.interior()), f"{what}: y16 against encode(y32)")
            want = R.scale_shift_act(x, scale, shift, res if use_res else None, relu)
            if kind == "grid":
                _exact(y32.interior(), want, what)
                if not use_res:
                    assert not (Q.unpack(_act_words(y16))[1] & 0x7FFF).any(), "a grid activation with a lo half"
            else:
                bound = _ssa_bound(x, scale, shift, res if use_res else None)
                _bounded("scale_shift_act_s16_f32", y32.interior(), want, 2 * bound, what)
            _digest(f"ssa {what}", y16.buf, y32.buf)


@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", C.POOL_SHAPES)
def test_scale_shift_act_s16_with_the_pooled_output(shape, kind):
    """against the reference, not against the two-pass composition: y32 to the reference, y16 = encode(y32), the pooled twin =
    the (hi, lo) bits of the first maximum of the decoded window, idx = its position"""
    lib = _lib.load()
    b, h, w, c = shape
    ph, pw = h // 2, w // 2
    x, scale, shift = C.pool_case(kind, shape)
    X = _in_act(x, c + 8, 4)
    sc_d, sh_d = _dev(scale, shift)
    for relu in (0, 1):
        what = f"{shape} {kind} relu={relu}"

        def run(with32, hh=h):
            y16, y32 = _out_act(b, h, w, c, c + 8, 8), _out_act(b, h, w, c, c + 8, 8)
            p16, idx = _out_act(b, ph, pw, c, c, 0), _idx_buf(b * ph * pw * c)
            rc = lib.ammc_scale_shift_act_s16_pool_f32(X.pix0(), *X.strides, _ptr(sc_d), _ptr(sh_d), y32.pix0() if with32 else None, y16.pix0(),
                                                       *y16.strides, p16.pix0(), *p16.strides, idx.data_ptr(), relu, b, hh, w, c, _s())
            return rc, y16, y32, p16, idx

        rc, y16, y32, p16, idx = run(1)
        sup = lib.ammc_scale_shift_act_s16_pool_supported(c, h, w, X.rs, X.ps, y16.rs, y16.ps, p16.ps)
        assert sup == int(C.rows_form(c) and ROWS_ON)
        if not sup:                                                    # the predicate agrees with what the entry does
            torch.cuda.synchronize()
            assert rc == EUNSUP
            for t in (y16.buf, y32.buf, p16.buf):
                assert bool((t.view(torch.int32) == SENT).all())
            continue
        _lib.check(rc, "scale_shift_act_s16_pool")
        n = b * ph * pw * c
        for a in (y16, y32, p16):
            _untouched(a)
        assert bool((idx[n:] == BYTE_SENT).all()), "idx written behind its last byte"
        rc2, z16, z32, q16, jdx = run(0)
        _lib.check(rc2, "scale_shift_act_s16_pool (no y32)")
        assert bool((z32.buf.view(torch.int32) == SENT).all())
        _same_buf(y16.buf, z16.buf, f"{what}: the twin without the fp32 output")
        _same_buf(p16.buf, q16.buf, f"{what}: the pooled twin without the fp32 output")
        _same_buf(idx, jdx, f"{what}: idx without the fp32 output")
        rc3, t16, t32, r16, kdx = run(1)
        for u, v in ((y16.buf, t16.buf), (y32.buf, t32.buf), (p16.buf, r16.buf), (idx, kdx)):
            _same_buf(u, v, f"{what}: a second launch")
        want = R.scale_shift_act(x, scale, shift, None, relu)
        if kind == "grid":
            _exact(y32.interior(), want, what)
        else:
            _bounded("scale_shift_act_s16_pool_f32", y32.interior(), want, 2 * _ssa_bound(x, scale, shift, None), what)
        _twin_is(y16, _np32(y32.interior()), f"{what}: y16 against encode(y32)")
        yw = _act_words(y16)
        arg = R.maxpool2x2_arg(torch.from_numpy(Q.decode(yw)))
        hi, lo = Q.unpack(yw)
        pick = lambda t: R._windows(torch.from_numpy(t.astype(np.int64))).gather(3, arg[:, :, :, None]).squeeze(3).numpy().astype(np.uint16)
        _same_words(_act_words(p16), Q.pack(pick(hi), pick(lo)), f"{what}: the pooled twin")
        got_idx = idx[:n].view(b, ph, pw, c).cpu().long()
        assert torch.equal(got_idx, arg), f"{what}: idx; {int((got_idx != arg).sum())} positions differ"
        if kind == "grid":                                            # the six planted pairs: the first maximum in row-major order
            pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
            first = torch.tensor([pairs[i % 6][0] for i in range(b * ph * pw)]).view(b, ph, pw)
            assert torch.equal(got_idx[..., 0], first) and torch.equal(got_idx[..., 1], first), f"{what}: a tie not won by the first maximum"
    # an odd size is refused before any launch, and the predicate says so
    rc, y16, y32, p16, idx = run(1, h - 1)
    torch.cuda.synchronize()
    assert rc == EUNSUP and lib.ammc_scale_shift_act_s16_pool_supported(c, h - 1, w, X.rs, X.ps, y16.rs, y16.ps, p16.ps) == 0
    assert bool((y16.buf.view(torch.int32) == SENT).all()) and bool((idx == BYTE_SENT).all())


# ---- max-pool on S16 and its gradient from the recorded positions ----------------------------------------------------------

@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("c", [8, 128])
@pytest.mark.parametrize("fh,fw", K.POOL_BWD_SIZES)
def test_maxpool2x2_s16_idx_and_the_gradient_from_idx(fh, fw, c, kind):
    """selections and at most one fp32 addition: bit-exact for both kinds.  The input twin is encoded on the host."""
    lib = _lib.load()
    b, h, w = 2, fh // 2, fw // 2
    x, dp, add = K.pool_bwd_case(kind, b, fh, fw, c)
    X16 = _twin_in(x, c + 8, 8)
    Pa, Pb, idx = _out_act(b, h, w, c, c + 8, 0), _out_act(b, h, w, c, c, 0), _idx_buf(b * h * w * c)
    n = b * h * w * c
    _lib.check(lib.ammc_maxpool2x2_s16(X16.pix0(), *X16.strides, Pa.pix0(), *Pa.strides, b, h, w, c, _s()), "maxpool_s16")
    _lib.check(lib.ammc_maxpool2x2_s16_idx(X16.pix0(), *X16.strides, Pb.pix0(), *Pb.strides, idx.data_ptr(), b, h, w, c, _s()), "maxpool_s16_idx")
    _untouched(Pa)
    _untouched(Pb)
    assert bool((idx[n:] == BYTE_SENT).all())
    hi, lo = Q.encode(x.numpy())
    arg = R.maxpool2x2_arg(torch.from_numpy(Q.decode(Q.pack(hi, lo))))
    pick = lambda t: R._windows(torch.from_numpy(t.astype(np.int64))).gather(3, arg[:, :, :, None]).squeeze(3).numpy().astype(np.uint16)
    want = Q.pack(pick(hi), pick(lo))
    _same_words(_act_words(Pa), want, "maxpool2x2_s16")
    _same_words(_act_words(Pb), want, "maxpool2x2_s16_idx")
    got_idx = idx[:n].view(b, h, w, c).cpu().long()
    assert torch.equal(got_idx, arg), int((got_idx != arg).sum())
    if kind == "grid":
        pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
        first = torch.tensor([pairs[i % 6][0] for i in range(b * h * w)]).view(b, h, w)
        assert torch.equal(got_idx[..., 0], first) and torch.equal(got_idx[..., 1], first)
    idx2 = _idx_buf(n)
    Pc = _out_act(b, h, w, c, c, 0)
    _lib.check(lib.ammc_maxpool2x2_s16_idx(X16.pix0(), *X16.strides, Pc.pix0(), *Pc.strides, idx2.data_ptr(), b, h, w, c, _s()), "again")
    _same_buf(Pb.buf, Pc.buf, "a second launch")
    _same_buf(idx, idx2, "a second launch (idx)")
    # the gradient routed by those bytes (read from a buffer of their own: the reference's positions)
    idx_in = _idx_buf(n)
    idx_in[:n] = arg.to(torch.uint8).reshape(-1).to(DEV)
    P, A = _in_act(dp, c, 0), _in_act(add, c + 8, 8)
    for with_add in (0, 1):
        O = _out_act(b, fh, fw, c, c + 12, 4)
        a_args = (A.pix0(), *A.strides) if with_add else (None, 0, 0, 0)
        _lib.check(lib.ammc_maxpool2x2_bwd_idx_f32(idx_in.data_ptr(), P.pix0(), *P.strides, *a_args, O.pix0(), *O.strides, b, h, w, fh, fw, c,
                                                   _s()), "maxpool_bwd_idx")
        _untouched(O)
        want_dx = R.unpool2x2(dp, arg, fh, fw) + (add.double() if with_add else 0.0)
        _exact(O.interior(), want_dx, f"dx {fh}x{fw} c={c} add={with_add}")
        if fh & 1:
            _exact(O.interior()[:, -1], add[:, -1].double() if with_add else torch.zeros(b, fw, c), "the odd last row")
        if fw & 1:
            _exact(O.interior()[:, :, -1], add[:, :, -1].double() if with_add else torch.zeros(b, fh, c), "the odd last column")


# ---- BatchNorm backward: the reductions with the two maxima ----------------------------------------------------------------

def _check_reduce_bound(lib, kernel, shape, kind, relu, x, g32, scale, shift, mean, invstd, part, nb, k_extra):
    """part[nb][4][C] of chan_reduce_kernel<3>: sums as test_bn_bwd_reduce (chain with U = 4), the two maxima.  g32 = the fp32
    gradient the kernel sees before the mask (for the unpool form: add + scatter(dpo), one rounding, k_extra = 1)"""
    b, h, w, c = shape
    m = b * h * w
    _partial_ok(part, nb)
    out = _sent(2, 4 * c)
    _lib.check(lib.ammc_reduce_partials_seg_f32(_ptr(part), nb, 4 * c, nb, 2 * c, _ptr(out), _s()), "reduce_seg")
    assert bool((out.view(torch.int32)[1] == SENT).all())
    tot = out[0]
    _bits(tot[:2 * c], _reduce(lib, part, nb, 4 * c)[:2 * c], "one segment of all rows == ammc_reduce_partials_f32")
    sg, sgx = R.bn_bwd_sums(x, g32, mean, invstd, scale, shift, relu)
    xd, gd = x.double(), g32.double()
    xh = (xd - mean.double()) * invstd.double()
    g = R.bn_masked_grad(x, g32, scale, shift, relu)
    what = f"{shape} {kind} relu={relu}"
    if kind == "grid":
        _exact(tot[:c], sg, f"sum g {what}")
        _exact(tot[c:2 * c], sgx, f"sum g xhat {what}")
        _exact(tot[2 * c:3 * c], g.abs().amax((0, 1, 2)), f"max |g| {what}")
        _exact(tot[3 * c:], xh.abs().amax((0, 1, 2)), f"max |xhat| {what}")
        return
    n = _chain(lib, m, c, 4)
    amb = _amb(x, scale, shift, relu)
    b_g = 2 * ((n + 1 + k_extra) * U * g.abs().sum((0, 1, 2)) + (amb * gd.abs()).sum((0, 1, 2)))
    b_gx = 2 * ((n + 4 + k_extra) * U * (g * xh).abs().sum((0, 1, 2)) + (amb * (gd * xh).abs()).sum((0, 1, 2)))
    _bounded(kernel, tot[:c], sg, b_g, f"sum g {what}")
    _bounded(kernel, tot[c:2 * c], sgx, b_gx, f"sum g xhat {what}")
    # max |g|: a selection among the fp32 values - exact, but for elements whose mask is ambiguous, which may count or not
    lo = (g.abs() * (1 - amb)).amax((0, 1, 2))
    hi = torch.maximum(g.abs(), amb * gd.abs()).amax((0, 1, 2))
    got = tot[2 * c:3 * c].double().cpu()
    assert bool(((got >= lo) & (got <= hi)).all()), f"max |g| {what}: {got.tolist()} outside [{lo.tolist()}, {hi.tolist()}]"
    # max |xhat|: xhat = (x - mean) invstd, two roundings
    _bounded(kernel, tot[3 * c:], xh.abs().amax((0, 1, 2)), 2 * 2 * U * xh.abs().amax((0, 1, 2)), f"max |xhat| {what}")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", K.CHAN_SHAPES)
def test_bn_bwd_reduce_bound_and_its_unpool_form(shape, kind, relu):
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    x, dy, mean, invstd, scale, shift = K.bn_bwd_case(kind, shape, relu)
    X, D = _in_act(x, c + 8, 4), _in_act(dy, c, 0)
    p_d = _dev(mean, invstd, scale, shift)
    stats = [_ptr(t) for t in p_d]
    nb = lib.ammc_chan_reduce_blocks(m)
    part, again = _partial(nb, 4, c), _partial(nb, 4, c)
    for p in (part, again):
        _lib.check(lib.ammc_bn_bwd_reduce_bound_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, *stats, relu, b, h, w, c, _ptr(p), _s()), "reduce_bound")
    _same_buf(part, again, "a second launch")
    _check_reduce_bound(lib, "bn_bwd_reduce_bound_f32", shape, kind, relu, x, dy, scale, shift, mean, invstd, part, nb, 0)
    # the gradient formed on the fly: add + scatter(dpo by idx)
    ph, pw = h // 2, w // 2
    add, dpo, idx = C.unpool_case(kind, shape)
    A = _in_act(add, c + 8, 8 if c % 8 == 0 else 4)
    P = _in_act(dpo if ph and pw else torch.zeros(b, 1, 1, c), c, 0)
    idx_d = _idx_buf(b * ph * pw * c)
    idx_d[:b * ph * pw * c] = idx.reshape(-1).to(DEV)
    partu, againu = _partial(nb, 4, c), _partial(nb, 4, c)
    rcs = [lib.ammc_bn_bwd_reduce_bound_unpool_f32(X.pix0(), *X.strides, A.pix0(), *A.strides, P.pix0(), *P.strides, idx_d.data_ptr(), ph, pw,
                                                   *stats, relu, b, h, w, c, _ptr(p), _s()) for p in (partu, againu)]
    if c % 8 or ph == 0 or pw == 0:                                     # c & 7, or no window at all: refused before a launch
        torch.cuda.synchronize()
        assert rcs == [EINVAL, EINVAL] and bool((partu.view(torch.int32) == SENT).all())
        return
    _lib.check(rcs[0], "reduce_bound_unpool")
    _same_buf(partu, againu, "a second launch (unpool)")
    g32 = C.unpool_grad(add, dpo, idx).float()
    _check_reduce_bound(lib, "bn_bwd_reduce_bound_unpool_f32", shape, kind, relu, x, g32, scale, shift, mean, invstd, partu, nb, 1)


@pytest.mark.parametrize("nblocks,c", C.FINALIZE_CASES)
def test_bn_bwd_finalize_sums_and_bound_from_given_rows(nblocks, c):
    """the rows are the kernel's input: sums = the correctly rounded float64 column sums; slot (c / 8) & 255 = the maximum over
    its columns of |scale| (max|g| + |sum_g| / M + max|xhat| |sum_gx| / M), within 8 u of the formula in float64"""
    lib = _lib.load()
    pixels = 1000
    rows = S.hashed_normal(f"fin-{nblocks}-{c}", (nblocks, 4, c), 2.0)
    rows[:, 2:] = rows[:, 2:].abs()
    scale = S.hashed_uniform(f"fin-s-{nblocks}-{c}", (c,), 0.25, 2.0) * K.pick(f"fin-n-{nblocks}-{c}", (c,), [-1.0, 1.0])
    part = _partial(nblocks, 4, c)
    part[:nblocks] = rows.to(DEV)
    sc_d, = _dev(scale)
    outs = []
    for _ in range(2):
        sums, slots = _sent(2 * c + 8), _slots()
        _lib.check(lib.ammc_bn_bwd_finalize_f32(_ptr(part), nblocks, c, pixels, _ptr(sc_d), _ptr(sums), slots.data_ptr(), _s()), "bn_bwd_finalize")
        assert bool((sums.view(torch.int32)[2 * c:] == SENT).all())
        _slot_max(slots)
        outs.append((sums, slots))
    _same_buf(outs[0][0], outs[1][0], "a second launch (sums)")
    _same_buf(outs[0][1], outs[1][1], "a second launch (slots)")
    sums, slots = outs[0]
    want = rows.double().sum(0)
    _bits(sums[:c], want[0].float(), "sum g")
    _bits(sums[c:2 * c], want[1].float(), "sum g xhat")
    ic = float(np.float32(1.0) / np.float32(pixels))
    sg32, sgx32 = sums[:c].double().cpu(), sums[c:2 * c].double().cpu()
    formula = scale.double().abs() * (rows[:, 2].double().amax(0) + sg32.abs() * ic + rows[:, 3].double().amax(0) * sgx32.abs() * ic)
    per_slot = torch.zeros(256, dtype=torch.float64)
    for blk in range((c + 7) // 8):
        per_slot[blk & 255] = max(float(per_slot[blk & 255]), float(formula[blk * 8:blk * 8 + 8].max()))
    _bounded("bn_bwd_finalize_f32", slots[:256].view(torch.float32), per_slot, 8 * U * per_slot, f"bound slots ({nblocks},{c})")


PIPE_CASES = ["generic", "all_masked", "negative_scales", "outlier"]


@pytest.mark.parametrize("shape", [(2, 16, 24, 64), (2, 10, 12, 72)])
@pytest.mark.parametrize("case", PIPE_CASES)
def test_bn_bwd_bound_covers_the_gradient_it_scales(case, shape):
    """reduce_bound -> finalize -> apply_s16: the bound in the slots is at least max |dc| (1 - 8 u), so dc f stays in the half
    range; every gradient masked: bound 0, slots 0, factor 1, twin all zero, inv_scale 1"""
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    x, dy, mean, invstd, scale, shift = K.bn_bwd_case("cont", shape, 1)
    if case == "all_masked":
        shift = torch.full_like(shift, -100.0)
    elif case == "negative_scales":
        scale = -scale.abs()
    elif case == "outlier":
        dy[0, 1, 1, 3] *= 1.0e6
    X, D = _in_act(x, c + 8, 4), _in_act(dy, c, 0)
    keep = _dev(mean, invstd, scale, shift)
    stats = [_ptr(t) for t in keep]
    nb = lib.ammc_chan_reduce_blocks(m)
    part = _partial(nb, 4, c)
    _lib.check(lib.ammc_bn_bwd_reduce_bound_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, *stats, 1, b, h, w, c, _ptr(part), _s()), "reduce_bound")
    sums, slots = _sent(2 * c + 8), _slots()
    _lib.check(lib.ammc_bn_bwd_finalize_f32(_ptr(part), nb, c, m, stats[2], _ptr(sums), slots.data_ptr(), _s()), "finalize")
    O16, O32, inv = _out_act(b, h, w, c, c + 8, 8), _out_act(b, h, w, c, c + 8, 8), _inv()
    _lib.check(lib.ammc_bn_bwd_apply_s16_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, *stats, _ptr(sums), 1, O16.pix0(), O32.pix0(),
                                             *O16.strides, b, h, w, c, slots.data_ptr(), _ptr(inv), N_INV, _s()), "apply_s16")
    _untouched(O16)
    _untouched(O32)
    bits = _slot_max(slots)
    f = Q.pow2_to_1024(bits)
    _inv_ok(inv, f, case)
    bound = float(np.array([bits], dtype=np.int32).view(np.float32)[0])
    want = R.bn_bwd_apply(x, dy, mean, invstd, scale, shift, sums[:c].cpu(), sums[c:2 * c].cpu(), 1)
    dc = _np32(O32.interior())
    _twin_is(O16, dc * np.float32(f), f"{case}: dc16 against encode(dc32 f)")
    amb = _amb(x, scale, shift, 1)
    top = float((want.abs() * (1 - amb)).max())
    print(f"RATIO bn_bwd_finalize_f32 {case} {shape}: max |dc| / bound {top / bound if bound else 0.0:.4g}")
    assert bound >= top * (1 - 8 * U), (bound, top)
    assert float(np.abs(dc).max()) * f < 2048.0 * (1 + 8 * U)
    if case == "all_masked":
        assert bits == 0 and int(slots[:256].abs().max()) == 0 and f == 1.0
        assert float(sums[:2 * c].abs().max()) == 0.0
        assert float(np.abs(Q.decode(_act_words(O16))).max()) == 0.0 and float(np.abs(dc).max()) == 0.0
    else:
        assert bound > 0 and top > 0


# ---- BatchNorm backward: the apply pass with the S16 twin as output ------------------------------------------------------

def _apply_bound(x, g64, mean, invstd, scale, shift, sg, sgx, relu, k):
    """test_bn_bwd_apply's bound: k roundings (8; 9 with the addition of the unpool form) over the intermediates'
    magnitudes; an element whose mask is ambiguous may differ by its whole gradient"""
    m = x.shape[0] * x.shape[1] * x.shape[2]
    xd = x.double()
    xh = (xd - mean.double()) * invstd.double()
    g = R.bn_masked_grad(x, g64, scale, shift, relu)
    mag = g.abs() + (sg.double() / m).abs() + (xh * sgx.double() / m).abs()
    return k * U * scale.double().abs() * mag + _amb(x, scale, shift, relu) * (scale.double() * g64).abs()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_bn_bwd_apply_s16_and_its_unpool_form(shape, kind, relu):
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    ph, pw = h // 2, w // 2
    x, dy, mean, invstd, scale, shift = K.bn_bwd_case(kind, shape, relu)
    sg, sgx = K.bn_apply_sums(kind, shape)
    X, D = _in_act(x, c + 8, 4), _in_act(dy, c, 0)
    keep = _dev(mean, invstd, scale, shift, torch.cat([sg, sgx]))
    stats = [_ptr(t) for t in keep]
    add, dpo, idx = C.unpool_case(kind, shape)
    A, P = _in_act(add, c + 16, 8), _in_act(dpo if ph and pw else torch.zeros(b, 1, 1, c), c, 0)
    idx_d = _idx_buf(b * ph * pw * c)
    idx_d[:b * ph * pw * c] = idx.reshape(-1).to(DEV)
    exact = kind == "grid" and K.is_pow2(m)                              # 1 / M exact
    for form in ("plain", "unpool"):
        what = f"{form} {shape} {kind} relu={relu}"
        g64 = dy.double() if form == "plain" else C.unpool_grad(add, dpo, idx)
        want = R.bn_bwd_apply(x, g64, mean, invstd, scale, shift, sg, sgx, relu)
        slots = _slots(1.5 * float(want.abs().max()), 0.3 * float(want.abs().max()))
        f = Q.pow2_to_1024(_slot_max(slots))

        def run(with32):
            o16, o32, inv = _out_act(b, h, w, c, c + 8, 8), (_out_act(b, h, w, c, c + 8, 8) if with32 else None), _inv()
            tail = (relu, o16.pix0(), o32.pix0() if with32 else None, *o16.strides, b, h, w, c, slots.data_ptr(), _ptr(inv), N_INV, _s())
            if form == "plain":
                rc = lib.ammc_bn_bwd_apply_s16_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, *stats, *tail)
            else:
                rc = lib.ammc_bn_bwd_apply_s16_unpool_f32(X.pix0(), *X.strides, A.pix0(), *A.strides, P.pix0(), *P.strides, idx_d.data_ptr(),
                                                          ph, pw, *stats, *tail)
            return rc, o16, o32, inv

        rc, o16, o32, inv = run(1)
        if form == "plain":
            _takes_rows(lib, c, X.ps, D.ps, o16.ps, w)
        else:
            refused = EINVAL if ph == 0 or pw == 0 else (0 if _takes_rows(lib, c, X.ps, A.ps, o16.ps, w) else EUNSUP)
            if refused:                                                # no window at all / the one-item form has no unpool
                torch.cuda.synchronize()
                assert rc == refused, (what, rc)
                for t in (o16.buf, o32.buf, inv):
                    assert bool((t.view(torch.int32) == SENT).all())
                continue
        _lib.check(rc, what)
        _untouched(o16)
        _untouched(o32)
        _inv_ok(inv, f, what)
        _, z16, _, zinv = run(0)
        _, t16, t32, _ = run(1)
        _same_buf(o16.buf, z16.buf, f"{what}: the twin without the fp32 output")
        _inv_ok(zinv, f, what)
        _same_buf(o16.buf, t16.buf, f"{what}: a second launch (twin)")
        _same_buf(o32.buf, t32.buf, f"{what}: a second launch (dc32)")
        dc = _np32(o32.interior())
        _twin_is(o16, dc * np.float32(f), f"{what}: dc16 against encode(dc32 f)")
        # the same arithmetic as the fp32 kernel, "operation for operation": dy of the unpool form = its one fp32 addition
        D2 = D if form == "plain" else _in_act(g64.float(), c, 0)
        F = _out_act(b, h, w, c, c + 4, 0)
        _lib.check(lib.ammc_bn_bwd_apply_f32(X.pix0(), *X.strides, D2.pix0(), *D2.strides, *stats, relu, F.pix0(), *F.strides, b, h, w, c, None,
                                             _s()), "bn_bwd_apply_f32")
        _bits(o32.interior(), F.interior(), f"{what}: dc32 against ammc_bn_bwd_apply_f32")
        if exact:
            _exact(o32.interior(), want, what)
        else:
            bound = _apply_bound(x, g64, mean, invstd, scale, shift, sg, sgx, relu, 8 if form == "plain" else 9)
            _bounded("bn_bwd_apply_s16_f32" if form == "plain" else "bn_bwd_apply_s16_unpool_f32", o32.interior(), want, 2 * bound, what)
        _digest(f"apply {what}", o16.buf, o32.buf, inv)


# ---- the power-of-two factor: the scale cases, once, for its three consumers ---------------------------------------------

@pytest.mark.parametrize("c", [16, 24])
@pytest.mark.parametrize("name", list(C.SCALE_CASES))
def test_scale_factor_boundaries(name, c):
    """max |x| exactly a power of two, one ulp below it, 2^-30, an fp32 subnormal (exponent field 0: the clamp at 2^60), all
    zero (factor 1), a negative largest element, the maximum in the last group: `ammc_absmax_bits_f32` +
    `ammc_split_rows_scaled_f32`, `ammc_chan_sum_absmax_f32` + `ammc_split_scaled_strided_f32`, and
    `ammc_bn_bwd_apply_s16_f32` with statistics that make dc == dy (c = 16: the row form, 24: the one-item form)"""
    lib = _lib.load()
    shape = b, h, w, _ = 2, 3, 5, c
    x = C.scale_values(name, shape, f"sc{c}")
    amax = float(x.abs().max())
    bits = Q.f32_bits(amax)
    f = Q.pow2_to_1024(bits)
    xf = x.numpy() * np.float32(f)                                       # exact: a power of two, no underflow (f >= 2^-60)
    assert np.array_equal(xf.astype(np.float64), x.numpy().astype(np.float64) * f) and float(np.abs(xf).max()) < 2048.0
    n = x.numel()
    # dense
    x_d, slots = x.to(DEV).contiguous(), _slots()
    _lib.check(lib.ammc_absmax_bits_f32(_ptr(x_d), n, slots.data_ptr(), _s()), "absmax_bits")
    assert _slot_max(slots) == bits, (hex(_slot_max(slots)), hex(bits))
    dst, inv = _sent(n + 64), _inv()
    _lib.check(lib.ammc_split_rows_scaled_f32(_ptr(x_d), n, _ptr(dst), slots.data_ptr(), _ptr(inv), N_INV, _s()), "split_rows_scaled")
    _same_words(dst[:n].view(torch.int32).cpu().numpy().reshape(-1, 8), Q.words(xf.reshape(-1, 8)), f"{name}: split_rows_scaled")
    assert bool((dst.view(torch.int32)[n:] == SENT).all())
    _inv_ok(inv, f, name)
    # a channel slice
    X = _in_act(x, c + 8, 8)
    nb = lib.ammc_chan_reduce_blocks(b * h * w)
    part, slots2 = _partial(nb, 1, c), _slots()
    _lib.check(lib.ammc_chan_sum_absmax_f32(X.pix0(), *X.strides, b, h, w, c, _ptr(part), slots2.data_ptr(), _s()), "chan_sum_absmax")
    assert _slot_max(slots2) == bits
    Y, inv2 = _out_act(b, h, w, c, c + 8, 0), _inv()
    _lib.check(lib.ammc_split_scaled_strided_f32(X.pix0(), *X.strides, Y.pix0(), *Y.strides, b, h, w, c, slots2.data_ptr(), _ptr(inv2), N_INV, _s()),
               "split_scaled_strided")
    _untouched(Y)
    _twin_is(Y, xf, f"{name}: split_scaled_strided")
    _inv_ok(inv2, f, name)
    # the BatchNorm-backward apply with mean 0, invstd 1, scale 1, shift 0, sums 0, no mask: dc = 1 (dy - 0 - xhat 0) = dy
    zero, one = torch.zeros(2 * c, device=DEV), torch.ones(c, device=DEV)
    D = _in_act(x, c, 0)
    O16, O32, inv3 = _out_act(b, h, w, c, c + 8, 8), _out_act(b, h, w, c, c + 8, 8), _inv()
    _lib.check(lib.ammc_bn_bwd_apply_s16_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, _ptr(zero), _ptr(one), _ptr(one), _ptr(zero), _ptr(zero),
                                             0, O16.pix0(), O32.pix0(), *O16.strides, b, h, w, c, slots.data_ptr(), _ptr(inv3), N_INV, _s()), "apply_s16")
    _untouched(O16)
    _untouched(O32)
    _exact(O32.interior(), x.double(), f"{name}: dc32 == dy")
    _twin_is(O16, _np32(O32.interior()) * np.float32(f), f"{name}: dc16")
    _inv_ok(inv3, f, name)


def test_absmax_bits_second_trip_of_the_grid_stride_loop():
    """the grid caps at 2048 workgroups of 256 threads, a thread takes 8 floats: 4,194,304 + 2,400 floats put 300 groups into a
    second trip, and the maximum sits there (16 MB)"""
    lib = _lib.load()
    n = 4_194_304 + 2_400
    i = torch.arange(n, device=DEV, dtype=torch.int64)
    x = ((i * 2654435761) % 2039).float() / 2048.0 - 0.5
    x[n - 7] = -3.0
    slots = _slots()
    _lib.check(lib.ammc_absmax_bits_f32(_ptr(x), n, slots.data_ptr(), _s()), "absmax_bits")
    assert _slot_max(slots) == Q.f32_bits(3.0), hex(_slot_max(slots))
    f = Q.pow2_to_1024(Q.f32_bits(3.0))
    dst, inv = _sent(n + 64), _inv()
    _lib.check(lib.ammc_split_rows_scaled_f32(_ptr(x), n, _ptr(dst), slots.data_ptr(), _ptr(inv), N_INV, _s()), "split_rows_scaled")
    assert f == 512.0
    _inv_ok(inv, f, "16 MB")
    assert bool((dst.view(torch.int32)[n:] == SENT).all())
    _same_words(dst[:n].view(torch.int32).cpu().numpy().reshape(-1, 8), Q.words((x.cpu().numpy() * np.float32(f)).reshape(-1, 8)), "16 MB: the twin")


# ---- the encoders and the decoder --------------------------------------------------------------------------------------

def _codec_tensor(tag, n):
    t = torch.from_numpy(C.codec_values(tag, n).copy())
    edge = [0.0, -0.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1.0, -1.0 - 2.0 ** -12]
    if n >= 2 * len(edge):
        t[n // 2:n // 2 + len(edge)] = torch.tensor(edge)
    return t


@pytest.mark.parametrize("n", [8, 8 * 257, 8 * 1000])
def test_split_rows_and_the_range_flag(n):
    """bits against `encode`; the flag is sticky and raised by 65504 < |v|; a NULL flag is accepted; the last group is written
    and nothing behind it"""
    lib = _lib.load()
    x = _codec_tensor(f"split-{n}", n)
    x_d, = _dev(x)
    want = Q.words(x.numpy().reshape(-1, 8))

    def run(src, flag):
        dst = _sent(n + 64)
        _lib.check(lib.ammc_split_rows_guarded_f32(_ptr(src), n, _ptr(dst), flag.data_ptr() if flag is not None else None, _s()), "split_guarded")
        assert bool((dst.view(torch.int32)[n:] == SENT).all())
        return dst[:n].view(torch.int32).cpu().numpy().reshape(-1, 8)

    dst = _sent(n + 64)
    _lib.check(lib.ammc_split_rows_f32(_ptr(x_d), n, _ptr(dst), _s()), "split_rows")
    assert bool((dst.view(torch.int32)[n:] == SENT).all())
    _same_words(dst[:n].view(torch.int32).cpu().numpy().reshape(-1, 8), want, "split_rows")
    flag = torch.tensor([0, SENT], dtype=torch.int32, device=DEV)
    _same_words(run(x_d, flag), want, "split_rows_guarded")
    assert flag.tolist() == [0, SENT], "in range, and the flag moved"
    _same_words(run(x_d, None), want, "split_rows_guarded, NULL flag")
    bad = x.clone()
    bad[n - 1] = 65505.0                                               # rounds to 65504 in hi, yet beyond the range
    if n > 8:
        bad[1] = -1.0e6                                                # hi = -inf
    bad_d, = _dev(bad)
    _same_words(run(bad_d, flag), Q.words(bad.numpy().reshape(-1, 8)), "split_rows_guarded, out of range")
    assert flag.tolist() == [1, SENT], "65504 < |v| did not raise the flag"
    run(x_d, flag)
    assert flag.tolist() == [1, SENT], "the flag is not sticky"


@pytest.mark.parametrize("c,cp", [(3, 8), (12, 16), (16, 16)])
def test_nchw_to_s16_and_back(c, cp):
    lib = _lib.load()
    b, h, w = 2, 5, 7
    x = S.hashed_normal(f"n2s-{c}", (b, c, h, w), 3.0)
    x[0, 0, 0, 0], x[0, 0, 0, 1] = 0.0, -0.0
    x_d, = _dev(x)
    Y = _out_act(b, h, w, cp, cp + 8, 8)
    _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(x_d), b, c, h, w, Y.pix0(), *Y.strides, cp, _s()), "nchw_to_s16")
    _untouched(Y)
    _twin_is(Y, R.nchw_to_nhwc(x, cp).float().numpy(), "nchw_to_s16")
    yw = _act_words(Y)
    hi, lo = Q.unpack(yw)
    assert not hi[..., c:].any() and not lo[..., c:].any(), "padding channels are not +0 in both halves"
    n = b * cp * h * w
    back = _sent(n + 32)
    _lib.check(lib.ammc_s16_to_nchw_f32(Y.pix0(), *Y.strides, b, cp, h, w, _ptr(back), _s()), "s16_to_nchw")
    assert bool((back.view(torch.int32)[n:] == SENT).all())
    dec = Q.decode(yw)                                                 # exact in fp32 (tests/test_s16_stream_refs_host.py)
    _bits(back[:n].view(b, cp, h, w), torch.from_numpy(dec).permute(0, 3, 1, 2).float(), "s16_to_nchw against decode")


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("kind", ["grid", "cont"])
def test_lrelu_s16_on_a_channel_slice(kind, slope):
    """decode (exact), one correctly rounded multiplication or none, encode: the numpy float32 emulation, bit for bit; in place
    on channels [32, 72) of a 96-wide twin whose other bits stay"""
    lib = _lib.load()
    b, h, w, ctot, c0, c = 2, 5, 7, 96, 32, 40
    x = K.values(kind, f"lr16-{kind}", (b, h + 2, w + 2, ctot), 3.0)
    x[0, 1, 1, c0], x[0, 1, 1, c0 + 1], x[0, 1, 2, c0] = 0.0, -0.0, -0.0
    before = Q.words(x.numpy())
    buf = torch.from_numpy(before.copy()).to(DEV).view(torch.float32)
    a = Act(buf, b, h, w, c, c0, 1)
    _lib.check(lib.ammc_lrelu_s16(a.pix0(), *a.strides, b, h, w, c, slope, _s()), "lrelu_s16")
    hi, lo = Q.unpack(before)
    v = hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32) * np.float32(1.0 / 2048.0)
    out = np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)
    want_hi, want_lo = Q.encode(out)
    sl = (slice(None), slice(1, h + 1), slice(1, w + 1), slice(c0, c0 + c))
    hi[sl], lo[sl] = want_hi[sl], want_lo[sl]
    _same_words(buf.view(torch.int32).cpu().numpy(), Q.pack(hi, lo), f"lrelu_s16 {kind} slope={slope}")


# ---- reductions of partial rows, channel sums with the maximum ---------------------------------------------------------

@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", K.CHAN_SHAPES)
def test_chan_sum_absmax_and_the_strided_split(shape, kind):
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    x = K.values(kind, f"csa-{kind}-{shape}", shape)
    if kind == "cont":
        x = x + 0.5
    X = _in_act(x, c + 8, 8)
    nb = lib.ammc_chan_reduce_blocks(m)
    part, part1, slots = _partial(nb, 1, c), _partial(nb, 1, c), _slots()
    _lib.check(lib.ammc_chan_sum_absmax_f32(X.pix0(), *X.strides, b, h, w, c, _ptr(part), slots.data_ptr(), _s()), "chan_sum_absmax")
    _lib.check(lib.ammc_chan_sum_f32(X.pix0(), *X.strides, b, h, w, c, _ptr(part1), _s()), "chan_sum")
    _partial_ok(part, nb)
    _bits(part[:nb], part1[:nb], "the rows of chan_sum_absmax == chan_sum's (the same walk)")
    tot = _reduce(lib, part, nb, c)
    s, _ = R.chan_sums(x)
    if kind == "grid":
        _exact(tot, s, f"chan_sum_absmax {shape}")
    else:
        n = _chain(lib, m, c, 8)
        _bounded("chan_sum_absmax_f32", tot, s, 2 * (n + 1) * U * x.double().abs().sum((0, 1, 2)), f"sum {shape}")
    bits = Q.f32_bits(float(x.abs().max()))
    assert _slot_max(slots) == bits, "the slots' maximum is not the bit pattern of max |x|"
    f = Q.pow2_to_1024(bits)
    Y, inv = _out_act(b, h, w, c, c + 8 if c % 8 == 0 else c + 4, 0), _inv()
    rc = lib.ammc_split_scaled_strided_f32(X.pix0(), *X.strides, Y.pix0(), *Y.strides, b, h, w, c, slots.data_ptr(), _ptr(inv), N_INV, _s())
    if c % 8:
        torch.cuda.synchronize()
        assert rc == EINVAL and bool((Y.buf.view(torch.int32) == SENT).all())
        return
    _lib.check(rc, "split_scaled_strided")
    _untouched(Y)
    _twin_is(Y, x.numpy() * np.float32(f), f"split_scaled_strided {shape} {kind}")
    _inv_ok(inv, f, "split_scaled_strided")
    Y2 = _out_act(b, h, w, c, c + 8, 0)
    _lib.check(lib.ammc_split_scaled_strided_f32(X.pix0(), *X.strides, Y2.pix0(), *Y2.strides, b, h, w, c, slots.data_ptr(), _ptr(_inv()), N_INV,
                                                 _s()), "again")
    _same_buf(Y.buf, Y2.buf, "a second launch")


@pytest.mark.parametrize("rows,seg", C.SEG_CASES)
def test_reduce_partials_in_segments(rows, seg):
    """sums = the correctly rounded float64 sums of each run of rows, maxima exact (non-negative columns: see the header)"""
    lib = _lib.load()
    nseg = (rows + seg - 1) // seg
    for qc in C.SEG_QC:
        part = S.hashed_uniform(f"seg-{rows}-{qc}", (rows, qc), 0.0, 1.0)
        p_d = _partial(rows, 1, qc)
        p_d[:rows, 0] = part.to(DEV)
        for max_from in (0, (qc // 2) & ~7, qc):
            assert max_from % 8 == 0
            out = _sent(nseg + 1, qc)
            _lib.check(lib.ammc_reduce_partials_seg_f32(_ptr(p_d), rows, qc, seg, max_from, _ptr(out), _s()), "reduce_seg")
            assert bool((out.view(torch.int32)[nseg] == SENT).all()), "a write behind the last segment"
            runs = [part[i * seg:(i + 1) * seg] for i in range(nseg)]
            what = f"({rows},{seg}) qc={qc} max_from={max_from}"
            _bits(out[:nseg, :max_from], torch.stack([r.double().sum(0).float() for r in runs])[:, :max_from], f"sums {what}")
            _bits(out[:nseg, max_from:], torch.stack([r.max(0).values for r in runs])[:, max_from:], f"maxima {what}")


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 5, 7, 12)])
def test_zero_halo(shape):
    """the one-pixel ring of a dense [B][H+2][W+2][C] buffer becomes +0, the interior and what lies behind stay"""
    lib = _lib.load()
    b, h, w, c = shape
    n = b * (h + 2) * (w + 2) * c
    flat = _sent(n + 64)
    _lib.check(lib.ammc_zero_halo_f32(_ptr(flat), b, h, w, c, _s()), "zero_halo")
    bits = flat.view(torch.int32)
    assert bool((bits[n:] == SENT).all())
    img = bits[:n].view(b, h + 2, w + 2, c)
    ring = torch.ones(b, h + 2, w + 2, c, dtype=torch.bool, device=DEV)
    ring[:, 1:-1, 1:-1] = False
    assert bool((img[ring] == 0).all()), "the ring is not +0"
    assert bool((img[~ring] == SENT).all()), "the interior was touched"


# ---- refusals: arguments that are turned away before any launch ------------------------------------------------------

def test_refusals_before_any_launch():
    lib = _lib.load()
    s = _s()
    t = torch.zeros(8192, device=DEV)
    i = torch.zeros(256, dtype=torch.int32, device=DEV)
    by = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p, ip, bp = _ptr(t), i.data_ptr(), by.data_ptr()
    odd = _ptr(t, 4)                                                   # 16 bytes in: not a 32-byte twin address
    st, bad_st = (512, 128, 16), (512, 128, 12)                        # a pixel stride that is no multiple of 8
    # scale_shift_act_s16: c & 7, c > 1024, a misaligned twin, strides, NULL pointers
    ssa = lambda x=p, sc=p, sh=p, y16=p, yst=st, c=16: lib.ammc_scale_shift_act_s16_f32(x, *st, sc, sh, None, 0, 0, 0, None, y16, *yst, 1, 1, 2, 2, c, s)
    assert [ssa(c=12), ssa(c=1032), ssa(y16=odd), ssa(yst=bad_st), ssa(x=None), ssa(sc=None), ssa(y16=None)] == [EINVAL] * 7
    assert lib.ammc_scale_shift_act_f32(p, *st, p, p, None, 0, 0, 0, None, *st, 1, 1, 2, 2, 16, s) == EINVAL
    assert lib.ammc_scale_shift_act_f32(p, *st, p, p, None, 0, 0, 0, p, *st, 1, 1, 2, 2, 6, s) == EINVAL
    pool = lambda y16=p, p16=p, idx=bp, yst=st, pst=st, c=16, h=2: lib.ammc_scale_shift_act_s16_pool_f32(p, *st, p, p, None, y16, *yst, p16, *pst, idx, 1, 1, h, 2, c, s)
    assert [pool(c=12), pool(y16=odd), pool(p16=odd), pool(idx=bp + 4), pool(yst=bad_st), pool(pst=bad_st), pool(idx=None), pool(p16=None)] == [EINVAL] * 8
    assert pool(h=3) == EUNSUP
    # bn_bwd_apply_s16 and its unpool form
    app = lambda dc16=p, ost=st, c=16, amax=ip, inv=p, n_inv=8, dy=p: lib.ammc_bn_bwd_apply_s16_f32(p, *st, dy, *st, p, p, p, p, p, 1, dc16, None, *ost, 1, 2, 2, c,
                                                                                                    amax, inv, n_inv, s)
    assert [app(c=12), app(c=1032), app(dc16=odd), app(ost=bad_st), app(amax=None), app(inv=None), app(n_inv=0), app(dy=None), app(dc16=None)] == [EINVAL] * 9
    unp = lambda ph=1, pw=1, dpo=p, idx=bp, pst=st, c=16, dc16=p: lib.ammc_bn_bwd_apply_s16_unpool_f32(p, *st, p, *st, dpo, *pst, idx, ph, pw, p, p, p, p, p, 1, dc16, None,
                                                                                                       *st, 1, 2, 2, c, ip, p, 8, s)
    assert [unp(ph=2), unp(pw=0), unp(dpo=None), unp(idx=None), unp(idx=bp + 4), unp(pst=(512, 128, 6)), unp(c=12), unp(dc16=odd)] == [EINVAL] * 8
    red = lambda ph=1, pw=1, dpo=p, idx=bp, c=16, part=p: lib.ammc_bn_bwd_reduce_bound_unpool_f32(p, *st, p, *st, dpo, *st, idx, ph, pw, p, p, p, p, 1, 1, 2, 2, c, part, s)
    assert [red(ph=2), red(pw=2), red(dpo=None), red(idx=None), red(c=12), red(c=1032), red(part=None)] == [EINVAL] * 7
    assert lib.ammc_bn_bwd_reduce_bound_f32(p, *st, None, *st, p, p, p, p, 1, 1, 2, 2, 16, p, s) == EINVAL
    assert lib.ammc_bn_bwd_reduce_bound_f32(p, *st, p, *st, p, p, p, p, 1, 1, 2, 2, 6, p, s) == EINVAL
    assert lib.ammc_bn_bwd_finalize_f32(p, 0, 16, 4, p, p, ip, s) == EINVAL
    assert lib.ammc_bn_bwd_finalize_f32(p, 1, 16, 4, p, p, None, s) == EINVAL
    assert lib.ammc_bn_bwd_finalize_f32(None, 1, 16, 4, p, p, ip, s) == EINVAL
    # the strided split and the channel sum with the maximum
    spl = lambda x=p, y=p, xst=st, yst=st, c=16, amax=ip, inv=p, n=8: lib.ammc_split_scaled_strided_f32(x, *xst, y, *yst, 1, 2, 2, c, amax, inv, n, s)
    assert [spl(c=12), spl(y=odd), spl(yst=bad_st), spl(x=_ptr(t, 1)), spl(xst=(512, 128, 6)), spl(amax=None), spl(inv=None), spl(n=0), spl(y=None)] == [EINVAL] * 9
    assert lib.ammc_chan_sum_absmax_f32(p, *st, 1, 2, 2, 16, p, None, s) == EINVAL
    assert lib.ammc_chan_sum_absmax_f32(p, *st, 1, 2, 2, 1028, p, ip, s) == EINVAL
    # partial rows in segments
    assert lib.ammc_reduce_partials_seg_f32(p, 4, 16, 0, 16, p, s) == EINVAL
    assert lib.ammc_reduce_partials_seg_f32(p, 4, 16, 2, 4, p, s) == EINVAL              # max_from & 7
    assert lib.ammc_reduce_partials_seg_f32(p, 4, 16, 2, 24, p, s) == EINVAL             # max_from > qc
    assert lib.ammc_reduce_partials_seg_f32(p, 70000, 16, 1, 16, p, s) == EUNSUP         # more than 65535 segments
    # dense encoders, layout, pool, LeakyReLU, halo
    assert lib.ammc_split_rows_f32(p, 12, p, s) == EINVAL
    assert lib.ammc_split_rows_f32(_ptr(t, 1), 8, p, s) == EINVAL
    assert lib.ammc_split_rows_guarded_f32(p, 8, None, ip, s) == EINVAL
    assert lib.ammc_absmax_bits_f32(p, 12, ip, s) == EINVAL
    assert lib.ammc_absmax_bits_f32(p, 8, None, s) == EINVAL
    assert lib.ammc_split_rows_scaled_f32(p, 8, p, None, p, 8, s) == EINVAL
    assert lib.ammc_split_rows_scaled_f32(p, 8, p, ip, p, 0, s) == EINVAL
    assert lib.ammc_nchw_to_s16_f32(p, 1, 12, 2, 2, p, *st, 8, s) == EINVAL              # cp < c
    assert lib.ammc_nchw_to_s16_f32(p, 1, 3, 2, 2, p, *st, 12, s) == EINVAL              # cp & 7
    assert lib.ammc_nchw_to_s16_f32(p, 1, 3, 2, 2, odd, *st, 8, s) == EINVAL
    assert lib.ammc_nchw_to_s16_f32(p, 1, 3, 2, 2, p, *bad_st, 8, s) == EINVAL
    assert lib.ammc_s16_to_nchw_f32(p, *st, 1, 12, 2, 2, p, s) == EINVAL
    assert lib.ammc_s16_to_nchw_f32(p, *st, 1, 8, 2, 2, None, s) == EINVAL
    assert lib.ammc_maxpool2x2_s16(p, *st, p, *st, 1, 1, 1, 12, s) == EINVAL
    assert lib.ammc_maxpool2x2_s16(p, *bad_st, p, *st, 1, 1, 1, 8, s) == EINVAL
    assert lib.ammc_maxpool2x2_s16_idx(p, *st, p, *st, None, 1, 1, 1, 8, s) == EINVAL
    assert lib.ammc_maxpool2x2_s16_idx(p, *st, p, *st, bp + 4, 1, 1, 1, 8, s) == EINVAL
    assert lib.ammc_maxpool2x2_bwd_idx_f32(bp, p, *st, None, 0, 0, 0, p, *st, 1, 1, 1, 4, 2, 8, s) == EINVAL     # in_h / 2 != h
    assert lib.ammc_maxpool2x2_bwd_idx_f32(bp, p, *st, None, 0, 0, 0, p, *st, 1, 1, 1, 2, 2, 12, s) == EINVAL
    assert lib.ammc_maxpool2x2_bwd_idx_f32(None, p, *st, None, 0, 0, 0, p, *st, 1, 1, 1, 2, 2, 8, s) == EINVAL
    assert lib.ammc_maxpool2x2_bwd_idx_f32(bp, p, *(512, 128, 6), None, 0, 0, 0, p, *st, 1, 1, 1, 2, 2, 8, s) == EINVAL
    assert lib.ammc_lrelu_s16(p, *st, 1, 2, 2, 12, 0.1, s) == EINVAL
    assert lib.ammc_lrelu_s16(odd, *st, 1, 2, 2, 8, 0.1, s) == EINVAL
    assert lib.ammc_lrelu_s16(p, *bad_st, 1, 2, 2, 8, 0.1, s) == EINVAL
    assert lib.ammc_zero_halo_f32(None, 1, 2, 2, 4, s) == EINVAL
    assert lib.ammc_zero_halo_f32(p, 1, 2, 2, 6, s) == EINVAL
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and int(i.abs().max()) == 0 and int(by.max()) == 0


# ---- AMMC_ROW_KERNELS=0: the one-item forms, in one child process ----------------------------------------------------

CHILD_K = "scale_shift_act or bn_bwd_apply_s16 or scale_factor_boundaries"


def test_one_item_forms_in_a_child_process(tmp_path):
    """the apply passes again in a child pytest process with AMMC_ROW_KERNELS=0 (the pattern of
    tests/test_gpu_wgrad_kernels.py): there every shape takes the one-item form (`_takes_rows` asserts it), passes its own
    parity, and its outputs' SHA-256 must be the ones this process got from the row forms.  A child that timed out, aborted
    or died of a signal ends the test: nothing more is started on the device."""
    if SWITCH in os.environ:
        pytest.skip("already inside a run with the switch set")
    for shape in C.SHAPES:                                             # the digests of cases this process has not run yet
        for kind in ("grid", "cont"):
            if not any(k.startswith("ssa ") and f"{shape} {kind}" in k for k in DIGESTS):
                test_scale_shift_act_f32_and_s16(shape, kind)
            for relu in (0, 1):
                if f"apply plain {shape} {kind} relu={relu}" not in DIGESTS:
                    test_bn_bwd_apply_s16_and_its_unpool_form(shape, kind, relu)
    ref = {k: v for k, v in DIGESTS.items() if not k.startswith("apply unpool")}        # (the unpool form has a row form only)
    assert len(ref) == len(C.SHAPES) * 2 * (4 + 2)
    torch.cuda.synchronize()                                           # (a fault met earlier surfaces here: no child then)
    path = tmp_path / "row_form_digests.json"
    path.write_text(json.dumps(ref))
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-rf", "-p", "no:cacheprovider", "-k", CHILD_K],
                       env=dict(os.environ, **{SWITCH: "0", DIGEST_ENV: str(path)}), capture_output=True, text=True, timeout=300)
    out = r.stdout.splitlines()
    print("\n".join([ln for ln in out if ln.startswith("RATIO ") or ln.startswith("FAILED ")]))
    print(f"child {SWITCH}=0: {time.time() - t0:.1f} s, return code {r.returncode}")
    assert r.returncode in (0, 1), (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])      # 124, 134, 137, 139, < 0: stop here
    want = len(C.SHAPES) * 2 + len(C.POOL_SHAPES) * 2 + len(C.SHAPES) * 4 + len(C.SCALE_CASES) * 2
    m = re.search(r"(\d+) passed", out[-1]) if out else None
    assert r.returncode == 0 and m and int(m.group(1)) == want, (want, r.stdout[-3000:] + r.stderr[-1000:])
