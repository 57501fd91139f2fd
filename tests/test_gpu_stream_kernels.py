"""The streaming kernels of the training path, each alone through ctypes against the fp64 references of
tests/stream_refs.py (csrc/train_kernels.hip, flownet.hip, layout_pool.hip; shapes and inputs: tests/stream_cases.py).

Two kinds of input.  "grid": every fp32 operation of the kernel is exact (tests/test_stream_refs_host.py checks that the
reference results fit fp32), so the result must EQUAL the reference rounded to fp32 - a dropped, doubled or misplaced
element moves a sum by a grid unit.  (+0 and -0 compare equal where a value is computed: the sign of an exact zero
depends on whether the compiler contracts a multiply-add.)  "cont": hashed normal values, per element against a
forward error bound derived from the kernel, u = 2^-24, times 2 for slack; the worst error / bound ratio per kernel is
printed (`RATIO ...`, and appended to the file AMMC_STREAM_RATIOS names) - DESIGN.md 5.10 has the measured table.

Every output is a view inside a larger buffer prefilled with a sentinel bit pattern (a one-pixel halo, more channels
than c where the entry point takes strides, a tail row on dense outputs): what the kernel does not own must still hold
it.  Inputs sit in buffers of other widths than the outputs, one of them a channel slice."""
import os

import pytest
import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd.engine import Act, _ptr

import stream_cases as K
import stream_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENT = 0x7FA5A5A5                     # a NaN pattern no kernel produces
EINVAL, EUNSUP = -1, -2
RATIOS = {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _sent(*shape, dtype=torch.float32):
    t = torch.empty(*shape, device=DEV, dtype=torch.int32)
    t.fill_(SENT)
    return t.view(dtype) if dtype != torch.int32 else t


def _in_act(t, ctot=None, c_off=0):
    """the NHWC tensor t as a channel slice [c_off, c_off + c) of a ctot-wide buffer with a one-pixel halo; everything
    else in the buffer is a large finite value (a kernel that reads off its view shows)"""
    b, h, w, c = t.shape
    buf = torch.full((b, h + 2, w + 2, ctot or c), 1.0e4, device=DEV)
    a = Act(buf, b, h, w, c, c_off, 1)
    a.interior().copy_(t.to(DEV))
    return a


def _out_act(b, h, w, c, ctot=None, c_off=0):
    return Act(_sent(b, h + 2, w + 2, ctot or c), b, h, w, c, c_off, 1)


def _untouched(a: Act, c=None):
    """everything of the buffer outside the interior's channels [c_off, c_off + c) still holds the sentinel"""
    own = torch.zeros(a.buf.shape, dtype=torch.bool, device=DEV)
    own[:, 1:1 + a.H, 1:1 + a.W, a.c_off:a.c_off + (c or a.c)] = True
    bits = a.buf.view(torch.int32)
    assert bool((bits[~own] == SENT).all()), "the kernel wrote outside its view"
    assert not bool((bits[own] == SENT).any()), "the kernel left an element of its view unwritten"


def _first(bad, got, want):
    idx = torch.nonzero(bad)[:5].tolist()
    return [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]


def _exact(got, want64, what):
    """bit equality with the reference rounded to fp32 (+0 == -0)"""
    got, want = got.detach().float().cpu(), R.d(want64).float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} differ; (index, got, want): {_first(bad, got, want)}"


def _bits(got, want, what):
    """the same bits, signs of zero included (copies, selections, one correctly-rounded operation)"""
    got, want = got.detach().float().cpu().contiguous(), want.detach().float().cpu().contiguous()
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} differ; (index, got, want): {_first(bad, got, want)}"


def _bounded(kernel, got, want64, bound64, what):
    """|got - want| <= bound per element; records the worst ratio of the kernel"""
    got, want, bound = got.detach().double().cpu(), R.d(want64), R.d(bound64).expand_as(R.d(want64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), worst)
    line = f"RATIO {kernel} {what} {worst:.4g}"
    print(line)
    if os.environ.get("AMMC_STREAM_RATIOS"):
        with open(os.environ["AMMC_STREAM_RATIOS"], "a") as fp:
            fp.write(line + "\n")
    bad = ratio > 1.0
    assert not bool(bad.any()), f"{what}: worst error / bound {worst:.3g}; (index, got, want): {_first(bad, got, want)}"


def _ordered(t):
    """fp32 bit patterns as integers that order like the values: a difference is a distance in ulps"""
    i = t.detach().float().cpu().contiguous().view(torch.int32).long()
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


# ---- per-channel reductions (chan_reduce_kernel modes 0, 1, 2) and the BatchNorm finalizer -----------------------------

def _chain(lib, m, c, u):
    """additions on the longest chain of one partial row: a thread adds its U streams' values trip after trip
    (ceil(M / (gridDim U PY)) trips of U), then thread row 0 adds the other PY - 1 rows of the workgroup"""
    py = 256 // (c // 4)
    trips = -(-m // (lib.ammc_chan_reduce_blocks(m) * u * py))
    return trips * u + py - 1


def _reduce(lib, part, nb, qc):
    """`ammc_reduce_partials_f32`: the partial rows added in double, one rounding to fp32"""
    out = _sent(qc + 4)
    _lib.check(lib.ammc_reduce_partials_f32(_ptr(part), nb, qc, 1.0, _ptr(out), _s()), "reduce_partials")
    assert bool((out.view(torch.int32)[qc:] == SENT).all())
    return out[:qc]


def _partial(nb, q, c):
    return _sent(nb + 1, q, c)


def _partial_ok(part, nb):
    bits = part.view(torch.int32)
    assert bool((bits[nb:] == SENT).all()) and not bool((bits[:nb] == SENT).any())


@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", K.CHAN_SHAPES)
def test_bn_stats_chan_sum_and_finalize(shape, kind):
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    x = K.values(kind, f"bns-{kind}-{shape}", shape)
    if kind == "cont":
        x = x + 0.5
    X = _in_act(x, c + 8, 4)                                           # a channel slice of a wider buffer
    nb = lib.ammc_chan_reduce_blocks(m)
    part, part1 = _partial(nb, 2, c), _partial(nb, 1, c)
    _lib.check(lib.ammc_bn_stats_f32(X.pix0(), *X.strides, b, h, w, c, _ptr(part), _s()), "bn_stats")
    _lib.check(lib.ammc_chan_sum_f32(X.pix0(), *X.strides, b, h, w, c, _ptr(part1), _s()), "chan_sum")
    _partial_ok(part, nb)
    _partial_ok(part1, nb)
    tot, tot1 = _reduce(lib, part, nb, 2 * c), _reduce(lib, part1, nb, c)
    s, ss = R.chan_sums(x)
    # n = _chain additions per partial row (U = 8); c = 1: the one rounding of the double total (the rows are added in
    # double); the squares add one rounding per term
    n = _chain(lib, m, c, 8)
    xa = x.double().abs()
    b_s, b_ss = 2 * (n + 1) * U * xa.sum((0, 1, 2)), 2 * (n + 2) * U * (xa * xa).sum((0, 1, 2))
    if kind == "grid":
        _exact(tot[:c], s, "bn_stats sum")
        _exact(tot[c:], ss, "bn_stats sum of squares")
        _exact(tot1, s, "chan_sum")
    else:
        _bounded("bn_stats_f32", tot[:c], s, b_s, f"sum {shape}")
        _bounded("bn_stats_f32", tot[c:], ss, b_ss, f"sumsq {shape}")
        _bounded("chan_sum_f32", tot1, s, b_s, f"sum {shape}")
    _bits(part[:nb, 0], part1[:nb, 0], "chan_sum rows == bn_stats' first rows")         # the same walk, the same order

    # the finalizer over the partial rows (double arithmetic, each output rounded once)
    gamma, beta = K.values(kind, f"bnf-g-{shape}", (c,)), K.values(kind, f"bnf-b-{shape}", (c,))
    rm, rv = K.values(kind, f"bnf-m-{shape}", (c,)), K.values(kind, f"bnf-v-{shape}", (c,)).abs()
    mom, eps = (0.5, 2.0 ** -10) if kind == "grid" else (0.1, 1e-5)
    out = _sent(6, c + 4)
    out[4, :c], out[5, :c] = rm.to(DEV), rv.to(DEV)
    g_d, b_d = _dev(gamma, beta)
    _lib.check(lib.ammc_bn_finalize_f32(_ptr(part), nb, c, float(m), _ptr(g_d), _ptr(b_d), eps, mom, _ptr(out[4]), _ptr(out[5]),
                                        _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _s()), "bn_finalize")
    assert bool((out.view(torch.int32)[:, c:] == SENT).all())
    eps32, mom32 = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(mom, dtype=torch.float32))
    fin = R.bn_finalize(s, ss, m, gamma, beta, eps32, mom32, rm, rv)
    names = ("mean", "invstd", "scale", "shift", "running_mean", "running_var")
    if kind == "grid" and K.is_pow2(m):
        # exact sums, an exact 1/M: mean, var are exact in double and invstd = one sqrt and one division, correctly rounded
        for i in (0, 1, 2, 4):
            _exact(out[i, :c], fin[names[i]].float() if i != 2 else gamma.double() * fin["invstd"].float().double(), names[i])
    # propagated bounds: d_s, d_ss = the partial rows' errors (no final rounding: the finalizer reads the rows in double)
    if kind == "grid":
        d_s = d_ss = torch.zeros(c, dtype=torch.float64)
    else:
        d_s, d_ss = n * U * xa.sum((0, 1, 2)), (n + 1) * U * (xa * xa).sum((0, 1, 2))
    mean, var, invstd, scale = fin["mean"], fin["var"], fin["invstd"], fin["scale"]
    d_mean = d_s / m + U * mean.abs()
    d_var = d_ss / m + 2 * mean.abs() * d_s / m + 4 * 2.0 ** -53 * (ss / m)           # (double roundings of ss / M - mean^2)
    d_is = 0.5 * invstd / (var + eps32) * d_var + U * invstd
    d_sc = gamma.double().abs() * d_is + U * scale.abs()
    d_sh = d_mean * scale.abs() + mean.abs() * d_sc + 2 * U * (beta.double().abs() + (mean * scale).abs())
    unb = var * m / (m - 1.0) if m > 1 else var
    d_rm = mom32 * d_mean + 3 * U * (((1 - mom32) * rm.double()).abs() + (mom32 * mean).abs())
    d_rv = mom32 * (d_var * (m / (m - 1.0) if m > 1 else 1.0) + U * unb) + 3 * U * (((1 - mom32) * rv.double()).abs() + mom32 * unb)
    for i, bd in enumerate((d_mean, d_is, d_sc, d_sh, d_rm, d_rv)):
        _bounded("bn_finalize_f32", out[i, :c], fin[names[i]], 2 * bd, f"{names[i]} {kind} {shape}")


def test_bn_finalize_variance_when_mean_is_100_std():
    """var = E[x^2] - mean^2 from fp32 partial sums with |mean| = 100 std: what the one-pass formula delivers.  Bound (the
    formula's conditioning): the relative error of var is u (n + c) (mean^2 + var) / var, n = the partial rows' chain,
    c = 2 (a square's rounding, the row's own last addition); var is read back from invstd (one more rounding: 2 u var)."""
    lib = _lib.load()
    shape = b, h, w, c = 2, 16, 24, 64
    m = b * h * w
    x = S.hashed_normal("bn100", shape) + 100.0
    X = _in_act(x, c + 8, 4)
    nb = lib.ammc_chan_reduce_blocks(m)
    part = _partial(nb, 2, c)
    _lib.check(lib.ammc_bn_stats_f32(X.pix0(), *X.strides, b, h, w, c, _ptr(part), _s()), "bn_stats")
    out = _sent(6, c)
    out[4:].zero_()
    one, zero = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib.ammc_bn_finalize_f32(_ptr(part), nb, c, float(m), _ptr(one), _ptr(zero), 1e-5, 0.1, _ptr(out[4]), _ptr(out[5]),
                                        _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _s()), "bn_finalize")
    eps32 = float(torch.tensor(1e-5, dtype=torch.float32))
    s, ss = R.chan_sums(x)
    fin = R.bn_finalize(s, ss, m, one, zero, eps32, 0.1, zero, zero)
    var_got = 1.0 / out[1].double().cpu() ** 2 - eps32
    n = _chain(lib, m, c, 8)
    bound = 2 * (U * (n + 2) * (fin["mean"] ** 2 + fin["var"]) + 3 * U * (fin["var"] + eps32))
    _bounded("bn_finalize_f32(mean/std=100)", var_got, fin["var"], bound, "var")
    rel = float(((var_got - fin["var"]).abs() / fin["var"]).max())
    print(f"RATIO bn_finalize_f32(mean/std=100) worst relative error of var {rel:.3g}")
    assert 0.5 < float(fin["var"].min()) and 99.0 < float(fin["mean"].min())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("shape", K.CHAN_SHAPES)
def test_bn_bwd_reduce(shape, kind, relu):
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    x, dy, mean, invstd, scale, shift = K.bn_bwd_case(kind, shape, relu)
    X, D = _in_act(x, c + 8, 4), _in_act(dy, c, 0)                     # different strides: a slice and a dense tensor
    p_d = _dev(mean, invstd, scale, shift)
    nb = lib.ammc_chan_reduce_blocks(m)
    part = _partial(nb, 2, c)
    _lib.check(lib.ammc_bn_bwd_reduce_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, *[_ptr(t) for t in p_d], relu, b, h, w, c,
                                          _ptr(part), _s()), "bn_bwd_reduce")
    _partial_ok(part, nb)
    tot = _reduce(lib, part, nb, 2 * c)
    sg, sgx = R.bn_bwd_sums(x, dy, mean, invstd, scale, shift, relu)
    if kind == "grid":
        _exact(tot[:c], sg, f"sum g relu={relu}")
        _exact(tot[c:], sgx, f"sum g xhat relu={relu}")
        return
    # n = the chain with U = 4; c = 1 for sum g (the total's rounding), c = 4 for sum g xhat (xhat = (x - mean) invstd: two
    # roundings, the product one, the total one).  An element whose pre = x scale + shift is within its own rounding
    # error of zero (2 u (|x scale| + |shift|)) may be masked either way: its whole term is added to the bound.
    n = _chain(lib, m, c, 4)
    xd, gd = x.double(), dy.double()
    xh = (xd - mean.double()) * invstd.double()
    g = R.bn_masked_grad(x, dy, scale, shift, relu)
    amb = torch.zeros_like(xd)
    if relu:
        pre = xd * scale.double() + shift.double()
        amb = (pre.abs() <= 2 * U * ((xd * scale.double()).abs() + shift.double().abs())).double()
    b_g = 2 * ((n + 1) * U * g.abs().sum((0, 1, 2)) + (amb * gd.abs()).sum((0, 1, 2)))
    b_gx = 2 * ((n + 4) * U * (g * xh).abs().sum((0, 1, 2)) + (amb * (gd * xh).abs()).sum((0, 1, 2)))
    _bounded("bn_bwd_reduce_f32", tot[:c], sg, b_g, f"sum g {shape} relu={relu}")
    _bounded("bn_bwd_reduce_f32", tot[c:], sgx, b_gx, f"sum g xhat {shape} relu={relu}")


APPLY_CASES = [(shape, kind) for shape in K.CHAN_SHAPES for kind in ("grid", "cont")
               if kind == "cont" or K.is_pow2(shape[0] * shape[1] * shape[2])]


@pytest.mark.parametrize("amax", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape,kind", APPLY_CASES)
def test_bn_bwd_apply(shape, kind, relu, amax):
    """grid: the shapes with a power-of-two pixel count (1/M exact); cont: every shape.  amax = 1: the 256 slots end with the
    bit pattern of max |dc|; amax = 0: the tail workgroup's spare threads return early."""
    lib = _lib.load()
    b, h, w, c = shape
    m = b * h * w
    x, dy, mean, invstd, scale, shift = K.bn_bwd_case(kind, shape, relu)
    sg, sgx = K.bn_apply_sums(kind, shape)
    X, D = _in_act(x, c + 8, 4), _in_act(dy, c, 0)
    O = _out_act(b, h, w, c, c + 4, 0)
    p_d = _dev(mean, invstd, scale, shift, torch.cat([sg, sgx]))
    slots = torch.zeros(256, dtype=torch.int32, device=DEV)
    _lib.check(lib.ammc_bn_bwd_apply_f32(X.pix0(), *X.strides, D.pix0(), *D.strides, *[_ptr(t) for t in p_d], relu, O.pix0(),
                                         *O.strides, b, h, w, c, slots.data_ptr() if amax else None, _s()), "bn_bwd_apply")
    _untouched(O)
    got = O.interior()
    want = R.bn_bwd_apply(x, dy, mean, invstd, scale, shift, sg, sgx, relu)
    if amax:
        assert int(slots.max()) == int(got.abs().max().reshape(1).view(torch.int32)), "amax slots != bits of max |dc|"
    else:
        assert int(slots.abs().max()) == 0
    if kind == "grid":
        _exact(got, want, f"dc relu={relu}")
        return
    # dc = scale (g - sg ic - xhat sgx ic), ic = fl(1 / M): roundings on the longest path: ic 1, xhat 2, xhat sgx 1, (.) ic 1,
    # two subtractions, the product with scale: k = 8 over the sum of the intermediates' magnitudes; an element whose
    # mask is ambiguous (see test_bn_bwd_reduce) may differ by its whole gradient
    xd = x.double()
    xh = (xd - mean.double()) * invstd.double()
    g = R.bn_masked_grad(x, dy, scale, shift, relu)
    mag = g.abs() + (sg.double() / m).abs() + (xh * sgx.double() / m).abs()
    bound = 8 * U * scale.double().abs() * mag
    if relu:
        pre = xd * scale.double() + shift.double()
        amb = (pre.abs() <= 2 * U * ((xd * scale.double()).abs() + shift.double().abs())).double()
        bound = bound + amb * (scale.double() * dy.double()).abs()
    _bounded("bn_bwd_apply_f32", got, want, 2 * bound, f"dc {shape} relu={relu}")


# ---- max-pool, tanh, LeakyReLU ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_add", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("c", [4, 128])
@pytest.mark.parametrize("fh,fw", K.POOL_BWD_SIZES)
def test_maxpool2x2_bwd(fh, fw, c, kind, with_add):
    """a selection and at most one addition of fp32 values: bit-exact for both kinds of input"""
    lib = _lib.load()
    b, hh, ww = 2, fh // 2, fw // 2
    x, dp, add = K.pool_bwd_case(kind, b, fh, fw, c)
    X, P, A = _in_act(x, c + 4, 4), _in_act(dp, c, 0), _in_act(add, c + 8, 8)
    O = _out_act(b, fh, fw, c, c + 12, 4)
    a_args = (A.pix0(), *A.strides) if with_add else (None, 0, 0, 0)
    _lib.check(lib.ammc_maxpool2x2_bwd_f32(X.pix0(), *X.strides, P.pix0(), *P.strides, *a_args, O.pix0(), *O.strides,
                                           b, hh, ww, fh, fw, c, _s()), "maxpool_bwd")
    _untouched(O)
    want = R.maxpool2x2_bwd(x, dp, add if with_add else None)
    _exact(O.interior(), want, f"dx {fh}x{fw} c={c} add={with_add}")
    if fh & 1:
        _exact(O.interior()[:, -1], add[:, -1].double() if with_add else torch.zeros(b, fw, c), "the odd last row")
    if fw & 1:
        _exact(O.interior()[:, :, -1], add[:, :, -1].double() if with_add else torch.zeros(b, fh, c), "the odd last column")


@pytest.mark.parametrize("fh,fw", [(1, 2), (2, 1)])
def test_maxpool2x2_bwd_refuses_a_size_without_a_window(fh, fw):
    """full sizes 1x2 and 2x1 hold no 2x2 window (MaxPool2d floors to an empty tensor): the entry point refuses h or w = 0
    before any launch and the output stays as it was"""
    lib = _lib.load()
    c = 4
    x = _in_act(R.grid("mp0", (1, fh, fw, c)))
    O = _out_act(1, fh, fw, c)
    assert lib.ammc_maxpool2x2_bwd_f32(x.pix0(), *x.strides, x.pix0(), *x.strides, None, 0, 0, 0, O.pix0(), *O.strides,
                                       1, fh // 2, fw // 2, fh, fw, c, _s()) == EINVAL
    torch.cuda.synchronize()
    assert bool((O.buf.view(torch.int32) == SENT).all())


@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("c,cp", [(3, 4), (3, 32), (8, 8)])
def test_tanh_bwd_nhwc(c, cp, kind):
    lib = _lib.load()
    b, h, w = 2, 5, 7
    dout = K.values(kind, f"tb-d-{kind}-{c}", (b, c, h, w))
    out = K.values(kind, f"tb-o-{kind}-{c}", (b, c, h, w)) if kind == "grid" else torch.tanh(S.hashed_normal(f"tb-o-{c}", (b, c, h, w)))
    d_d, o_d = _dev(dout, out)
    Y = _out_act(b, h, w, cp, cp + 4, 0)                               # strided: the pixel stride is wider than cp
    _lib.check(lib.ammc_tanh_bwd_nhwc_f32(_ptr(d_d), _ptr(o_d), b, c, h, w, Y.pix0(), *Y.strides, cp, _s()), "tanh_bwd")
    _untouched(Y)                                                      # owns [0, cp): zeros from c up
    want = R.tanh_bwd_nhwc(dout, out, cp)
    assert cp == c or float(Y.interior()[..., c:].abs().max()) == 0.0
    if kind == "grid":
        _exact(Y.interior(), want, "tanh_bwd")
    else:
        # dout (1 - out^2): out^2, the subtraction, the product: k = 3 over |dout| (1 + out^2)
        bound = torch.zeros_like(want)
        bound[..., :c] = (3 * U * dout.double().abs() * (1.0 + out.double() ** 2)).permute(0, 2, 3, 1)
        _bounded("tanh_bwd_nhwc_f32", Y.interior(), want, 2 * bound, f"c={c} cp={cp}")


def _lrelu_values(kind, tag, shape):
    t = K.values(kind, tag, shape, 3.0)
    t[0, 1, 1, 0], t[0, 1, 1, 1], t[0, 1, 2, 0] = 0.0, -0.0, -0.0
    return t


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("c", [4, 36, 64])
def test_lrelu_forward_in_place_and_backward(c, kind, slope):
    """one correctly-rounded multiplication (or none): the same bits as the fp64 reference rounded to fp32, whatever the input -
    zeros and negative zeros included.  In place on the first c channels of a wider buffer: the rest keeps its bits."""
    lib = _lib.load()
    b, h, w, ctot = 2, 5, 7, c + 8
    s32 = float(torch.tensor(slope, dtype=torch.float32))
    full = _lrelu_values(kind, f"lr-{kind}-{c}", (b, h + 2, w + 2, ctot)).to(DEV)
    Y = Act(full.clone(), b, h, w, c, 0, 1)
    _lib.check(lib.ammc_lrelu_f32(Y.pix0(), *Y.strides, b, h, w, c, slope, _s()), "lrelu")
    want = full.clone()
    want[:, 1:-1, 1:-1, :c] = R.lrelu(full[:, 1:-1, 1:-1, :c], s32).float().to(DEV)
    _bits(Y.buf, want, f"lrelu c={c} slope={slope}")
    # backward: g *= (y > 0 ? 1 : slope), y another buffer with other strides
    yv = _lrelu_values(kind, f"lrb-y-{kind}-{c}", (b, h, w, c))
    Yin = _in_act(yv, c + 4, 4)
    gfull = _lrelu_values(kind, f"lrb-g-{kind}-{c}", (b, h + 2, w + 2, ctot)).to(DEV)
    G = Act(gfull.clone(), b, h, w, c, 0, 1)
    _lib.check(lib.ammc_lrelu_bwd_f32(Yin.pix0(), *Yin.strides, G.pix0(), *G.strides, b, h, w, c, slope, _s()), "lrelu_bwd")
    wantg = gfull.clone()
    wantg[:, 1:-1, 1:-1, :c] = R.lrelu_bwd(yv, gfull[:, 1:-1, 1:-1, :c], s32).float().to(DEV)
    _bits(G.buf, wantg, f"lrelu_bwd c={c} slope={slope}")


# ---- memory module ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("has_dq", [0, 1])
@pytest.mark.parametrize("has_ddiff", [0, 1])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("n,dim,k", K.COMMIT_CASES)
def test_commit_bwd(n, dim, k, kind, has_ddiff, has_dq):
    lib = _lib.load()
    z, e, idx, ddiff, dq = K.commit_case(kind, n, dim, k)
    z_d, e_d, i_d, dd_d, dq_d = _dev(z, e, idx, ddiff, dq)
    out = _sent(n + 1, dim)
    _lib.check(lib.ammc_commit_bwd_f32(_ptr(z_d), _ptr(e_d), i_d.data_ptr(), k, _ptr(dd_d) if has_ddiff else None,
                                       _ptr(dq_d) if has_dq else None, _ptr(out), n, dim, _s()), "commit_bwd")
    assert bool((out.view(torch.int32)[n:] == SENT).all())
    want = R.commit_bwd(z, e, idx, ddiff if has_ddiff else None, dq if has_dq else None)
    if not has_ddiff or (kind == "grid" and K.is_pow2(n * dim)):
        _exact(out[:n], want, f"dz ddiff={has_ddiff} dq={has_dq}")       # 0 (z - e) + dq, or an exact 2 / (N D)
        return
    # g = ddiff coef, coef = fl(2 / (fl(N) fl(D))): three roundings; z - e one, the product one, + dq one: k = 6
    t = (float(ddiff[0]) * 2.0 / (n * dim)) * (z.double() - e.double()[idx[:, 0].long()])
    bound = 6 * U * (t.abs() + (dq.double().abs() if has_dq else 0.0))
    _bounded("commit_bwd_f32", out[:n], want, 2 * bound, f"({n},{dim},{k}) dq={has_dq}")


def _ema_bounds(x, idx, m, cs0, ea0, counts, sums, decay, omd, eps, exact_sums):
    """cluster_size' = decay cs + omd count: two products and a sum, k = 3.
    sums: a wave adds its hits one by one in row order (at most min(count, chunk) additions), then the 16 wave sums are added
    in wave order: n = min(count, chunk) + 16 over sum |x| of the slot's rows.
    embed_avg' = decay ea + omd sum: k = 3, plus omd times the sum's error.
    embed = embed_avg' / smoothed, smoothed = (cs' + eps) / (n + M eps) n with n = the sum of cs' (256 threads stride over the
    slots, then an 8-level tree: ceil(M / 256) + 8 additions of positive terms, and n enters twice): relative error
    of smoothed <= rel(cs') + (6 + 2 (ceil(M / 256) + 8)) u, one more rounding for the division."""
    n_rows, dim = x.shape
    chunk = K.ema_chunk(n_rows)
    i0 = idx[:, 0].long()
    absum = torch.zeros(dim, m, dtype=torch.float64).index_add_(1, i0, x.double().abs().t().contiguous())
    nadd = counts.clamp(max=chunk) + 16
    d_sum = torch.zeros_like(absum) if exact_sums else nadd * U * absum
    cs, ea, embed = R.ema_update(cs0, ea0, counts, sums, decay, omd, eps)
    d_cs = 3 * U * ((decay * cs0.double()).abs() + omd * counts)
    d_ea = 3 * U * ((decay * ea0.double()).abs() + (omd * sums).abs()) + omd * d_sum
    ntree = -(-m // 256) + 8
    smoothed = (cs + eps) / (cs.sum() + m * eps) * cs.sum()
    rel_sm = d_cs / (cs + eps) + (6 + 2 * ntree) * U
    d_embed = d_ea / smoothed + (rel_sm + U) * embed.abs()
    return (cs, ea, embed), (d_cs, d_ea, d_embed), d_sum


@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("n,dim,m,k,pattern", K.EMA_CASES)
def test_codebook_ema_fused_and_raw(n, dim, m, k, pattern, kind):
    lib = _lib.load()
    x, idx, cs0, ea0, decay = K.ema_case(kind, n, dim, m, k, pattern)
    d32 = float(torch.tensor(decay, dtype=torch.float32))
    o32 = float(torch.tensor(1 - decay, dtype=torch.float32))
    eps32 = float(torch.tensor(1e-5, dtype=torch.float32))
    x_d, i_d = _dev(x, idx)
    counts, sums = R.ema_counts_sums(x, idx, m)
    (cs, ea, embed), (d_cs, d_ea, d_embed), d_sum = _ema_bounds(x, idx, m, cs0, ea0, counts, sums, d32, o32, eps32, kind == "grid")
    what = f"({n},{dim},{m},{k},{pattern})"

    def fused():
        st = _sent(1 + 2 * dim + 1, m)                                      # rows: cluster_size, embed_avg [D], embed [D], a tail
        st[0], st[1:1 + dim] = cs0.to(DEV), ea0.to(DEV)
        _lib.check(lib.ammc_codebook_ema_f32(_ptr(x_d), i_d.data_ptr(), k, n, dim, m, decay, 1 - decay, 1e-5, _ptr(st[0]), _ptr(st[1]),
                                             _ptr(st[1 + dim]), _s()), "codebook_ema")
        assert bool((st.view(torch.int32)[-1] == SENT).all())
        return st[:-1].clone()

    def raw():
        rw = _sent(1 + dim + 1, m)
        _lib.check(lib.ammc_codebook_count_f32(_ptr(x_d), i_d.data_ptr(), k, n, dim, m, _ptr(rw[0]), _ptr(rw[1]), _s()), "codebook_count")
        assert bool((rw.view(torch.int32)[-1] == SENT).all()) and not bool((rw.view(torch.int32)[:-1] == SENT).any())
        return rw[:-1].clone()

    f1, f2, r1, r2 = fused(), fused(), raw(), raw()
    assert torch.equal(f1.view(torch.int32), f2.view(torch.int32)), "two fused launches differ"
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)), "two count launches differ"
    _exact(r1[0], counts, "counts")                                          # integers
    if kind == "grid":
        _exact(r1[1:], sums, "raw sums")
        _exact(f1[0], cs, "cluster_size")
        _exact(f1[1:1 + dim], ea, "embed_avg")
    else:
        _bounded("codebook_count_f32", r1[1:], sums, 2 * d_sum, f"sums {what}")
        _bounded("codebook_ema_f32", f1[0], cs, 2 * d_cs, f"cluster_size {what}")
        _bounded("codebook_ema_f32", f1[1:1 + dim], ea, 2 * d_ea, f"embed_avg {what}")
    _bounded("codebook_ema_f32", f1[1 + dim:], embed, 2 * d_embed, f"embed {kind} {what}")
    # count, then apply (the form data-parallel training uses, the all-reduce between the two) = the fused kernel
    st = _sent(1 + 2 * dim + 1, m)
    st[0], st[1:1 + dim] = cs0.to(DEV), ea0.to(DEV)
    _lib.check(lib.ammc_codebook_ema_apply_f32(_ptr(r1[0]), _ptr(r1[1]), dim, m, decay, 1 - decay, 1e-5, _ptr(st[0]), _ptr(st[1]),
                                               _ptr(st[1 + dim]), _s()), "codebook_ema_apply")
    assert bool((st.view(torch.int32)[-1] == SENT).all())
    ulps = int((_ordered(st[:-1]) - _ordered(f1)).abs().max())
    print(f"RATIO codebook_ema_apply_f32 vs fused {what} {kind}: {ulps} ulp")
    if os.environ.get("AMMC_STREAM_RATIOS"):
        with open(os.environ["AMMC_STREAM_RATIOS"], "a") as fp:
            fp.write(f"ULPS count+apply vs fused {what} {kind} {ulps}\n")
    assert ulps <= 2, ulps
    _bounded("codebook_ema_apply_f32", st[1 + dim:-1], embed, 2 * d_embed, f"embed {kind} {what}")


# ---- FlowNet2-SD element-wise ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("b,h,w", K.PREP_SHAPES)
def test_flownet_prep(b, h, w, kind):
    """32 slices per (sample, colour) plane: (1,3,3) leaves slices empty (2HW = 18), (3,17,23) has a ragged last slice"""
    lib = _lib.load()
    x = K.prep_case(kind, b, h, w)
    rgb_max = 256.0 if kind == "grid" else 255.0
    x_d, = _dev(x)
    Y = _out_act(b, h, w, 6, 8, 0)                                     # the kernel writes channels 0..5 of the 8-wide activation
    scratch = torch.full((lib.ammc_flownet_prep_scratch_doubles(b) + 4,), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(lib.ammc_flownet_prep_f32(_ptr(x_d), b, h, w, Y.pix0(), *Y.strides, rgb_max, scratch.data_ptr(), _s()), "flownet_prep")
    _untouched(Y)
    assert bool((scratch[-4:] == -7.0).all())
    want = R.flownet_prep(x, rgb_max)
    if kind == "grid":
        _exact(Y.interior(), want, "flownet_prep")
        return
    # the mean: double sums, one rounding to fp32 (u |mean|); x - mean one rounding, the division one: k = 3 over
    # (|mean| + 2 |x - mean|) / rgb_max
    xd = x.double()
    mean = xd.reshape(b, 3, -1).mean(-1).view(b, 3, 1, 1, 1)
    bound = (U * (mean.abs() + 2 * (xd - mean).abs()) / rgb_max).permute(0, 3, 4, 2, 1).reshape(b, h, w, 6)
    _bounded("flownet_prep_f32", Y.interior(), want, 2 * bound, f"({b},{h},{w})")


@pytest.mark.parametrize("premul", [1.0, 5.0, 20.0])
@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("h,w", K.UP_SHAPES)
def test_upsample4_bilinear(h, w, kind, premul):
    """premul = div_flow (20 in flownet.py; 1 and 5: a power of two and an odd one).  The weights are multiples of 1/8, so the
    grid case is exact for all three.  The input is channels [0, 2) of an 8-wide NHWC buffer."""
    lib = _lib.load()
    b = 2
    x = K.values(kind, f"up-{kind}-{h}-{w}", (b, h, w, 2))
    X = _in_act(x, 8, 0)
    n_out = b * 2 * 16 * h * w
    out = _sent(n_out + 64)
    _lib.check(lib.ammc_upsample4_bilinear_f32(X.pix0(), *X.strides, b, h, w, 2, premul, _ptr(out), _s()), "upsample4")
    assert bool((out.view(torch.int32)[n_out:] == SENT).all())
    got = out[:n_out].view(b, 2, 4 * h, 4 * w)
    want = R.upsample4(x, premul)
    if kind == "grid":
        _exact(got, want, f"upsample4 {h}x{w} premul={premul}")
    else:
        # v premul, two weighted products and their sum per row, the two rows weighted and added: k = 6 roundings on the
        # longest path over the weighted sum of |v| premul (the weights themselves are exact)
        bound = 6 * U * R.upsample4(x.abs(), premul)
        _bounded("upsample4_bilinear_f32", got, want, 2 * bound, f"{h}x{w} premul={premul}")


# ---- layout ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,cp", [(3, 4), (3, 8), (12, 12)])
def test_nchw_to_nhwc_and_back(c, cp):
    lib = _lib.load()
    b, h, w = 2, 5, 7
    x = S.hashed_normal(f"lay-{c}", (b, c, h, w))
    x_d, = _dev(x)
    Y = _out_act(b, h, w, cp, cp + 4, 4)
    _lib.check(lib.ammc_nchw_to_nhwc_f32(_ptr(x_d), b, c, h, w, Y.pix0(), *Y.strides, cp, _s()), "nchw_to_nhwc")
    _untouched(Y)
    _bits(Y.interior(), R.nchw_to_nhwc(x, cp).float(), "nchw_to_nhwc")          # the padded channels are zero
    back = _sent(b * c * h * w + 32)
    _lib.check(lib.ammc_nhwc_to_nchw_f32(Y.pix0(), *Y.strides, b, c, h, w, _ptr(back), _s()), "nhwc_to_nchw")   # from a strided slice
    assert bool((back.view(torch.int32)[b * c * h * w:] == SENT).all())
    _bits(back[:b * c * h * w].view(b, c, h, w), x, "nhwc_to_nchw")


@pytest.mark.parametrize("fh,fw,c", [(4, 6, 4), (5, 7, 12), (9, 2, 128)])
def test_maxpool2x2_forward(fh, fw, c):
    lib = _lib.load()
    b, h, w = 2, fh // 2, fw // 2
    x = S.hashed_normal(f"mpf-{fh}-{fw}", (b, fh, fw, c))
    X = _in_act(x, c + 4, 4)
    Y = _out_act(b, h, w, c, c + 8, 0)
    _lib.check(lib.ammc_maxpool2x2_f32(X.pix0(), *X.strides, Y.pix0(), *Y.strides, b, h, w, c, _s()), "maxpool")
    _untouched(Y)
    _bits(Y.interior(), F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), "maxpool vs F.max_pool2d")
    _bits(Y.interior(), R.maxpool2x2(x).float(), "maxpool vs the reference")


@pytest.mark.parametrize("dim,m", [(4, 1), (64, 256), (100, 300)])
def test_pack_codebook_and_bn_fold(dim, m):
    lib = _lib.load()
    e = S.hashed_normal(f"pc-{dim}-{m}", (dim, m), 0.9)
    e_d, = _dev(e)
    out = _sent(m + 2, dim)                                            # rows [0, m): e_md; row m: a tail
    norm = _sent(m + 4)
    _lib.check(lib.ammc_pack_codebook_f32(_ptr(e_d), dim, m, _ptr(out), _ptr(norm), _s()), "pack_codebook")
    assert bool((out.view(torch.int32)[m:] == SENT).all()) and bool((norm.view(torch.int32)[m:] == SENT).all())
    e_md, nrm = R.pack_codebook(e)
    _bits(out[:m], e_md.float(), "the transpose")
    # a left-to-right sum of D squares: D additions and one rounding per square: n + c = D + 1
    _bounded("pack_codebook_f32", norm[:m], nrm, 2 * (dim + 1) * U * nrm, f"norms ({dim},{m})")
    # eval-BN fold over m channels: scale = gamma / sqrt(var + eps): the sum, the root, the division: k = 3;
    # shift = beta - mean scale: the scale's error times |mean|, two more roundings
    gamma, beta, mean = (S.hashed_normal(f"bf-{n}-{m}", (m,)) for n in "gbm")
    var = S.hashed_uniform(f"bf-v-{m}", (m,), 0.01, 3.0)
    ins = _dev(gamma, beta, mean, var)
    ss = _sent(2, m + 4)
    _lib.check(lib.ammc_bn_fold_f32(*[_ptr(t) for t in ins], 1e-5, m, _ptr(ss[0]), _ptr(ss[1]), _s()), "bn_fold")
    assert bool((ss.view(torch.int32)[:, m:] == SENT).all())
    scale, shift = R.bn_fold(gamma, beta, mean, var, float(torch.tensor(1e-5, dtype=torch.float32)))
    d_sc = 3 * U * scale.abs()
    _bounded("bn_fold_f32", ss[0, :m], scale, 2 * d_sc, f"scale ({m})")
    _bounded("bn_fold_f32", ss[1, :m], shift, 2 * (mean.double().abs() * d_sc + 2 * U * (beta.double().abs() + (mean.double() * scale).abs())), f"shift ({m})")


# ---- refusals: arguments that are turned away before any launch ------------------------------------------------------

def test_refusals_before_any_launch():
    lib = _lib.load()
    s = _s()
    t = torch.zeros(4096, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, ip = _ptr(t), i.data_ptr()
    st = (64, 64, 8)
    # d > 256 on the two accumulate forms
    assert lib.ammc_codebook_ema_f32(p, ip, 1, 4, 260, 4, 0.5, 0.5, 1e-5, p, p, p, s) == EUNSUP
    assert lib.ammc_codebook_count_f32(p, ip, 1, 4, 260, 4, p, p, s) == EUNSUP
    assert lib.ammc_codebook_ema_f32(None, ip, 1, 4, 64, 4, 0.5, 0.5, 1e-5, p, p, p, s) == EINVAL
    assert lib.ammc_codebook_count_f32(p, None, 1, 4, 64, 4, p, p, s) == EINVAL
    assert lib.ammc_codebook_ema_apply_f32(p, None, 64, 4, 0.5, 0.5, 1e-5, p, p, p, s) == EINVAL
    # d % 4 on the commit gradient
    assert lib.ammc_commit_bwd_f32(p, p, ip, 1, None, None, p, 4, 6, s) == EINVAL
    assert lib.ammc_commit_bwd_f32(p, p, None, 1, None, None, p, 4, 8, s) == EINVAL
    # c % 4 or c > 1024 on the BatchNorm group and the channel sum
    for c in (6, 1028):
        assert lib.ammc_bn_stats_f32(p, *st, 1, 1, 1, c, p, s) == EINVAL
        assert lib.ammc_chan_sum_f32(p, *st, 1, 1, 1, c, p, s) == EINVAL
        assert lib.ammc_bn_bwd_reduce_f32(p, *st, p, *st, p, p, p, p, 1, 1, 1, 1, c, p, s) == EINVAL
        assert lib.ammc_bn_bwd_apply_f32(p, *st, p, *st, p, p, p, p, p, 1, p, *st, 1, 1, 1, c, None, s) == EINVAL
    assert lib.ammc_bn_stats_f32(None, *st, 1, 1, 1, 8, p, s) == EINVAL
    assert lib.ammc_bn_stats_f32(p, *st, 1, 1, 1, 8, None, s) == EINVAL
    assert lib.ammc_bn_bwd_reduce_f32(p, *st, None, *st, p, p, p, p, 1, 1, 1, 1, 8, p, s) == EINVAL
    assert lib.ammc_bn_bwd_apply_f32(p, *st, p, *st, p, p, p, p, None, 1, p, *st, 1, 1, 1, 8, None, s) == EINVAL
    # cp < c or cp % 4 on tanh_bwd and the layout change
    assert lib.ammc_tanh_bwd_nhwc_f32(p, p, 1, 8, 2, 2, p, *st, 4, s) == EINVAL
    assert lib.ammc_tanh_bwd_nhwc_f32(p, p, 1, 3, 2, 2, p, *st, 6, s) == EINVAL
    assert lib.ammc_tanh_bwd_nhwc_f32(p, None, 1, 3, 2, 2, p, *st, 4, s) == EINVAL
    assert lib.ammc_nchw_to_nhwc_f32(p, 1, 8, 2, 2, p, *st, 4, s) == EINVAL
    assert lib.ammc_nhwc_to_nchw_f32(None, *st, 1, 3, 2, 2, p, s) == EINVAL
    assert lib.ammc_maxpool2x2_f32(p, *st, p, *st, 1, 1, 1, 6, s) == EINVAL
    assert lib.ammc_maxpool2x2_bwd_f32(p, *st, p, *st, None, 0, 0, 0, p, *st, 1, 1, 1, 4, 2, 4, s) == EINVAL      # in_h / 2 != h
    assert lib.ammc_lrelu_f32(p, *st, 1, 1, 1, 6, 0.1, s) == EINVAL
    assert lib.ammc_lrelu_bwd_f32(p, *st, None, *st, 1, 1, 1, 4, 0.1, s) == EINVAL
    assert lib.ammc_flownet_prep_f32(p, 1, 2, 2, p, *st, 0.0, p, s) == EINVAL
    assert lib.ammc_flownet_prep_f32(p, 1, 2, 2, p, *st, 255.0, None, s) == EINVAL
    assert lib.ammc_upsample4_bilinear_f32(p, *st, 1, 0, 2, 2, 1.0, p, s) == EINVAL
    assert lib.ammc_pack_codebook_f32(p, 4, 4, None, p, s) == EINVAL
    assert lib.ammc_bn_fold_f32(p, p, p, None, 1e-5, 4, p, p, s) == EINVAL
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0 and int(i.abs().max()) == 0
