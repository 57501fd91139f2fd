"""The case table of tests/patch_cases.py without a device: every instance `conv_tap_s16_try` can launch has a case, every
tap / outc case reaches the kernel it claims (the library's own dispatch through `ammc_conv_gemm_s16_variant`, which
launches nothing), the table holds the tile totals and epilogues it was built for, the fp64 `reference` of every kind
agrees with an independent formulation, the truth of every case moves by at least ten gates when x loses its lo halves,
and the entry points of conv_first / conv_up refuse what their kernels cannot take (they return before any launch)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import patch_cases as P
from conftest import ROOT
from oracle import ammc_oracle as O


def dispatcher_instances():
    """the instances `conv_tap_s16_try` can launch, parsed from its `launch_tap<WGM, WGN, TM, TN, AS, MF[, KH]>` calls, as
    the labels `launch_tap` prints for them"""
    text = open(os.path.join(ROOT, "ammcnet_aaai2021_amd", "csrc", "conv_tap_s16.hip")).read()
    body = text[text.index("int conv_tap_s16_try(const AmmcConvDesc& d"):]
    return {"conv_tap_s16<%s>" % ", ".join(a.strip() for a in m.group(1).split(","))
            for m in re.finditer(r"launch_tap<([\d, ]+)>\(", body)}


def base(label: str) -> str:
    return re.sub(r"\+(stats|bnbwd)$", "", label)


def test_the_dispatcher_has_the_ten_instances_the_table_is_built_for():
    assert dispatcher_instances() == set(P.TAP_INSTANCES)


def test_the_table_covers_every_instance_of_the_dispatcher():
    """an instance added to the dispatcher without a case fails here; so does an instance whose cases were deleted"""
    reached = {base(c.label) for c in P.CASES if c.kind in ("tap", "outc")}
    assert reached >= dispatcher_instances(), dispatcher_instances() - reached
    assert {base(c.label) for c in P.SHARED} == set(P.TAP_INSTANCES)


@pytest.mark.parametrize("case", P.CASES + P.SHARED, ids=lambda c: c.name)
def test_every_case_reaches_the_kernel_it_claims(case):
    assert P.label_of(case) == case.label


def test_the_table_holds_the_totals_and_epilogues_it_was_built_for():
    tap = [c for c in P.CASES if c.kind == "tap"]
    floor = {P.KH64: 192, P.T64_1: 192, P.T64_0: 192, P.W8_1: 192, P.W8_0: 192, P.T128_1: 512, P.T128_0: 512, P.KH128: 1024,
             P.O4: 192, P.O8: 192}
    for inst, fl in floor.items():
        mine = [c for c in tap if base(c.label) == inst]
        assert any(P.tiles(c) == fl for c in mine), inst                          # a case at the instance's tile-count floor
        assert any(c.y_f32 for c in mine), inst                                     # an fp32 store
        if inst not in (P.O4, P.O8):
            assert any(c.act == P.ACT_LRELU for c in mine) and any(c.res == "s16" for c in mine) and any(c.pool for c in mine), inst
            assert any(c.x_slice for c in mine) and any(c.y_slice for c in mine) and any(c.res == "f32" for c in mine), inst
        else:
            assert any(c.n_store and c.sq for c in mine), inst
        if inst.endswith("0>") or inst.endswith("0, 1>"):                          # the 32x32x16 forms have the statistics epilogue
            assert any(c.stats and not c.bnbwd for c in mine), inst
        if inst.endswith("0, 1>"):
            assert any(c.bnbwd for c in mine), inst
    # one tile short of each threshold lands on the neighbouring instance
    assert {(P.tiles(c), base(c.label)) for c in tap} >= {(511, P.W8_1), (511, P.W8_0), (1023, P.W8_1)}
    assert {c.cin for c in tap} >= {32, 64, 128} and any(c.n == 256 for c in tap)
    assert {c.label.endswith("1>") and not c.label.endswith("0, 1>") for c in tap if c.overflow} == {True, False}   # both S16 store forms
    outc = [c for c in P.CASES if c.kind == "outc"]
    on = [c for c in outc if c.label == P.OUTC]
    for tot in (192, 256, 257, 784):
        assert {c.cin for c in on if P.tiles(c) == tot and c.sq} == {32, 64}, tot
    assert {c.n_store for c in on if c.sq} == {1, 2, 3, 4} and {c.n_store for c in on if not c.sq} >= {2, 3, 4}
    assert any(c.n_store == 5 and c.label == P.O8 for c in outc)             # five columns: off the streaming kernel AND off the four-filter tap instance
    assert any(c.sq0 and c.sq for c in on) and any(c.sq0 and not c.sq for c in on) and any(c.t_off % 4 for c in on)
    first = [c for c in P.CASES if c.kind == "first"]
    assert {c.cin for c in first} == {1, 3, 6, 12, 13, 16}
    assert {(c.cin, c.act) for c in first} >= {(cc, a) for cc in (1, 3, 6, 12, 13, 16) for a in (P.ACT_NONE, P.ACT_RELU)}
    assert {(c.H, c.W) for c in first} >= {(8, 32), (16, 64), (24, 96)}
    assert {c.B * (c.H // 8) * (c.W // 32) for c in first} >= {512, 513}
    assert {(c.scale == "none", not c.shift) for c in first} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(c.win == c.cin for c in first) and any(0 < c.win < c.cin for c in first) and any(c.win == 0 for c in first)
    assert any(c.y_slice for c in first) and any(c.overflow for c in first)
    up = [c for c in P.CASES if c.kind == "up"]
    assert {(c.H, c.W, c.n, c.B) for c in up} >= {(h, w, n, b) for (h, w) in ((8, 32), (16, 32), (8, 64)) for n in (64, 128) for b in (1, 3)}
    assert any(c.n == 256 for c in up) and any(c.cin == 32 for c in up) and any(c.y_slice for c in up) and any(c.overflow for c in up)
    assert {c.act for c in up} == {P.ACT_NONE, P.ACT_RELU}


# ---- the references against independent formulations, on tiny shapes ----------------------------------------------------------
def _im2col_conv(x, w):
    """3x3 pad-1 convolution as unfold + matmul"""
    B, Cc, H, W = x.shape
    cols = F.unfold(F.pad(x, (1, 1, 1, 1)), 3)                                   # [B][C 9][H W]
    return (w.reshape(w.shape[0], -1) @ cols).view(B, -1, H, W)


@pytest.mark.parametrize("form", ["bn-relu-res", "lrelu", "pow2-f32res", "tanh-nstore"])
def test_tap_reference_against_unfold_matmul(form):
    kw = {"bn-relu-res": dict(**P.BN, res="s16"), "lrelu": P.LR, "pow2-f32res": P.F32,
          "tanh-nstore": dict(**P.OC, n_store=3, sq=True, sq0=1.5)}[form]
    c = P.Case("tiny-" + form, "tap", 2, 8, 32, 32, 32 if form == "tanh-nstore" else 64, "", **kw)
    o = P.host_ops(c)
    want = P.reference(c, o)
    nt = P.out_channels(c)
    y = _im2col_conv(P.s16_round(o.x), P.s16_round(o.w))
    if o.scale is not None:
        y = y * o.scale.double()[:nt].view(1, -1, 1, 1)
    if o.shift is not None:
        y = y + o.shift.double()[:nt].view(1, -1, 1, 1)
    y = {P.ACT_RELU: lambda t: torch.relu(t), P.ACT_LRELU: lambda t: F.leaky_relu(t, 0.1), P.ACT_TANH: torch.tanh,
         P.ACT_NONE: lambda t: t}[c.act](y)
    if c.res == "s16":
        y = y + P.s16_round(o.res)
    elif c.res == "f32":
        y = y + o.res.double()
    assert tuple(want.shape) == (2, nt, 8, 32)
    assert float((want - y).abs().max()) <= 1e-12
    if c.sq:
        sq = torch.stack([(((o.target[b].double() + 1) / 2 - (want[b] + 1) / 2) ** 2).sum() for b in range(c.B)]) + 1.5
        assert float((P.want_sq(c, o, want) - sq).abs().max()) <= 1e-9           # the header's expression, sample by sample


@pytest.mark.parametrize("act", [P.ACT_RELU, P.ACT_NONE])
def test_up_reference_against_the_oracles_module_sequence(act):
    """`up` of the oracle (ConvTranspose2d + pad + cat([skip, .]) + double_conv) with BatchNorm parameters that fold to
    the case's scale / shift; its second conv is the identity (a centre-tap delta filter, BatchNorm of mean 0 and
    variance 1 - eps), so with ReLU the oracle's output is the case's; without, the first conv's BatchNorm output is
    compared before the oracle's ReLU through the same state dict"""
    c = P.Case("tiny-up", "up", 2, 8, 32, 32, 64, P.UP, scale="bn", shift=True, act=act)
    o = P.host_ops(c)
    x, x2 = P.s16_round(o.x), P.s16_round(o.x2)
    want = P.reference(c, o)
    n = c.n
    eye = torch.zeros(n, n, 3, 3, dtype=torch.float64)
    eye[torch.arange(n), torch.arange(n), 1, 1] = 1.0
    one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    sd = {"u.up.weight": o.wt.double(), "u.up.bias": o.bt.double(), "u.conv.conv.0.weight": o.w.double(),
          "u.conv.conv.1.weight": o.scale.double(), "u.conv.conv.1.bias": o.shift.double(),
          "u.conv.conv.1.running_mean": zero, "u.conv.conv.1.running_var": one - O.BN_EPS,
          "u.conv.conv.3.weight": eye, "u.conv.conv.4.weight": one, "u.conv.conv.4.bias": zero,
          "u.conv.conv.4.running_mean": zero, "u.conv.conv.4.running_var": one - O.BN_EPS}
    got = O.up(sd, "u", x2, x)
    assert float((got - want.clamp_min(0)).abs().max()) <= 1e-12
    if act == P.ACT_NONE:
        assert float(want.min()) < -0.1                                              # (the comparison above did clamp something)
        pre = O._bn(sd, "u.conv.conv.1", F.conv2d(torch.cat([x, F.conv_transpose2d(x2, sd["u.up.weight"], sd["u.up.bias"], stride=2)], 1),
                                                   sd["u.conv.conv.0.weight"], None, padding=1), False)
        assert float((pre - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("win", [-1, 12, 3, 0])
def test_first_reference_against_conv2d_of_the_padded_clip(win):
    c = P.Case("tiny-first", "first", 3, 8, 32, 12, 64, "", **P.BN, win=win)
    o = P.host_ops(c)
    want = P.reference(c, o)
    planes = P.s16_round(o.x)
    step = {-1: 12, 12: 12, 3: 3, 0: 0}[win]
    assert planes.shape[0] == 2 * step + 12
    for b in range(c.B):
        clip = planes[b * step:b * step + 12].unsqueeze(0)                          # the window, by explicit slicing
        y = F.conv2d(F.pad(clip, (1, 1, 1, 1)), P.s16_round(o.w))                   # no padding argument: the clip is padded
        y = (y * o.scale.double().view(1, -1, 1, 1) + o.shift.double().view(1, -1, 1, 1)).clamp_min(0)
        assert float((y[0] - want[b]).abs().max()) <= 1e-12
    if win == 0:
        assert torch.equal(want[0], want[1]) and torch.equal(want[0], want[2])
    if win == 3:                                                                     # overlapping: clip 1 starts at clip 0's plane 3
        assert torch.equal(P.first_clips(c, o.x)[1, :9], P.first_clips(c, o.x)[0, 3:])


def test_s16_round_is_the_split_of_the_library_header():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -12, 0.1, -3.14159274, 65000.0, 1e-3])
    r = P.s16_round(v)
    assert float(((r - v.double()).abs() / v.double().abs()).max()) < 2.0 ** -21
    assert torch.equal(P.hi_only(v), v.half().double())


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_zeroing_the_lo_halves_moves_the_truth_by_ten_gates(case):
    """a kernel that dropped a cross term of the S16 product could not pass this case's gate"""
    s = P.sensitivity(case, P.host_ops(case))
    print(f"{case.name}: x.lo sensitivity {s:.1f} gates")
    assert s >= P.SENS_MIN, s


# ---- the refusals of the entry points -----------------------------------------------------------------------------------------
def test_conv_first_refuses_what_its_kernel_cannot_take():
    for what, got, want in P.first_refusals():
        assert got == want, (what, got, want)


def test_conv_up_refuses_what_its_kernel_cannot_take():
    for what, got, want in P.up_refusals():
        assert got == want, (what, got, want)
