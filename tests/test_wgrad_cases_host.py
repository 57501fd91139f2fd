"""The case table of tests/wgrad_cases.py without a device: every instance the S16 weight-gradient dispatch can
launch has a case, every case reaches the kernel it claims (the library's own dispatch through
`ammc_conv_wgrad_s16_variant`, which launches nothing and makes no HIP call; the switch form in a child process with
the switch set - the dispatcher reads it once per process), every descriptor a halo-patch kernel can take reaches one,
the fp64 reference agrees with an independent formulation, the truth of every parity case moves by at least ten gates
when either operand loses its lo half, the placement operands are exact in S16, and both entries refuse what their
kernels cannot take."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import wgrad_cases as W
from conftest import ROOT
from ammcnet_aaai2021_amd import _lib

CSRC = os.path.join(ROOT, "ammcnet_aaai2021_amd", "csrc")


def dispatcher_instances():
    """the instances the dispatcher can launch, parsed from the `launch_wgrad_tap3<NG, NA, NP, PH[, ROLL[, G11]]>` calls of
    wgrad_tap3_s16_try, as the labels the launcher prints for them (a literal 1 stands before ROLL)"""
    text = open(os.path.join(CSRC, "wgrad_tap3_s16.hip")).read()
    m = re.search(r"\bint wgrad_tap3_s16_try\([^;{]*\)\s*\{", text)
    assert m, "wgrad_tap3_s16.hip: the definition of wgrad_tap3_s16_try was not found"
    out = set()
    for m in re.finditer(r"launch_wgrad_tap3<([\d, ]+)>\(", text[m.start():]):
        a = [int(v) for v in m.group(1).split(",")]
        assert 4 <= len(a) <= 6, a
        roll, g11 = (a + [0, 0])[4:6]
        shown = a[:4] + ([1, roll] if roll or g11 else []) + ([g11] if g11 else [])
        out.add("wgrad_tap3_s16<%s>" % ", ".join(str(v) for v in shown))
    return out


def test_the_dispatcher_has_the_six_instances_the_table_is_built_for():
    assert dispatcher_instances() == set(W.TAP3_INSTANCES)
    assert len(W.TAP3_INSTANCES) == 6


def test_the_table_covers_every_instance_the_im2col_windows_and_the_slab_form():
    """an instance added to a dispatcher without a case fails here; so does an instance whose cases were deleted"""
    for cases, what in ((W.PARITY, "parity"), ([c for c in W.PLACEMENT if c.kind == "conv3"], "placement")):
        assert {c.label for c in cases} == set(W.INSTANCES), (what, set(W.INSTANCES) - {c.label for c in cases})
    par = W.PARITY
    assert {c.ntaps for c in par if c.label == W.IM2COL} == {9, 16, 4}
    for inst in W.INSTANCES:
        mine = [c for c in par if c.label == inst]
        assert any(c.inv_null for c in mine), inst                                  # g_inv_scale = NULL, unscaled operands
        if inst != W.IM2COL:
            assert any(c.slab for c in mine), inst
    for inst in (W.R64, W.R128, W.O32, W.F32C, W.IM2COL):                           # operand geometry on every default kernel
        assert {c.geom for c in par if c.label == inst and c.kind == "conv3"} >= {"dense", "slice", "crop"}, inst
    assert any(c.geom == "oddcrop" and c.scaled == "a" for c in par if c.kind == "convt")
    mags = [c.gmag for c in par]
    assert min(mags) == 2e-8 and max(mags) == 1.0
    assert any(c.slab and c.cout and c.cout < c.n for c in par) and any(c.slab and c.cin_true and c.cin_true < c.cin for c in par)
    assert {c.switch for c in W.CASES} == {"", "AMMC_WGRAD_G11=1"}
    # the 4x4 window: both strides, an odd input, the first layer's and the head's channel counts
    c4 = [c for c in par if c.kind == "conv4"]
    assert {c.a_step for c in c4} == {1, 2} and any(c.a_odd for c in c4)
    assert {(c.cin, c.chans) for c in c4} >= {(8, 3), (64, 64)} and {(c.n, c.rows) for c in c4} >= {(32, 1), (64, 64)}


def _check_labels(case, got, slab_got, slab_count):
    rc, label = got
    assert rc == 0 and label == case.label, (case.name, rc, label)
    src, slab_label = slab_got
    assert (src == 0) == case.slab, (case.name, src, slab_label)
    if case.slab:
        # both entries go through wgrad_tap3_s16_try: the instance is the case's
        m = re.fullmatch(r"(wgrad_tap3_s16<[\d, ]+>)\+slabs(\d+)", slab_label)
        assert m and m.group(1) == case.label and int(m.group(2)) == slab_count >= 1, (case.name, slab_label, slab_count)
    else:
        assert src == -2 and slab_count == 0


@pytest.mark.parametrize("case", W.DEFAULT, ids=lambda c: c.name)
def test_every_default_case_reaches_the_kernel_it_claims(case):
    if any(k in os.environ for k in W.SWITCHES):
        pytest.skip("a dispatch switch is set in this process")
    d = W.desc(case)
    _check_labels(case, W.variant(d), W.slabs_variant(d), W.slab_count(d))


_CHILD = """
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import wgrad_cases as W
out = {{}}
for c in W.active(W.CASES):
    d = W.desc(c)
    out[c.name] = [W.variant(d), W.slabs_variant(d), W.slab_count(d)]
print("LABELS " + json.dumps(out))
"""


def _child(env_extra, script):
    env = {k: v for k, v in os.environ.items() if k not in W.SWITCHES}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("switch", sorted({c.switch for c in W.CASES if c.switch}))
def test_every_switch_case_reaches_the_kernel_it_claims(switch):
    """one child process per switch (read once per process) over that switch's sub-table"""
    k, v = switch.split("=")
    out = _child({k: v}, _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT))
    got = json.loads(out[out.index("LABELS ") + 7:].splitlines()[0])
    mine = [c for c in W.CASES if c.switch == switch]
    assert sorted(got) == sorted(c.name for c in mine) and mine
    for c in mine:
        g, s, n = got[c.name]
        _check_labels(c, tuple(g), tuple(s), n)


def test_every_descriptor_a_halo_patch_kernel_can_take_reaches_one():
    """the routing over a grid of descriptors: the default labels are the four halo-patch instances and the im2col form and
    nothing else, and what the retired four-product dispatcher accepted lands on a three-MFMA instance.  Through the
    library's own dispatch, over cin 8 .. 512, n 32 .. 512 in steps of 32, H 1 .. 12, W in {7, 32, 64}."""
    if any(k in os.environ for k in W.SWITCHES):
        pytest.skip("a dispatch switch is set in this process")
    lib = _lib.load()
    buf = C.create_string_buffer(96)
    seen = {}
    for cin in (8, 16, 32, 64, 128, 256, 512):
        for n in range(32, 513, 32):
            for H in range(1, 13):
                for Wd in (7, 32, 64):
                    d = W.desc(W.Case("grid", "conv3", 2, H, Wd, n, cin, ""))
                    assert lib.ammc_conv_wgrad_s16_variant(C.byref(d), buf, 96) == 0
                    lab = buf.value.decode()
                    seen[lab] = seen.get(lab, 0) + 1
                    # what the four-product dispatcher accepted is taken by the three-MFMA one
                    if H % 4 == 0 and Wd % 32 == 0 and ((n % 128 == 0 and cin % 16 == 0) or (n % 64 == 0 and cin % 32 == 0)):
                        assert lab.startswith("wgrad_tap3_s16<"), (cin, n, H, Wd, lab)
    assert set(seen) == {W.R64, W.R128, W.O32, W.F32C, W.IM2COL}, seen


# ---- the reference against an independent formulation ---------------------------------------------------------------------------
_OPS = {}


def _ops(c):
    key = c.name.split("-", 1)[1] if c.switch else c.name           # (a switch case shares its default case's operands)
    if key not in _OPS:
        _OPS[key] = W.host_ops(c)
    return _OPS[key]


def _distinct(cases):
    """one case per set of operands and operator (the switch copies of a default case share both)"""
    seen, out = set(), []
    for c in cases:
        key = (c.kind, c.B, c.H, c.W, c.rows, c.chans, c.a_step, c.a_odd, c.gmag, c.scaled, c.name.split("-", 1)[1] if c.switch else c.name)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _distinct(W.CASES), ids=lambda c: c.name)
def test_reference_against_the_sum_over_unfolded_taps(case):
    o = _ops(case)
    want = W.reference(case, o=o)
    assert tuple(want.shape) == W.wshape(case)
    other = W.reference_unfolded(case, o.g, o.a)
    assert float((want - other).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("case", _distinct(W.PARITY), ids=lambda c: c.name)
def test_losing_a_lo_half_moves_the_truth_by_ten_gates(case):
    """a kernel that dropped a cross term of the S16 product (hi x lo of either side) could not pass this case's gate"""
    sg, sa = W.sensitivity(case, _ops(case))
    print(f"{case.name}: g.lo sensitivity {sg:.1f} gates, a.lo {sa:.1f} gates")
    assert sg >= W.SENS_MIN and sa >= W.SENS_MIN, (sg, sa)


def test_s16_round_is_the_split_of_the_library_header():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -12, 0.1, -3.14159274, 65000.0, 1e-3])
    r = W.s16_round(v)
    assert float(((r - v.double()).abs() / v.double().abs()).max()) < 2.0 ** -21
    assert torch.equal(W.hi_only(v), v.half().double())


@pytest.mark.parametrize("case", _distinct(W.PLACEMENT), ids=lambda c: c.name)
def test_placement_operands_are_exact_in_s16(case):
    o = _ops(case)
    assert torch.equal(W.s16_round(o.a), o.a.double())
    assert float((o.a.half().float() - o.a).abs().max()) > 0                  # (lo halves are in play)
    hot = o.g[o.g != 0]
    assert hot.numel() == len(case.hot) == 13 and bool((hot == case.gmag).all())
    m, e = torch.frexp(hot)
    assert bool((m == 0.5).all())                                             # powers of two
    assert {(b, y, x) for b, y, x in case.hot} >= {(0, 0, 0), (0, 0, case.W - 1), (0, case.H - 1, 0), (0, case.H - 1, case.W - 1),
                                                   (0, 5, 31), (0, 5, 32), (case.B - 1, case.H - 1, case.W - 1)}
    # the placement truth is the reference operator's own gradient
    assert torch.equal(W.placement_want(case, o).double(), W.reference(case, o=o))


# ---- the refusals of the entry points -------------------------------------------------------------------------------------------
def test_both_entries_refuse_what_their_kernels_cannot_take():
    if any(k in os.environ for k in W.SWITCHES):
        pytest.skip("a dispatch switch is set in this process")
    for what, got, want in W.refusals():
        assert got == want, (what, got, want)


def test_the_abi_version_is_42():
    assert _lib.ABI_VERSION == 42 == _lib.load().ammc_abi_version()
