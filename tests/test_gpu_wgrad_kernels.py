"""The S16 weight-gradient kernels alone, case by case (tests/wgrad_cases.py), against the fp64 weight gradient of the
reference operator (autograd of conv2d / conv_transpose2d) on the fp32 operands.

Gate: max|got - want| / max|want| <= 3e-6, the project's gate for this entry (tests/test_gpu_wgrad_s16.py), for every
default instance; `AMMC_WGRAD_G11=1`: at most 3e-4 and at least 3e-6 (the same file).  That the gate can see a lost
cross term of the S16 product is a property of the operands and is checked on the CPU (tests/test_wgrad_cases_host.py: at
least ten gates for either operand, every parity case).  Printed and not gated: the error against fp64 of the DECODED S16
operands (the kernel's own arithmetic) and the error of torch's fp32 autograd on the CPU (a witness).  DESIGN.md 5.14
holds the measured table.

Every case also asserts the dispatch label, and
  atomics form  dw inside a flat zeroed buffer between two 4-KB canaries: after one launch rows cout .. n, the channels
                beyond the true input channels of every tap and the columns ntaps * cin .. kpad are exactly zero, every
                canary (dw's, the operands', `zeros`') is bit-unchanged; a second launch gives twice the gradient;
  slab form     slabs and dw_oihw [cout][cin_true][3][3] pre-filled with NaN between canaries: every element overwritten
                and finite, canaries unchanged, two launches bit-equal, within 2e-6 of max|dw| of the atomics form;
  geometry      the other half of a sliced buffer, g's halo ring, everything of a larger buffer outside the window, the
                ConvTranspose crop's odd row and column hold a NaN half pattern, `zeros` is 128 zero floats and then that
                pattern: the result must be finite and within the gate.

Placement (test_one_hot_gradient_copies_the_neighbourhood_bit_for_bit): g is zero except 1 (or 2^-20, through the
rescaling) at thirteen pixels, one channel each - image corners, both sides of the x = 31 | 32 patch seam and of the
patch-row seams, the last row of one image and the first of the next, the last pixel.  a lies on a 2^-16 grid, exact in
S16.  Row j of dW must EQUAL a's 3 x 3 neighbourhood of spot j times the hot value, every other row must be zero:
  wgrad_tap3_s16   the scaled g is hi = 2^k, lo = 0.  acc = GH x AH + (2^-11 GH) x AL [+ (2^-11 GL) x AH = 0]: 2^k a_hi and
                   2^(k-11) a_lo are exact products (2^-11 GH = 2^(k-11) is an exact half, down to 2^-24), every other
                   product of the 16-pixel MFMA and of every other patch is zero, and their sum 2^k (a_hi + 2^-11 a_lo) = 2^k a
                   has 17 significant bits: exact in fp32.  x inv = 2^-k x value: exact.  G11 drops only the GL term: 0.
                   Slabs: every other slab holds 0 for the element; atomics: every other addend is 0.
  wgrad_s16        four plane products in four accumulator registers, folded as (hh + 2^-11 lh) + 2^-11 (hl + 2^-11 ll):
                   lh = ll = 0 (g's lo), hh = 2^k a_hi, hl = 2^k a_lo, the same exact sum.

Switch form: one child pytest process over the sub-table of AMMC_WGRAD_G11=1 (the dispatcher reads the switch once per
process), under its own timeout; a child that did not end with pytest's 0 or 1 ends the test."""
import os
import re
import subprocess
import sys
import time

import pytest
import torch

import wgrad_cases as W

pytestmark = pytest.mark.gpu

_ACTIVE_PARITY = W.active(W.PARITY)
_ACTIVE_PLACEMENT = W.active(W.PLACEMENT)


def _ids(c):
    return c.name


def _finite(t):
    return bool(torch.isfinite(t).all())


def _check_packed(c, packed):
    """what one launch of the atomics form leaves outside the true gradient: exactly zero"""
    assert _finite(packed), "a sentinel was read (NaN in the packed gradient)"
    if c.rows < c.n:
        assert float(packed[c.rows:].abs().max()) == 0.0, "rows cout .. n"
    taps = packed[:, :c.ntaps * c.cin].view(c.n, c.ntaps, c.cin)
    if c.chans < c.cin:
        assert float(taps[:, :, c.chans:].abs().max()) == 0.0, "channels beyond the true input channels"
    if c.kpad > c.ntaps * c.cin:
        assert float(packed[:, c.ntaps * c.cin:].abs().max()) == 0.0, "columns ntaps * cin .. kpad"


@pytest.mark.parametrize("case", _ACTIVE_PARITY, ids=_ids)
def test_wgrad_kernel_vs_fp64(case):
    c = case
    o = W.host_ops(c)
    r = W.run_case(c, o)
    assert r["status_q"] == 0 and r["label"] == c.label, (r["status_q"], r["label"])
    assert r["status"] == 0
    assert (r["inv"] is None) == c.inv_null
    want = W.reference(c, o=o)
    lo, hi = W.gate(c)
    e_hip = W.rel_err(r["dw"], want)
    e_dec = W.rel_err(r["dw"], W.reference(c, g=r["g_seen"].cpu(), a=r["a_seen"].cpu()))
    e_wit = W.rel_err(W.reference(c, torch.float32, o=o), want)
    e_twice = W.rel_err(r["dw_twice"], 2 * want)
    print(f"wgrad {c.name} [{c.label}]{' ' + c.switch if c.switch else ''}: e_hip {e_hip:.3e} (gate {hi:.0e}) e_decoded {e_dec:.3e} "
          f"e_witness_fp32 {e_wit:.3e} second launch {e_twice:.3e}")
    assert _finite(r["dw"]) and lo <= e_hip <= hi, e_hip
    _check_packed(c, r["packed"])
    assert r["guards"]["atomics"], "a canary of the atomics form changed"
    assert e_twice <= hi, e_twice                              # accumulation: twice the gradient within the gate
    assert (r["need"] > 0) == c.slab and (r["slab_status_q"] == 0) == c.slab, (r["need"], r["slab_status_q"])
    if c.slab:
        assert r["slab_status"] == 0
        assert r["slab_label"].endswith(f"+slabs{r['need'] // (c.n * c.kpad)}"), r["slab_label"]
        dws = r["dws"]
        assert _finite(dws), "an element of dw_oihw was not overwritten, or a slab element was read unwritten"
        assert r["guards"]["slab"], "a canary of the slab form changed"
        assert r["slab_same"], "two launches of the slab form differ"
        e_slab = W.rel_err(dws, want)
        # G11 is also the slab launch's arithmetic: both entries go through wgrad_tap3_s16_try
        g11 = c.switch == "AMMC_WGRAD_G11=1"
        d_at = float((dws - r["dw"]).abs().max() / r["dw"].abs().max())
        print(f"wgrad {c.name} slab form [{r['slab_label']}]: e_hip {e_slab:.3e}, against the atomics form {d_at:.3e}")
        assert e_slab <= (W.GATE_G11[1] if g11 else W.GATE), e_slab
        assert d_at <= W.GATE_SLAB, d_at


@pytest.mark.parametrize("case", _ACTIVE_PLACEMENT, ids=_ids)
def test_one_hot_gradient_copies_the_neighbourhood_bit_for_bit(case):
    c = case
    o = W.host_ops(c)
    r = W.run_case(c, o)
    assert r["status_q"] == 0 and r["label"] == c.label and r["status"] == 0
    want = W.placement_want(c, o)
    got = r["dw"].cpu()
    nhot = len(c.hot)
    for j in range(nhot):
        assert torch.equal(got[j], want[j]), (c.name, "hot spot", j, c.hot[j], float((got[j] - want[j]).abs().max()))
    assert float(got[nhot:].abs().max()) == 0.0, "a row without a hot spot is not zero"
    _check_packed(c, r["packed"])
    assert r["guards"]["atomics"]
    assert torch.equal(r["dw_twice"].cpu(), 2 * want)          # (doubling is exact)
    assert (r["need"] > 0) == c.slab
    if c.slab:
        assert r["slab_status"] == 0 and r["guards"]["slab"] and r["slab_same"]
        assert torch.equal(r["dws"].cpu(), want), float((r["dws"].cpu() - want).abs().max())


def test_the_default_dispatch_reaches_five_kernels_and_the_child_the_other_two():
    """the labels asserted case by case above and in the child below, together: all seven"""
    assert {c.label for c in W.PARITY if not c.switch} == {W.R64, W.R128, W.O32, W.F32C, W.IM2COL}
    assert {c.label for c in W.PARITY if c.switch} == {W.G64, W.G128}


def test_switch_forms_in_child_processes():
    """the sub-table of AMMC_WGRAD_G11=1 (parity and placement) in a child pytest process with the switch set; a child that
    timed out, aborted or died of a signal ends the test: nothing more is started on the device"""
    if any(k in os.environ for k in W.SWITCHES):
        pytest.skip("already inside a run with a switch set")
    failed = []
    for switch in sorted({c.switch for c in W.CASES if c.switch}):
        k, v = switch.split("=")
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-rf", "-k", "vs_fp64 or bit_for_bit"],
                           env=dict(os.environ, **{k: v}), capture_output=True, text=True, timeout=300)
        out = r.stdout.splitlines()
        print("\n".join([ln[ln.index("wgrad "):] for ln in out if "wgrad " in ln and "FAILED" not in ln] +
                        [ln for ln in out if ln.startswith("FAILED ")]))
        print(f"child {switch}: {time.time() - t0:.1f} s, return code {r.returncode}")
        assert r.returncode in (0, 1), (switch, r.returncode, r.stdout[-2000:] + r.stderr[-2000:])      # 124, 134, 137, 139, < 0: stop here
        want = len([c for c in W.CASES if c.switch == switch])
        m = re.search(r"^(\d+) passed", out[-1]) if out else None
        if r.returncode != 0 or not m or int(m.group(1)) != want:
            failed.append((switch, want, r.stdout[-3000:] + r.stderr[-1000:]))
    assert not failed, failed
