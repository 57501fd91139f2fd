"""`ammc_conv_gemm_s16` and `ammc_conv_gemm_f32` alone, case by case (tests/conv_gemm_cases.py), against an fp64
evaluation of the operands as the kernel sees them.

S16: max|got - want| / max|want| <= 2e-6, the per-kernel gate of test_gpu_conv_tap.py / test_gpu_conv_up.py (S16 outputs
compared after decoding; the fused squared error at 2e-5 as test_output_layer_vs_fp64).  Before the launch every case
checks that the gate can see a lost cross term: the same fp64 truth with x's lo halves zeroed differs by >= 2e-5
(measured 1.2e-4 .. 3.6e-4 over the table).

fp32: nothing in the project fixed a per-kernel number for the fmaf chain, so torch's own fp32 evaluation of the same
operands on the CPU is the witness: e_hip <= 3 e_witness (the 1.5 DESIGN 5.4 records for a sequential chain over K <=
4608 against blocked sums, times 2).  Measured figures per family: DESIGN.md section 7.

Every case also asserts that nothing outside the output is written (halo, the other slice of a concat buffer, a canary
after an exact-size NCHW tensor, the pad row / column of the odd up = 2 crop) and that every output element is."""
import os
import subprocess
import sys

import pytest
import torch

import conv_gemm_cases as G

pytestmark = pytest.mark.gpu


def _ids(c):
    return c.name


@pytest.mark.parametrize("case", G.CASES, ids=_ids)
def test_conv_gemm_s16_vs_fp64(case):
    h = G.host_half(case)                                   # the condition on the inputs, on the CPU, before any launch
    assert h["sens"] >= G.SENS_MIN, h["sens"]
    o = h["ops"]
    r = G.run_case(case, o, True)
    assert r["status"] == case.status
    assert r["labels"] and all(lb == case.label for lb in r["labels"]), r["labels"]
    want = G.device_want(case, o, r)
    mask = G.compare_mask(case, want)
    want_hi = G.reference(case, o, torch.float64, G.hi_only(r["x"]), r["w"], r["res"])
    sens = G.rel_err(want_hi, want, mask)
    err = G.rel_err(r["got"], want, mask)
    print(f"s16 {case.name} [{case.label}]: err {err:.3e} (gate {G.GATE_S16:.0e}), x.lo sensitivity {sens:.3e}")
    assert sens >= G.SENS_MIN, sens
    assert bool(torch.isfinite(r["got"][mask]).all()), "an output element was never written"
    assert err <= G.GATE_S16, err
    assert r["flag"] == (1 if case.overflow else 0)
    if case.sq:
        want_sq = ((o.target.double() - want) * 0.5).pow(2).sum(dim=(1, 2, 3))
        e_sq = float(((r["sq"].double() - want_sq).abs() / want_sq).max())
        print(f"s16 {case.name}: squared error {e_sq:.3e}")
        assert e_sq <= G.GATE_SQ, e_sq


@pytest.mark.parametrize("case", [c for c in G.CASES if not c.overflow], ids=_ids)
def test_conv_gemm_f32_vs_fp64_and_witness(case):
    """Measured on MI355X (e_witness 1.5e-7 .. 6.2e-7 throughout): e_hip 1.4e-7 .. 3.9e-7, e_hip / e_witness 0.37 .. 1.49
    over the 36 cases, the same at K = 72 and K = 4608 (tail-h1 1.49, cin512-k4608 1.33, splitk7-capped 1.24,
    splitk35-k4608 1.07, dgrad3-128to64 1.07).  Before the kernel summed pairs of K chunks in a second accumulator set
    the ratio followed the length of its single fmaf chain: <= 1.08 at K <= 128, 1.5 .. 3.15 at K = 288 .. 1024, 4.30 at
    K = 1152, 8.5 .. 9.0 at K = 4608, and eight cases failed this gate (DESIGN.md sections 7 and 8)."""
    h = G.host_half(case)
    o = h["ops"]
    r = G.run_case(case, o, False)
    assert r["status"] == case.status
    want = h["want_f32"]
    assert bool(torch.isfinite(r["got"]).all()), "an output element was never written"
    e_hip, e_wit = G.rel_err(r["got"], want), h["e_witness"]
    print(f"f32 {case.name}: e_hip {e_hip:.3e} e_witness {e_wit:.3e} ratio {e_hip / e_wit:.2f}")
    assert e_hip <= G.WITNESS_FACTOR * e_wit, (e_hip, e_wit)
    if case.sq:
        want_sq = ((o.target.double() - want) * 0.5).pow(2).sum(dim=(1, 2, 3))
        assert float(((r["sq"].double() - want_sq).abs() / want_sq).max()) <= G.GATE_SQ


@pytest.mark.parametrize("case", [c for c in G.CASES if "+splitk" in c.label], ids=_ids)
def test_splitk_equals_no_splitk(case):
    """the same layer with and without the workspace: both within the fp64 gate, within the gate of each other, and the
    split result the same bits on a second run (fixed summation order)"""
    o = G.host_ops(case)
    a = G.run_case(case, o, True)
    b = G.run_case(case, o, True)
    plain = G.run_case(case, o, True, splitk=False)
    assert a["labels"] == [case.label] and plain["labels"] == [G.L128]
    want = G.device_want(case, o, a)
    e_split, e_plain, e_both = G.rel_err(a["got"], want), G.rel_err(plain["got"], want), G.rel_err(a["got"], plain["got"])
    print(f"splitk {case.name}: split {e_split:.3e} plain {e_plain:.3e} split vs plain {e_both:.3e}")
    assert e_split <= G.GATE_S16 and e_plain <= G.GATE_S16 and e_both <= G.GATE_S16
    assert torch.equal(a["got"], b["got"])


@pytest.mark.parametrize("case", [c for c in G.CASES if c.label == G.L256], ids=_ids)
def test_256_row_tile_equals_128_row_tile(case, tmp_path):
    """the same layer in a child process with AMMC_S16_BIG=0 (the switch is read once per process) runs on <128x128>;
    the two outputs agree to the gate (the whole tensor is checked against fp64 by test_conv_gemm_s16_vs_fp64)"""
    o = G.host_ops(case)
    big = G.run_case(case, o, True)
    assert big["labels"] == [G.L256]
    out = tmp_path / "small.pt"
    root = os.path.dirname(os.path.dirname(os.path.abspath(G.__file__)))
    env = dict(os.environ, AMMC_S16_BIG="0", PYTHONPATH=os.pathsep.join([root] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    p = subprocess.run([sys.executable, os.path.abspath(G.__file__), case.name, str(out)], env=env, capture_output=True,
                       text=True, timeout=600, cwd=os.path.dirname(os.path.abspath(G.__file__)))
    assert p.returncode == 0, p.stderr[-3000:]
    small = torch.load(out)
    assert small["status"] == 0 and small["labels"] == [G.L128], small["labels"]
    e = G.rel_err(big["got"], small["got"])
    print(f"256 vs 128 rows {case.name}: {e:.3e}")
    assert e <= G.GATE_S16, e
