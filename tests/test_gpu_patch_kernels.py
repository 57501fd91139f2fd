"""The four patch-resident S16 forward kernels alone, case by case (tests/patch_cases.py), against an fp64 evaluation of
the reference model's operator sequence on the operands as the kernel sees them.

Gates: tap and outc frames max|got - want| / max|want| <= 2e-6 (the project's per-kernel gate), the fused squared error
2e-5, conv_up and conv_first 3e-6 (tests/test_gpu_conv_up.py).  That each gate can see a lost cross term of the S16
product is a property of the operands and is checked on the CPU (tests/test_patch_cases_host.py: >= 10 gates for
every case).  The fp64 references are computed on the CPU, except for the cases of at least 1024 tiles (patch_cases.BIG),
whose convolution torch evaluates in fp64 on the device: the same operator, and the CPU evaluation of those shapes alone
would take longer than all the other cases together.

Every case also asserts what the guarded buffers of patch_cases.Guard see - every interior element written; the halo
ring on all four sides, the other channel slice of a concat buffer and the bytes before and behind the tensor untouched -
the dispatch label, the overflow flag, and that a second launch gives the same bits (frames, pooled output, statistics;
the squared error goes through fp32 atomics and is compared to its gate only).

Statistics bound: a per-patch sum is 256 stored values added in fp32 through nine levels (two rows in the lane, five DPP
levels, four waves - at most nine roundings on any path, each <= 2^-24 of a partial sum <= sum|v|), plus one rounding
per product for the sums of squares / of g xhat and two for xhat: |sum - fp64 sum of the stored values| <= 20 x 2^-24
sum|v| holds with room; the maxima of the stored values are exact.

Measured figures per kernel and instance: DESIGN.md section 5.13."""
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

import patch_cases as P

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def _ids(c):
    return c.name


def _patch_sums(t):
    """[B][n][H][W] -> [patches][n]: sums over the 8 x 32 patches, patch = (b, ty, tx)"""
    B, n, H, W = t.shape
    return t.view(B, n, H // 8, 8, W // 32, 32).sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(-1, n)


def _patch_max(t):
    B, n, H, W = t.shape
    return t.view(B, n, H // 8, 8, W // 32, 32).amax(dim=(3, 5)).permute(0, 2, 3, 1).reshape(-1, n)


def _check_stats(c, o, r):
    got = r["got"].double()
    st = r["stats"].double()
    if not c.bnbwd:
        for row, v in ((0, got), (1, got * got)):
            want, mag = _patch_sums(v), _patch_sums(v.abs())
            assert bool(((st[:, row] - want).abs() <= 20 * EPS * mag + 1e-30).all()), (c.name, row)
        return
    bn = {k: v.to(P.DEV) for k, v in o.bn.items()}
    vec = lambda t: t.double().view(1, -1, 1, 1)
    bc = bn["c"].double()
    pre = bc * vec(bn["scale"]) + vec(bn["shift"])
    assert float(pre.abs().min()) >= 1.0 / 256                                       # exact, never zero: no rounding case in the mask
    g = torch.where(pre > 0, got, torch.zeros_like(got))
    xh = (bc - vec(bn["mean"])) * vec(bn["invstd"])
    for row, v in ((0, g), (1, g * xh)):
        want, mag = _patch_sums(v), _patch_sums(v.abs())
        assert bool(((st[:, row] - want).abs() <= 20 * EPS * mag + 1e-30).all()), (c.name, row)
    assert torch.equal(st[:, 2], _patch_max(g.abs()))
    mx = _patch_max(xh.abs())
    assert bool(((st[:, 3] - mx).abs() <= 4 * EPS * mx).all())


@pytest.mark.parametrize("case", P.CASES, ids=_ids)
def test_patch_kernel_vs_fp64(case):
    c = case
    o = P.host_ops(c)
    r = P.run_case(c, o)                                       # (asserts the guards of every output)
    assert r["status"] == 0
    assert r["label"] == c.label
    dev = P.DEV if c in P.BIG else "cpu"
    want = P.device_want(c, o, r, dev)
    mask = P.compare_mask(c, want)
    got = r["got"].to(dev)
    assert bool(torch.isfinite(got[mask]).all())
    err = P.rel_err(got, want, mask)
    print(f"{c.kind} {c.name} [{c.label}]: err {err:.3e} (gate {P.gate(c):.0e})")
    assert err <= P.gate(c), err
    assert r["flag"] == (1 if c.overflow else 0)
    assert r["same"], "a second launch gave other bits"
    if c.n_store:
        if c.sq:
            wsq = P.want_sq(c, o, want)
            e_sq = float(((r["sq"].double() - wsq).abs() / wsq).max())
            print(f"{c.kind} {c.name}: squared error {e_sq:.3e} (gate {P.GATE_SQ:.0e}), sq_acc on entry {c.sq0}")
            assert e_sq <= P.GATE_SQ, e_sq
        else:                                                   # no target: sq_acc is not touched
            assert torch.equal(r["sq"], torch.full((c.B,), c.sq0))
    if c.pool:
        # S16 rounding is monotone, so the pooled output is EXACTLY the max-pool of the stored (fp64-checked) output
        assert torch.equal(r["pool"], F.max_pool2d(r["got"], 2))
    if c.stats:
        _check_stats(c, o, r)


def test_every_tap_instance_agrees_on_shared_operands():
    """the same activations and filter bank through all ten instances (patch_cases.SHARED): each within the gate of the
    k-half-major 128-filter instance's output (its leading images / filters), which test_patch_kernel_vs_fp64 ties to fp64
    at this very size (kh128-* cases)"""
    ref = None
    for c in P.SHARED:
        r = P.run_case(c, P.host_ops(c))
        assert r["status"] == 0 and r["label"] == c.label and r["same"]
        if ref is None:
            ref = r["got"]
            continue
        e = P.rel_err(r["got"], ref[:c.B, :P.out_channels(c)])
        print(f"shared {c.name} [{c.label}] against [{P.SHARED[0].label}]: {e:.3e}")
        assert e <= P.GATE_S16, (c.name, e)


@pytest.mark.parametrize("case", [c for c in P.CASES if c.kind == "outc" and c.label == P.OUTC], ids=_ids)
def test_outc_streaming_kernel_against_halo_patch_kernel(case):
    """the same descriptor with outc_stream = 1: frames equal to fp32 rounding of the sums (1e-6, as
    test_output_layer_streaming_kernel_vs_halo_patch_kernel), squared errors to 1e-5 of their value"""
    o = P.host_ops(case)
    a = P.run_case(case, o)
    tapc = replace(case, outc=P.TAPK, label=P.O4)
    b = P.run_case(tapc, o)
    assert a["label"] == P.OUTC and b["label"] == P.O4
    assert float((a["got"] - b["got"]).abs().max()) <= 1e-6
    if case.sq:
        assert float(((a["sq"] - b["sq"]).abs() / b["sq"]).max()) <= 1e-5
    else:
        assert torch.equal(a["sq"], b["sq"])


def test_entry_points_refuse_on_the_device_what_they_refuse_on_the_host():
    for what, got, want in P.first_refusals() + P.up_refusals():
        assert got == want, (what, got, want)
