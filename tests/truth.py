"""The fp64 TRUTH of a training step on the branch the evaluation under test took - the one gradient gate of this repo.

Test infrastructure (imported by tests/ and by bench.py's parity blocks only; like everything under oracle/ it is the
checker, never the thing measured or shipped).

Why "same branch" (tools/flip_count.py, tools/grad_truth.py): the training step of the path is piecewise
smooth and its one violent discontinuity is the memory lookup (`Quantize_topk`, models/unet.py:282-297).  ONE top-2
lookup whose two candidate slots tie within fp32 resolution falling the other way moves every gradient downstream by
~1e-2 - for ANY fp32 evaluation, the reference's own included.  Distances between two fp32 evaluations (the 1e-2 max /
2e-3 median envelopes the tests of rounds 2-5 were fitted to) therefore gate nothing.  Here every evaluation E is
compared with the oracle in FLOAT64 taking the lookups E itself made (`oracle.quantize_topk(force_idx=...)`) and, where E
records them (the HIP training engine's default path does), the routes of its max-pools (`oracle.maxpool2x2_forced`: a 2x2
window whose two largest values tie inside rounding noise is the second discontinuity), so that what is left is E's
arithmetic plus the handful of ReLU masks that flip inside fp32 noise.

The gates ("gradients rel <= 1e-3 per tensor").  e_ref / norm_ref: what the REFERENCE's own fp32
arithmetic is away from the truth on ITS branch - from the dense samples and lookups the reference recorded in a fixture
(`ref=`, tests/golden/make_golden.py) or, where no fixture of the case exists, from the oracle's fp32 evaluation on the
host (pinned to the reference <= 1e-6 by tests/test_oracle_golden.py).

mode "timed_batch" (batch >= 16: the batches bench.py times; a tensor's error is the sum of tens of flipped masks):
  * the norm of every gradient tensor within 1e-3 of the truth's;
  * entry by entry (L2 over the tensor): e(n) <= max(1e-3, 2 e_ref(n)) for EVERY tensor n;
  * the median over tensors of e / e_ref <= 1.5 (tensors with e_ref > 5e-4).
mode "small_batch" (the batch-2 / batch-4 fixtures): here a tensor's error is ZERO TO THREE flipped ReLU masks (one flip
  at the 8x8 bottleneck of a 64x64 batch-2 step moves a 512-entry BatchNorm gradient by 4e-3), so the ratio of two
  evaluations' errors on one tensor is a ratio of two tiny Poisson counts: tools/truth_survey.py (profiles/
  r06_truth_survey.txt) has the oracle's fp32 evaluation on the device (MIOpen) FAIL the per-tensor gate against the
  oracle's fp32 evaluation on the host (oneDNN) and vice versa on every batch-2 fixture, with per-tensor ratios up to 9
  and norm errors of the witnesses themselves up to 1.2e-3.  What is stable is the envelope: with E = the worst tensor of
  two fp32 witnesses (the reference / host oracle, and the oracle on the device),
  * every tensor's norm error <= max(1e-3, 2 E_norm), every tensor's e <= max(1e-3, 2 E_e);
  * the median over tensors of e <= max(1e-3, 2 x the witnesses' larger median).
  The per-tensor ARITHMETIC gate at these sizes is the mask-free fixture of tests/test_gpu_train.py (no ReLU can flip:
  1e-4 against fp64 per tensor, every frame size the small fixtures use).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import ammc_oracle as O  # noqa: E402

NORM_TOL = 1e-3
L2_FLOOR = 1e-3
L2_FACTOR = 2.0
RATIO_MEDIAN = 1.5
DENSE = 4096


def l2rel(a, b) -> float:
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def dense(g: torch.Tensor, n: int = DENSE) -> torch.Tensor:
    """the sample positions of `gs4k.*` / `ggs4k.*` / `dgs4k.*` (make_golden.py) and `gs64*.*` (make_fp64_truth.py)"""
    return g.flatten()[:: max(1, g.numel() // n)][:n].contiguous()


def hip_lookups(net) -> dict:
    """The branch the HIP training forward just took: the memory lookups {"rgb": int64 [N, k], "op": ...} and - where the
    engine records them (the split-fp16 training path: one byte per pooled element, `_Stream.pool_idx`) - the routes
    of its max-pools, "pool": {"rgb.down1": int64 [B, C, h, w] in 0..3, ...} (oracle.maxpool2x2_forced)."""
    st = net._train_engine._last
    out = {p: st["streams"][si].idx.reshape(-1, 2).long().clone() for si, p in enumerate(("rgb", "op"))}
    pools = {}
    for si, p in enumerate(("rgb", "op")):
        stream = st["streams"][si]
        pi = getattr(stream, "pool_idx", None)
        if pi:
            for lvl, t in enumerate(pi):
                pools[f"{p}.down{lvl + 1}"] = t.permute(0, 3, 1, 2).long().contiguous()       # [B, h, w, C] bytes -> [B, C, h, w]
        elif not getattr(stream, "twins", True):
            # exact-fp32 training path: no recorded routes, but the fp32 skip tensors the pooling read are still in the
            # workspace - their first maxima (row-major, what `ammc_maxpool2x2_bwd_f32` routes to) are the routes taken
            for lvl in range(3):
                sk = stream.skip[lvl]
                pools[f"{p}.down{lvl + 1}"] = O.maxpool2x2_routes(sk.interior().permute(0, 3, 1, 2).float())[1]
    if pools:
        out["pool"] = pools
    return out


def branch_to(idx: dict, device="cpu") -> dict:
    """a branch (lookups + pool routes) moved to `device` (ranks exchange theirs through all_gather_object)"""
    return {k: ({kk: vv.to(device) for kk, vv in v.items()} if isinstance(v, dict) else v.to(device)) for k, v in idx.items()}


def cat_branches(parts: list) -> dict:
    """the branch of ONE step on the concatenated batch from the branches of its shards (rank order = batch order)"""
    out = {p: torch.cat([e[p] for e in parts]) for p in ("rgb", "op")}
    if all("pool" in e for e in parts):
        out["pool"] = {k: torch.cat([e["pool"][k] for e in parts]) for k in parts[0]["pool"]}
    return out


def _cast(sd, dtype, device, requires_grad):
    return O.clone_state({k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device))
                          for k, v in sd.items()}, requires_grad=requires_grad)


def g_step(sd, clips, dtype, device, force_idx=None, loss_scale: float = 1.0):
    """One generator-only step of the oracle (forward in training mode, `generator_loss`, autograd).
    -> (loss, {name: grad}, {"rgb": idx [N, k], "op": idx}, state after the forward: BatchNorm / EMA buffers updated)"""
    rgb_x, op_x, rgb_t, op_t = (t.to(device=device, dtype=dtype) for t in clips)
    m = _cast(sd, dtype, device, True)
    out = O.twostream_forward(m, rgb_x, op_x, 2, training=True, want_aux=True, force_idx=force_idx)
    loss = O.generator_loss(out, rgb_t, op_t)
    (loss * loss_scale).backward()
    grads = {k: v.grad.detach() for k, v in m.items() if v.requires_grad}
    return float(loss.detach()), grads, _branch(out[-1]), m


def _branch(aux: dict) -> dict:
    """the branch an oracle evaluation took, in the structure it accepts as `force_idx`"""
    idx = {p: aux[f"{p}.idx"].reshape(-1, 2).detach() for p in ("rgb", "op")}
    idx["pool"] = {k: v.detach() for k, v in aux["pool"].items()}
    return idx


def gan_step(sd_g, sd_d, sd_f, clips, lams, dtype, device, force_idx=None):
    """One joint G / D iteration of the reference's loop (run_helper/train_helper.py:296-339) in the oracle: G forward,
    FlowNet2-SD on (target, prediction.detach()) and (target, target) - `rgb_input_last` IS the target frame, :299 -,
    D(prediction) for the adversarial term, `Twostream_vq_Loss` (loss_zoo.py:323-336), `Discriminate_Loss` on
    (D(target), D(prediction.detach())).  -> dict(g_loss, d_loss, g = {name: dL_g/dparam of G}, d = {name: dL_d/dparam of D}, idx)"""
    rgb_x, op_x, rgb_t, op_t = (t.to(device=device, dtype=dtype) for t in clips)
    mg = _cast(sd_g, dtype, device, True)
    md = _cast(sd_d, dtype, device, True)
    out = O.twostream_forward(mg, rgb_x, op_x, 2, training=True, want_aux=True, force_idx=force_idx)
    rgb_out = out[0]
    fp = fg = None
    if sd_f is not None:
        mf = _cast(sd_f, dtype, device, False)
        with torch.no_grad():
            def flow(cur):
                pair = torch.cat([rgb_t.unsqueeze(2), cur.unsqueeze(2)], 2)
                return O.flownet2sd_forward(mf, (pair * 0.5 + 0.5) * 255.0) / 255.0
            fp, fg = flow(rgb_out.detach()), flow(rgb_t)
        del mf
    d_gen = O.pixel_discriminator(md, rgb_out)
    g_loss = O.generator_loss_full(out, rgb_t, op_t, d_gen, fp, fg, **lams)
    d_loss = O.discriminate_loss(O.pixel_discriminator(md, rgb_t), O.pixel_discriminator(md, rgb_out.detach()))
    dn = [k for k, v in md.items() if v.requires_grad]
    gn = [k for k, v in mg.items() if v.requires_grad]
    dg = torch.autograd.grad(d_loss, [md[k] for k in dn])
    gg = torch.autograd.grad(g_loss, [mg[k] for k in gn])
    return dict(g_loss=float(g_loss.detach()), d_loss=float(d_loss.detach()), g=dict(zip(gn, gg)), d=dict(zip(dn, dg)),
                idx=_branch(out[-1]))


def reference_errors(ref_samples: dict, ref_norms: dict, truth_on_ref_branch: dict):
    """e_ref / norm_ref per tensor from reference-recorded dense samples (`*gs4k.*`) and norms (`*gn.*`) against the
    truth evaluated with the reference's recorded lookups"""
    e, nrm = {}, {}
    for n, t in truth_on_ref_branch.items():
        e[n] = l2rel(ref_samples[n], dense(t))
        n64 = float(t.double().norm())
        nrm[n] = abs(float(ref_norms[n]) - n64) / max(n64, 1e-300)
    return e, nrm


def witness_errors(witness: dict, truth_on_witness_branch: dict):
    """the same from whole tensors of a live fp32 evaluation (the oracle on the host or on the device)"""
    e, nrm = {}, {}
    for n, t in truth_on_witness_branch.items():
        e[n] = l2rel(witness[n], t)
        n64 = float(t.double().norm())
        nrm[n] = abs(float(witness[n].double().norm()) - n64) / max(n64, 1e-300)
    return e, nrm


def _stat(vals):
    v = sorted(vals)
    return {"max": v[-1], "median": v[len(v) // 2]} if v else None


def verdict(g_hip: dict, truth: dict, refs: list, mode: str = "timed_batch", what: str = "") -> dict:
    """The gates of this module's header for one set of gradients.  `g_hip`, `truth`: {name: tensor}, the truth evaluated
    on g_hip's branch; `refs`: [(e_ref {name: float}, norm_ref {name: float}), ...] - the reference's own errors first,
    further fp32 witnesses behind it (small_batch)."""
    assert mode in ("timed_batch", "small_batch") and refs
    e_ref, norm_ref = refs[0]
    rows = []
    for n, g in g_hip.items():
        t = truth[n]
        n64 = float(t.double().norm())
        rows.append(dict(name=n, e=l2rel(g, t), norm=abs(float(g.double().norm()) - n64) / max(n64, 1e-300),
                         e_ref=float(e_ref[n]), norm_ref=float(norm_ref[n])))
    ratios = sorted(r["e"] / r["e_ref"] for r in rows if r["e_ref"] > 5e-4)
    med_ratio = ratios[len(ratios) // 2] if len(ratios) >= 10 else None
    med_e = _stat([r["e"] for r in rows])["median"]
    if mode == "timed_batch":
        lim_norm = lambda r: NORM_TOL                                                   # noqa: E731
        lim_e = lambda r: max(L2_FLOOR, L2_FACTOR * r["e_ref"])                         # noqa: E731
        ok_med = med_ratio is None or med_ratio <= RATIO_MEDIAN
        gates = {"grad_norm_rel": NORM_TOL, "grad_l2_rel": f"max({L2_FLOOR}, {L2_FACTOR} x reference), per tensor",
                 "ratio_median": RATIO_MEDIAN}
    else:
        env_norm = max(max(nr.values()) for _, nr in refs)
        env_e = max(max(er.values()) for er, _ in refs)
        env_med = max(_stat(list(er.values()))["median"] for er, _ in refs)
        lim_norm = lambda r: max(NORM_TOL, L2_FACTOR * env_norm)                        # noqa: E731
        lim_e = lambda r: max(L2_FLOOR, L2_FACTOR * env_e)                              # noqa: E731
        ok_med = med_e <= max(L2_FLOOR, L2_FACTOR * env_med)
        gates = {"grad_norm_rel": max(NORM_TOL, L2_FACTOR * env_norm), "grad_l2_rel": max(L2_FLOOR, L2_FACTOR * env_e),
                 "grad_l2_rel_median": max(L2_FLOOR, L2_FACTOR * env_med),
                 "from": f"max(1e-3, {L2_FACTOR} x the worst tensor of {len(refs)} fp32 witnesses on their own branches)"}
    bad = [r for r in rows if r["norm"] > lim_norm(r) or r["e"] > lim_e(r)]
    worst = sorted(rows, key=lambda r: -max(r["norm"] / lim_norm(r), r["e"] / lim_e(r)))[:3]

    def fmt(r):
        return f"{r['name']} e {r['e']:.2e} (ref {r['e_ref']:.2e}) norm {r['norm']:.2e} (ref {r['norm_ref']:.2e})"
    return {"what": what, "mode": mode, "tensors": len(rows),
            "grad_norm_rel": _stat([r["norm"] for r in rows]), "grad_l2_rel": _stat([r["e"] for r in rows]),
            "reference_grad_norm_rel": _stat([r["norm_ref"] for r in rows]), "reference_grad_l2_rel": _stat([r["e_ref"] for r in rows]),
            "witnesses": [{"grad_norm_rel": _stat(list(nr.values())), "grad_l2_rel": _stat(list(er.values()))} for er, nr in refs],
            "ratio_over_reference": {"median": med_ratio, "max": ratios[-1]} if med_ratio is not None else None,
            "gates": gates, "worst": [fmt(r) for r in worst], "failing": [fmt(r) for r in bad],
            "ok": bool(not bad and ok_med)}


def assert_ok(v: dict) -> None:
    assert v["ok"], {k: v[k] for k in ("what", "mode", "failing", "gates", "ratio_over_reference", "grad_norm_rel", "grad_l2_rel", "witnesses")}


def same_branch_verdict(step, g_hip: dict, idx_hip, device, mode: str, ref=None, what: str = "") -> dict:
    """`step(dtype, device, force_idx) -> ({name: grad}, idx)`: one evaluation of the oracle's step (idx: whatever
    structure `step` itself accepts as `force_idx`).  The truth on the HIP branch; the reference's own error from a
    fixture (`ref = (samples {name: array at the dense positions}, norms {name: float}, idx)`) or from the oracle's fp32
    evaluation on the host; in small_batch mode a second witness, the oracle in fp32 on the device."""
    refs = []
    if ref is not None:
        smp, nrm, ridx = ref
        t_ref, _ = step(torch.float64, device, ridx)
        refs.append(reference_errors(smp, nrm, t_ref))
    else:
        w, widx = step(torch.float32, "cpu", None)
        t_ref, _ = step(torch.float64, device, widx)
        refs.append(witness_errors(w, t_ref))
    del t_ref
    if mode == "small_batch":
        w, widx = step(torch.float32, device, None)
        t_w, _ = step(torch.float64, device, widx)
        refs.append(witness_errors(w, t_w))
        del t_w, w
    t_hip, _ = step(torch.float64, device, idx_hip)
    return verdict(g_hip, t_hip, refs, mode, what)


def g_stepper(sd, clips):
    """`step` of `same_branch_verdict` for a generator-only step on one batch"""
    def step(dtype, device, force_idx):
        _, g, idx, _ = g_step(sd, clips, dtype, device, force_idx=force_idx)
        return g, idx
    return step


def gan_stepper(sd_g, sd_d, sd_f, clips, lams):
    """... for the joint G / D iteration: gradients of both networks in one dict ("G." / "D." prefixes)"""
    def step(dtype, device, force_idx):
        r = gan_step(sd_g, sd_d, sd_f, clips, lams, dtype, device, force_idx=force_idx)
        g = {"G." + n: v for n, v in r["g"].items()}
        g.update({"D." + n: v for n, v in r["d"].items()})
        return g, r["idx"]
    return step


def fixture_idx(d, prefix="idx.") -> dict:
    return {p: torch.as_tensor(np.asarray(d[f"{prefix}{p}"]).astype(np.int64)) for p in ("rgb", "op")}
