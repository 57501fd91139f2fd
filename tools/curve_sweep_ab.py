"""What the curve sweep costs, inside ONE process on the MI355X, every leg on the same data:

1. `ops.curve_sweep` over the whole grid between device events, min / median / max over REPS repetitions after warm-up
   (all chunks of the grid, where the workspace limit splits it);
2. `ops.fusion_sweep` over the same grid, timed the same way: the pass whose integers the curve sweep repeats;
3. the numpy restatement of tests/curve_cases.py over the same grid, once, by the wall clock; the device's integers and
   thresholds are checked against it with ==, the sums within the header's bound.

Cases: the reference's 100 x 20 grid on the committed ped2 fixture (1962 scored frames) and on section 5.20's seeded
synthetic set of 40 000 scored frames.  Then the 100 x 20 launch against the two class sizes - a smaller class of 1
leaves the larger class's sort, its row and a trivial pass; equal classes add the second sort and the pass whose searches
go to the row in global memory: where a workgroup's time goes.

    python tools/curve_sweep_ab.py > profiles/curve_sweep_ab.txt
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import curve_cases as CC
import fusion_cases as FC
from fusion_sweep_ab import synthetic_records
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops

DEV = "cuda:0"
REPS = 20


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def timed(launch):
    for _ in range(3):
        launch()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        launch()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"reps": REPS, "ms_min": round(ms[0], 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_max": round(ms[-1], 4)}


def device_legs(chan, pos, neg, weights, smooth):
    d = (_up(chan, torch.float32), _up(pos, torch.int32), _up(neg, torch.int32), _up(weights, torch.float32),
         _up(smooth, torch.float32))
    g, s = len(weights), len(smooth)
    out = {"two_u": torch.empty(g, s, dtype=torch.int64, device=DEV), "pts": torch.empty(g, s, 4, dtype=torch.int32, device=DEV),
           "thr": torch.empty(g, s, 2, device=DEV), "sums": torch.empty(g, s, 2, dtype=torch.float64, device=DEV)}
    two_u = torch.empty(g, s, dtype=torch.int64, device=DEV)
    curve = timed(lambda: ops.curve_sweep(*d, out=out))
    fusion = timed(lambda: ops.fusion_sweep(*d, out=two_u))
    assert torch.equal(two_u, out["two_u"])
    row = _lib.load().ammc_curve_sweep_workspace_bytes(1, len(pos), len(neg))
    launches = -(-g // ((64 << 20) // row // s)) if (64 << 20) // row >= s else g * -(-s // ((64 << 20) // row))
    return {k: v.cpu().numpy() for k, v in out.items()}, curve, fusion, {"row_bytes": row, "launches": launches}


def case(name, rec, gt, channels=("rgb_img_pred", "rgb_fea_comm")):
    chan = Hn.fusion_channels(rec, channels)
    labels = np.concatenate([np.asarray(g)[Hn.DECIDABLE_IDX:] for g in gt])
    pos, neg = np.flatnonzero(labels == 0).astype(np.int32), np.flatnonzero(labels != 0).astype(np.int32)
    grid = Hn.fusion_grid(len(channels))
    weights, smooth = grid["weights"], grid["smooth"]
    got, curve, fusion, ws = device_legs(chan, pos, neg, weights, smooth)
    CC.curve_point(FC.scores(chan, weights[0], *smooth[0]), pos, neg)          # (first-call costs stay out of the timed loop)
    t0 = time.perf_counter()
    want = CC.curve_grid(chan, weights, smooth, pos, neg)
    host_s = time.perf_counter() - t0
    P, Q = len(pos), len(neg)
    for k in ("two_u", "pts", "thr"):
        assert np.array_equal(got[k], want[k]), k
    err = float(np.abs(got["sums"] / P - want["sums"] / P).max())
    assert err <= CC.gate(P), err
    m = Hn.curve_metrics(got["two_u"], got["pts"], got["thr"], got["sums"], P, Q)
    points = got["two_u"].size
    row = {"case": name, "channels": list(channels), "scored_frames": int(chan.shape[1]), "n_pos": P, "n_neg": Q,
           "grid": [len(weights), len(smooth)], "curve_sweep": curve, "fusion_sweep": fusion, **ws,
           "curve_over_fusion": round(curve["ms_median"] / fusion["ms_median"], 2),
           "curve_us_per_point": round(1e3 * curve["ms_median"] / points, 4), "restatement_loop_s": round(host_s, 3),
           "restatement_ms_per_point": round(1e3 * host_s / points, 4),
           "restatement_over_device": round(1e3 * host_s / curve["ms_median"], 1), "integers_and_thresholds": "equal",
           "max_sum_difference_over_p": err, "bound": CC.gate(P), "auc_best": float(m["auc"].max()), "eer_best": float(m["eer"].min()),
           "ap_best": float(m["ap"].max()), "pr_auc_at_ap_best": float(m["pr_auc"].ravel()[np.argmax(m["ap"])])}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def class_size_scan(sizes=(1024, 4096, 8192, 16384, 32768)):
    """the 100 x 20 launch at two channels against (larger class, smaller class): the smaller class 1, then equal"""
    grid = Hn.fusion_grid(2)
    rows = []
    for big in sizes:
        for small in (1, big):
            c = FC.synthetic(big + small, 2, m=small, small="neg")
            got, curve, fusion, ws = device_legs(c["chan"], c["pos"], c["neg"], grid["weights"], grid["smooth"])
            g, s = 37, 11
            want = CC.curve_point(FC.scores(c["chan"], grid["weights"][g], *grid["smooth"][s]), c["pos"], c["neg"])
            assert np.array_equal(got["pts"][g, s], want["pts"]) and np.array_equal(got["thr"][g, s], want["thr"])
            pad = 1 << (big - 1).bit_length()
            rows.append({"larger": big, "smaller": small, "threads": 256 if pad <= 4096 else 1024, "lds_bytes": max(4 * pad, 16) + 400,
                         **ws, "curve_sweep": curve, "fusion_sweep": fusion})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def main() -> None:
    fx = FC.fixture()
    rec, gt = synthetic_records()
    out = {"device": torch.cuda.get_device_name(0), "source_digests": _lib.load().ammc_source_digests().decode(),
           "max_class": ops.CURVE_MAX_CLASS,
           "cases": [case("ped2 fixture, reference grid", fx["records"], fx["gt"]),
                     case("synthetic 40000 frames, reference grid", rec, gt)],
           "class_size_scan": class_size_scan()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
