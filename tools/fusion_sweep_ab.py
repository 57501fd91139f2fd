"""What the score-fusion sweep costs against the host loop it replaces, inside ONE call on the
MI355X, both legs on the same data:

1. device: the one launch of `ammc_fusion_sweep_f32` over the whole grid between device events, min / median / max over
   REPS repetitions after warm-up (the inputs are resident: uploading them is a few hundred KB once per sweep);
2. host: one pass of the loop the launch replaces, timed with the wall clock - at two channels `harness.fuse_scores_auc`
   per grid point (the project's existing fusion: normalisation, fused score, smoothing, ROC), at four channels the
   numpy restatement of tests/fusion_cases.py per grid point (fused score, smoothing, sort, two searches) on the already
   normalised channels.  The device's integers are checked against the host's results on the way.

Cases: the reference's 100 x 20 grid on the committed ped2 fixture (1962 scored frames), and a seeded synthetic set of
40 000 scored frames (20 videos) at two channels (100 x 20) and four channels (286 x 20).  Then, at 40 000 frames and two
channels, the launch against the size of the sorted class: where a workgroup's time goes.

    python tools/fusion_sweep_ab.py > profiles/fusion_sweep_ab.txt
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fusion_cases as FC
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops

DEV = "cuda:0"
REPS = 20


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def device_leg(chan, pos, neg, weights, smooth):
    d = (_up(chan, torch.float32), _up(pos, torch.int32), _up(neg, torch.int32), _up(weights, torch.float32),
         _up(smooth, torch.float32))
    out = torch.empty(len(weights), len(smooth), dtype=torch.int64, device=DEV)
    for _ in range(3):
        ops.fusion_sweep(*d, out=out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        ops.fusion_sweep(*d, out=out)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return out.cpu().numpy(), {"reps": REPS, "ms_min": round(ms[0], 4), "ms_median": round(ms[len(ms) // 2], 4),
                               "ms_max": round(ms[-1], 4)}


def synthetic_records(videos=20, frames=2004, seed=0):
    """records with the fixture's structure: a PSNR-like and a commit-like record per video, labels correlated with both"""
    rng = np.random.default_rng(seed)
    rec = {"dataset": "ped2", "rgb_img_pred_records": [], "rgb_fea_comm_records": [], "op_img_pred_records": [],
           "op_fea_comm_records": []}
    gt = []
    for _ in range(videos):
        anomalous = np.zeros(frames, dtype=np.int8)
        for start in rng.choice(frames - 120, size=6, replace=False):
            anomalous[start:start + int(rng.integers(30, 120))] = 1
        for st in ("rgb", "op"):
            rec[f"{st}_img_pred_records"].append((36.0 - 3.0 * anomalous + rng.normal(0, 1.5, frames)).astype(np.float32))
            rec[f"{st}_fea_comm_records"].append((1e-3 * (1.0 + 0.8 * anomalous + rng.normal(0, 0.4, frames)) ** 2).astype(np.float32))
        gt.append(anomalous)
    return rec, gt


def case(name, rec, gt, channels):
    k = len(channels)
    chan = Hn.fusion_channels(rec, channels)
    labels = np.concatenate([np.asarray(g)[Hn.DECIDABLE_IDX:] for g in gt])
    pos, neg = np.flatnonzero(labels == 0).astype(np.int32), np.flatnonzero(labels != 0).astype(np.int32)
    grid = Hn.fusion_grid(k)
    weights, smooth = grid["weights"], grid["smooth"]
    two_u, dev = device_leg(chan, pos, neg, weights, smooth)
    denom = 2.0 * len(pos) * len(neg)
    Hn.fuse_scores_auc(rec, gt, (0.5, 0.5))                 # (first-call costs stay out of the timed loop)
    t0 = time.perf_counter()
    if k == 2:
        host = np.array([[Hn.fuse_scores_auc(rec, gt, (l1, l2))["auc_raw"] for l2 in grid["lam_smooth"]] for l1 in grid["lam_fea"]])
        yardstick = "harness.fuse_scores_auc per grid point"
    else:
        host = FC.two_u_grid(chan, weights, smooth, pos, neg)
        yardstick = "numpy restatement (tests/fusion_cases.py) per grid point"
    host_s = time.perf_counter() - t0
    if k == 2:
        agree = float(np.abs(two_u / denom - host).max())
        assert agree <= 1e-12, agree
    else:
        agree = int(np.abs(two_u - host).max())
        assert agree == 0
    auc = two_u / denom
    row = {"case": name, "channels": list(channels), "scored_frames": int(chan.shape[1]), "n_pos": len(pos), "n_neg": len(neg),
           "grid": [len(weights), len(smooth)], "device": dev, "host_yardstick": yardstick, "host_loop_s": round(host_s, 3),
           "host_ms_per_point": round(1e3 * host_s / auc.size, 4), "device_us_per_point": round(1e3 * dev["ms_median"] / auc.size, 4),
           "host_over_device": round(1e3 * host_s / dev["ms_median"], 1), "max_disagreement": agree,
           "auc_best": float(auc.max()), "auc_first_point": float(auc[0, 0])}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def sorted_size_scan(n=40000, sizes=(1, 1024, 4096, 4097, 8192, 16384, 20000)):
    """the 100 x 20 launch at n frames and two channels against the size of the sorted class: m = 1 leaves the keys of
    the n - 1 other frames and a trivial search; the growth from there is the sort and the deeper searches"""
    grid = Hn.fusion_grid(2)
    rows = []
    for m in sizes:
        c = FC.synthetic(n, 2, m=m, small="neg")
        two_u, dev = device_leg(c["chan"], c["pos"], c["neg"], grid["weights"], grid["smooth"])
        g, s = 37, 11
        assert two_u[g, s] == FC.two_u_point(FC.scores(c["chan"], grid["weights"][g], *grid["smooth"][s]), c["pos"], c["neg"])
        mpad = 1 << max(m - 1, 0).bit_length()
        rows.append({"frames": n, "sorted": m, "padded": mpad, "threads": 256 if mpad <= 4096 else 1024, "lds_bytes": max(4 * mpad, 128),
                     "sort_stages": (mpad.bit_length() - 1) * mpad.bit_length() // 2, **dev})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def main() -> None:
    fx = FC.fixture()
    rec, gt = synthetic_records()
    out = {"device": torch.cuda.get_device_name(0), "source_digests": _lib.load().ammc_source_digests().decode(),
           "max_sorted": ops.FUSION_MAX_SORTED,
           "cases": [case("ped2 fixture, reference grid", fx["records"], fx["gt"], ("rgb_img_pred", "rgb_fea_comm")),
                     case("synthetic 40000 frames, reference grid", rec, gt, ("rgb_img_pred", "rgb_fea_comm")),
                     case("synthetic 40000 frames, four channels, simplex step 0.1", rec, gt,
                          ("rgb_img_pred", "rgb_fea_comm", "op_img_pred", "op_fea_comm"))],
           "sorted_size_scan": sorted_size_scan()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
