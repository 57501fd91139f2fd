"""What the per-video pair counts and their bootstrap form cost, inside ONE process on the
MI355X, every leg on the same data:

1. `ops.video_pairs` over the whole grid, and `ops.bootstrap_pairs` over its blocks with REPLICAS multiplicity rows, each
   between device events: median (min - max) of REPS launches after warm-up, the inputs resident;
2. `ops.fusion_sweep` over the same grid, timed the same way: what the split by video costs over the pooled count;
3. the numpy restatement of tests/video_cases.py on one host thread (`pairs_searchsorted` per grid point, `bootstrap_brute`
   per block), timed once with the wall clock over the first HOST_POINTS grid points of the weight row 37 - a whole grid
   on the host would take minutes - and scaled to the grid; its integers are checked against the device's on the way,
   and the device's block sums against `ops.fusion_sweep` over the whole grid.

Cases: the reference's 100 x 20 grid on the committed ped2 fixture (12 videos, 1962 scored frames) and on seeded synthetic
records of about 40 000 scored frames in 21 and in 107 videos.

    python tools/video_pairs_ab.py > profiles/video_pairs_ab.txt
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

import fusion_cases as FC
import video_cases as VC
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops
from fusion_sweep_ab import synthetic_records

DEV = "cuda:0"
REPS = 20
REPLICAS = 1000
HOST_POINTS = 10


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def timed(fn):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"reps": REPS, "ms_min": round(ms[0], 4), "ms_median": round(ms[len(ms) // 2], 4), "ms_max": round(ms[-1], 4)}


def case(name, rec, gt):
    chan = Hn.fusion_channels(rec, ("rgb_img_pred", "rgb_fea_comm"))
    labels = np.concatenate([np.asarray(g)[Hn.DECIDABLE_IDX:] for g in gt])
    pos, neg = np.flatnonzero(labels == 0).astype(np.int32), np.flatnonzero(labels != 0).astype(np.int32)
    vo = Hn.video_offsets(gt, 0)
    V = len(gt)
    grid = Hn.fusion_grid(2)
    weights, smooth = grid["weights"], grid["smooth"]
    G, S = len(weights), len(smooth)
    mult = Hn.bootstrap_multiplicities(V, REPLICAS, 0)
    d = (_up(chan, torch.float32), _up(pos, torch.int32), _up(neg, torch.int32))
    d_off = (_up(vo["pos_off"], torch.int32), _up(vo["neg_off"], torch.int32))
    d_grid = (_up(weights, torch.float32), _up(smooth, torch.float32))
    d_mult = _up(mult, torch.int32)
    blocks = torch.empty(G, S, V, V, dtype=torch.int64, device=DEV)
    table = torch.empty(REPLICAS, G * S, dtype=torch.int64, device=DEV)
    two_u = torch.empty(G, S, dtype=torch.int64, device=DEV)
    t_pairs = timed(lambda: ops.video_pairs(*d, *d_off, *d_grid, out=blocks))
    t_boot = timed(lambda: ops.bootstrap_pairs(blocks.view(-1, V, V), d_mult, out=table))
    t_pool = timed(lambda: ops.fusion_sweep(*d, *d_grid, out=two_u))
    h_blocks, h_table = blocks.cpu().numpy(), table.cpu().numpy()
    assert np.array_equal(h_blocks.sum((2, 3)), two_u.cpu().numpy())

    g = 37
    t0 = time.perf_counter()
    host = [VC.pairs_searchsorted(FC.scores(chan, weights[g], *smooth[s]), pos, neg, vo["pos_off"], vo["neg_off"])
            for s in range(HOST_POINTS)]
    host_pairs_s = time.perf_counter() - t0
    assert np.array_equal(np.array(host), h_blocks[g, :HOST_POINTS])
    t0 = time.perf_counter()
    host_table = VC.bootstrap_brute(np.array(host), mult)
    host_boot_s = time.perf_counter() - t0
    assert np.array_equal(host_table, h_table[:, g * S:g * S + HOST_POINTS])

    seg = int(np.diff(vo["neg_off"] if len(neg) <= len(pos) else vo["pos_off"]).max())
    row = {"case": name, "videos": V, "scored_frames": int(chan.shape[1]), "n_pos": len(pos), "n_neg": len(neg), "grid": [G, S],
           "replicas": REPLICAS, "longest_sorted_segment": seg, "blocks_bytes": int(blocks.numel() * 8),
           "video_pairs": t_pairs, "bootstrap_pairs": t_boot, "fusion_sweep": t_pool,
           "video_pairs_over_fusion_sweep": round(t_pairs["ms_median"] / t_pool["ms_median"], 2),
           "host_points": HOST_POINTS, "host_pairs_ms_per_point": round(1e3 * host_pairs_s / HOST_POINTS, 3),
           "host_boot_ms_per_point": round(1e3 * host_boot_s / HOST_POINTS, 3),
           "host_pairs_s_per_grid_scaled": round(host_pairs_s / HOST_POINTS * G * S, 2),
           "host_boot_s_per_grid_scaled": round(host_boot_s / HOST_POINTS * G * S, 2),
           "host_over_device_pairs": round(1e3 * host_pairs_s / HOST_POINTS * G * S / t_pairs["ms_median"], 1),
           "host_over_device_boot": round(1e3 * host_boot_s / HOST_POINTS * G * S / t_boot["ms_median"], 1)}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main() -> None:
    fx = FC.fixture()
    out = {"device": torch.cuda.get_device_name(0), "source_digests": _lib.load().ammc_source_digests().decode(),
           "max_segment": ops.VIDEO_PAIRS_MAX_SEGMENT, "max_videos": ops.VIDEO_PAIRS_MAX_VIDEOS,
           "cases": [case("ped2 fixture, reference grid", fx["records"], fx["gt"]),
                     case("synthetic 40000 frames in 21 videos, reference grid", *synthetic_records(videos=21, frames=1909)),
                     case("synthetic 40000 frames in 107 videos, reference grid", *synthetic_records(videos=107, frames=378))]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
