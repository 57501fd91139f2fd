"""What the region-based pass costs on the MI355X.  Two steps, each a child process of its own
under its own time limit; the parent never opens the GPU and stops at the first step that fails:

  launches  (a) the launches of `ops.region_scores` (one per chunk of thresholds under its workspace budget) between
            device events at batch 16 and 64 thresholds, for 256x256 maps (the pixel map) and 16x16 maps (the patch-16
            map): smooth random maps with about 10, 100 and 1000 components per frame (fewer on the small map), three
            rectangles of ground truth per frame; median and min..max of REPS repetitions after warm-up; and the one
            launch of `ops.label_regions` on the same masks;
            (b) beside it the host restatement (tests/region_cases.py: flood fill, a loop over components and regions)
            on the same tensors - on HOST_SAMPLES x HOST_THRESHOLDS of the 16 x 64 pairs at 256x256, all pairs at
            16x16 - with equality of all four outputs checked before anything is timed;
  loop      (c) frames/s of `harness.evaluate_dataset_region` against `harness.evaluate_dataset_pixel` on run_test's
            synthetic set, the two alternating three times.

    python tools/region_scores_ab.py [videos] [frames] > profiles/region_scores_ab.txt
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
B, T = 16, 64
REPS = 100
HOST_SAMPLES, HOST_THRESHOLDS = 1, 4                           # of the 256x256 case: a labelling takes the host ~0.1 s
STEP_LIMITS = {"launches": 420, "loop": 420}                   # seconds, per child process
KEYS = ("n_px", "n_comp", "n_fp", "hit")


def _timed(torch, call) -> list:
    for _ in range(10):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)


def _us(ms: list) -> dict:
    return {"us_median": round(ms[len(ms) // 2] * 1e3, 2), "us_min": round(ms[0] * 1e3, 2), "us_max": round(ms[-1] * 1e3, 2)}


def step_launches() -> dict:
    import numpy as np
    import torch
    import region_cases as RC
    from ammcnet_aaai2021_amd import _lib, harness as Hn, ops
    lib = _lib.load()
    values = Hn.region_thresholds(T)
    rows = []
    for hw, cells in ((256, (28, 9, 3)), (16, (8, 3, 1))):
        masks = RC.rectangles(B, hw, hw, 3, seed=hw)
        d_mask = torch.tensor(masks, device=DEV)
        lab = ops.label_regions(d_mask)
        want_lab = [RC.label_regions(m) for m in masks]
        assert np.array_equal(lab["labels"].cpu().numpy(), np.stack([l for l, _ in want_lab]))
        assert lab["count"].tolist() == [c for _, c in want_lab]
        row = {"pass": "ops.label_regions", "batch": B, "size": hw, "reps": REPS, **_us(_timed(torch, lambda: ops.label_regions(d_mask, out=lab)))}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        for cell in cells:
            maps = RC.smooth_maps(B, hw, hw, cell, seed=cell)
            d_map = torch.tensor(maps, device=DEV)
            thr = values * np.float32(maps.max())
            d_thr = torch.tensor(thr, device=DEV)
            out = ops.region_scores(d_map, lab["labels"], d_thr)
            got = {k: out[k].cpu().numpy() for k in KEYS}
            assert int(got["n_comp"].min()) >= 0
            ns, nt = (HOST_SAMPLES, HOST_THRESHOLDS) if hw == 256 else (B, T)
            cols = np.linspace(0, T - 1, nt).round().astype(int)
            t0 = time.perf_counter()
            want = RC.batch_scores(maps[:ns], [l for l, _ in want_lab[:ns]], thr[cols])
            host_s = time.perf_counter() - t0
            agree = all(np.array_equal(got[k][:ns][:, cols], want[k]) for k in KEYS)
            assert agree, (hw, cell)
            ms = _timed(torch, lambda: ops.region_scores(d_map, lab["labels"], d_thr, out=out))
            per_t = lib.ammc_region_workspace_bytes(B, 1, hw, hw)
            row = {"pass": "ops.region_scores", "batch": B, "thresholds": T, "size": hw, "cell": cell,
                   "components_per_frame_at_the_middle_threshold": round(float(got["n_comp"][:, T // 2].mean()), 1),
                   "components_per_frame_largest_over_thresholds": round(float(got["n_comp"].mean(axis=0).max()), 1),
                   "launches_per_call": -(-T // max(1, min(T, ops.REGION_WORKSPACE_BUDGET // per_t))), "reps": REPS, **_us(ms),
                   "host_restatement_pairs": ns * nt, "host_restatement_s": round(host_s, 3),
                   "host_restatement_us_per_pair": round(host_s / (ns * nt) * 1e6, 1),
                   "device_us_per_pair": round(ms[len(ms) // 2] * 1e3 / (B * T), 3), "agrees_with_restatement": agree}
            print(json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
    return {"device": torch.cuda.get_device_name(0), "source_digests": lib.ammc_source_digests().decode(), "launches": rows}


def step_loop(n_videos: int, frames: int) -> dict:
    import torch
    import ammcnet_aaai2021_amd as A
    from ammcnet_aaai2021_amd import harness as Hn, run_region, run_test, synthetic as S
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state())
    model = model.to(DEV).eval()
    model.precision = "s16"
    videos, _ = run_test.synthetic_dataset(n_videos, frames, 256)
    masks = run_region.synthetic_region_masks(n_videos, frames, 256, 256)
    values = Hn.region_thresholds(T)
    n_pred = sum(v[0].shape[0] - Hn.RGB_LEN_CLIP + 1 for v in videos)

    def leg(region: bool, n=None) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if region:
            Hn.evaluate_dataset_region(model, videos[:n], masks[:n], "ped2", 16, values, device=DEV)
        else:
            Hn.evaluate_dataset_pixel(model, videos[:n], masks[:n], "ped2", 16, (2, 5), device=DEV)
        torch.cuda.synchronize()
        return n_pred / (time.perf_counter() - t0)
    for flag in (False, True):                                  # warm both: plans, packs, the workspace
        leg(flag, 1)
    legs = []
    for rnd in range(3):
        for flag in (False, True):
            legs.append({"round": rnd, "region": flag, "fps": round(leg(flag), 2)})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    pix = sorted(x["fps"] for x in legs if not x["region"])
    reg = sorted(x["fps"] for x in legs if x["region"])
    return {"videos": n_videos, "frames": frames, "predicted_frames": n_pred, "thresholds": T, "fps_evaluate_dataset_pixel": pix,
            "fps_evaluate_dataset_region": reg, "median_pixel": pix[1], "median_region": reg[1],
            "region_over_pixel": round(reg[1] / pix[1], 4),
            "ms_per_frame_added": round(1e3 / reg[1] - 1e3 / pix[1], 4)}


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        what = sys.argv[2]
        rec = step_launches() if what == "launches" else step_loop(int(sys.argv[3]), int(sys.argv[4]))
        print(json.dumps(rec))
        return
    n_videos = sys.argv[1] if len(sys.argv) > 1 else "4"
    frames = sys.argv[2] if len(sys.argv) > 2 else "60"
    rec = {"batch": B, "thresholds": T, "iou": [1, 10], "reps": REPS}
    for what, extra in (("launches", []), ("loop", [n_videos, frames])):
        # a child per step: a step that faults, hangs or runs into its limit ends the measurement there
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", what] + extra, stdout=subprocess.PIPE,
                           timeout=STEP_LIMITS[what])
        if r.returncode != 0:
            raise SystemExit(f"step {what} ended with status {r.returncode}: nothing further is started")
        rec[what] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
