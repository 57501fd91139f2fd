"""What the fused-map pass costs on the MI355X.  Two steps, each a child process of its own under
its own time limit; the parent never opens the GPU and stops at the first step that fails:

  launches  (a) the two launches of `ops.fuse_maps` between device events at batch 16, 256x256, four channels (cells 1, 1,
            8, 8), patch 16, radius 0, 2 and 4: median and min..max of REPS calls after warm-up;
            (b) beside it the same quantity composed from torch ops on the same tensors (`repeat_interleave` expansion,
            weighted sum, `avg_pool2d(count_include_pad=False)`, patch pooling, `amax`), with agreement of both with
            `harness.fuse_maps_reference` within the test's bound checked before anything is timed;
  loop      (c) frames/s of `harness.evaluate_dataset_fused` (3 settings, region on and off) against
            `harness.evaluate_dataset_region` on run_test's synthetic set, the three alternating three times.

    python tools/fuse_maps_ab.py [videos] [frames] > profiles/fuse_maps_ab.txt
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
B, SIZE, PATCH = 16, 256, 16
CELLS = (1, 1, 8, 8)
RADII = (0, 2, 4)
REPS = 100
WEIGHTS = [(1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 1)]
STEP_LIMITS = {"launches": 300, "loop": 480}                   # seconds, per child process


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
    import torch
    import fuse_cases as FC
    from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, synthetic as S
    F = torch.nn.functional
    lib = _lib.load()
    src = [S.hashed_uniform(f"ab:src{c}", (B, SIZE // cell, SIZE // cell), 0, 1).to(DEV) for c, cell in enumerate(CELLS)]
    coef = torch.tensor([1.0, 0.5, 2.0, 0.25], device=DEV)

    def composed(radius: int) -> dict:
        raw = None
        for c, cell in enumerate(CELLS):
            m = src[c] if cell == 1 else src[c].repeat_interleave(cell, dim=1).repeat_interleave(cell, dim=2)
            raw = coef[c] * m if raw is None else raw + coef[c] * m
        k = 2 * radius + 1
        pixel = F.avg_pool2d(raw[:, None], k, stride=1, padding=radius, count_include_pad=False)[:, 0] if radius else raw
        return {"pixel": pixel, "patch_mean": F.avg_pool2d(pixel[:, None], PATCH)[:, 0], "frame_max": pixel.amax(dim=(1, 2))}
    rows = []
    moved = 4 * B * (2 * SIZE * SIZE + 2 * (SIZE // 8) ** 2 + SIZE * SIZE + (SIZE // PATCH) ** 2)
    for radius in RADII:
        ref = Hn.fuse_maps_reference(src, CELLS, coef, radius, PATCH)
        out = ops.fuse_maps(src, CELLS, coef, radius, PATCH)
        alt = composed(radius)
        bound = FC.pixel_bound(len(CELLS), radius)
        errs = {}
        for name, got in (("kernel", out), ("torch", alt)):
            errs[name] = float(((got["pixel"].double() - ref["pixel"]).abs() / ref["pixel"]).max())
            assert errs[name] <= bound, (name, radius, errs[name], bound)
            pm = float(((got["patch_mean"].double() - ref["patch_mean"]).abs() / ref["patch_mean"]).max())
            assert pm <= bound + FC.U * (PATCH * PATCH + 1) * 1.01, (name, radius, pm)
        assert torch.equal(out["frame_max"], out["pixel"].amax(dim=(1, 2)))
        ms_k = _timed(torch, lambda: ops.fuse_maps(src, CELLS, coef, radius, PATCH, out))
        ms_t = _timed(torch, lambda: composed(radius))
        row = {"batch": B, "size": SIZE, "channels": len(CELLS), "radius": radius, "patch": PATCH, "reps": REPS,
               "bytes_moved": moved, "ops.fuse_maps": _us(ms_k), "torch_composition": _us(ms_t),
               "GB_per_s_at_the_median": round(moved / (ms_k[len(ms_k) // 2] * 1e-3) / 1e9, 1),
               "rel_err_kernel": errs["kernel"], "rel_err_torch": errs["torch"], "bound": bound,
               "torch_over_kernel": round(ms_t[len(ms_t) // 2] / ms_k[len(ms_k) // 2], 2)}
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
    videos, _ = run_test.synthetic_dataset(n_videos, frames, SIZE)
    masks = run_region.synthetic_region_masks(n_videos, frames, SIZE, SIZE)
    values = Hn.region_thresholds(64)
    n_pred = sum(v[0].shape[0] - Hn.RGB_LEN_CLIP + 1 for v in videos)
    kinds = ("region", "fused", "fused_no_region")

    def leg(kind: str, n=None) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "region":
            Hn.evaluate_dataset_region(model, videos[:n], masks[:n], "ped2", PATCH, values, device=DEV)
        else:
            Hn.evaluate_dataset_fused(model, videos[:n], masks[:n], WEIGHTS, "ped2", 2, PATCH, thresholds=values,
                                      region=kind == "fused", device=DEV)
        torch.cuda.synchronize()
        return n_pred / (time.perf_counter() - t0)
    for kind in kinds:                                          # warm all: plans, packs, the workspaces
        leg(kind, 1)
    legs = []
    for rnd in range(3):
        for kind in kinds:
            legs.append({"round": rnd, "pass": kind, "fps": round(leg(kind), 2)})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    fps = {kind: sorted(x["fps"] for x in legs if x["pass"] == kind) for kind in kinds}
    return {"videos": n_videos, "frames": frames, "predicted_frames": n_pred, "settings": len(WEIGHTS), "thresholds": 64, "radius": 2,
            "fps": fps, "median": {kind: fps[kind][1] for kind in kinds},
            "fused_over_region": round(fps["fused"][1] / fps["region"][1], 4),
            "fused_no_region_over_region": round(fps["fused_no_region"][1] / fps["region"][1], 4)}


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        what = sys.argv[2]
        rec = step_launches() if what == "launches" else step_loop(int(sys.argv[3]), int(sys.argv[4]))
        print(json.dumps(rec))
        return
    n_videos = sys.argv[1] if len(sys.argv) > 1 else "4"
    frames = sys.argv[2] if len(sys.argv) > 2 else "60"
    rec = {"batch": B, "size": SIZE, "cells": list(CELLS), "patch": PATCH, "reps": REPS}
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
