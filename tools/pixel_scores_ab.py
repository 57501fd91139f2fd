"""What the pixel-level pass costs on the MI355X.  Two steps, each a child process of its own
under its own time limit; the parent never opens the GPU and stops at the first step that fails:

  launches  (a) the one launch of `ammc_pixel_scores_f32` between device events at batch 16, for 256x256 (the pixel map)
            and 32x32 (the patch-8 map), with masks of 1 %, 5 %, 40 % and 100 % (one rectangle per sample): median and
            min..max of REPS repetitions after warm-up;
            (b) the same quantities from torch alone, on the same device, in the same process, on the same tensors:
            masked fill with -inf, a per-sample descending sort and a gather at rank k for `kth`, `amax` for the two
            maxima, a sum for `m` - timed the same way, and checked to agree with (a) before anything is timed;
  loop      (c) frames/s of `harness.evaluate_dataset_pixel` against `harness.evaluate_dataset_localised(pixel=False)`
            on run_test's synthetic set, the two alternating three times.

    python tools/pixel_scores_ab.py [videos] [frames] > profiles/pixel_scores_ab.txt
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
B = 16
REPS = 100
STEP_LIMITS = {"launches": 240, "loop": 420}                   # seconds, per child process
FRAC = (2, 5)


def _rect_masks(torch, hw: int, share: float):
    """uint8 [B, hw, hw]: one rectangle per sample covering `share` of the frame, at a place that moves with the sample"""
    mk = torch.zeros(B, hw, hw, dtype=torch.uint8)
    rh = max(1, min(hw, round(hw * share ** 0.5)))
    rw = max(1, min(hw, round(hw * hw * share / rh)))
    for b in range(B):
        y0, x0 = (b * 37) % (hw - rh + 1), (b * 53) % (hw - rw + 1)
        mk[b, y0:y0 + rh, x0:x0 + rw] = 1
    return mk


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


def step_launches() -> dict:
    import torch
    from ammcnet_aaai2021_amd import _lib, ops
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for hw in (256, 32):
        g = torch.Generator().manual_seed(hw)
        # squared errors as the error maps hold them: non-negative, most of them small
        amap = (torch.randn(B, hw, hw, generator=g) * 0.05).square().to(DEV)
        for share in (0.01, 0.05, 0.40, 1.00):
            mask = _rect_masks(torch, hw, share).to(DEV)
            out = ops.pixel_scores(amap, mask, FRAC)
            args = (amap.data_ptr(), amap.stride(0), mask.data_ptr(), mask.stride(0), B, hw, hw, *FRAC, out["m"].data_ptr(),
                    out["kth"].data_ptr(), out["max_in"].data_ptr(), out["max_out"].data_ptr(), stream)

            def kernel():
                assert lib.ammc_pixel_scores_f32(*args) == 0

            inside = mask.reshape(B, -1) != 0
            flat = amap.reshape(B, -1)
            ninf = torch.full((), float("-inf"), device=DEV)

            def composed():
                m = inside.sum(dim=1)
                vin = torch.where(inside, flat, ninf)
                k = (m * FRAC[0] + FRAC[1] - 1) // FRAC[1]
                kth = torch.sort(vin, dim=1, descending=True).values.gather(1, (k - 1).clamp_min(0)[:, None])[:, 0]
                return m, kth, vin.amax(dim=1), torch.where(inside, ninf, flat).amax(dim=1)

            m, kth, max_in, max_out = composed()
            agree = bool(torch.equal(m.to(torch.int32), out["m"]) and torch.equal(kth, out["kth"])
                         and torch.equal(max_in, out["max_in"]) and torch.equal(max_out, out["max_out"]))
            assert agree, (hw, share)
            for what, call in (("ammc_pixel_scores_f32", kernel), ("torch: where / sort / gather / amax", composed)):
                ms = _timed(torch, call)
                row = {"pass": what, "batch": B, "size": hw, "mask_share": share, "mask_pixels": int(m[0]), "reps": REPS,
                       "us_median": round(ms[len(ms) // 2] * 1e3, 2), "us_min": round(ms[0] * 1e3, 2),
                       "us_max": round(ms[-1] * 1e3, 2), "agrees_with_torch": agree}
                print(json.dumps(row), file=sys.stderr, flush=True)
                rows.append(row)
    return {"device": torch.cuda.get_device_name(0), "source_digests": lib.ammc_source_digests().decode(), "launches": rows}


def step_loop(n_videos: int, frames: int) -> dict:
    import torch
    import ammcnet_aaai2021_amd as A
    from ammcnet_aaai2021_amd import harness as Hn, run_pixel, run_test, synthetic as S
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state())
    model = model.to(DEV).eval()
    model.precision = "s16"
    videos, _ = run_test.synthetic_dataset(n_videos, frames, 256)
    masks = run_pixel.synthetic_masks(n_videos, frames, 256, 256)
    n_pred = sum(v[0].shape[0] - Hn.RGB_LEN_CLIP + 1 for v in videos)

    def leg(pixel: bool, n=None) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if pixel:
            Hn.evaluate_dataset_pixel(model, videos[:n], masks[:n], "ped2", 16, FRAC, device=DEV)
        else:
            Hn.evaluate_dataset_localised(model, videos[:n], "ped2", 16, False, device=DEV)
        torch.cuda.synchronize()
        return n_pred / (time.perf_counter() - t0)
    for flag in (False, True):                                  # warm both: plans, packs
        leg(flag, 1)
    legs = []
    for rnd in range(3):
        for flag in (False, True):
            legs.append({"round": rnd, "pixel": flag, "fps": round(leg(flag), 2)})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    loc = sorted(x["fps"] for x in legs if not x["pixel"])
    pix = sorted(x["fps"] for x in legs if x["pixel"])
    return {"videos": n_videos, "frames": frames, "predicted_frames": n_pred, "fps_evaluate_dataset_localised": loc,
            "fps_evaluate_dataset_pixel": pix, "median_localised": loc[1], "median_pixel": pix[1],
            "pixel_over_localised": round(pix[1] / loc[1], 4)}


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        what = sys.argv[2]
        rec = step_launches() if what == "launches" else step_loop(int(sys.argv[3]), int(sys.argv[4]))
        print(json.dumps(rec))
        return
    n_videos = sys.argv[1] if len(sys.argv) > 1 else "4"
    frames = sys.argv[2] if len(sys.argv) > 2 else "60"
    rec = {"batch": B, "frac": list(FRAC), "reps": REPS}
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
