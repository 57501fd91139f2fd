"""What the error maps cost, inside ONE call on the MI355X:

1. the two launches of `ops.error_maps` (patch sums / means / pixel map, then the per-sample tail) between device
   events at batch 16, 256x256, 3 channels, for patch 8, 16 and 32, with and without the pixel map: min / median / max
   over REPS repetitions after warm-up, and the bytes per second of (pred + target read, maps written) over the median.
   The prediction is written by a kernel right before each timed pair, as the output layer does in the loop, so part of
   it is still in L2 / Infinity Cache: the figure is the rate of this pass in its place, not an HBM rate;
2. frames/s of `harness.evaluate_dataset` against `harness.evaluate_dataset_localised` on run_test's synthetic set, the
   two alternating three times: the maps' share of the scoring loop.

    python tools/score_maps_ab.py [videos] [frames] > profiles/score_maps_ab.txt
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_test, synthetic as S

DEV = "cuda:0"
B, C, HW = 16, 3, 256
REPS = 100


def kernel_times(B: int = B, patches=(8, 16, 32)) -> list:
    g = torch.Generator().manual_seed(1)
    src = torch.tanh(torch.randn(B, C, HW, HW, generator=g)).to(DEV)
    target = (torch.rand(B, C, HW, HW, generator=g) * 2 - 1).to(DEV)
    pred = torch.empty_like(src)
    rows = []
    for patch in patches:
        for pixel in (False, True):
            out = {k: v for k, v in ops.error_maps(src, target, patch, pixel).items() if k != "psnr"}
            lib, args = _raw_call(pred, target, patch, out, B)
            for _ in range(10):
                pred.copy_(src)
                lib.ammc_error_maps_f32(*args)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
            for e0, e1 in ev:
                pred.copy_(src)                            # the prediction is fresh from a kernel, as behind `outc`
                e0.record()
                rc = lib.ammc_error_maps_f32(*args)
                e1.record()
                assert rc == 0
            torch.cuda.synchronize()
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            ph = HW // patch
            read = 2 * B * C * HW * HW * 4
            written = (2 * B * ph * ph + 3 * B) * 4 + (B * HW * HW * 4 if pixel else 0)
            med = ms[len(ms) // 2]
            rows.append({"batch": B, "patch": patch, "pixel": pixel, "reps": REPS, "us_min": round(ms[0] * 1e3, 2),
                         "us_median": round(med * 1e3, 2), "us_max": round(ms[-1] * 1e3, 2), "bytes_read": read,
                         "bytes_written": written, "TB_per_s_at_median": round((read + written) / (med * 1e-3) / 1e12, 3)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def _raw_call(pred, target, patch, out, B):
    """the C entry with its arguments bound (no torch op between the two events)"""
    from ammcnet_aaai2021_amd import _lib
    lib = _lib.load()
    px = out.get("pixel")
    args = (pred.data_ptr(), *ops._nchw_strides(pred), target.data_ptr(), *ops._nchw_strides(target), B, C, HW, HW, patch,
            out["patch_sum"].data_ptr(), out["patch_sum"].stride(0), out["patch_mean"].data_ptr(),
            px.data_ptr() if px is not None else None, px.stride(0) if px is not None else 0, out["frame_sq"].data_ptr(),
            out["worst"].data_ptr(), out["worst_idx"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    return lib, args


def loop_rates(n_videos: int, frames: int) -> dict:
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state())
    model = model.to(DEV).eval()
    model.precision = "s16"
    videos, _ = run_test.synthetic_dataset(n_videos, frames, HW)
    n_pred = sum(v[0].shape[0] - Hn.RGB_LEN_CLIP + 1 for v in videos)

    def leg(localised: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if localised:
            Hn.evaluate_dataset_localised(model, videos, "ped2", 16, False, device=DEV)
        else:
            Hn.evaluate_dataset(model, videos, "ped2", device=DEV)
        torch.cuda.synchronize()
        return n_pred / (time.perf_counter() - t0)
    for flag in (False, True):                                  # warm both: plans, packs
        Hn.evaluate_dataset_localised(model, videos[:1], "ped2", 16, False, device=DEV) if flag else \
            Hn.evaluate_dataset(model, videos[:1], "ped2", device=DEV)
    legs = []
    for rnd in range(3):
        for flag in (False, True):
            legs.append({"round": rnd, "localised": flag, "fps": round(leg(flag), 2)})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    plain = sorted(x["fps"] for x in legs if not x["localised"])
    loc = sorted(x["fps"] for x in legs if x["localised"])
    return {"videos": n_videos, "frames": frames, "predicted_frames": n_pred, "patch": 16, "fps_evaluate_dataset": plain,
            "fps_evaluate_dataset_localised": loc, "median_plain": plain[1], "median_localised": loc[1],
            "localised_over_plain": round(loc[1] / plain[1], 4)}


def main() -> None:
    n_videos = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    rows = kernel_times()
    big = kernel_times(4 * B, (16,))
    # two sizes of one shape separate the fixed part of the pair (two dependent launches; the second is `batch`
    # workgroups of serial adds) from the streaming part: t = fixed + bytes / rate
    fit = []
    for small, large in zip([r for r in rows if r["patch"] == 16], big):
        nb = lambda r: r["bytes_read"] + r["bytes_written"]
        rate = (nb(large) - nb(small)) / ((large["us_median"] - small["us_median"]) * 1e-6)
        fit.append({"pixel": small["pixel"], "streaming_TB_per_s": round(rate / 1e12, 3),
                    "fixed_us": round(small["us_median"] - nb(small) / rate * 1e6, 2)})
    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "channels": C, "size": HW,
           "scoring_launches": rows, "scoring_launches_batch_%d" % (4 * B): big, "fixed_and_streaming_part_patch_16": fit,
           "scoring_loop": loop_rates(n_videos, frames)}
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
