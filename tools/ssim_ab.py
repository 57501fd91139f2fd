"""What the SSIM / MSE pass costs, inside ONE call on the MI355X:

1. the two launches of `ammc_ssim_f32` (the tile kernel, then the per-sample tail) between device events at batch 16,
   256x256, for 3 and 2 channels, with and without the map: min / median / max over REPS repetitions after warm-up.  The
   prediction is rewritten by a copy kernel right before each timed pair, as the output layer does in the loop, so part
   of it is still in L2 / Infinity Cache: the figure is the cost of this pass in its place.  Beside it, in the same
   process and on the same tensors, `ammc_error_maps_f32` (patch 16, with and without its pixel map) as the yardstick:
   it moves the same bytes with a handful of operations per pixel;
2. frames/s of `harness.evaluate_dataset` against `harness.evaluate_dataset_quality` on run_test's synthetic set, the two
   alternating three times: the pass's share of the scoring loop.

    python tools/ssim_ab.py [videos] [frames] > profiles/ssim_ab.txt
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, run_test, synthetic as S

DEV = "cuda:0"
B, HW = 16, 256
REPS = 100


def _timed(call, pred, src) -> list:
    for _ in range(10):
        pred.copy_(src)
        assert call() == 0
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        pred.copy_(src)                                    # the prediction is fresh from a kernel, as behind `outc`
        e0.record()
        rc = call()
        e1.record()
        assert rc == 0
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)


def kernel_times() -> list:
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for C in (3, 2):
        g = torch.Generator().manual_seed(1)
        src = torch.tanh(torch.randn(B, C, HW, HW, generator=g)).to(DEV)
        target = (torch.rand(B, C, HW, HW, generator=g) * 2 - 1).to(DEV)
        pred = torch.empty_like(src)
        read = 2 * B * C * HW * HW * 4
        for want_map in (False, True):
            out = ops.ssim(src, target, map=want_map)
            ws = torch.empty(int(lib.ammc_ssim_workspace_floats(B, C, HW, HW)), device=DEV)
            win = ops._ssim_window_c
            mp = out.get("map")
            args = (pred.data_ptr(), *ops._nchw_strides(pred), target.data_ptr(), *ops._nchw_strides(target), B, C, HW, HW, win,
                    out["ssim"].data_ptr(), out["ssim_c"].data_ptr(), out["sq"].data_ptr(),
                    mp.data_ptr() if mp is not None else None, mp.stride(0) if mp is not None else 0, ws.data_ptr(), ws.numel(),
                    stream)
            ms = _timed(lambda: lib.ammc_ssim_f32(*args), pred, src)
            written = (ws.numel() + B * (C + 2)) * 4 + (B * HW * HW * 4 if want_map else 0)
            rows.append(_row("ssim", C, want_map, ms, read, written))
            em = {k: v for k, v in ops.error_maps(src, target, 16, want_map).items() if k != "psnr"}
            px = em.get("pixel")
            eargs = (pred.data_ptr(), *ops._nchw_strides(pred), target.data_ptr(), *ops._nchw_strides(target), B, C, HW, HW, 16,
                     em["patch_sum"].data_ptr(), em["patch_sum"].stride(0), em["patch_mean"].data_ptr(),
                     px.data_ptr() if px is not None else None, px.stride(0) if px is not None else 0, em["frame_sq"].data_ptr(),
                     em["worst"].data_ptr(), em["worst_idx"].data_ptr(), stream)
            ms = _timed(lambda: lib.ammc_error_maps_f32(*eargs), pred, src)
            ph = HW // 16
            rows.append(_row("error_maps_patch16", C, want_map, ms, read, (2 * B * ph * ph + 3 * B) * 4 + (B * HW * HW * 4 if want_map else 0)))
    return rows


def _row(what, C, want_map, ms, read, written) -> dict:
    med = ms[len(ms) // 2]
    row = {"pass": what, "batch": B, "channels": C, "map": want_map, "reps": REPS, "us_min": round(ms[0] * 1e3, 2),
           "us_median": round(med * 1e3, 2), "us_max": round(ms[-1] * 1e3, 2), "bytes_read": read, "bytes_written": written,
           "TB_per_s_at_median": round((read + written) / (med * 1e-3) / 1e12, 3)}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def loop_rates(n_videos: int, frames: int) -> dict:
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state())
    model = model.to(DEV).eval()
    model.precision = "s16"
    videos, _ = run_test.synthetic_dataset(n_videos, frames, HW)
    n_pred = sum(v[0].shape[0] - Hn.RGB_LEN_CLIP + 1 for v in videos)

    def leg(quality: bool, vids=videos) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if quality:
            Hn.evaluate_dataset_quality(model, vids, "ped2", device=DEV)
        else:
            Hn.evaluate_dataset(model, vids, "ped2", device=DEV)
        torch.cuda.synchronize()
        return n_pred / (time.perf_counter() - t0)
    for flag in (False, True):                                  # warm both: plans, packs
        leg(flag, videos[:1])
    legs = []
    for rnd in range(3):
        for flag in (False, True):
            legs.append({"round": rnd, "quality": flag, "fps": round(leg(flag), 2)})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    plain = sorted(x["fps"] for x in legs if not x["quality"])
    qual = sorted(x["fps"] for x in legs if x["quality"])
    return {"videos": n_videos, "frames": frames, "predicted_frames": n_pred, "fps_evaluate_dataset": plain,
            "fps_evaluate_dataset_quality": qual, "median_plain": plain[1], "median_quality": qual[1],
            "quality_over_plain": round(qual[1] / plain[1], 4)}


def main() -> None:
    n_videos = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "size": HW, "tile": ops.SSIM_TILE,
           "source_digests": _lib.load().ammc_source_digests().decode(), "scoring_launches": kernel_times(),
           "scoring_loop": loop_rates(n_videos, frames)}
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
