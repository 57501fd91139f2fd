"""What the per-clip memory scores cost, inside ONE call on the MI355X:

1. the two launches of `ammc_memory_scores_f32` (the scoring kernel, then the per-clip tail) between device events at
   batch 16, bottleneck 32x32, c 512, m 256 and 2000, k 2, with the slot indices: min / median / max over REPS
   repetitions after warm-up, the MACs of the two contractions over the median, and the ideal time of those MACs on the
   fp32 matrix pipe's 157.3 TFLOP/s.  The codebook pack of `ops.memory_scores` (one launch per call) is timed beside it;
2. frames/s of `harness.evaluate_dataset` against `harness.evaluate_dataset_memory` on run_test's synthetic set, the two
   alternating three times: the pass's share of the scoring loop (S16 plans: the decode of the two bottlenecks to fp32
   NHWC - a kernel and a channels-last copy per stream and batch - is part of the price);
3. the largest relative difference of a clip's `rgb_clip_comm` / `op_clip_comm` between one sub-video evaluated in
   batches of 16 and in batches of 3: how batch-invariant the convolutions IN FRONT of the pass are (the pass is
   invariant given its input; reported, not gated).

    python tools/memory_scores_ab.py [videos] [frames] > profiles/memory_scores_ab.txt
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, run_test, synthetic as S
from ammcnet_aaai2021_amd.engine import _Packer

DEV = "cuda:0"
B, G, C, D, K = 16, 32, 512, 64, 2
REPS = 100
PEAK_TFLOPS = 157.3


def _times(fn) -> dict:
    for _ in range(10):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        rc = fn()
        e1.record()
        assert rc == 0
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"reps": REPS, "us_min": round(ms[0] * 1e3, 2), "us_median": round(ms[len(ms) // 2] * 1e3, 2),
            "us_max": round(ms[-1] * 1e3, 2)}


def kernel_times(ms=(256, 2000)) -> list:
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, G, G, C), generator=g).to(DEV)
    enc_w = (torch.randn((D, C), generator=g) / C ** 0.5).to(DEV)
    enc_b = (0.1 * torch.randn((D,), generator=g)).to(DEV)
    rows = []
    for m in ms:
        embed = torch.randn((D, m), generator=g).to(DEV)
        e_md, enorm = _Packer(torch.device(DEV)).codebook(embed)
        mp = torch.empty((B, G, G), device=DEV)
        idx = torch.empty((B, G, G, K), device=DEV, dtype=torch.int32)
        commit, worst = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
        worst_idx = torch.empty(B, device=DEV, dtype=torch.int32)
        stream = torch.cuda.current_stream().cuda_stream
        args = (x.data_ptr(), *ops._nhwc_strides(x), B, G, G, C, enc_w.data_ptr(), enc_b.data_ptr(), embed.data_ptr(),
                e_md.data_ptr(), enorm.data_ptr(), D, m, K, mp.data_ptr(), G * G, idx.data_ptr(), commit.data_ptr(),
                worst.data_ptr(), worst_idx.data_ptr(), stream)
        row = {"batch": B, "grid": [G, G], "c": C, "m": m, "k": K, **_times(lambda: lib.ammc_memory_scores_f32(*args))}
        macs = B * G * G * D * (C + m)
        row["GMAC"] = round(macs / 1e9, 3)
        row["TFLOPS_at_median"] = round(2 * macs / (row["us_median"] * 1e-6) / 1e12, 2)
        row["ideal_us_at_157.3_TFLOPS"] = round(2 * macs / (PEAK_TFLOPS * 1e12) * 1e6, 2)
        row["codebook_pack"] = _times(lambda: lib.ammc_pack_codebook_f32(embed.data_ptr(), D, m, e_md.data_ptr(),
                                                                        enorm.data_ptr(), stream))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def _model():
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state())
    model = model.to(DEV).eval()
    model.precision = "s16"
    return model


def loop_rates(model, n_videos: int, frames: int) -> dict:
    videos, _ = run_test.synthetic_dataset(n_videos, frames, 256)
    n_pred = sum(v[0].shape[0] - Hn.RGB_LEN_CLIP + 1 for v in videos)

    def run(memory: bool, vids):
        if memory:
            Hn.evaluate_dataset_memory(model, vids, "ped2", device=DEV)
        else:
            Hn.evaluate_dataset(model, vids, "ped2", device=DEV)

    def leg(memory: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(memory, videos)
        torch.cuda.synchronize()
        return n_pred / (time.perf_counter() - t0)
    for flag in (False, True):                                  # warm both: plans, packs
        run(flag, videos[:1])
    legs = []
    for rnd in range(3):
        for flag in (False, True):
            legs.append({"round": rnd, "memory": flag, "fps": round(leg(flag), 2)})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    plain = sorted(x["fps"] for x in legs if not x["memory"])
    mem = sorted(x["fps"] for x in legs if x["memory"])
    return {"videos": n_videos, "frames": frames, "size": 256, "predicted_frames": n_pred, "precision": "s16",
            "fps_evaluate_dataset": plain, "fps_evaluate_dataset_memory": mem, "median_plain": plain[1],
            "median_memory": mem[1], "memory_over_plain": round(mem[1] / plain[1], 4)}


def batch_agreement(model, frames: int) -> dict:
    (rgb, op), = run_test.synthetic_dataset(1, frames, 256)[0]
    rgb, op = rgb.to(DEV), op.to(DEV)
    a = Hn.memory_subvideo(model, rgb, op, batch=16)
    b = Hn.memory_subvideo(model, rgb, op, batch=3)
    out = {"frames": frames, "size": 256, "precision": "s16", "batches": [16, 3]}
    for st in ("rgb", "op"):
        x, y = a[f"{st}_clip_comm"].astype(np.float64), b[f"{st}_clip_comm"].astype(np.float64)
        out[f"{st}_clip_comm_max_rel_diff"] = float(np.max(np.abs(x - y) / np.abs(x)))
        out[f"{st}_clip_comm_equal_bits"] = bool(np.array_equal(a[f"{st}_clip_comm"], b[f"{st}_clip_comm"]))
        x, y = a[f"{st}_comm"].astype(np.float64), b[f"{st}_comm"].astype(np.float64)
        out[f"{st}_comm_per_batch_max_rel_diff"] = float(np.max(np.abs(x - y) / np.abs(x)))   # the reference's value: batching itself
    return out


def main() -> None:
    n_videos = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    rows = kernel_times()
    model = _model()
    rec = {"device": torch.cuda.get_device_name(0), "pass": rows, "scoring_loop": loop_rates(model, n_videos, frames),
           "batch_16_against_batch_3": batch_agreement(model, frames)}
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
