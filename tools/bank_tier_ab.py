"""What the host tier of `pipeline.ClipBank` costs, inside ONE call (boxes differ by several per cent, so nothing is
compared across calls), at batch 32, 256x256:

  (a) the gather alone, between events, from an all-device bank and from an all-host bank (every frame in pinned host
      memory, read by `ammc_gather_clips_tiered` over the host link), and the host-link GB/s the latter achieves;
  (b) `ms_per_iter` of the joint iteration (`harness.train_step_gan`, flow term on) fed from three sources, alternated
      three times each: an all-device bank; an all-host bank with `ClipBank.prefetch` one iteration ahead (the loop of
      `run_train --bank_host_gb`); an all-host bank without prefetch.

    python tools/bank_tier_ab.py [batch] [steps]       # writes the record to stdout: profiles/bank_tier_ab.txt is one run

The claim to confirm or refute: with prefetch, the all-host iteration lies inside the spread of the three all-device
repetitions.  The set is synthetic (.npy frames and flows written to a temporary folder, 8 sub-videos of 24 frames).
"""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, pipeline as P, synthetic as S

DEV = "cuda:0"
HW = 256
VIDEOS, FRAMES = 8, 24


def write_set(root: str) -> None:
    rng = np.random.default_rng(7)
    for v in range(VIDEOS):
        dr, do = os.path.join(root, "rgb", f"{v:02d}"), os.path.join(root, "op", f"{v:02d}")
        os.makedirs(dr)
        os.makedirs(do)
        for i in range(FRAMES):
            np.save(os.path.join(dr, f"{i:04d}.npy"), rng.integers(0, 256, (HW, HW, 3), dtype=np.uint8))
        for i in range(FRAMES - 1):
            np.save(os.path.join(do, f"{i:04d}.npy"), rng.normal(0, 2, (HW, HW, 2)).astype(np.float32))


def gather_alone(bank, draws, reps: int) -> list:
    """ms of `reps` gathers, each between its own pair of events (the upload of its 256 B of indices included)"""
    for d in draws[:3]:
        bank.gather(*d)
    torch.cuda.synchronize()
    ms = []
    for d in draws[3:3 + reps]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = bank.gather(*d)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    return ms


def main() -> None:
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    root = tempfile.mkdtemp(prefix="bank_tier_ab_")
    try:
        write_set(root)
        roots = (os.path.join(root, "rgb"), os.path.join(root, "op"))
        dev_bank = P.ClipBank(*roots, HW, DEV, budget_gb=8.0)
        host_bank = P.ClipBank(*roots, HW, DEV, budget_gb=0.0, host_budget_gb=8.0)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    assert dev_bank.host_nbytes == 0 and host_bank.device_nbytes == 0 and host_bank.host_nbytes == dev_bank.nbytes
    sampler = P.ClipSampler(dev_bank.rgb_count, dev_bank.op_count, seed=2017)
    draws = [dev_bank.global_index(*sampler.draw(batch)) for _ in range(64)]
    a, b = dev_bank.gather(*draws[0]), host_bank.gather(*draws[0])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                # the two sources hand out the same clips
    del a, b

    # (a) the gather alone
    mb = batch * (5 * 3 * HW * HW + 4 * 4 * HW * HW) / 1e6             # bank bytes one batch reads
    ga = {"device": gather_alone(dev_bank, draws, 20), "host": gather_alone(host_bank, draws, 20)}
    med = {k: sorted(v)[len(v) // 2] for k, v in ga.items()}
    print(json.dumps({"part": "gather_alone", "batch": batch, "bank_MB_read": round(mb, 2),
                      "device_ms": {"median": round(med["device"], 4), "min": round(min(ga["device"]), 4), "max": round(max(ga["device"]), 4)},
                      "host_ms": {"median": round(med["host"], 4), "min": round(min(ga["host"]), 4), "max": round(max(ga["host"]), 4)},
                      "host_link_GBps": round(mb / med["host"], 2), "device_GBps": round(mb / med["device"], 1)}), flush=True)

    # (b) the iteration
    G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    G.load_state_dict(S.make_twostream_state())
    G = G.to(DEV).train()
    D = A.PixelDiscriminator(3, [128, 256, 512, 512])
    D.load_state_dict(S.make_discriminator_state())
    D = D.to(DEV).train()
    F2 = A.FlowNet2SD()
    F2.load_state_dict(S.make_flownet2sd_state())
    flow_fn = Hn.flownet_flow_fn(F2.to(DEV).eval())
    opt_g, opt_d = Hn.adam(G.parameters(), lr=2e-4), Hn.adam(D.parameters(), lr=2e-5)

    def leg(source: str, n: int, at: int):
        bank = dev_bank if source == "device" else host_bank
        pre = source == "host_prefetch"
        use = [draws[(at + i) % len(draws)] for i in range(n + 1)]
        if pre:
            bank.prefetch(*use[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            rgb, op = bank.gather(*use[i])
            if pre:
                bank.prefetch(*use[i + 1])
            gl, dl = Hn.train_step_gan(G, D, opt_g, opt_d, rgb, op, flow_fn, **Hn.LAMS_ANOPRED)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        bank.gather(*use[0])                                           # (drops the prefetch left over)
        return ms, float(gl), float(dl)

    sources = ("device", "host_prefetch", "host")
    for s in sources:                                                  # warm: workspaces, first-call work
        leg(s, 2, 0)
    legs = []
    for rnd in range(3):
        for s in sources:
            ms, gl, dl = leg(s, steps, 8 * rnd)                        # the same clips for the three sources of a round
            legs.append({"part": "iteration", "round": rnd, "source": s, "ms_per_iter": round(ms, 3), "g_loss": gl, "d_loss": dl})
            print(json.dumps(legs[-1]), flush=True)
    by = {s: [x["ms_per_iter"] for x in legs if x["source"] == s] for s in sources}
    lo, hi = min(by["device"]), max(by["device"])
    print(json.dumps({"part": "summary", "batch": batch, "size": HW, "steps_per_leg": steps, "device": torch.cuda.get_device_name(0),
                      "ms_per_iter": by, "median": {s: sorted(v)[1] for s, v in by.items()},
                      "device_spread_ms": [lo, hi],
                      "host_prefetch_inside_device_spread": bool(lo <= sorted(by["host_prefetch"])[1] <= hi),
                      "host_prefetch_minus_device_ms": round(sorted(by["host_prefetch"])[1] - sorted(by["device"])[1], 3),
                      "host_minus_device_ms": round(sorted(by["host"])[1] - sorted(by["device"])[1], 3)}))


if __name__ == "__main__":
    main()
