"""A/B of `harness.FUSED_LOSS` inside ONE call: the joint G / D iteration (`harness.train_step_gan`, flow term on) at
batch 32, 256x256 with the flag alternating 0 / 1 three times - the flag-off legs are the baseline, boxes differ by up
to 7 % so nothing is compared across calls - and the launch count of the loss section of each setting.

    python tools/loss_ab.py [batch] [steps]            # writes the record to stdout: profiles/loss_ab.txt is one run

The launch count comes from `rocprofv3 --kernel-trace --stats -- python tools/loss_ab.py --section <0|1>` run as two
fresh child processes: the child evaluates the loss section alone (`generator_loss_full` on leaf tensors of the
generator's output shapes, forward + backward) SECTION_RUNS times and launches nothing else, so the dispatches of its
trace divided by SECTION_RUNS are the launches of one loss section.
"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, synthetic as S

DEV = "cuda:0"
SECTION_RUNS = 3
HW = 256


def section(flag: int, batch: int) -> None:
    """the loss section alone; inputs are made on the host and copied (copies are not kernel dispatches)"""
    Hn.FUSED_LOSS = bool(flag)
    mk = lambda tag, shape, s=1.0: (S.hashed_uniform(tag, shape) * s).to(DEV)
    rgb_t = mk("ab-rgb-clip", (batch, 5, 3, HW, HW))[:, -1]
    op_t = mk("ab-op-clip", (batch, 4, 2, HW, HW))[:, -1]
    rgb, op = mk("ab-rgb", (batch, 3, HW, HW)).requires_grad_(True), mk("ab-op", (batch, 2, HW, HW)).requires_grad_(True)
    rd, od = mk("ab-rd", (1,)).requires_grad_(True), mk("ab-od", (1,)).requires_grad_(True)
    d_gen = mk("ab-dgen", (batch, 1, 34, 34)).requires_grad_(True)
    fp, fg = mk("ab-fp", (batch, 2, HW, HW), 0.1), mk("ab-fg", (batch, 2, HW, HW), 0.1)
    torch.cuda.synchronize()
    for _ in range(SECTION_RUNS):
        loss = Hn.generator_loss_full((rgb, op, (rd, od), None), rgb_t, op_t, d_gen, fp, fg, **Hn.LAMS_ANOPRED)
        loss.backward()
    torch.cuda.synchronize()


def count_launches(flag: int, batch: int) -> dict:
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="loss_ab_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--section", str(flag), str(batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not stats:
            return {"error": f"rocprofv3 rc {r.returncode}", "tail": (r.stderr or r.stdout)[-300:]}
        rows = list(csv.DictReader(open(stats[0])))
        calls = sum(int(x["Calls"]) for x in rows)
        ns = sum(float(x["TotalDurationNs"]) for x in rows)
        ours = sum(int(x["Calls"]) for x in rows if "ammc_impl" in x["Name"])
        return {"dispatches": calls, "launches_per_section": round(calls / SECTION_RUNS, 2),
                "library_launches_per_section": round(ours / SECTION_RUNS, 2),
                "kernel_us_per_section": round(ns / 1e3 / SECTION_RUNS, 1),
                "kernels": {x["Name"][:90]: int(x["Calls"]) for x in rows}}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main() -> None:
    if "--section" in sys.argv:
        i = sys.argv.index("--section")
        section(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
        return
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
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
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(batch, HW, HW, tag="loss-ab"))
    rgb = torch.cat([rgb_x.view(batch, 4, 3, HW, HW), rgb_t[:, None]], 1)
    op = torch.cat([op_x.view(batch, 3, 2, HW, HW), op_t[:, None]], 1)

    def leg(flag: int, n: int):
        Hn.FUSED_LOSS = bool(flag)
        for _ in range(n):
            gl, dl = Hn.train_step_gan(G, D, opt_g, opt_d, rgb, op, flow_fn, **Hn.LAMS_ANOPRED)
        torch.cuda.synchronize()
        return float(gl), float(dl)
    for flag in (0, 1):                                         # warm both paths: workspaces, first-call work
        leg(flag, 2)
    legs = []
    for rnd in range(3):
        for flag in (0, 1):
            t0 = time.perf_counter()
            gl, dl = leg(flag, steps)
            ms = (time.perf_counter() - t0) / steps * 1e3
            legs.append({"round": rnd, "fused_loss": flag, "ms_per_iteration": round(ms, 3), "g_loss": gl, "d_loss": dl})
            print(json.dumps(legs[-1]), flush=True)
    off = [x["ms_per_iteration"] for x in legs if not x["fused_loss"]]
    on = [x["ms_per_iteration"] for x in legs if x["fused_loss"]]
    del G, D, F2, opt_g, opt_d
    torch.cuda.empty_cache()
    counts = {f"fused_loss_{flag}": count_launches(flag, batch) for flag in (0, 1)}
    mb = batch * HW * HW * 4 / 1e6
    print(json.dumps({"batch": batch, "size": HW, "steps_per_leg": steps, "device": torch.cuda.get_device_name(0),
                      "ms_off": off, "ms_on": on, "median_off": sorted(off)[1], "median_on": sorted(on)[1],
                      "loss_section": counts,
                      "algorithmic_MB_fused": {"read": round(2 * (3 + 3 + 2 + 2) * mb + 2 * 2 * mb, 1),
                                               "written": round((3 + 2) * mb, 1)}}))


if __name__ == "__main__":
    main()
