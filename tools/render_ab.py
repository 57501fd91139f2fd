"""What the render pass costs on the MI355X.  One child process under its own time limit; the
parent never opens the GPU:

  launches  at batch 16, 256x256, between device events, median and min..max of REPS repetitions after warm-up:
            (a) `ammc_render_stats_f32` alone, `ammc_render_panels_u8` alone (all six tiles), and the two together as
                `ops.render_panels` issues them;
            (b) the same panels composed with torch operations on the same device, in the same process, on the same
                tensors (`compose_torch`: the definitions of include/ammc_hip.h restated op by op) - checked to agree
                with (a) to one grey level before anything is timed;
            (c) the evaluation forward of that batch (`forward_scored`, s16): what the pass stands beside.
  shares    the share of flow-tile and heat-tile values that differ from `harness.render_reference` (by one grey level:
            a larger difference ends the run), pooled over the shapes of tests/render_cases.py, and the same for the
            colour code against the reference's own output (tests/golden/flow_colour.npz): what tests/test_gpu_render.py
            gates at four times.

    python tools/render_ab.py > profiles/render_ab.txt
"""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
B, HW = 16, 256
REPS = 100
STEP_LIMIT = 420                                               # seconds, for the child process


def _timed(torch, call) -> dict:
    for _ in range(10):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"us_median": round(ms[len(ms) // 2] * 1e3, 2), "us_min": round(ms[0] * 1e3, 2), "us_max": round(ms[-1] * 1e3, 2)}


def compose_torch(torch, wheel, rp, rt, fp, ft, scale=(1.0, 1.0), alpha=0.6):
    """the default 2 x 3 panels from torch operations alone (fp32, on the tensors' device)"""
    def frame(x):
        return ((x.clamp(-1, 1) + 1) * 127.5 + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)

    def parts(f):
        u, v = scale[0] * f[:, 0], scale[1] * f[:, 1]
        known = (u.abs() <= 1e7) & (v.abs() <= 1e7)
        u, v = torch.where(known, u, 0.0), torch.where(known, v, 0.0)
        return u, v, torch.sqrt(u * u + v * v), known

    def colour(f, maxrad):
        u, v, raw, known = parts(f)
        mr = maxrad[:, None, None]
        rad = (raw * (1.0 / (mr + 2.0 ** -52))).clamp(max=1.0)
        fk = (torch.atan2(-v, -u) / math.pi + 1) / 2 * 54 + 1
        k0f = fk.floor().clamp(1, 55)
        k0 = k0f.long()
        k1 = torch.where(k0 == 55, 1, k0 + 1)
        f_ = (fk - k0f)[..., None]
        col = (1 - f_) * wheel[k0 - 1] + f_ * wheel[k1 - 1]
        col = torch.where((raw <= mr)[..., None], 1 - rad[..., None] * (1 - col), col * 0.75)
        return torch.where(known[..., None], (255 * col).floor().clamp(0, 255), 0.0).to(torch.uint8)

    def heat(e, grey):
        hm = e.amax(dim=(1, 2), keepdim=True)
        t = torch.where(hm > 0, (e / hm).clamp(max=1.0), 0.0)[..., None]
        c = (1.5 - (4 * t - torch.tensor([3.0, 2.0, 1.0], device=e.device)).abs()).clamp(0, 1)
        return ((1 - alpha) * grey[..., None] + alpha * 255 * c + 0.5).floor().clamp(0, 255).to(torch.uint8)

    ft_u, ft_v, ft_raw, ft_known = parts(ft)
    maxrad = ft_raw.amax(dim=(1, 2))
    t_rgb = frame(rt)
    e_rgb = ((0.5 * (rt - rp)) ** 2).sum(1) / 3.0
    e_op = torch.where(ft_known & parts(fp)[3], ((0.5 * (ft - fp)) ** 2).sum(1) / 2.0, 0.0)
    top = torch.cat([t_rgb, frame(rp), heat(e_rgb, t_rgb.float().sum(-1) / 3.0)], dim=2)
    bottom = torch.cat([colour(ft, maxrad), colour(fp, maxrad), heat(e_op, torch.full_like(e_op, 128.0))], dim=2)
    return torch.cat([top, bottom], dim=1)


def step() -> dict:
    import ctypes
    import numpy as np
    import torch
    import ammcnet_aaai2021_amd as A
    from ammcnet_aaai2021_amd import _lib, harness as Hn, ops, synthetic as S
    import render_cases as K
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "size": HW, "reps": REPS,
           "source_digests": lib.ammc_source_digests().decode()}

    # ---- shares of values one grey level off the witness
    def off_by(a, b):
        d = np.abs(a.astype(np.int16) - b.astype(np.int16))
        assert d.max(initial=0) <= 1, "a value more than one grey level off the witness"
        return int((d != 0).sum()), int(d.size)
    tally = {"frame": [0, 0], "flow": [0, 0], "heat": [0, 0]}
    kinds = {"rgb_target": "frame", "rgb_pred": "frame", "op_target": "flow", "op_pred": "flow", "rgb_heat": "heat", "op_heat": "heat"}
    for shape in K.DEVICE_SHAPES:
        got = ops.render_panels(*(t.to(DEV) for t in K.inputs(shape)), flow_scale=K.FLOW_SCALE).cpu().numpy()
        ref = K.reference(shape)
        _, h, w = shape
        for i, name in enumerate(Hn.RENDER_TILES):
            r, c = divmod(i, 3)
            n, total = off_by(got[:, r * h:(r + 1) * h, c * w:(c + 1) * w], ref[name])
            tally[kinds[name]][0] += n
            tally[kinds[name]][1] += total
    g = np.load(os.path.join(ROOT, "tests", "golden", "flow_colour.npz"))
    flows = np.ascontiguousarray(np.stack([g[f"{name}_flow"].transpose(2, 0, 1) for name in K.GOLDEN_CASES]))
    got = ops.flow_to_rgb(torch.from_numpy(flows).to(DEV)).cpu().numpy()
    gold = [0, 0]
    for i, name in enumerate(K.GOLDEN_CASES):
        r = Hn.flow_colour_reference(flows[i:i + 1])
        cmp = K.compared(r["raw"][0], r["max_rad"][0]) | ~r["known"][0]
        n, total = off_by(got[i][cmp], g[f"{name}_image"][cmp])
        gold[0], gold[1] = gold[0] + n, gold[1] + total
    rec["shares"] = {k: {"differ": n, "values": t, "share": n / t} for k, (n, t) in tally.items()}
    rec["shares"]["flow_vs_flow_to_image"] = {"differ": gold[0], "values": gold[1], "share": gold[0] / gold[1]}
    print(json.dumps(rec["shares"]), file=sys.stderr, flush=True)

    # ---- launches at the evaluation shape
    model = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    model.load_state_dict(S.make_twostream_state())
    model = model.to(DEV).eval()
    model.precision = "s16"
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(B, HW, HW, tag="render_ab"))
    with torch.no_grad():
        (rgb_p, op_p, _, _), *_ = model.forward_scored(rgb_x, op_x, rgb_t, op_t)
    rgb_p, op_p = rgb_p.contiguous(), op_p.contiguous()
    scale = (float(HW), float(HW))
    n = HW * HW
    out = torch.empty((B, 2 * HW, 3 * HW, 3), device=DEV, dtype=torch.uint8)
    stats = torch.empty((B, 4), device=DEV)
    ins = [rgb_p.data_ptr(), 3 * n, rgb_t.data_ptr(), rgb_t.stride(0), op_p.data_ptr(), 2 * n, op_t.data_ptr(), op_t.stride(0)]
    tiles = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)

    def k_stats():
        assert lib.ammc_render_stats_f32(*ins, B, HW, HW, *scale, stats.data_ptr(), stream) == 0

    def k_panels():
        assert lib.ammc_render_panels_u8(*ins, B, HW, HW, *scale, tiles, 2, 3, stats.data_ptr(), 0, None, None, None, 0.6,
                                         out.data_ptr(), out.stride(0), stream) == 0

    def k_both():
        ops.render_panels(rgb_p, rgb_t, op_p, op_t, flow_scale=scale, out=out)

    wheel = torch.from_numpy(Hn.colour_wheel()).to(DEV)

    def composed():
        return compose_torch(torch, wheel, rgb_p, rgb_t, op_p, op_t, scale)

    def forward():
        with torch.no_grad():
            model.forward_scored(rgb_x, op_x, rgb_t, op_t)

    k_both()
    d = (out.to(torch.int16) - composed().to(torch.int16)).abs()
    assert int(d.max()) <= 1, "the torch composition and the kernels disagree by more than one grey level"
    rec["composition_agrees"] = {"values_one_level_off": int((d != 0).sum()), "values": d.numel()}
    bytes_in = B * n * 4 * (3 + 3 + 2 + 2)
    rows = []
    for what, call, moved in (("ammc_render_stats_f32 (memset + kernel)", k_stats, bytes_in),
                              ("ammc_render_panels_u8, six tiles", k_panels, bytes_in + out.numel()),
                              ("ops.render_panels: both, as issued from python", k_both, 2 * bytes_in + out.numel()),
                              ("torch: the same panels composed op by op", composed, None),
                              ("forward_scored, s16, the same batch", forward, None)):
        row = {"pass": what, **_timed(torch, call)}
        if moved is not None:
            row.update(bytes_moved=moved, TB_per_s_at_median=round(moved / row["us_median"] / 1e6, 3))
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    rec["launches"] = rows
    return rec


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        print(json.dumps(step()))
        return
    # a child process: if it faults, hangs or runs into its limit the measurement ends there
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"], stdout=subprocess.PIPE, timeout=STEP_LIMIT)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with status {r.returncode}")
    print(json.dumps(json.loads(r.stdout.decode().strip().splitlines()[-1]), indent=1))


if __name__ == "__main__":
    main()
