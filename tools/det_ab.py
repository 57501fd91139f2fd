"""What `deterministic` costs, and that the default path did not move: the generator step (`harness.train_step`) and
the joint G / D iteration (`harness.train_step_gan`, flow term on) at the bench's batch 32, 256x256, default against
deterministic, alternating three times inside ONE process (boxes differ by several per cent: nothing is compared across
calls), each leg a host clock around `steps` iterations that end in a device synchronise, after a warm-up of both paths.

    python tools/det_ab.py [--batch 32] [--steps 8] [--out profiles/det_ab.txt]
    python tools/det_ab.py --against LIB [...]        # first: this tree's DEFAULT legs against another build of the
                                                      # library (the parent commit's: `python -m ammcnet_aaai2021_amd.build
                                                      # --variant parent` in a checkout of it, copied beside the in-tree one),
                                                      # as child processes alternating LIB / in-tree three times
    python tools/det_ab.py --default-only [...]       # what such a child runs: the default legs, one JSON line

The record also holds, per workload, the weight-gradient launches the switch re-routes - layer, kernel + "+det<k>" (k =
the pixel splits = slabs), workspace floats - and the slab bytes each HIP stream's workspace needs (the largest launch of
the stream: launches of one stream use the workspace one after the other).  The margin of every comparison is the spread
between the alternations of the same setting, stated beside it.  Every child process runs under its own timeout; run the
tool itself under one (`timeout -k 10 900 python tools/det_ab.py ...`)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
HW = 256
DET_ENTRIES = [f"ammc_conv_wgrad_{f}_det{t}" for f in ("s16", "f32") for t in ("", "_floats", "_variant")]


def _models(batch):
    import torch
    import ammcnet_aaai2021_amd as A
    from ammcnet_aaai2021_amd import harness as Hn, synthetic as S
    G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    G.load_state_dict(S.make_twostream_state())
    D = A.PixelDiscriminator(3, [128, 256, 512, 512])
    D.load_state_dict(S.make_discriminator_state())
    F2 = A.FlowNet2SD()
    F2.load_state_dict(S.make_flownet2sd_state())
    G, D, F2 = G.to(DEV).train(), D.to(DEV).train(), F2.to(DEV).eval()
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(batch, HW, HW, tag="det-ab"))
    rgb = torch.cat([rgb_x.view(batch, 4, 3, HW, HW), rgb_t[:, None]], 1)
    op = torch.cat([op_x.view(batch, 3, 2, HW, HW), op_t[:, None]], 1)
    return G, D, Hn.flownet_flow_fn(F2), rgb, op


class _Recorder:
    """wraps the library's two `_det` launch entries for one recorded iteration: (layer, label, workspace floats, stream)"""

    def __init__(self, lib):
        self.lib, self.rows, self.layer = lib, [], "?"
        self.streams = {}                                    # HIP stream handle -> index in order of first use
        self.real = {n: getattr(lib, n) for n in ("ammc_conv_wgrad_s16_det", "ammc_conv_wgrad_f32_det")}

    def _wrap(self, form):
        real = self.real[f"ammc_conv_wgrad_{form}_det"]

        def call(d_ref, *rest):
            d = d_ref._obj
            buf = C.create_string_buffer(96)
            getattr(self.lib, f"ammc_conv_wgrad_{form}_det_variant")(C.byref(d), buf, 96)
            floats = int(getattr(self.lib, f"ammc_conv_wgrad_{form}_det_floats")(C.byref(d)))
            self.rows.append({"layer": self.layer, "kernel": buf.value.decode(), "n": d.n, "cin": d.cin, "ntaps": d.ntaps,
                              "pixels": d.batch * d.height * d.width, "slab_floats": floats,
                              "stream": self.streams.setdefault(int(rest[-1] or 0), len(self.streams))})
            return real(d_ref, *rest)
        return call

    def __enter__(self):
        from ammcnet_aaai2021_amd import discriminator, train
        for form in ("s16", "f32"):
            setattr(self.lib, f"ammc_conv_wgrad_{form}_det", self._wrap(form))
        self.saved = (train._Ops.wgrad_s16, train._Ops.wgrad, discriminator._chk)
        rec = self

        def named(fn):
            def f(ops, *a, **kw):
                rec.layer = kw.get("what", "?")
                return fn(ops, *a, **kw)
            return f
        train._Ops.wgrad_s16, train._Ops.wgrad = named(self.saved[0]), named(self.saved[1])

        def chk(rc, what):                                   # the discriminator names its launch when it checks the status
            if what.startswith("disc.wgrad") and self.rows and self.rows[-1]["layer"] == "?":
                self.rows[-1]["layer"] = what.split("(")[0]
            return self.saved[2](rc, what)
        discriminator._chk = chk
        return self

    def __exit__(self, *exc):
        from ammcnet_aaai2021_amd import discriminator, train
        for n, f in self.real.items():
            setattr(self.lib, n, f)
        train._Ops.wgrad_s16, train._Ops.wgrad, discriminator._chk = self.saved


def _legs(batch, steps, settings, record=True):
    """-> {"train": {...}, "joint": {...}}: ms per step of every leg, the setting alternating `settings` three times"""
    import torch
    from ammcnet_aaai2021_amd import _lib, harness as Hn
    G, D, flow_fn, rgb, op = _models(batch)
    opt_g, opt_d = Hn.adam(G.parameters(), lr=2e-4), Hn.adam(D.parameters(), lr=2e-5)

    def run(workload, det, n):
        G.deterministic = D.deterministic = bool(det)
        for _ in range(n):
            if workload == "train":
                Hn.train_step(G, opt_g, rgb, op)
            else:
                Hn.train_step_gan(G, D, opt_g, opt_d, rgb, op, flow_fn, **Hn.LAMS_ANOPRED)
        torch.cuda.synchronize()
    out = {}
    for workload in ("train", "joint"):
        for det in settings:                                 # warm every path: workspaces, code objects, first-call work
            run(workload, det, 2)
        res = {"legs": []}
        if record and 1 in settings:
            with _Recorder(_lib.load()) as rec:
                run(workload, 1, 1)
            res["rerouted_launches"] = rec.rows
            per_stream = {}
            for r in rec.rows:
                per_stream[r["stream"]] = max(per_stream.get(r["stream"], 0), 4 * r["slab_floats"])
            res["slab_bytes_per_stream"] = sorted(per_stream.values(), reverse=True)
        for rnd in range(3):
            for det in settings:
                t0 = time.perf_counter()
                run(workload, det, steps)
                ms = (time.perf_counter() - t0) / steps * 1e3
                res["legs"].append({"round": rnd, "deterministic": det, "ms_per_step": round(ms, 3)})
                print(json.dumps({"workload": workload, **res["legs"][-1]}), flush=True)
        for det in settings:
            ms = sorted(x["ms_per_step"] for x in res["legs"] if x["deterministic"] == det)
            res[f"ms_det{det}"] = ms
            res[f"median_det{det}"] = ms[1]
            res[f"spread_det{det}"] = round(ms[-1] - ms[0], 3)
        out[workload] = res
    return out


def _default_only(batch, steps):
    """the default legs alone.  A library from before the deterministic entries loads too: they are not called here."""
    from ammcnet_aaai2021_amd import _lib
    handle = C.CDLL(_lib.LIB_PATH)
    missing = [n for n in DET_ENTRIES if not hasattr(handle, n)]
    for n in missing:
        _lib.SIGNATURES.pop(n)
    res = _legs(batch, steps, (0,), record=False)
    print("DEFAULT_ONLY " + json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "has_det_entries": not missing,
                                        **{w: {"ms": r["ms_det0"], "median": r["median_det0"], "spread": r["spread_det0"]}
                                           for w, r in res.items()}}), flush=True)


def _against(lib_path, batch, steps):
    """alternating child processes: LIB, in-tree, LIB, in-tree, LIB, in-tree - each the default legs, each under a timeout"""
    rows = []
    for rnd in range(3):
        for which, path in (("other", os.path.abspath(lib_path)), ("in-tree", None)):
            env = {k: v for k, v in os.environ.items() if k not in ("AMMC_LIB", "AMMC_DETERMINISTIC")}
            if path:
                env["AMMC_LIB"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--default-only", "--batch", str(batch), "--steps", str(steps)],
                               env=env, capture_output=True, text=True, timeout=420)
            if r.returncode != 0:                            # nothing more is started on the device
                raise SystemExit(f"child ({which}, round {rnd}) ended with {r.returncode}:\n{r.stdout[-1500:]}{r.stderr[-1500:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEFAULT_ONLY ")][-1]
            rows.append({"round": rnd, "library": which, **json.loads(line[len("DEFAULT_ONLY "):])})
            print(json.dumps(rows[-1]), flush=True)
    out = {"children": rows}
    for w in ("train", "joint"):
        for which in ("other", "in-tree"):
            med = sorted(x[w]["median"] for x in rows if x["library"] == which)
            out[f"{w}_{which}_medians"] = med
        both = out[f"{w}_other_medians"], out[f"{w}_in-tree_medians"]
        out[f"{w}_in-tree_minus_other_ms"] = round(both[1][1] - both[0][1], 3)
        out[f"{w}_margin_ms"] = round(max(m[-1] - m[0] for m in both), 3)       # the spread between alternations of ONE library
        by = {(x["round"], x["library"]): x[w]["median"] for x in rows}          # the paired view: the two children of one round
        out[f"{w}_paired_in-tree_minus_other_ms"] = [round(by[(r, "in-tree")] - by[(r, "other")], 3) for r in range(3)]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_ab.txt"))
    p.add_argument("--against", default=None, metavar="LIB")
    p.add_argument("--default-only", action="store_true")
    a = p.parse_args()
    if a.default_only:
        _default_only(a.batch, a.steps)
        return
    record = {"batch": a.batch, "size": HW, "steps_per_leg": a.steps}
    if a.against:
        record["default_path_against_" + os.path.basename(a.against)] = _against(a.against, a.batch, a.steps)
    import torch
    record["device"] = torch.cuda.get_device_name(0)
    record.update(_legs(a.batch, a.steps, (0, 1)))
    for w in ("train", "joint"):
        r = record[w]
        r["det_minus_default_ms"] = round(r["median_det1"] - r["median_det0"], 3)
        r["margin_ms"] = max(r["spread_det0"], r["spread_det1"])
    text = json.dumps(record, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write(text + "\n")


if __name__ == "__main__":
    main()
