"""Qualitative evaluation entry: `run_test`'s evaluation with pictures.  The same model,
checkpoint and data-source options as `run_test`; every sub-video is scored by the localisation loop (`run_maps`'
records), then the batches that hold a chosen frame run again with the render pass behind the forward
(`harness.render_subvideo`, `ops.render_panels`): per frame one panel of tiles - the target and predicted frame, the
heat map of their per-pixel error, the colour-coded target and predicted flow, the heat map of the flow error - written
to `--panels_dir`/NNNN/FFFFFF.png (sub-video, frame) by a pool of writer threads.  One JSON line: `run_test`'s fields
plus "panels_written", "render_ms_per_batch" (the render launches between device events), "write_s" (the writers'
busy seconds, summed over the threads), "fps" (pictures on disk) and "fps_no_writers" (the time this process waited for
the writers taken out).  One GPU.

    python -m ammcnet_aaai2021_amd.run_panels --synthetic --panels_dir panels
    python -m ammcnet_aaai2021_amd.run_panels --synthetic --panels_dir panels --top 10          # the 10 worst frames of each sub-video
    python -m ammcnet_aaai2021_amd.run_panels --rgb_root DIR --op_root DIR --panels_dir panels --every 5 --heat_max 0.05

--tiles: names separated by commas, rows by '/', an ordered subset of rgb_target, rgb_pred, rgb_heat, op_target,
op_pred, op_heat (default all six: rgb_target,rgb_pred,rgb_heat/op_target,op_pred,op_heat).
--flow_norm target: both flow tiles by the target flow's largest radius (comparable with each other; default);
each: every flow by its own (the reference's per-image colouring); a number: that radius for every frame.
--heat_max frame: a heat tile is scaled by its own frame's largest error (default: every picture uses the whole
colour range, and says nothing about how large the error is); a number V: the error that maps to the hottest colour,
the same for every frame - pictures of different frames are then COMPARABLE (errors are on the [0, 1] range, squared).
--every N: every N-th predicted frame.  --top K: only the K frames of each sub-video with the lowest PSNR.
Flows are scaled by (H, W) before they are coloured, as the reference's `get_vis_tensor` does (without its uint8 cast).
"""
from __future__ import annotations

import argparse
import json

from . import _entry, harness

MAX_WORKERS = harness.OrderedWriterPool.MAX_WORKERS


def parse_tiles(text: str):
    """'a,b/c,d' -> [['a', 'b'], ['c', 'd']], checked by `harness.panel_layout` (ValueError)"""
    rows = [[t.strip() for t in row.split(",") if t.strip()] for row in text.split("/")]
    return harness.panel_layout([row for row in rows if row] or [[]])


def mode_or_number(text: str, modes, what: str):
    """one of `modes`, or a positive finite number (ValueError otherwise)"""
    if text in modes:
        return text
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{what} must be {' | '.join(modes)} or a positive number, got {text!r}") from None
    if not 0.0 < v < float("inf"):
        raise ValueError(f"{what} must be {' | '.join(modes)} or a positive number, got {text!r}")
    return v


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--panels_dir", required=True, help="folder that receives NNNN/FFFFFF.png per sub-video and frame")
    p.add_argument("--format", default="png", choices=("png", "npy"))
    p.add_argument("--tiles", default="/".join(",".join(row) for row in harness.RENDER_DEFAULT_TILES))
    p.add_argument("--flow_norm", default="target", help="target | each | a radius")
    p.add_argument("--heat_max", default="frame", help="frame | the error that maps to the hottest colour")
    p.add_argument("--alpha", type=float, default=0.6, help="weight of the heat colour over the grey frame, 0 .. 1")
    p.add_argument("--every", type=int, default=1, help="every N-th predicted frame")
    p.add_argument("--top", type=int, default=None, help="only the K lowest-PSNR frames of each sub-video")
    p.add_argument("--workers", type=int, default=8, help=f"writer threads (at most {MAX_WORKERS})")
    _entry.add_common_args(p)
    return p


def parse_options(argv=None):
    """the parsed arguments with `tiles`, `flow_norm`, `heat_max` and `workers` in the form the harness takes; a bad
    value ends the run (SystemExit) before anything touches the device"""
    a = build_parser().parse_args(argv)
    try:
        a.tiles = parse_tiles(a.tiles)
        a.flow_norm = mode_or_number(a.flow_norm, ("target", "each"), "--flow_norm")
        a.heat_max = mode_or_number(a.heat_max, ("frame",), "--heat_max")
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if not 0.0 <= a.alpha <= 1.0:
        raise SystemExit(f"--alpha must lie in [0, 1], got {a.alpha}")
    if a.every < 1:
        raise SystemExit(f"--every N needs N >= 1, got {a.every}")
    if a.top is not None and a.top < 1:
        raise SystemExit(f"--top K needs K >= 1, got {a.top}")
    if a.workers < 1:
        raise SystemExit(f"--workers needs at least 1, got {a.workers}")
    a.workers = min(a.workers, MAX_WORKERS)
    if not _entry.has_source(a):
        raise SystemExit("give --data, --rgb_root/--op_root or --synthetic")
    return a


def main(argv=None):
    a = parse_options(argv)
    dev = _entry.one_gpu("run_panels", "sharded picture writing")
    model = _entry.load_model(a, dev)
    sources, gt, streamed = _entry.load_sources(a)

    def loop(srcs, panels_dir, stats):
        st = _entry.stager(a, srcs, dev, streamed)
        rec = harness.evaluate_dataset_panels(model, st if streamed else srcs, a.dataset_name, panels_dir, a.format, a.every,
                                              a.top, a.workers, device=dev, stats=stats, tiles=a.tiles, flow_norm=a.flow_norm,
                                              heat_max=a.heat_max, alpha=a.alpha)
        return rec, st
    stats: dict = {}
    (rec, st), used = _entry.timed(loop, (sources[:1], None, None), (sources, a.panels_dir, stats))
    out = _entry.base_report(a, model, rec["n_frames"], used, st, "evaluation")
    n_pred = out["predicted_frames"]
    if gt is not None:
        out["auc"] = harness.fuse_scores_auc(rec, gt)["auc"]
        out["auc_note"] = "synthetic labels" if a.synthetic else "labels from --data"
    batches = max(stats.get("render_batches", 0), 1)
    out.update(panels_written=len(rec["panel_files"]), panels_dir=a.panels_dir, format=a.format,
               tiles="/".join(",".join(row) for row in a.tiles),
               render_ms_per_batch=round(stats.get("render_ms", 0.0) / batches, 4), render_batches=stats.get("render_batches", 0),
               write_s=round(stats.get("write_s", 0.0), 3), writers=a.workers,
               fps_no_writers=round(n_pred / max(used - stats.get("write_wait_s", 0.0), 1e-9), 2),
               fps_note="every sub-video is scored, then the batches with a chosen frame run again with the render pass")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
