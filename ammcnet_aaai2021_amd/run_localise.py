"""Fused localisation entry: `run_test`'s evaluation with the fused-map pass behind the forward.
The rgb error map, the flow error map and the two memory blocks' commit maps are weighted, summed, smoothed by a box window
(`ops.fuse_maps`) and scored by the pixel-level criterion of `run_pixel` and the region-based criterion of `run_region` -
every weight vector of --weights from ONE forward of the data set.  The same model, checkpoint and data-source options as
`run_test` and the mask sources of `run_pixel`; one JSON line: `run_test`'s fields, "settings" (per weight vector its
"auc_pixel", "auc_pixel_patch", "auc_frame_max", "pointing", "rbdc", "tbdc", "rbdc_patch", "tbdc_patch"), "best" (the
setting with the largest "auc_pixel", the first one on ties), "radius", "normalise", "track_note".  One GPU.

    python -m ammcnet_aaai2021_amd.run_localise --synthetic --weights "1,0,0,0;1,1,0,0;1,1,1,1" [--radius 2]
    python -m ammcnet_aaai2021_amd.run_localise --synthetic --normalise none --scales 1,4,0.5,0.5 --no_region
    python -m ammcnet_aaai2021_amd.run_localise --rgb_root DIR --op_root DIR --mask_root DIR --out figures.npz
    python -m ammcnet_aaai2021_amd.run_localise --data blob.pt                      # its optional "masks" list

Weights: settings separated by ';', at most 8, each 1..4 values >= 0 (not all 0) for the channels rgb_err, op_err,
rgb_commit, op_commit in that order.  --normalise video divides each channel by its largest value over the sub-video
before weighting; --normalise none multiplies it by --scales instead.  Masks: as `run_region` takes them.
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import _entry, harness
from .run_region import _pair, synthetic_region_masks

FIGURES = ("auc_pixel", "auc_pixel_patch", "auc_frame_max", "pointing", "rbdc", "tbdc", "rbdc_patch", "tbdc_patch")


def parse_weights(text: str):
    """"1,0,0,0;1,1,1,1" -> [[1, 0, 0, 0], [1, 1, 1, 1]], checked by `harness.check_fusion_weights` (SystemExit otherwise)"""
    try:
        rows = [[float(v) for v in part.split(",")] for part in text.split(";") if part.strip()]
    except ValueError:
        raise SystemExit(f"--weights: numbers separated by ',' in settings separated by ';', got {text!r}") from None
    try:
        return harness.check_fusion_weights(rows)
    except ValueError as e:
        raise SystemExit(f"--weights: {e}") from None


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--weights", default="1,0,0,0;1,1,0,0;1,1,1,1", help="weight vectors over rgb_err,op_err,rgb_commit,op_commit, ';' between settings")
    p.add_argument("--radius", type=int, default=2, metavar="R", help="the box window is (2 R + 1)^2 pixels, R in 0..8")
    p.add_argument("--normalise", default="video", choices=("video", "none"),
                   help="each channel divided by its largest value over the sub-video, or multiplied by --scales")
    p.add_argument("--scales", default=None, metavar="a,b,c,d", help="with --normalise none: one factor per channel (default 1)")
    p.add_argument("--patch", type=int, default=16, choices=(8, 16, 32), help="patch size of the patch map in pixels")
    p.add_argument("--frac", type=int, nargs=2, default=[2, 5], metavar=("NUM", "DEN"),
                   help="the share of the ground-truth pixels that must be detected (2 5: the 40 %% rule)")
    p.add_argument("--no_region", action="store_true", help="leave the region-based criterion out (rbdc, tbdc)")
    p.add_argument("--thresholds", type=int, default=64, metavar="T", help="the number of thresholds of the region criterion")
    p.add_argument("--spacing", default="linear", choices=("linear", "log"), help="i / T, or 1e-3 ** ((T - i) / T)")
    p.add_argument("--iou", type=int, nargs=2, default=[1, 10], metavar=("NUM", "DEN"),
                   help="a detected region matches a ground-truth region at IoU >= NUM / DEN")
    p.add_argument("--alpha", type=int, nargs=2, default=[1, 10], metavar=("NUM", "DEN"),
                   help="a track is detected when NUM / DEN of its regions are")
    p.add_argument("--min_area", type=int, default=1, help="detected regions with fewer pixels are dropped")
    p.add_argument("--min_gt_area", type=int, default=1, help="ground-truth regions with fewer pixels are dropped")
    p.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    p.add_argument("--mask_root", default=None, help="with --rgb_root / --op_root: folder of <sub-video folder name>.npy masks [T,h,w]")
    p.add_argument("--out", default=None, metavar="FILE.npz", help="save the weights and every setting's figures and region curves")
    _entry.add_common_args(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    weights = parse_weights(a.weights)
    n_ch = len(weights[0])
    if not 0 <= a.radius <= 8:
        raise SystemExit(f"--radius needs a value in 0..8, got {a.radius}")
    frac, iou, alpha = _pair("frac", a.frac, 4096), _pair("iou", a.iou, 4096), _pair("alpha", a.alpha)
    if a.thresholds < 1 or a.min_area < 1 or a.min_gt_area < 1:
        raise SystemExit("--thresholds, --min_area and --min_gt_area need values >= 1")
    scales = None
    if a.scales is not None:
        if a.normalise != "none":
            raise SystemExit("--scales goes with --normalise none")
        try:
            scales = [float(v) for v in a.scales.split(",")]
        except ValueError:
            raise SystemExit(f"--scales: numbers separated by ',', got {a.scales!r}") from None
        if len(scales) != n_ch or not all(np.isfinite(v) and v >= 0 for v in scales):
            raise SystemExit(f"--scales: {n_ch} finite values >= 0 (one per weight), got {a.scales!r}")
    values = harness.region_thresholds(a.thresholds, a.spacing)
    dev = _entry.one_gpu("run_localise", "sharded fused localisation")
    model = _entry.load_model(a, dev)
    if not a.data and a.rgb_root and a.op_root and not a.mask_root:
        raise SystemExit("--rgb_root / --op_root need --mask_root DIR for the pixel ground truth")
    blob: dict = {}
    sources, gt, streamed = _entry.load_sources(a, blob=blob)
    masks = _entry.load_masks(a, sources, blob, synthetic_region_masks)

    def loop(srcs, mks):
        st = _entry.stager(a, srcs, dev, streamed)
        rec = harness.evaluate_dataset_fused(model, st if streamed else srcs, mks, weights, a.dataset_name, a.radius, a.patch, frac,
                                             values, not a.no_region, a.normalise, scales, iou, a.min_area, a.connectivity,
                                             min_gt_area=a.min_gt_area, device=dev)
        return rec, st
    try:
        (rec, st), used = _entry.timed(loop, (sources[:1], masks[:1]), (sources, masks))
    except ValueError as e:
        if "--min_gt_area" in str(e) or "budget" in str(e):
            raise SystemExit(str(e)) from None
        raise
    first = rec["settings"][0]
    out = _entry.base_report(a, model, first["n_frames"], used, st, "fused localisation")
    if gt is not None:
        out["auc"] = harness.fuse_scores_auc(first, gt)["auc"]
    settings, saved = [], {"weights": np.asarray(weights, dtype=np.float32)}
    for gi, one in enumerate(rec["settings"]):
        fig = harness.pixel_level_auc(one)
        if not a.no_region:
            reg = harness.region_level_auc(one, alpha)
            for key, arr in reg.pop("curves").items():
                saved[f"{key}_{gi}"] = arr
            out["track_note"] = reg["track_note"]
            fig.update(reg)
        entry = {"weights": weights[gi]}
        entry.update({key: fig.get(key) for key in FIGURES if not (a.no_region and key[:4] in ("rbdc", "tbdc"))})
        settings.append(entry)
        out.update(n_anomalous=fig["n_anomalous"], n_normal=fig["n_normal"])
    out["settings"] = settings
    ranked = [(-s["auc_pixel"], gi) for gi, s in enumerate(settings) if s["auc_pixel"] is not None]
    out["best"] = dict(settings[min(ranked)[1]], index=min(ranked)[1]) if ranked else None
    out.update(radius=a.radius, normalise=a.normalise, scales=scales, channels=list(harness.FUSE_CHANNELS[:n_ch]), patch=a.patch,
               frac=list(frac), region=not a.no_region, mask_videos=len(first["mask_videos"]))
    if not a.no_region:
        out.update(iou=list(iou), alpha=list(alpha), thresholds=a.thresholds, spacing=a.spacing, min_area=a.min_area,
                   min_gt_area=a.min_gt_area, connectivity=a.connectivity)
    else:
        out["track_note"] = None
    out["auc_note"] = "synthetic masks" if a.synthetic else ("masks from --data" if a.data else "masks from --mask_root")
    if a.out:
        for key in FIGURES:
            saved[key] = np.asarray([np.nan if s.get(key) is None else s[key] for s in settings], dtype=np.float64)
        np.savez(a.out, values=values, **saved)
        out["figures_file"] = a.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
