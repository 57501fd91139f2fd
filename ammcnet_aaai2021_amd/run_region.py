"""Region-based evaluation entry: `run_test`'s evaluation with the connected-component pass behind the forward (DESIGN.md
section 5.24).  The same model, checkpoint and data-source options as `run_test` and the mask sources of `run_pixel`;
one JSON line: `run_test`'s fields and the figures of `harness.region_level_auc` - "rbdc" (the region-based detection
criterion of Ramachandra and Jones on the per-pixel error map: the area under detected-region rate against false-positive
regions per frame, up to one per frame), "tbdc" (the same per track), "rbdc_patch", "tbdc_patch" (on the patch map).  One
GPU.

    python -m ammcnet_aaai2021_amd.run_region --synthetic [--patch 8|16|32] [--iou 1 10] [--alpha 1 10] [--thresholds 64]
    python -m ammcnet_aaai2021_amd.run_region --synthetic --spacing log --log_floor 1e-3 --out curves.npz
    python -m ammcnet_aaai2021_amd.run_region --rgb_root DIR --op_root DIR --mask_root DIR  # the reference's folder layout
    python -m ammcnet_aaai2021_amd.run_region --data blob.pt                        # its optional "masks" list

Masks: as `run_pixel` takes them (`--data`: the blob's "masks"; `--mask_root DIR`: DIR/<sub-video folder name>.npy;
`--synthetic`: `synthetic_region_masks`).  The mask files carry no track identity: tracks are derived from the overlap
of the regions of consecutive frames, and the JSON line says so in "track_note".  A frame may hold at most 32 regions
(`--min_gt_area` drops specks).
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import _entry, harness, synthetic


def synthetic_region_masks(n_videos: int, frames: int, h: int, w: int):
    """deterministic stand-ins for region ground truth: uint8 [T, h, w] per sub-video with the lengths of
    `run_test.synthetic_dataset` (frames + 7 * (i % 3)); about a fifth of the frames carry one to three rectangles of
    ones (which may touch or overlap: then they are one region)"""
    out = []
    for i in range(n_videos):
        t = frames + 7 * (i % 3)
        u = synthetic.hashed_uniform(f"rr:mask{i}", (t, 14), 0, 1).numpy()
        mk = np.zeros((t, h, w), dtype=np.uint8)
        for f in np.nonzero(u[:, 0] > 0.8)[0]:
            for k in range(1 + min(2, int(u[f, 1] * 3))):
                a = u[f, 2 + 4 * k:6 + 4 * k]
                rh, rw = 1 + int(a[0] * (h // 3)), 1 + int(a[1] * (w // 3))
                y0, x0 = int(a[2] * (h - rh + 1)), int(a[3] * (w - rw + 1))
                mk[f, y0:min(y0 + rh, h), x0:min(x0 + rw, w)] = 1
        out.append(mk)
    return out


def _pair(name: str, v, top=None):
    num, den = v
    if not 1 <= num <= den or (top is not None and den > top):
        raise SystemExit(f"--{name} NUM DEN needs 1 <= NUM <= DEN{'' if top is None else f' <= {top}'}, got {num} {den}")
    return num, den


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--patch", type=int, default=16, choices=(8, 16, 32), help="patch size of the patch map in pixels")
    p.add_argument("--iou", type=int, nargs=2, default=[1, 10], metavar=("NUM", "DEN"),
                   help="a detected region matches a ground-truth region at IoU >= NUM / DEN")
    p.add_argument("--alpha", type=int, nargs=2, default=[1, 10], metavar=("NUM", "DEN"),
                   help="a track is detected when NUM / DEN of its regions are")
    p.add_argument("--thresholds", type=int, default=64, metavar="T", help="the number of thresholds")
    p.add_argument("--spacing", default="linear", choices=("linear", "log"), help="i / T, or log_floor ** ((T - i) / T)")
    p.add_argument("--log_floor", type=float, default=1e-3, help="the smallest value of --spacing log is above it")
    p.add_argument("--normalise", default="video", choices=("video", "none"),
                   help="thresholds times a sub-video's largest map value, or times --t_max")
    p.add_argument("--t_max", type=float, default=None, help="with --normalise none: the largest threshold")
    p.add_argument("--min_area", type=int, default=1, help="detected regions with fewer pixels are dropped")
    p.add_argument("--min_gt_area", type=int, default=1, help="ground-truth regions with fewer pixels are dropped")
    p.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    p.add_argument("--mask_root", default=None, help="with --rgb_root / --op_root: folder of <sub-video folder name>.npy masks [T,h,w]")
    p.add_argument("--out", default=None, metavar="CURVES.npz", help="save the curves (fpr, rbdr, tbdr, ..._patch)")
    _entry.add_common_args(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    iou, alpha = _pair("iou", a.iou, 4096), _pair("alpha", a.alpha)
    if a.thresholds < 1 or a.min_area < 1 or a.min_gt_area < 1:
        raise SystemExit("--thresholds, --min_area and --min_gt_area need values >= 1")
    if a.normalise == "none" and (a.t_max is None or not a.t_max > 0):
        raise SystemExit("--normalise none needs --t_max > 0, the largest threshold")
    try:
        values = harness.region_thresholds(a.thresholds, a.spacing, a.log_floor)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    dev = _entry.one_gpu("run_region", "sharded region-based evaluation")
    model = _entry.load_model(a, dev)
    if not a.data and a.rgb_root and a.op_root and not a.mask_root:
        raise SystemExit("--rgb_root / --op_root need --mask_root DIR for the pixel ground truth")
    blob: dict = {}
    sources, gt, streamed = _entry.load_sources(a, blob=blob)
    masks = _entry.load_masks(a, sources, blob, synthetic_region_masks)

    def loop(srcs, mks):
        st = _entry.stager(a, srcs, dev, streamed)
        rec = harness.evaluate_dataset_region(model, st if streamed else srcs, mks, a.dataset_name, a.patch, values, iou,
                                              a.min_area, a.connectivity, a.normalise, a.t_max, a.min_gt_area, device=dev)
        return rec, st
    try:
        (rec, st), used = _entry.timed(loop, (sources[:1], masks[:1]), (sources, masks))
    except ValueError as e:
        if "--min_gt_area" in str(e):
            raise SystemExit(str(e)) from None
        raise
    out = _entry.base_report(a, model, rec["n_frames"], used, st, "region-based")
    if gt is not None:
        out["auc"] = harness.fuse_scores_auc(rec, gt)["auc"]
    fig = harness.region_level_auc(rec, alpha)
    curves = fig.pop("curves")
    out.update(fig)
    out.update(iou=list(iou), alpha=list(alpha), patch=a.patch, thresholds=a.thresholds, spacing=a.spacing, normalise=a.normalise,
               min_area=a.min_area, min_gt_area=a.min_gt_area, connectivity=a.connectivity, mask_videos=len(rec["mask_videos"]))
    out["auc_note"] = "synthetic masks" if a.synthetic else ("masks from --data" if a.data else "masks from --mask_root")
    if a.out:
        np.savez(a.out, values=values, **curves)
        out["curves_file"] = a.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
