"""Anomaly localisation entry: `run_test`'s evaluation with the error-map pass in place of the scoring loop (DESIGN.md
section 5.16).  The same model, checkpoint and data-source options as `run_test`; for every sub-video one `NNNN.npz`
with the per-frame patch error maps, worst-patch scores, fixed-order PSNR and commit values of both streams
(`harness.localise_subvideo`), and one JSON line: `run_test`'s fields plus "maps" and - when labels exist - "auc_patch",
the score fusion with the worst-patch PSNR in place of the frame PSNR.  One GPU: sharded map writing is not implemented.

    python -m ammcnet_aaai2021_amd.run_maps --synthetic --maps_dir maps [--patch 8|16|32] [--pixel_maps]
    python -m ammcnet_aaai2021_amd.run_maps --synthetic --raw --maps_dir maps            # through the input pipeline
    python -m ammcnet_aaai2021_amd.run_maps --rgb_root DIR --op_root DIR --maps_dir maps  # the reference's folder layout
"""
from __future__ import annotations

import argparse
import json

from . import _entry, harness


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--maps_dir", required=True, help="folder that receives one NNNN.npz per sub-video")
    p.add_argument("--patch", type=int, default=16, choices=(8, 16, 32), help="patch size in pixels")
    p.add_argument("--pixel_maps", action="store_true", help="per-pixel error maps [T,H,W] as well")
    _entry.add_common_args(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    dev = _entry.one_gpu("run_maps", "sharded map writing")
    model = _entry.load_model(a, dev)
    sources, gt, streamed = _entry.load_sources(a)

    def loop(srcs, maps_dir):
        st = _entry.stager(a, srcs, dev, streamed)
        rec = harness.evaluate_dataset_localised(model, st if streamed else srcs, a.dataset_name, a.patch, a.pixel_maps,
                                                 maps_dir=maps_dir, device=dev)
        return rec, st
    (rec, st), used = _entry.timed(loop, (sources[:1], None), (sources, a.maps_dir))
    out = _entry.base_report(a, model, rec["n_frames"], used, st, "localisation")
    out["maps"] = {"dir": a.maps_dir, "patch": a.patch, "files": len(rec["map_files"]), "pixel": bool(a.pixel_maps)}
    if gt is not None:
        out["auc"] = harness.fuse_scores_auc(rec, gt)["auc"]
        # the same fusion with the worst-patch PSNR in place of the frame PSNR
        out["auc_patch"] = harness.fuse_scores_auc({**rec, "rgb_img_pred_records": rec["rgb_patch_psnr_records"]}, gt)["auc"]
        out["auc_note"] = "synthetic labels" if a.synthetic else "labels from --data"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
