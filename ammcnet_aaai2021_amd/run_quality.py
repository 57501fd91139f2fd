"""Frame-quality entry: `run_test`'s evaluation with the SSIM / MSE pass in place of the scoring loop (DESIGN.md section
5.19) - the three record types the reference's evaluation selects by `loss_name` (psnr_error, mse_error, ssim_error) from
one run.  The same model, checkpoint and data-source options as `run_test`; one JSON line: `run_test`'s fields plus
"mean_ssim_rgb", "mean_ssim_op" and - when labels exist - "auc_ssim" and "auc_mse", the score fusion with the SSIM
resp. the negated MSE records in place of the PSNR records.  With `--maps_dir` one `NNNN.npz` per sub-video with the
per-frame arrays of `harness.quality_subvideo` (`--ssim_maps`: the per-pixel SSIM maps as well).  One GPU: sharded map
writing is not implemented.

    python -m ammcnet_aaai2021_amd.run_quality --synthetic [--maps_dir DIR [--ssim_maps]]
    python -m ammcnet_aaai2021_amd.run_quality --synthetic --raw                         # through the input pipeline
    python -m ammcnet_aaai2021_amd.run_quality --rgb_root DIR --op_root DIR              # the reference's folder layout
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from . import _entry, harness


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--maps_dir", default=None, help="folder that receives one NNNN.npz per sub-video")
    p.add_argument("--ssim_maps", action="store_true", help="per-pixel SSIM maps [T,H,W] as well (needs --maps_dir)")
    _entry.add_common_args(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.ssim_maps and not a.maps_dir:
        raise SystemExit("--ssim_maps writes into --maps_dir: give one")
    dev = _entry.one_gpu("run_quality", "sharded map writing")
    model = _entry.load_model(a, dev)
    sources, gt, streamed = _entry.load_sources(a)

    def loop(srcs, maps_dir):
        st = _entry.stager(a, srcs, dev, streamed)
        rec = harness.evaluate_dataset_quality(model, st if streamed else srcs, a.dataset_name, a.ssim_maps,
                                               maps_dir=maps_dir, device=dev)
        return rec, st
    (rec, st), used = _entry.timed(loop, (sources[:1], None), (sources, a.maps_dir))
    out = _entry.base_report(a, model, rec["n_frames"], used, st, "quality")
    out["mean_ssim_rgb"] = float(np.mean(np.concatenate(rec["rgb_ssim_records"]).astype(np.float64)))
    out["mean_ssim_op"] = float(np.mean(np.concatenate(rec["op_ssim_records"]).astype(np.float64)))
    if a.maps_dir:
        out["maps"] = {"dir": a.maps_dir, "files": len(rec["map_files"]), "ssim_maps": bool(a.ssim_maps)}
    if gt is not None:
        out["auc"] = harness.fuse_scores_auc(rec, gt)["auc"]
        # the same fusion with the SSIM records, and with the negated MSE records (a LOWER error is the normal class; the
        # min-max normalisation of the fusion makes the sign the only thing that matters), in place of the PSNR records
        out["auc_ssim"] = harness.fuse_scores_auc({**rec, "rgb_img_pred_records": rec["rgb_ssim_records"]}, gt)["auc"]
        out["auc_mse"] = harness.fuse_scores_auc({**rec, "rgb_img_pred_records": [-m for m in rec["rgb_mse_records"]]}, gt)["auc"]
        out["auc_note"] = "synthetic labels" if a.synthetic else "labels from --data"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
