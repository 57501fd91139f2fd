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
import time

import numpy as np
import torch

from . import harness, parallel, pipeline, synthetic
from .run_test import synthetic_dataset, synthetic_raw_sources
from .unet import get_twostream


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--maps_dir", default=None, help="folder that receives one NNNN.npz per sub-video")
    p.add_argument("--ssim_maps", action="store_true", help="per-pixel SSIM maps [T,H,W] as well (needs --maps_dir)")
    # the model and the data source, as run_test takes them
    p.add_argument("--dataset_name", default="ped2", choices=sorted(harness.LAM_MAP))
    p.add_argument("--ckpt", default=None, help="state_dict of the reference's twostream generator (.pth)")
    p.add_argument("--data", default=None, help="torch.save'd dict with 'videos' and optional 'gt'")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--raw", action="store_true", help="with --synthetic: uint8 frames + flows through pipeline.SubVideoStager")
    p.add_argument("--rgb_root", default=None, help="folder of sub-video folders of frames (jpg/png/.npy)")
    p.add_argument("--op_root", default=None, help="folder of sub-video folders of flows (.flo/.npy)")
    p.add_argument("--videos", type=int, default=4)
    p.add_argument("--frames", type=int, default=60)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--precision", choices=("fp32", "s16"), default="s16")
    p.add_argument("--embed_dim", type=int, default=64)
    p.add_argument("--n_embed", type=int, default=256)
    p.add_argument("--k", type=int, default=2)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.ssim_maps and not a.maps_dir:
        raise SystemExit("--ssim_maps writes into --maps_dir: give one")
    _, world, dev = parallel.init_distributed()
    if world > 1:
        raise SystemExit("run_quality runs on one GPU: sharded map writing is not implemented (start a single process)")
    if dev.type != "cuda":
        raise SystemExit("run_quality needs a GPU: the HIP path has no CPU fallback")
    model = get_twostream((12, 6), (3, 2), a.embed_dim, a.n_embed, a.k)
    if a.ckpt:
        model.load_state_dict(torch.load(a.ckpt, map_location="cpu"), strict=True)
    else:
        model.load_state_dict(synthetic.make_twostream_state(embed_dim=a.embed_dim, n_embed=a.n_embed, k=a.k))
    model = model.to(dev).eval()
    model.precision = a.precision
    streamed = bool(a.rgb_root and a.op_root or (a.synthetic and a.raw))
    if a.data:
        blob = torch.load(a.data, map_location="cpu")
        sources, gt = blob["videos"], blob.get("gt")
    elif a.rgb_root and a.op_root:
        sources, gt = pipeline.list_subvideos(a.rgb_root, a.op_root), None
    elif a.synthetic and a.raw:
        sources, gt = synthetic_raw_sources(a.videos, a.frames)
    elif a.synthetic:
        sources, gt = synthetic_dataset(a.videos, a.frames, a.size)
    else:
        raise SystemExit("give --data, --rgb_root/--op_root or --synthetic")

    def loop(srcs, maps_dir):
        # raw inputs stream: sub-video v + 1 / v + 2 are read, uploaded and resized on a side stream while v is scored
        st = pipeline.SubVideoStager(srcs, dev, size=(a.size, a.size), shard=(0, 1), ahead=2) if streamed else None
        rec = harness.evaluate_dataset_quality(model, st if streamed else srcs, a.dataset_name, a.ssim_maps,
                                               maps_dir=maps_dir, device=dev)
        return rec, st
    loop(sources[:1], None)                                                      # warm-up: plans, packs, pinned pools
    torch.cuda.synchronize()
    t0 = time.time()
    rec, st = loop(sources, a.maps_dir)
    torch.cuda.synchronize()
    used = time.time() - t0
    n_pred = sum(t - harness.RGB_LEN_CLIP + 1 for t in rec["n_frames"])
    out = {"dataset": a.dataset_name, "videos": len(rec["n_frames"]), "predicted_frames": n_pred, "gpus": 1,
           "total_time_s": round(used, 3), "fps": round(n_pred / used, 2), "precision": a.precision,
           "s16_fallbacks": getattr(model, "s16_fallbacks", 0)}
    if st is not None:
        out.update(host_read_s=round(st.host_seconds, 3), uploaded_MB=round(st.bytes_uploaded / 2**20, 1),
                   staging="streamed: overlapped with the quality loop (total_time_s covers it)")
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
