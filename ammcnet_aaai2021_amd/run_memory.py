"""Per-clip memory scores entry: `run_test`'s evaluation with the memory-score pass behind every forward (DESIGN.md section
5.17).  The same model, checkpoint and data-source options as `run_test`; one JSON line: `run_test`'s fields plus "maps"
(the number of `NNNN.npz` files written, one per sub-video, when `--maps_dir` is given: the arrays of
`harness.memory_subvideo` - per-frame commit maps on the H/8 x W/8 bottleneck grid, per-clip commit distances, their
worst positions, PSNR, the reference's per-batch commit values and, with `--slots`, the memory items addressed) and - when
labels exist - "auc_clip", the score fusion with the per-clip commit distances in place of the per-batch ones.  One GPU:
sharded map writing is not implemented.

    python -m ammcnet_aaai2021_amd.run_memory --synthetic [--maps_dir maps] [--slots]
    python -m ammcnet_aaai2021_amd.run_memory --synthetic --raw --maps_dir maps            # through the input pipeline
    python -m ammcnet_aaai2021_amd.run_memory --rgb_root DIR --op_root DIR --maps_dir maps  # the reference's folder layout
"""
from __future__ import annotations

import argparse
import json
import time

import torch

from . import harness, parallel, pipeline, synthetic
from .run_test import synthetic_dataset, synthetic_raw_sources
from .unet import get_twostream


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--maps_dir", default=None, help="folder that receives one NNNN.npz per sub-video (optional)")
    p.add_argument("--slots", action="store_true", help="the k nearest memory items per position [T,H/8,W/8,k] as well")
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
    _, world, dev = parallel.init_distributed()
    if world > 1:
        raise SystemExit("run_memory runs on one GPU: sharded map writing is not implemented (start a single process)")
    if dev.type != "cuda":
        raise SystemExit("run_memory needs a GPU: the HIP path has no CPU fallback")
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
        rec = harness.evaluate_dataset_memory(model, st if streamed else srcs, a.dataset_name, a.slots, maps_dir=maps_dir,
                                              device=dev)
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
                   staging="streamed: overlapped with the scoring loop (total_time_s covers it)")
    out["maps"] = len(rec["map_files"])
    if gt is not None:
        out["auc"] = harness.fuse_scores_auc(rec, gt)["auc"]
        # the same fusion with the per-clip commit distances in place of the per-batch ones
        out["auc_clip"] = harness.fuse_scores_auc({**rec, "rgb_fea_comm_records": rec["rgb_clip_comm_records"],
                                                   "op_fea_comm_records": rec["op_clip_comm_records"]}, gt)["auc"]
        out["auc_note"] = "synthetic labels" if a.synthetic else "labels from --data"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
