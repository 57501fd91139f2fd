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

from . import _entry, harness


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--maps_dir", default=None, help="folder that receives one NNNN.npz per sub-video (optional)")
    p.add_argument("--slots", action="store_true", help="the k nearest memory items per position [T,H/8,W/8,k] as well")
    _entry.add_common_args(p)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    dev = _entry.one_gpu("run_memory", "sharded map writing")
    model = _entry.load_model(a, dev)
    sources, gt, streamed = _entry.load_sources(a)

    def loop(srcs, maps_dir):
        st = _entry.stager(a, srcs, dev, streamed)
        rec = harness.evaluate_dataset_memory(model, st if streamed else srcs, a.dataset_name, a.slots, maps_dir=maps_dir,
                                              device=dev)
        return rec, st
    (rec, st), used = _entry.timed(loop, (sources[:1], None), (sources, a.maps_dir))
    out = _entry.base_report(a, model, rec["n_frames"], used, st, "scoring")
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
