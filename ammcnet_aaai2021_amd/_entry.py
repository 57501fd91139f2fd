"""What the evaluation entries (`run_test`, `run_maps`, `run_memory`, `run_quality`, `run_pixel`, `run_region`,
`run_localise`, `run_fusion`, `run_panels`) share: the model and data-source options, the device checks, the model, the four-way source selection, the
warm-up and timed loop, and the fields every entry's JSON line starts with."""
from __future__ import annotations

import os
import time
from typing import Callable, Optional

import numpy as np
import torch

from . import harness, parallel, pipeline, synthetic
from .unet import get_twostream


def synthetic_dataset(n_videos: int, frames: int, size: int):
    vids, gts = [], []
    for i in range(n_videos):
        t = frames + 7 * (i % 3)
        rgb = synthetic.hashed_uniform(f"rt:rgb{i}", (t, 3, size, size))
        u = synthetic.hashed_normal(f"rt:op{i}", (t - 1, 1, size, size), 2.0) / 256.0
        vids.append((rgb, torch.cat([u, u / 256.0], 1)))
        gts.append((synthetic.hashed_uniform(f"rt:gt{i}", (t,), 0, 1) > 0.8).numpy().astype(np.int8))
    return vids, gts


def synthetic_raw_sources(n_videos: int, frames: int, h: int = 240, w: int = 360):
    """decoded-frame stand-ins at a camera resolution (ped2 is 240x360): uint8 RGB frames and .flo-like flows"""
    def make(i):
        t = frames + 7 * (i % 3)
        rgb = ((synthetic.hashed_uniform(f"raw:rgb{i}", (t, h, w, 3)) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8)
        flow = synthetic.hashed_normal(f"raw:op{i}", (t - 1, h, w, 2), 2.0)
        return rgb.numpy(), flow.numpy()
    gts = [(synthetic.hashed_uniform(f"rt:gt{i}", (frames + 7 * (i % 3),), 0, 1) > 0.8).numpy().astype(np.int8)
           for i in range(n_videos)]
    return [(lambda i=i: make(i)) for i in range(n_videos)], gts


def add_common_args(p) -> None:
    """the model and the data source, as every entry takes them"""
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


def needs_gpu(name: str, dev) -> None:
    if dev.type != "cuda":
        raise SystemExit(f"{name} needs a GPU: the HIP path has no CPU fallback")


def one_gpu(name: str, not_implemented: str = ""):
    """the device of an entry that runs as a single process; `not_implemented`: what a sharded run would need"""
    _, world, dev = parallel.init_distributed()
    if world > 1:
        why = f": {not_implemented} is not implemented" if not_implemented else ""
        raise SystemExit(f"{name} runs on one GPU{why} (start a single process)")
    needs_gpu(name, dev)
    return dev


def load_model(a, dev):
    model = get_twostream((12, 6), (3, 2), a.embed_dim, a.n_embed, a.k)
    if a.ckpt:
        model.load_state_dict(torch.load(a.ckpt, map_location="cpu"), strict=True)      # test_helper.py:558
    else:
        model.load_state_dict(synthetic.make_twostream_state(embed_dim=a.embed_dim, n_embed=a.n_embed, k=a.k))
    model = model.to(dev).eval()
    model.precision = a.precision
    return model


def has_source(a) -> bool:
    return bool(a.data or (a.rgb_root and a.op_root) or a.synthetic)


def load_sources(a, options: str = "--data, --rgb_root/--op_root or --synthetic", blob: Optional[dict] = None):
    """-> (sources, gt, streamed): the sub-videos of --data (tensors), --rgb_root / --op_root (folders), --synthetic --raw
    (decoded-frame stand-ins) or --synthetic (tensors), their frame labels or None, and whether the sources are raw: such
    sources go through `stager`.  `blob`: a dict that receives the other entries of the --data file."""
    streamed = False
    if a.data:
        loaded = torch.load(a.data, map_location="cpu")
        sources, gt = loaded["videos"], loaded.get("gt")
        if blob is not None:
            blob.update(loaded)
    elif a.rgb_root and a.op_root:
        sources, gt, streamed = pipeline.list_subvideos(a.rgb_root, a.op_root), None, True
    elif a.synthetic and a.raw:
        (sources, gt), streamed = synthetic_raw_sources(a.videos, a.frames), True
    elif a.synthetic:
        sources, gt = synthetic_dataset(a.videos, a.frames, a.size)
    else:
        raise SystemExit(f"give {options}")
    return sources, gt, streamed


RAW_SIZE = (240, 360)        # `synthetic_raw_sources`' camera resolution


def masks_from_root(names, mask_root: str):
    """`names`: the sub-video folder names in evaluation order -> [T, h0, w0] arrays read from mask_root/<name>.npy, None
    where there is no such file; a .npy file that matches no sub-video raises ValueError"""
    known = set(names)
    stray = sorted(f for f in os.listdir(mask_root) if f.endswith(".npy") and f[:-4] not in known)
    if stray:
        raise ValueError(f"--mask_root {mask_root}: {stray} match no sub-video folder ({len(known)} folders)")
    out = []
    for name in names:
        path = os.path.join(mask_root, name + ".npy")
        out.append(np.load(path) if os.path.isfile(path) else None)
    return out


def load_masks(a, sources, blob: dict, synthetic_masks: Callable) -> list:
    """the pixel ground truth of `load_sources`' sub-videos, one [T, h0, w0] array or None each: the "masks" list of the
    --data blob, the files of --mask_root, or `synthetic_masks(videos, frames, h, w)` (SystemExit where they are missing,
    stray, or not one per sub-video)"""
    if a.data:
        masks = blob.get("masks")
        if masks is None:
            raise SystemExit("--data: the blob has no 'masks' list (one [T,h,w] array or None per sub-video)")
    elif a.rgb_root and a.op_root:
        try:
            masks = masks_from_root(sorted(os.listdir(a.rgb_root)), a.mask_root)
        except ValueError as e:
            raise SystemExit(str(e)) from None
    else:
        masks = synthetic_masks(a.videos, a.frames, *(RAW_SIZE if a.raw else (a.size, a.size)))
    if len(masks) != len(sources):
        raise SystemExit(f"{len(masks)} masks for {len(sources)} sub-videos")
    return masks


def stager(a, sources, dev, streamed: bool, shard=(0, 1)):
    """raw inputs stream: sub-video v + 1 / v + 2 are read, uploaded and resized on a side stream while v is scored"""
    return pipeline.SubVideoStager(sources, dev, size=(a.size, a.size), shard=shard, ahead=2) if streamed else None


def timed(loop, warm_args, args):
    """`loop(*warm_args)` (plans, packs, pinned pools), then `loop(*args)` between two device synchronisations
    -> (its result, seconds)"""
    loop(*warm_args)
    torch.cuda.synchronize()
    t0 = time.time()
    out = loop(*args)
    torch.cuda.synchronize()
    return out, time.time() - t0


def base_report(a, model, n_frames, used: float, st=None, noun: str = "scoring", gpus: int = 1) -> dict:
    """the fields every entry's JSON line starts with (test_helper.py:485-486); `st`: the run's `SubVideoStager`, if
    any; `noun`: what the staging note calls the loop it overlapped with"""
    n_pred = sum(t - harness.RGB_LEN_CLIP + 1 for t in n_frames)
    out = {"dataset": a.dataset_name, "videos": len(n_frames), "predicted_frames": n_pred, "gpus": gpus,
           "total_time_s": round(used, 3), "fps": round(n_pred / used, 2), "precision": a.precision,
           "s16_fallbacks": getattr(model, "s16_fallbacks", 0)}
    if st is not None:
        out.update(host_read_s=round(st.host_seconds, 3), uploaded_MB=round(st.bytes_uploaded / 2**20, 1),
                   staging=f"streamed: overlapped with the {noun} loop (total_time_s covers it)")
    return out
