"""Host-side counterparts of the two callers of the path (the reference's harness files do not
travel and are not importable without cv2/tensorboardX).

* `evaluate_subvideo` / `evaluate_dataset`: the scoring loop of
  `run_helper/test_helper.py:408-488` - sliding clips in order, batches of 16 (last one
  short), per-sample PSNR (`utils/utils.py:130-148`), ONE commit value per batch written to
  every frame of the batch, first `len_clip-1` frames back-filled - and the record dict the
  reference pickles (`:479-484`).  Multi-GPU: whole batches are sharded across ranks
  (`parallel.shard_batches`), never split.
* `generator_loss` / `train_step`: the G-only objective of SURVEY.md 3.2 (the part of
  `Twostream_vq_Loss`, `models/losses/loss_zoo.py:323-336`, that exercises the path's backward):
  lam_lp * L2norm(rgb) + lam_lp_op * L2norm(op) + lam_latent * (rgb_diff + op_diff).

The model is any callable with the reference's forward signature; with the HIP modules the
loop makes one device->host copy per BATCH (the reference syncs once per frame, `:452-453`).
"""
from __future__ import annotations

import contextlib
import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import parallel

EVAL_BATCH = 16            # hard-coded in the reference (test_helper.py:414-417)
RGB_LEN_CLIP, OP_LEN_CLIP = 5, 4


def psnr_per_sample(gen: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """[B] PSNR on the [0,1] range (utils/utils.py:141-148 applied to each sample)"""
    n = gen.shape[1] * gen.shape[2] * gen.shape[3]
    sq = ((gt + 1.0) / 2.0 - (gen + 1.0) / 2.0) ** 2
    return 10.0 * torch.log10(1.0 / ((1.0 / n) * sq.sum(dim=[1, 2, 3])))


def subvideo_batches(n_frames: int, batch: int = EVAL_BATCH, rgb_len_clip: int = RGB_LEN_CLIP):
    """[(first clip, last clip + 1)] of one sub-video, in order, last batch short"""
    n_clip = n_frames - rgb_len_clip + 1
    return [(s, min(s + batch, n_clip)) for s in range(0, max(n_clip, 0), batch)]


def clip_windows(frames: torch.Tensor, s: int, e: int, n_in: int) -> torch.Tensor:
    """clips [s, e) of a contiguous [T, c, H, W] sub-video as ONE overlapping view [e - s, n_in * c, H, W]: clip i is
    `frames[i:i + n_in].view(n_in * c, H, W)` (test_helper.py:433-438), so consecutive clips are one frame apart"""
    _, c, h, w = frames.shape
    return frames.as_strided((e - s, n_in * c, h, w), (c * h * w, h * w, w, 1), frames.storage_offset() + s * c * h * w)


def score_batch_device(model: Callable, rgb_frames: torch.Tensor, op_frames: torch.Tensor, s: int, e: int,
                       device=None, exact: bool = False) -> torch.Tensor:
    """run clips [s, e) of a sub-video as ONE batch; returns [2 b + 3] on the model's device: per-clip rgb PSNR, per-clip
    flow PSNR, the batch's two commit values and the S16 range flag of the batch (0 / 1; always 0 for models without
    one) - nothing is copied to the host, so batches can be queued back to back.  `exact`: run the HIP model's
    exact-fp32 kernels (the re-run of a flagged batch)."""
    b = e - s
    resident = device is None or (rgb_frames.device == torch.device(device) and op_frames.device == torch.device(device))
    if resident and rgb_frames.is_contiguous() and op_frames.is_contiguous():
        # the sub-video is where the model is: a batch of clips is an OVERLAPPING view of it (clip i = frames [i, i + 4),
        # batch stride = one frame) and the targets are a plain slice - nothing is gathered, the HIP model's first-layer
        # kernel reads the windows in place (ammc_conv_first_s16_bs); other callables make them contiguous themselves
        rgb_in = clip_windows(rgb_frames, s, e, RGB_LEN_CLIP - 1)
        op_in = clip_windows(op_frames, s, e, OP_LEN_CLIP - 1)
        rgb_t = rgb_frames[s + RGB_LEN_CLIP - 1:e + RGB_LEN_CLIP - 1]
        op_t = op_frames[s + OP_LEN_CLIP - 1:e + OP_LEN_CLIP - 1]
    else:
        rgb = torch.stack([rgb_frames[i:i + RGB_LEN_CLIP] for i in range(s, e)])
        op = torch.stack([op_frames[i:i + OP_LEN_CLIP] for i in range(s, e)])
        if device is not None:
            rgb, op = rgb.to(device, non_blocking=True), op.to(device, non_blocking=True)
        rgb_in = rgb[:, :-1].reshape(b, -1, *rgb.shape[-2:])
        op_in = op[:, :-1].reshape(b, -1, *op.shape[-2:])
        rgb_t, op_t = rgb[:, -1], op[:, -1]
    with torch.no_grad():
        flag = None
        if hasattr(model, "forward_scored") and rgb_in.is_cuda:
            # the HIP model accumulates the squared errors inside the `outc` kernel
            (_, _, (rgb_diff, op_diff), _), rgb_psnr, op_psnr = model.forward_scored(
                rgb_in, op_in, rgb_t, op_t, defer_guard=True, exact=exact)
            flag = getattr(model, "last_overflow", None)
        else:
            rgb_out, op_out, (rgb_diff, op_diff), _ = model(rgb_in, op_in)
            rgb_psnr, op_psnr = psnr_per_sample(rgb_out, rgb_t), psnr_per_sample(op_out, op_t)
        if flag is None:
            flag = torch.zeros(1, device=rgb_psnr.device, dtype=rgb_psnr.dtype)
        return torch.cat([rgb_psnr, op_psnr, rgb_diff.reshape(1), op_diff.reshape(1), flag.reshape(1).to(rgb_psnr.dtype)])


def _unpack_scores(stats: np.ndarray, b: int) -> Dict[str, np.ndarray]:
    return {"rgb_psnr": stats[:b], "op_psnr": stats[b:2 * b], "rgb_comm": stats[2 * b], "op_comm": stats[2 * b + 1],
            "overflow": bool(stats[2 * b + 2] != 0)}


def score_batch(model: Callable, rgb_frames: torch.Tensor, op_frames: torch.Tensor, s: int, e: int,
                device=None) -> Dict[str, np.ndarray]:
    """`score_batch_device` + the copy to the host (one sync); a batch whose S16 range flag is set is re-run on the
    exact-fp32 kernels"""
    sc = _unpack_scores(score_batch_device(model, rgb_frames, op_frames, s, e, device).cpu().numpy(), e - s)
    if sc["overflow"]:
        sc = _unpack_scores(score_batch_device(model, rgb_frames, op_frames, s, e, device, exact=True).cpu().numpy(), e - s)
        _count_fallback(model)
    return sc


def _count_fallback(model) -> None:
    if isinstance(model, torch.nn.Module):
        object.__setattr__(model, "s16_fallbacks", getattr(model, "s16_fallbacks", 0) + 1)


def assemble_records(n_frames: int, batches, scores: Sequence[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """per-frame arrays of one sub-video from its batch scores (test_helper.py:445-473)"""
    rec = {k: np.empty((n_frames,), dtype=np.float32) for k in ("rgb_psnr", "rgb_comm", "op_psnr", "op_comm")}
    for (s, e), sc in zip(batches, scores):
        for i in range(s, e):
            rec["rgb_psnr"][i + RGB_LEN_CLIP - 1] = sc["rgb_psnr"][i - s]
            rec["rgb_comm"][i + RGB_LEN_CLIP - 1] = sc["rgb_comm"]
            rec["op_psnr"][i + OP_LEN_CLIP - 1] = sc["op_psnr"][i - s]
            rec["op_comm"][i + OP_LEN_CLIP - 1] = sc["op_comm"]
    for key, lc in (("rgb_psnr", RGB_LEN_CLIP), ("rgb_comm", RGB_LEN_CLIP), ("op_psnr", OP_LEN_CLIP),
                    ("op_comm", OP_LEN_CLIP)):
        rec[key][:lc - 1] = rec[key][lc - 1]
    rec["op_psnr"][n_frames - 1] = rec["op_psnr"][n_frames - 2]
    rec["op_comm"][n_frames - 1] = rec["op_comm"][n_frames - 2]
    return rec


def evaluate_subvideo(model: Callable, rgb_frames: torch.Tensor, op_frames: torch.Tensor, device=None):
    """rgb_frames [T,3,H,W], op_frames [T-1,2,H,W] -> per-frame record arrays"""
    t = rgb_frames.shape[0]
    if op_frames.shape[0] != t - 1:
        raise ValueError("a sub-video of T frames has T-1 flows")
    batches = subvideo_batches(t)
    scores = [score_batch(model, rgb_frames, op_frames, s, e, device) for s, e in batches]
    return assemble_records(t, batches, scores)


def evaluate_dataset(model: Callable, videos: Sequence, dataset_name: str = "synthetic", device=None,
                     rank: int = 0, world: int = 1) -> Optional[dict]:
    """videos: sequence of (rgb_frames, op_frames) in sorted sub-video order.  Whole batches are
    sharded over `world` ranks; every rank returns the full record dict (test_helper.py:479-484)."""
    plan = [(v, s, e) for v, (rgb, _) in enumerate(videos) for s, e in subvideo_batches(rgb.shape[0])]
    mine = parallel.shard_batches(len(plan), rank, world)
    pending = []
    resident = (None, None)                 # one sub-video at a time lives on the device (<= ~150 MB for 180 frames)
    for i in mine:
        v, s, e = plan[i]
        if device is not None and resident[0] != v:
            resident = (v, (videos[v][0].to(device, non_blocking=True), videos[v][1].to(device, non_blocking=True)))
        rgb_v, op_v = resident[1] if device is not None else videos[v]
        pending.append((i, e - s, score_batch_device(model, rgb_v, op_v, s, e, None)))      # queued, not awaited
    local = {}
    if pending:                              # ONE device-to-host copy for all batches of this rank
        flat = torch.cat([t for _, _, t in pending]).cpu().numpy()
        off = 0
        for i, b, t in pending:
            local[i] = _unpack_scores(flat[off:off + t.numel()], b)
            off += t.numel()
        # S16 range guard (zero syncs in the loop above): the per-batch flags came back with the scores; batches
        # whose activations left the half range are re-run on the exact-fp32 kernels, the rest stand
        for i in [i for i in local if local[i]["overflow"]]:
            v, s, e = plan[i]
            rgb_v, op_v = videos[v]
            local[i] = _unpack_scores(score_batch_device(model, rgb_v, op_v, s, e, device, exact=True).cpu().numpy(), e - s)
            _count_fallback(model)
    allsc = parallel.gather_records(local, world)
    out = {"dataset": dataset_name, "rgb_img_pred_records": [], "rgb_fea_comm_records": [],
           "op_img_pred_records": [], "op_fea_comm_records": []}
    for v, (rgb, _) in enumerate(videos):
        idx = [i for i, p in enumerate(plan) if p[0] == v]
        rec = assemble_records(rgb.shape[0], [plan[i][1:] for i in idx], [allsc[i] for i in idx])
        out["rgb_img_pred_records"].append(rec["rgb_psnr"])
        out["rgb_fea_comm_records"].append(rec["rgb_comm"])
        out["op_img_pred_records"].append(rec["op_psnr"])
        out["op_fea_comm_records"].append(rec["op_comm"])
    return out


def evaluate_stream(model: Callable, subvideos, dataset_name: str = "synthetic", stats: Optional[dict] = None) -> dict:
    """`evaluate_dataset` for sub-videos that ARRIVE device-resident one after the other (`pipeline.SubVideoStager`: the
    upload and the resize / normalise kernels of sub-video v + 1 run on a side stream while v is scored) - the whole
    loop of run_helper/test_helper.py:408-488 without a host wait inside it:

      * every batch of a sub-video is queued back to back (`score_batch_device`: clips are overlapping windows of the
        resident tensors, PSNR comes out of the output layer's epilogue);
      * the scores and S16 range flags of a sub-video go to pinned host memory by ONE asynchronous copy;
      * they are read one sub-video LATE - the device is then busy with the next one - and batches whose flag is set are
        re-run on the exact-fp32 kernels while their sub-video is still resident.

    `stats` (optional dict) receives `score_copies`, `rerun_batches`."""
    out = {"dataset": dataset_name, "rgb_img_pred_records": [], "rgb_fea_comm_records": [],
           "op_img_pred_records": [], "op_fea_comm_records": []}
    copies = reruns = 0

    def finish(item):
        nonlocal reruns
        rgb, op, batches, host, ev = item
        ev.synchronize()
        flat, off, scores = host.numpy(), 0, []
        for s, e in batches:
            n = 2 * (e - s) + 3
            sc = _unpack_scores(flat[off:off + n].copy(), e - s)
            off += n
            if sc["overflow"]:
                sc = _unpack_scores(score_batch_device(model, rgb, op, s, e, None, exact=True).cpu().numpy(), e - s)
                _count_fallback(model)
                reruns += 1
            scores.append(sc)
        rec = assemble_records(rgb.shape[0], batches, scores)
        out["rgb_img_pred_records"].append(rec["rgb_psnr"])
        out["rgb_fea_comm_records"].append(rec["rgb_comm"])
        out["op_img_pred_records"].append(rec["op_psnr"])
        out["op_fea_comm_records"].append(rec["op_comm"])

    pending = None
    for rgb, op in subvideos:
        if op.shape[0] != rgb.shape[0] - 1:
            raise ValueError("a sub-video of T frames has T-1 flows")
        batches = subvideo_batches(rgb.shape[0])
        flat = torch.cat([score_batch_device(model, rgb, op, s, e, None) for s, e in batches])
        if flat.is_cuda:
            host = torch.empty(flat.numel(), dtype=flat.dtype, pin_memory=True)
            host.copy_(flat, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            copies += 1
        else:
            host, ev = flat, _Done()
        if pending is not None:
            finish(pending)
        pending = (rgb, op, batches, host, ev)
    if pending is not None:
        finish(pending)
    if stats is not None:
        stats.update(score_copies=copies, rerun_batches=reruns)
    return out


class _Done:
    def synchronize(self):
        pass


# ---- anomaly localisation: patch / pixel error maps and the fixed-order PSNR --------------
# A pass of its own behind the evaluation forward (`ops.error_maps`, csrc/error_maps.hip): the scoring loops above and the
# fused epilogue sums they read are not touched.

def error_maps_reference(pred: torch.Tensor, target: torch.Tensor, patch: int) -> Dict[str, torch.Tensor]:
    """the quantities of `ops.error_maps` in float64 with plain torch (any device; the reference of the tests): with
    e = (target - pred) / 2, `pixel` [B,H,W] = mean_c e^2, `patch_sum` / `patch_mean` [B,ph,pw] over patch x patch pixels
    anchored at (0, 0) (the last patch row / column ragged, means over the pixels that exist), `frame_sq` [B] = the sum of
    the patch sums, `worst` / `worst_idx` [B] = the largest patch mean and the lowest i * pw + j attaining it,
    `psnr` = 10 log10(C H W / frame_sq)"""
    b, c, h, w = pred.shape
    sq = ((target.double() - pred.double()) * 0.5) ** 2
    per_px = sq.sum(1)                                                      # [B,H,W], summed over channels
    ph, pw = (h + patch - 1) // patch, (w + patch - 1) // patch
    padded = torch.zeros((b, ph * patch, pw * patch), dtype=torch.float64, device=pred.device)
    padded[:, :h, :w] = per_px
    patch_sum = padded.view(b, ph, patch, pw, patch).sum(dim=(2, 4))
    rows = torch.clamp(h - torch.arange(ph, device=pred.device) * patch, max=patch)
    cols = torch.clamp(w - torch.arange(pw, device=pred.device) * patch, max=patch)
    count = (c * rows[:, None] * cols[None, :]).double()
    patch_mean = patch_sum / count
    frame_sq = patch_sum.sum(dim=(1, 2))
    flat = patch_mean.reshape(b, -1)
    worst = flat.max(dim=1).values
    first = (flat == worst[:, None]).int().argmax(dim=1)                     # argmax of 0/1: the first maximum
    return {"pixel": per_px / c, "patch_sum": patch_sum, "patch_mean": patch_mean, "frame_sq": frame_sq, "worst": worst,
            "worst_idx": first.to(torch.int32), "psnr": 10.0 * torch.log10(float(c * h * w) / frame_sq)}


def assemble_localised(n_frames: int, batches, parts: Sequence[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """per-frame arrays of one sub-video from its batches' outputs, with the frame indexing and the fills of
    `assemble_records`: clip i of a batch fills frame i + len_clip - 1 of its stream, a per-batch scalar (`*_comm`) every
    frame of the batch, the first len_clip - 1 frames copy frame len_clip - 1, and the flow stream's last frame copies
    the one before it.  parts[k]: {"rgb_psnr": [b], "rgb_patch": [b, ph, pw], "rgb_comm": scalar, "op_...": ...}"""
    rec: Dict[str, np.ndarray] = {}
    for key, v0 in parts[0].items():
        v0 = np.asarray(v0)
        lc = RGB_LEN_CLIP if key.startswith("rgb_") else OP_LEN_CLIP
        per_clip = v0.ndim > 0
        out = np.empty((n_frames,) + (v0.shape[1:] if per_clip else ()), dtype=v0.dtype)
        for (s, e), part in zip(batches, parts):
            out[s + lc - 1:e + lc - 1] = np.asarray(part[key])
        out[:lc - 1] = out[lc - 1]
        if key.startswith("op_"):
            out[n_frames - 1] = out[n_frames - 2]
        rec[key] = out
    return rec


# ---- the pass driver: one sub-video through a pass behind the evaluation forward -------------

_SLOT_DTYPES = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}


class _Slots:
    """one flat device buffer of 4-byte words, zeroed, carved into named sections [(name, shape, dtype)] of fp32, int32
    or uint8, each 16-byte aligned: the launches of a pass write straight into them and everything comes to the host by
    ONE copy (`flat.cpu().numpy()`, which `view(name, host)` carves the same way).  Words are reinterpreted, never
    converted: every bit pattern survives."""

    def __init__(self, sections, device):
        self.layout, off = {}, 0                           # name -> (first word, (shape, dtype))
        for name, shape, dtype in sections:
            self.layout[name] = (off, (tuple(shape), dtype))
            off += (self._words(shape, dtype) + 3) // 4 * 4
        self.flat = torch.zeros(off, device=device, dtype=torch.int32)

    @staticmethod
    def _words(shape, dtype) -> int:
        n = int(np.prod(shape, dtype=np.int64))
        return (n + 3) // 4 if dtype == torch.uint8 else n

    def view(self, name: str, host: Optional[np.ndarray] = None):
        off, (shape, dtype) = self.layout[name]
        v = (self.flat if host is None else host)[off:off + self._words(shape, dtype)]
        if dtype != torch.int32:
            v = v.view(dtype if host is None else _SLOT_DTYPES[dtype])
        return v[:int(np.prod(shape, dtype=np.int64))].reshape(shape)


def _checked_batches(who: Optional[str], rgb_frames: torch.Tensor, op_frames: torch.Tensor, batch: int):
    """the checks every per-sub-video pass makes, then `subvideo_batches(T, batch)`.  `who`: the public function's name
    for the residency message; None leaves that check out (the driver itself runs on tensors of any device)"""
    t = rgb_frames.shape[0]
    if op_frames.shape[0] != t - 1:
        raise ValueError("a sub-video of T frames has T-1 flows")
    if who is not None and not (rgb_frames.is_cuda and op_frames.is_cuda and rgb_frames.is_contiguous()
                                and op_frames.is_contiguous()):
        raise ValueError(f"{who} reads a sub-video resident on the GPU (contiguous tensors): move it there first")
    batches = subvideo_batches(t, batch)
    if not batches:
        raise ValueError(f"a sub-video needs at least {RGB_LEN_CLIP} frames")
    return batches


class _Forward(NamedTuple):
    """what `_forward_batch` hands to a pass: the predicted frames and flows, the memory blocks' two commit values, the
    [rgb, op] PSNR of the output layer's epilogue, the (rgb, op) targets and the S16 range flag ([1] tensor, or None)"""
    rgb_pred: torch.Tensor
    op_pred: torch.Tensor
    diffs: tuple
    fused: list
    targets: tuple
    overflow: Optional[torch.Tensor]


def _forward_batch(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, s: int, e: int, exact: bool) -> _Forward:
    """clips [s, e) of a resident sub-video through the model's evaluation forward: the clips are overlapping windows
    (`clip_windows`), the targets plain slices, the range guard is deferred (nothing waits for the device)"""
    rgb_in = clip_windows(rgb_frames, s, e, RGB_LEN_CLIP - 1)
    op_in = clip_windows(op_frames, s, e, OP_LEN_CLIP - 1)
    targets = (rgb_frames[s + RGB_LEN_CLIP - 1:e + RGB_LEN_CLIP - 1], op_frames[s + OP_LEN_CLIP - 1:e + OP_LEN_CLIP - 1])
    with torch.no_grad():
        (rgb_out, op_out, diffs, _), *fused = model.forward_scored(rgb_in, op_in, *targets, defer_guard=True, exact=exact)
    return _Forward(rgb_out, op_out, diffs, fused, targets, getattr(model, "last_overflow", None))


def _run_pass(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, batches, sections, ints, on_batch: Callable,
              predictions: Optional[list] = None, scratch=()) -> Dict[str, np.ndarray]:
    """One sub-video through a pass; the tensors may live on any device.  `sections`: [(name, shape of one clip's row)],
    every name with the prefix of its stream (`rgb_` / `op_`: it picks the clip length of the fills); `ints`: the names
    that hold int32 (the others fp32); `scratch`: names a kernel needs room for but the pass does not return.  The driver
    carves the sections, and behind them the per-batch commit values and range flags, out of one `_Slots` buffer.  For
    batch k = clips [s, e) it runs `_forward_batch`, then `on_batch(slots, s, e, k, forward)` under `no_grad`, which writes the
    pass's outputs into rows [s, e) of its sections (device work only: no wait, no host read).  Every batch is queued
    back to back; ONE device-to-host copy; the batches whose S16 range flag came back set run again with `exact=True`
    (one `_count_fallback` each) and the buffer is copied again.  `predictions` receives (s, e, rgb_pred, op_pred, fused)
    of every batch as scored: a re-run's tuple replaces the plain one.  -> `assemble_localised` over the sections that
    are not scratch, plus `rgb_comm` / `op_comm`."""
    n_clip = batches[-1][1]
    slots = _Slots([(name, (n_clip,) + tuple(shape), torch.int32 if name in ints else torch.float32) for name, shape in sections] +
                   [("comm", (len(batches), 2), torch.float32), ("flag", (len(batches),), torch.float32)], rgb_frames.device)

    def run(k: int, exact: bool):
        s, e = batches[k]
        fwd = _forward_batch(model, rgb_frames, op_frames, s, e, exact)
        with torch.no_grad():
            on_batch(slots, s, e, k, fwd)
            slots.view("comm")[k, 0], slots.view("comm")[k, 1] = fwd.diffs[0].reshape(()), fwd.diffs[1].reshape(())
            slots.view("flag")[k] = fwd.overflow.reshape(()).to(torch.float32) if fwd.overflow is not None else 0.0
        return (s, e, fwd.rgb_pred, fwd.op_pred, fwd.fused) if predictions is not None else None    # (else the frames are let go)

    done = [run(k, False) for k in range(len(batches))]
    host = slots.flat.cpu().numpy()                     # the sub-video's one copy (and its one wait)
    flagged = [k for k in range(len(batches)) if slots.view("flag", host)[k] != 0]
    if flagged:                                          # S16 range guard: those batches again on the exact-fp32 kernels
        for k in flagged:
            done[k] = run(k, True)
            _count_fallback(model)
        host = slots.flat.cpu().numpy()
    if predictions is not None:
        predictions.extend(done)
    names = [name for name, _ in sections if name not in scratch]
    parts = []
    for k, (s, e) in enumerate(batches):
        part = {name: slots.view(name, host)[s:e] for name in names}
        part["rgb_comm"], part["op_comm"] = slots.view("comm", host)[k]
        parts.append(part)
    return assemble_localised(rgb_frames.shape[0], batches, parts)


def _new_records(dataset_name: str, *more: str) -> dict:
    """the record dict of an `evaluate_dataset_*` loop: the reference's four lists, then the loop's own"""
    return {"dataset": dataset_name, "rgb_img_pred_records": [], "rgb_fea_comm_records": [], "op_img_pred_records": [],
            "op_fea_comm_records": [], **{key: [] for key in more}}


def _scored_subvideos(model, videos, out: dict, score: Callable, device=None):
    """the loop of the `evaluate_dataset_*` functions: every (rgb, op) of `videos` is moved to `device` (default: the
    model's) and made contiguous, `score(v, rgb, op)` returns its per-frame arrays, the four reference record lists and
    `n_frames` of `out` grow by one entry; yields (v, rgb, op, rec) for the caller's own records"""
    if device is None:
        device = next(model.parameters()).device
    for v, (rgb, op) in enumerate(videos):
        rgb, op = rgb.to(device, non_blocking=True).contiguous(), op.to(device, non_blocking=True).contiguous()
        rec = score(v, rgb, op)
        out["rgb_img_pred_records"].append(rec["rgb_psnr"])
        out["rgb_fea_comm_records"].append(rec["rgb_comm"])
        out["op_img_pred_records"].append(rec["op_psnr"])
        out["op_fea_comm_records"].append(rec["op_comm"])
        out["n_frames"].append(int(rgb.shape[0]))
        yield v, rgb, op, rec


def _write_maps(out: dict, maps_dir: Optional[str], v: int, rec: Dict[str, np.ndarray]) -> None:
    """with `maps_dir`: sub-video v's arrays to `maps_dir/NNNN.npz`, the path to `out["map_files"]`"""
    if maps_dir:
        os.makedirs(maps_dir, exist_ok=True)
        path = os.path.join(maps_dir, f"{v:04d}.npz")
        np.savez(path, **rec)
        out["map_files"].append(path)


def _worst_patch_psnr(worst: np.ndarray) -> np.ndarray:
    """10 log10(1 / worst patch mean) per frame, fp32 (inf where the worst patch has no error)"""
    with np.errstate(divide="ignore"):
        return (10.0 * np.log10(1.0 / worst.astype(np.float64))).astype(np.float32)


def localise_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, patch: int = 16, pixel: bool = False,
                      batch: int = EVAL_BATCH, predictions: Optional[list] = None) -> Dict[str, np.ndarray]:
    """Where the anomaly is: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W], contiguous and on the model's device ->
    per-frame numpy arrays of the sub-video: `rgb_patch` / `op_patch` [T,ph,pw] (patch means of the squared [0,1]-range
    error), `rgb_psnr` / `op_psnr` (from the fixed-order sum: the same bits for the same predictions), `rgb_worst` /
    `op_worst` (the largest patch mean), `rgb_worst_idx` / `op_worst_idx` (its i * pw + j), `rgb_comm` / `op_comm` [T],
    and with `pixel` `rgb_pixel` / `op_pixel` [T,H,W].  Clips, targets and batches are those of `score_batch_device`
    (`batch` clips at a time), the forward is the model's evaluation forward, frame indexing and fills are
    `assemble_records`' (`assemble_localised`).  Every batch is queued back to back; one device-to-host copy per
    sub-video; a batch whose S16 range flag is set is re-run with `exact=True`, as `score_batch` does (`_run_pass`).
    `predictions`: a testing and cross-check hook, not part of the scoring - an optional list that receives
    (s, e, rgb_pred, op_pred, fused) of every batch as scored (it keeps every batch's predicted frames alive); `fused` = the
    [rgb, op] PSNR of the output layer's epilogue from the same forward."""
    from . import ops
    batches = _checked_batches("localise_subvideo", rgb_frames, op_frames, batch)
    sections = []
    for st, (_, h, w) in (("rgb", rgb_frames.shape[1:]), ("op", op_frames.shape[1:])):
        grid = ((h + patch - 1) // patch, (w + patch - 1) // patch)
        sections += [(f"{st}_patch", grid), (f"{st}_patch_sum", grid)]
        sections += [(f"{st}_{key}", ()) for key in ("frame_sq", "psnr", "worst", "worst_idx")]
        if pixel:
            sections.append((f"{st}_pixel", (h, w)))

    def on_batch(slots, s, e, k, fwd):
        for st, pred, tgt in (("rgb", fwd.rgb_pred, fwd.targets[0]), ("op", fwd.op_pred, fwd.targets[1])):
            out = {"patch_mean": slots.view(f"{st}_patch")[s:e], "patch_sum": slots.view(f"{st}_patch_sum")[s:e]}
            for key in ("frame_sq", "worst", "worst_idx") + (("pixel",) if pixel else ()):
                out[key] = slots.view(f"{st}_{key}")[s:e]
            slots.view(f"{st}_psnr")[s:e] = ops.error_maps(pred, tgt, patch, pixel, out)["psnr"]

    return _run_pass(model, rgb_frames, op_frames, batches, sections, ("rgb_worst_idx", "op_worst_idx"), on_batch, predictions,
                     scratch=("rgb_patch_sum", "rgb_frame_sq", "op_patch_sum", "op_frame_sq"))


def evaluate_dataset_localised(model, videos, dataset_name: str = "synthetic", patch: int = 16, pixel: bool = False,
                               maps_dir: Optional[str] = None, device=None) -> dict:
    """`evaluate_dataset` with `localise_subvideo` in place of the scoring loop (one rank).  `videos`: a sequence of
    (rgb_frames, op_frames) - host tensors are moved to `device` (default: the model's) one sub-video at a time - or an
    iterator of device-resident sub-videos (`pipeline.SubVideoStager`).  Returns the four record lists of the
    reference with `*_img_pred_records` from the fixed-order PSNR, plus `rgb_patch_psnr_records` (10 log10(1 / worst
    patch mean) per frame: the worst-patch frame score, a drop-in for `rgb_img_pred_records` in `fuse_scores_auc`) and
    `n_frames`.  `maps_dir`: one `NNNN.npz` per sub-video with the arrays of `localise_subvideo` (`map_files`)."""
    out = _new_records(dataset_name, "rgb_patch_psnr_records", "n_frames", "map_files")
    for v, _, _, rec in _scored_subvideos(model, videos, out, lambda v, rgb, op: localise_subvideo(model, rgb, op, patch, pixel),
                                          device):
        out["rgb_patch_psnr_records"].append(_worst_patch_psnr(rec["rgb_worst"]))
        _write_maps(out, maps_dir, v, rec)
    return out


# ---- per-clip memory-commit scores and maps -------------------------------------------------
# A pass of its own behind the evaluation forward (`ops.memory_scores`, csrc/memory_scores.hip) over the bottleneck in
# front of each stream's memory block: the scoring loops above, the fused memory block and its one `diff` scalar per
# batch are not touched.

def memory_scores_reference(enc_w: torch.Tensor, enc_b: torch.Tensor, embed: torch.Tensor, x: torch.Tensor,
                            k: int) -> Dict[str, torch.Tensor]:
    """the quantities of `ops.memory_scores` in float64 with plain torch (any device; the reference of the tests).
    enc_w [d, c] (or [d, c, 1, 1]), enc_b [d], embed [d, m], x NHWC [B, h, w, c].  z = x enc_w^T + enc_b [B,h,w,d];
    dist = |z|^2 - 2 z E + |E|^2 (models/unet.py:284-288); `idx` [B,h,w,k] = the k nearest slots, nearest first, equal
    distances in ascending slot order; `map` [B,h,w] = sum_j (E[j][idx0] - z[j])^2 / d taken directly; `commit` [B] = the
    mean of `map`; `worst` / `worst_idx` [B] = the largest map value and the lowest y * w + x attaining it.  For the
    tests also `z`, `dist` [B,h,w,m], `order` [B,h,w,min(k+1,m)] (the first slots of the stable sort), `margin` [B,h,w] =
    the smallest gap between consecutive sorted distances among those (inf when there is one), `znorm` = |z|^2 and
    `scale` = (|z|^2 + |E[:, idx0]|^2) / d, what the rounding error of a map entry is proportional to."""
    d, m = embed.shape
    e = embed.double()
    z = x.double() @ enc_w.double().reshape(d, -1).t() + enc_b.double()
    b, h, w, _ = z.shape
    znorm = (z * z).sum(-1)
    dist = znorm[..., None] - 2.0 * (z @ e) + (e * e).sum(0)
    srt, order = torch.sort(dist, dim=-1, stable=True)
    n = min(k + 1, m)
    idx = order[..., :k]
    near = e.t()[idx[..., 0]]                                                  # [B,h,w,d]
    s = ((near - z) ** 2).sum(-1)
    mp = s / d
    gaps = srt[..., 1:n] - srt[..., :n - 1]
    margin = gaps.min(-1).values if n > 1 else torch.full_like(mp, float("inf"))
    flat = mp.reshape(b, -1)
    worst = flat.max(dim=1).values
    first = (flat == worst[:, None]).int().argmax(dim=1)                       # argmax of 0/1: the first maximum
    return {"z": z, "idx": idx.to(torch.int32), "map": mp, "commit": flat.mean(dim=1), "worst": worst,
            "worst_idx": first.to(torch.int32), "dist": dist, "order": order[..., :n], "margin": margin, "znorm": znorm,
            "scale": (znorm + (near * near).sum(-1)) / d}


def memory_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, batch: int = EVAL_BATCH,
                    indices: bool = False) -> Dict[str, np.ndarray]:
    """Which clips the memory does not hold: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W], contiguous and on the model's
    device -> per-frame numpy arrays of the sub-video.  `rgb_comm` / `op_comm` [T]: the reference's value, ONE number per
    batch written to every frame of it (unchanged).  `rgb_clip_comm` / `op_clip_comm` [T]: the commit distance of the
    frame's own clip, a function of that clip's bottleneck alone; `*_commit_map` [T,H/8,W/8]: the same per position of
    the bottleneck grid; `*_commit_worst`, `*_commit_worst_idx`: its largest value and where; `*_psnr`; with `indices`
    `*_slots` [T,H/8,W/8,k] int32, the memory items each position addresses.  Clips, targets, batches, frame indexing and
    fills are `localise_subvideo`'s; behind every forward `ops.memory_scores` runs on each stream's bottleneck
    (`model.bottleneck_inputs()`) with that stream's `vq_down3`.  One device-to-host copy per sub-video; a batch whose
    S16 range flag is set is re-run with `exact=True`, and its memory pass with it."""
    from . import ops
    batches = _checked_batches("memory_subvideo", rgb_frames, op_frames, batch)
    quans = {"rgb": model.rgb.vq_down3, "op": model.op.vq_down3}
    sections, ints = [], []
    for st, frames in (("rgb", rgb_frames), ("op", op_frames)):
        grid = (frames.shape[2] // 8, frames.shape[3] // 8)
        sections += [(f"{st}_commit_map", grid), (f"{st}_clip_comm", ()), (f"{st}_commit_worst", ()),
                     (f"{st}_commit_worst_idx", ()), (f"{st}_psnr", ())]
        ints.append(f"{st}_commit_worst_idx")
        if indices:
            sections.append((f"{st}_slots", grid + (int(getattr(quans[st], "quan", quans[st]).quantize.k),)))
            ints.append(f"{st}_slots")

    def on_batch(slots, s, e, k, fwd):
        for st, x4, ps in zip(("rgb", "op"), model.bottleneck_inputs(), fwd.fused):
            out = {"map": slots.view(f"{st}_commit_map")[s:e], "commit": slots.view(f"{st}_clip_comm")[s:e],
                   "worst": slots.view(f"{st}_commit_worst")[s:e], "worst_idx": slots.view(f"{st}_commit_worst_idx")[s:e]}
            if indices:
                out["idx"] = slots.view(f"{st}_slots")[s:e]
            ops.memory_scores(quans[st], x4.permute(0, 3, 1, 2), indices, out)
            slots.view(f"{st}_psnr")[s:e] = ps

    return _run_pass(model, rgb_frames, op_frames, batches, sections, ints, on_batch)


def evaluate_dataset_memory(model, videos, dataset_name: str = "synthetic", indices: bool = False,
                            maps_dir: Optional[str] = None, device=None, batch: int = EVAL_BATCH) -> dict:
    """`evaluate_dataset` with `memory_subvideo` in place of the scoring loop (one rank).  `videos`: a sequence of
    (rgb_frames, op_frames) - host tensors are moved to `device` (default: the model's) one sub-video at a time - or an
    iterator of device-resident sub-videos (`pipeline.SubVideoStager`).  Returns the four record lists of the reference
    (`*_fea_comm_records`: one value per batch, as the reference writes them) plus `rgb_clip_comm_records` /
    `op_clip_comm_records` (the per-clip commit distance per frame: drop-ins for the `*_fea_comm_records` in
    `fuse_scores_auc`), `n_frames` and `map_files`.  `maps_dir`: one `NNNN.npz` per sub-video with the arrays of
    `memory_subvideo`."""
    out = _new_records(dataset_name, "rgb_clip_comm_records", "op_clip_comm_records", "n_frames", "map_files")
    for v, _, _, rec in _scored_subvideos(model, videos, out, lambda v, rgb, op: memory_subvideo(model, rgb, op, batch, indices),
                                          device):
        out["rgb_clip_comm_records"].append(rec["rgb_clip_comm"])
        out["op_clip_comm_records"].append(rec["op_clip_comm"])
        _write_maps(out, maps_dir, v, rec)
    return out


# ---- SSIM and MSE frame scores --------------------------------------------------------------
# A pass of its own behind the evaluation forward (`ops.ssim`, csrc/ssim.hip): the two record types of the reference's
# evaluation loop beside PSNR (`loss_name` = ssim_error / mse_error, run_helper/test_helper.py:28-33, 396-400).  The
# scoring loops above and the fused epilogue sums they read are not touched.

def ssim_reference(pred: torch.Tensor, target: torch.Tensor, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """the quantities of `ops.ssim` with plain torch in `dtype` (any device; float64: the reference of the tests;
    float32: the reference's own arithmetic, utils/pytorch_ssim.py:20-40).  The window is the 2-D one exactly as the
    reference forms it - the fp32 outer product of the fp32 1-D window - then cast; zero padding; C1 = 0.01^2,
    C2 = 0.03^2 on the values as they are.  `map_c` [B,C,H,W] the SSIM map, `map` [B,H,W] its channel mean, `ssim_c`
    [B,C], `ssim` [B] (the reference's `size_average=False` value per sample), `sq` [B] = the sum of (target - pred)^2,
    `mse` = 256 sq / (C H W) (utils/utils.py:110-111), `psnr` = 10 log10(4 C H W / sq)."""
    import torch.nn.functional as F
    from .ops import ssim_window
    b, c, h, w = pred.shape
    w1 = ssim_window().unsqueeze(1)
    window = w1.mm(w1.t()).float().to(device=pred.device, dtype=dtype).expand(c, 1, 11, 11).contiguous()
    x1, x2 = pred.to(dtype), target.to(dtype)

    def conv(t):
        return F.conv2d(t, window, padding=5, groups=c)
    mu1, mu2 = conv(x1), conv(x2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(x1 * x1) - mu1_sq
    sigma2_sq = conv(x2 * x2) - mu2_sq
    sigma12 = conv(x1 * x2) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    map_c = ((2 * mu1_mu2 + c1) * (2 * sigma12 + c2)) / ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2))
    sq = ((x2 - x1) ** 2).sum(dim=(1, 2, 3))
    n = float(c * h * w)
    return {"map_c": map_c, "map": map_c.mean(1), "ssim_c": map_c.mean(dim=(2, 3)), "ssim": map_c.mean(1).mean(1).mean(1),
            "sq": sq, "mse": 256.0 * sq / n, "psnr": 10.0 * torch.log10(4.0 * n / sq)}


def quality_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, maps: bool = False, batch: int = EVAL_BATCH,
                     predictions: Optional[list] = None) -> Dict[str, np.ndarray]:
    """The reference's three frame scores of one sub-video: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W], contiguous and
    on the model's device -> per-frame numpy arrays `rgb_ssim` / `op_ssim`, `rgb_mse` / `op_mse`, `rgb_psnr` / `op_psnr`
    (all three from `ops.ssim`: fixed-order sums, the same bits for the same predictions), `rgb_comm` / `op_comm` [T], and
    with `maps` `rgb_ssim_map` / `op_ssim_map` [T,H,W].  Clips, targets and batches are those of `localise_subvideo`
    (`batch` clips at a time), the forward is the model's evaluation forward, frame indexing and fills are
    `assemble_records`' (`assemble_localised`).  Every batch is queued back to back; one flat device buffer and one
    device-to-host copy per sub-video; a batch whose S16 range flag is set is re-run with `exact=True`.  `predictions`:
    the testing hook of `localise_subvideo` - a list that receives (s, e, rgb_pred, op_pred, fused) of every batch."""
    from . import ops
    batches = _checked_batches("quality_subvideo", rgb_frames, op_frames, batch)
    sections = []
    for st, frames in (("rgb", rgb_frames), ("op", op_frames)):
        sections += [(f"{st}_{key}", ()) for key in ("ssim", "mse", "psnr")]
        if maps:
            sections.append((f"{st}_ssim_map", tuple(frames.shape[2:])))

    def on_batch(slots, s, e, k, fwd):
        for st, pred, tgt in (("rgb", fwd.rgb_pred, fwd.targets[0]), ("op", fwd.op_pred, fwd.targets[1])):
            out = {"ssim": slots.view(f"{st}_ssim")[s:e]}
            if maps:
                out["map"] = slots.view(f"{st}_ssim_map")[s:e]
            got = ops.ssim(pred, tgt, maps, out)
            slots.view(f"{st}_mse")[s:e] = got["mse"]
            slots.view(f"{st}_psnr")[s:e] = got["psnr"]

    return _run_pass(model, rgb_frames, op_frames, batches, sections, (), on_batch, predictions)


def evaluate_dataset_quality(model, videos, dataset_name: str = "synthetic", maps: bool = False,
                             maps_dir: Optional[str] = None, device=None) -> dict:
    """`evaluate_dataset` with `quality_subvideo` in place of the scoring loop (one rank).  `videos`: a sequence of
    (rgb_frames, op_frames) - host tensors are moved to `device` (default: the model's) one sub-video at a time - or an
    iterator of device-resident sub-videos (`pipeline.SubVideoStager`).  Returns the four record lists of the reference
    with `*_img_pred_records` from the fixed-order squared error (the reference's records for `loss_name` = psnr_error),
    plus `rgb_ssim_records` / `op_ssim_records` (ssim_error) and `rgb_mse_records` / `op_mse_records` (mse_error),
    `n_frames` and `map_files`.  `maps_dir`: one `NNNN.npz` per sub-video with the arrays of `quality_subvideo`."""
    out = _new_records(dataset_name, "rgb_ssim_records", "op_ssim_records", "rgb_mse_records", "op_mse_records", "n_frames",
                       "map_files")
    for v, _, _, rec in _scored_subvideos(model, videos, out, lambda v, rgb, op: quality_subvideo(model, rgb, op, maps), device):
        for st in ("rgb", "op"):
            out[f"{st}_ssim_records"].append(rec[f"{st}_ssim"])
            out[f"{st}_mse_records"].append(rec[f"{st}_mse"])
        _write_maps(out, maps_dir, v, rec)
    return out


# AMMC_FUSED_LOSS: 1 = the per-pixel terms of the generator's objective (intensity, gradient difference, flow) come from the
# library's loss kernels (`losses.py`: one forward and one backward launch per prediction pair), 0 (default) = the torch
# chains below.  Device tensors only: on the CPU the flag changes nothing.  profiles/loss_ab.txt holds the A/B.
FUSED_LOSS = os.environ.get("AMMC_FUSED_LOSS", "0") not in ("", "0")


def _fused(*tensors) -> bool:
    return FUSED_LOSS and all(t is not None and t.is_cuda for t in tensors)


def generator_loss(out, rgb_t: torch.Tensor, op_t: torch.Tensor, lam_lp: float = 1.0, lam_lp_op: float = 1.0,
                   lam_latent: float = 1.0) -> torch.Tensor:
    rgb, op, (rd, od), _ = out[:4]
    if _fused(rgb, op, rgb_t, op_t):
        from . import losses
        return lam_lp * losses.prediction_terms(rgb, rgb_t, False)[0] + \
            lam_lp_op * losses.prediction_terms(op, op_t, False)[0] + lam_latent * (rd + od).sum()
    l_rgb = torch.norm(rgb - rgb_t, p=2, dim=1).mean()            # `L2`, losses_utils.py:124-129
    l_op = torch.norm(op - op_t, p=2, dim=1).mean()
    return lam_lp * l_rgb + lam_lp_op * l_op + lam_latent * (rd + od).sum()


def adam(params, lr: float, **kw) -> torch.optim.Adam:
    """the reference's optimizer (`torch.optim.Adam(params, lr=...)`, optimizer/__init__.py:39-49) - the same update
    rule in torch's FUSED form when the parameters live on the GPU: one multi-tensor launch per ~chunk of parameters
    instead of the ~17 elementwise launches of the default foreach form (0.48 -> ~0.15 ms per batch-32 step)"""
    params = list(params)
    fused = bool(params) and all(p.is_cuda for p in params)
    return torch.optim.Adam(params, lr=lr, fused=fused, **kw)


def train_step(model: torch.nn.Module, optimizer: torch.optim.Optimizer, rgb: torch.Tensor, op: torch.Tensor,
               **lams) -> torch.Tensor:
    """one G step of the joint training loop (train_helper.py:296-339 without D / FlowNet terms).
    rgb [B,5,3,H,W], op [B,4,2,H,W]; targets are the last frame of each.  With a
    `parallel.BucketedGradReducer` attached to the model the gradients are averaged across ranks
    inside backward (RCCL over xGMI)."""
    b = rgb.shape[0]
    rgb_in = rgb[:, :-1].reshape(b, -1, *rgb.shape[-2:])
    op_in = op[:, :-1].reshape(b, -1, *op.shape[-2:])
    return _generator_iteration(model, optimizer,
                                lambda: (generator_loss(model(rgb_in, op_in), rgb[:, -1], op[:, -1], **lams), None))[0]


def _generator_iteration(model: torch.nn.Module, optimizer, forward: Callable):
    """The G-only iteration `train_step` and `train_step_single` share: `forward() -> (loss, kept)` runs the generator
    and builds its loss; the verdict on the loss is taken before the backward is enqueued, the update is refused on a
    non-finite one (`_FiniteWatch`).  -> (detached loss, kept)"""
    optimizer.zero_grad(set_to_none=True)
    loss, kept = forward()
    vote, group = _watch_group(model)
    watch = _FiniteWatch(loss, group=group, vote=vote)
    loss.backward()
    watch.step(optimizer)
    return loss.detach(), kept


def _watch_group(*models):
    """(vote, group) for `_FiniteWatch`: ranks share the verdict on the loss exactly when their gradients or statistics
    are shared - a `parallel.BucketedGradReducer` or `parallel.sync_statistics` attached to one of the models - and in
    THAT process group.  Models that train on their own (no reducer: per-rank runs inside an initialised world, the
    stress-style harnesses) do not vote: no rank waits in a collective the others never enter."""
    for m in models:
        red = getattr(m, "_grad_reducer", None)
        if red is not None:
            return True, getattr(red, "group", None)
        sync = getattr(m, "_sync_stats", None)
        if sync and sync[0]:
            return True, sync[1]
    return False, None


class _FiniteWatch:
    """`optimizer.step()` unless the loss is non-finite, without stalling the device.  The split-fp16 training kernels
    (`train_precision = "s16"`, the default) encode their operands in half range: an activation beyond 65504 becomes inf
    in the re-encoding and reaches the loss as inf / NaN; stepping would write that into the Adam moments and the
    weights for good.  The verdict on the loss is copied to pinned host memory right after the FORWARD (one 1-byte copy
    + an event, queued before the backward's kernels); `step` waits for that event only - by then the host has enqueued
    the whole backward, so the device keeps working while the host waits - and refuses the step loudly.  (The
    BatchNorm / EMA buffers of the refused step were updated in place by its forward, as the reference's would be.)
    Data parallel: the gradients are averaged across ranks INSIDE backward, so one rank's non-finite loss poisons every
    rank's gradients; the verdict is therefore all-reduced (MIN) on the device before it is copied, and all ranks refuse
    the step together (no rank steps on NaN gradients, none is left waiting in the next collective)."""

    def __init__(self, *losses, group=None, vote: bool = True, flags=()):
        """`vote` / `group`: whether the verdict is shared with other ranks, and in which process group - the group of
        the model's gradient reducer / synchronised statistics (`_watch_group`): ranks outside it, or ranks that train
        independently inside an initialised world, never enter this collective, so it must not run on the default group."""
        fin = torch.stack([torch.isfinite(v.detach()).all() for v in losses] +
                          [(f.reshape(-1)[0] == 0) for f in flags if f is not None])       # S16 range flags of frozen / side networks
        self.flag = torch.empty(fin.numel(), dtype=torch.bool).pin_memory() if losses[0].is_cuda else None
        if vote and parallel.dist.is_available() and parallel.dist.is_initialized() and parallel.dist.get_world_size(group) > 1:
            vote_t = fin.to(torch.int32)
            parallel.dist.all_reduce(vote_t, op=parallel.dist.ReduceOp.MIN, group=group)
            fin = vote_t.to(torch.bool)
        if self.flag is not None:
            self.flag.copy_(fin, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
        else:
            self.flag, self.event = fin, None

    def step(self, optimizer) -> None:
        if self.event is not None:
            self.event.synchronize()
        if not bool(self.flag.all()):
            raise FloatingPointError(
                "non-finite training loss: an operand left the fp16 range of the split-fp16 kernels (or the run diverged); "
                "optimizer.step() was NOT taken - set model.train_precision = 'fp32' to train this step on the exact kernels")
        optimizer.step()


# ---- the remaining loss terms and the alternating G / D step -----------------------------------

LAMS_ANOPRED = dict(lam_adv=0.05, lam_gdl=1.0, lam_flow=2.0, lam_lp=1.0, lam_lp_op=1.0, lam_latent=1.0)
"""the reference reads its lambdas from per-dataset .ini files that are not shipped (constant_train.py:282-292);
these are the values of the ano_pred recipe the training loop was taken from"""


def gradient_loss(gen: torch.Tensor, gt: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """`Gradient_Loss` (losses_utils.py:30-61): the [-1,1] filters sum over channels, zero pad on the left / top"""
    def dxy(t):
        s = t.sum(1, keepdim=True)
        dx = torch.cat([s[..., :1], s[..., 1:] - s[..., :-1]], dim=-1)
        dy = torch.cat([s[..., :1, :], s[..., 1:, :] - s[..., :-1, :]], dim=-2)
        return dx, dy
    gx, gy = dxy(gen)
    tx, ty = dxy(gt)
    ex, ey = (tx - gx).abs(), (ty - gy).abs()
    if alpha != 1:
        ex, ey = ex ** alpha, ey ** alpha
    return (ex + ey).mean()


def adversarial_loss(fake_outputs: torch.Tensor) -> torch.Tensor:
    """`Adversarial_Loss` (losses_utils.py:100-104)"""
    return ((fake_outputs - 1) ** 2 / 2).mean()


def discriminate_loss(real_outputs: torch.Tensor, fake_outputs: torch.Tensor) -> torch.Tensor:
    """`Discriminate_Loss` (losses_utils.py:106-110)"""
    return ((real_outputs - 1) ** 2 / 2).mean() + (fake_outputs ** 2 / 2).mean()


def flow_loss(gen_flows: torch.Tensor, gt_flows: torch.Tensor) -> torch.Tensor:
    """`Flow_Loss` (losses_utils.py:10-15)"""
    return (gen_flows - gt_flows).abs().mean()


def generator_loss_full(out, rgb_t, op_t, d_gen, flow_pred=None, flow_gt=None, lam_adv=0.05, lam_gdl=1.0, lam_flow=2.0,
                        lam_lp=1.0, lam_lp_op=1.0, lam_latent=1.0) -> torch.Tensor:
    """`Twostream_vq_Loss.forward` (loss_zoo.py:310-336); the FlowNet2-SD term enters only through precomputed
    flows"""
    rgb = out[0]
    if _fused(rgb, out[1], rgb_t, op_t):
        from . import losses
        # each prediction pair is visited once: the rgb pair's two terms in one forward (and one backward) launch
        l_rgb, l_gdl = losses.prediction_terms(rgb, rgb_t, True)
        l_op, _ = losses.prediction_terms(out[1], op_t, False)
        rd, od = out[2]
        loss = lam_lp * l_rgb + lam_lp_op * l_op + lam_latent * (rd + od).sum() + lam_adv * adversarial_loss(d_gen) + \
            lam_gdl * l_gdl
        if flow_pred is not None:
            loss = loss + lam_flow * _flow_term(flow_pred, flow_gt)
        return loss
    loss = generator_loss(out, rgb_t, op_t, lam_lp, lam_lp_op, lam_latent) + lam_adv * adversarial_loss(d_gen) + \
        lam_gdl * gradient_loss(rgb, rgb_t)
    if flow_pred is not None:
        loss = loss + lam_flow * flow_loss(flow_pred, flow_gt)
    return loss


def _flow_term(flow_pred: torch.Tensor, flow_gt: torch.Tensor) -> torch.Tensor:
    """`flow_loss` under `FUSED_LOSS`: the value-only kernel where no gradient is wanted (flows out of a `no_grad` block)"""
    if _fused(flow_pred, flow_gt) and not (flow_pred.requires_grad or flow_gt.requires_grad):
        from . import losses
        return losses.l1_mean(flow_pred.contiguous(), flow_gt.contiguous())
    return flow_loss(flow_pred, flow_gt)


def train_step_gan(generator: torch.nn.Module, discriminator: torch.nn.Module, optimizer_G, optimizer_D,
                   rgb: torch.Tensor, op: torch.Tensor, flow_fn: Optional[Callable] = None,
                   outputs: Optional[dict] = None, **lams):
    """One iteration of the joint loop (train_helper.py:296-339): G forward, D(G(x)) for the adversarial term, the D
    update on (target, detached prediction), then the G update.  The gradient that reaches G through D uses the
    filters D had when `d_gen` was computed (before its update), i.e. the exact derivative of the loss value.
    `flow_fn(prev_frame, frame) -> flow` stands in for FlowNet2-SD when given.  `outputs`: a dict that receives the
    detached predicted frames ("rgb", "op"; the train PSNR of the reference's log, train_helper.py:355-357) - they may
    alias the engine's buffers, so read them before the next iteration is enqueued."""
    b = rgb.shape[0]
    rgb_in = rgb[:, :-1].reshape(b, -1, *rgb.shape[-2:])
    op_in = op[:, :-1].reshape(b, -1, *op.shape[-2:])
    rgb_t, op_t = rgb[:, -1], op[:, -1]
    out = generator(rgb_in, op_in)
    losses = _adversarial_iteration(
        generator, discriminator, optimizer_G, optimizer_D, out[0], rgb_t, flow_fn,
        lambda d_gen, flow_pred, flow_gt: generator_loss_full(out, rgb_t, op_t, d_gen, flow_pred, flow_gt, **lams))
    if outputs is not None:
        outputs["rgb"], outputs["op"] = out[0].detach(), out[1].detach()
    return losses


def _adversarial_iteration(generator, discriminator, optimizer_G, optimizer_D, pred: torch.Tensor, target: torch.Tensor,
                           flow_fn: Optional[Callable], g_loss_fn: Callable):
    """The schedule of one adversarial iteration behind the generator's forward, shared by `train_step_gan` and
    `train_step_single_gan`: `pred` is the predicted frame / flow D sees (attached to the generator's graph), `target`
    its ground truth, `g_loss_fn(d_gen, flow_pred, flow_gt) -> g_loss` the caller's generator loss (the flows are None
    without `flow_fn`).  D is updated first, on (target, detached prediction); both updates are refused together on a
    non-finite verdict.  -> the detached (g_loss, d_loss)"""
    b = target.shape[0]
    vote, group = _watch_group(generator, discriminator)
    # `AMMC_GAN_OVERLAP` (default on): the D update is independent of everything the generator still has to do - it
    # reads the prediction detached, and the gradient that reaches G through D uses the filter packs of the `d_gen`
    # forward, not the live parameters - so its forward (beside FlowNet2-SD and the `d_gen` forward), its backward and its
    # Adam step (beside the generator's backward, whose BatchNorm passes leave the matrix pipe idle: the two-stream argument
    # of DESIGN.md section 4) run on a SECOND HIP stream, forked right behind the generator's forward.  Same kernels, same
    # order on each stream: every number is what the serial form computes.  Off with a gradient reducer / synchronised
    # statistics attached (their collectives are ordered on the caller's stream) and on the CPU.
    overlap = GAN_OVERLAP and pred.is_cuda and not vote and getattr(discriminator, "_grad_reducer", None) is None
    main = torch.cuda.current_stream(pred.device) if overlap else None
    lane = _gan_side_stream(pred.device) if overlap else None
    on_lane = (lambda: torch.cuda.stream(lane)) if overlap else contextlib.nullcontext
    if overlap:
        lane.wait_stream(main)
    with on_lane():
        # D(real) and D(fake.detach()) (train_helper.py:326-327) as one call on 2 b frames: the discriminator has no
        # batch-coupled layer, the patch maps and every gradient are those of the two calls
        d_both = discriminator(torch.cat([target, pred.detach()]))
        d_loss = discriminate_loss(d_both[:b], d_both[b:])
        d_flag = getattr(discriminator, "last_overflow", None)
    flow_pred = flow_gt = None
    flow_mods = [m for m in (getattr(flow_fn, "__self__", None), getattr(flow_fn, "net", None)) if m is not None]
    if flow_fn is not None:
        with torch.no_grad():
            # the reference pairs BOTH frames with `rgb_input_last = rgb[:, -1]`, i.e. with the target frame itself
            # (train_helper.py:299, 309-312), not with the frame before it: followed as written.  The two FlowNet2-SD
            # forwards run as ONE batch of 2 b pairs (every sample is independent in that network - its mean subtraction
            # is per sample - so the flows are the same; the layers below 1/16 resolution fill the chip twice as well)
            both = flow_fn(torch.cat([target, target]), torch.cat([pred.detach(), target]))
            flow_pred, flow_gt = both[:b], both[b:]
    d_params = [p for p in discriminator.parameters() if p.requires_grad]
    for p in d_params:                 # the G step needs dL/d(frame) through D, not D's weight gradients
        p.requires_grad_(False)
    try:
        d_gen = discriminator(pred)
    finally:
        for p in d_params:
            p.requires_grad_(True)
    g_loss = g_loss_fn(d_gen, flow_pred, flow_gt)
    if overlap:
        main.wait_stream(lane)                     # (the verdict below reads d_loss on the caller's stream)
        for t in (d_both, d_loss) + ((d_flag,) if d_flag is not None else ()):
            t.record_stream(main)
    # (the S16 range flags of the discriminator and - where `flow_fn` is a bound method / has `.net` - of the frozen flow
    # estimator join the verdict: `s16_guard = "defer"` on those modules leaves them on the device instead of syncing)
    watch = _FiniteWatch(d_loss, g_loss, group=group, vote=vote,
                         flags=[d_flag] + [getattr(m, "last_overflow", None) for m in flow_mods])
    with on_lane():
        optimizer_D.zero_grad(set_to_none=True)
        d_loss.backward()                          # (autograd runs it on the stream of its forward: the lane)
        watch.step(optimizer_D)
    optimizer_G.zero_grad(set_to_none=True)
    g_loss.backward()
    optimizer_G.step()
    if overlap:
        main.wait_stream(lane)                     # successors on the caller's stream see both updates
    return g_loss.detach(), d_loss.detach()


# (the two FlowNet2-SD forwards on a third stream, their no-gradient term joined to the loss value at the end, were built and
# measured as well: 80.2 / 80.4 ms against 80.2 / 79.3 - nothing; removed)
# AMMC_GAN_OVERLAP: on (default; any value but 0) = the D lane starts right behind the generator's forward (its own forward
# beside FlowNet2-SD and the d_gen forward), 0 = serial.  A late form, the lane starting behind g_loss, came first (81.69 /
# 81.59 -> 78.94 / 79.19 ms against serial); the present one beat it, 79.84 / 80.20 / 79.85 -> 79.04 / 78.82 / 78.88 ms, and
# the late form was retired after that A/B: it lives in the history of this file.
GAN_OVERLAP = os.environ.get("AMMC_GAN_OVERLAP", "1") != "0"
_GAN_LANES: Dict = {}


def _gan_side_stream(device, which: int = 0) -> "torch.cuda.Stream":
    key = (device.type, device.index, which)
    if key not in _GAN_LANES:
        _GAN_LANES[key] = torch.cuda.Stream(device=device)
    return _GAN_LANES[key]


# ---- stage 1 of the reference's recipe: one stream (`UNetMem_v7`) trained on its own ---------------------------------

SINGLE_LAMS = {"rgb": dict(lam_adv=0.05, lam_gdl=1.0, lam_flow=2.0, lam_lp=1.0, lam_latent=1.0),
               "op": dict(lam_lp_op=1.0, lam_adv_op=0.0, lam_latent=1.0)}
"""the loss weights of each single-stream stage and their defaults (the values of LAMS_ANOPRED; `lam_adv_op` lives in
a per-dataset .ini that is not shipped, and the README's stage 1 is prediction + commit loss only: 0 = no discriminator)"""


def clip_stream(clips: torch.Tensor) -> str:
    """"rgb" / "op" from a clip batch [B, T, c, H, W] (3 channels: frames, 2: flows)"""
    if clips.dim() != 5 or clips.shape[2] not in (2, 3):
        raise ValueError(f"expected clips [B, T, 3 or 2, H, W], got {tuple(clips.shape)}")
    return "rgb" if clips.shape[2] == 3 else "op"


def single_stream_loss(stream: str, pred, target, diff, d_gen=None, flow_pred=None, flow_gt=None, **lams):
    """`rgb_vq_Loss` (loss_zoo.py:101-137): lam_adv adv + lam_gdl gdl + lam_flow flow + lam_lp int + lam_latent latent,
    or `op_vq_Loss` (:171-198): lam_lp_op int + lam_adv_op adv + lam_latent latent - the adversarial term only where a
    discriminator output `d_gen` is given, the flow term only where flows are.  `int` is the channel-L2 intensity loss
    of `generator_loss`, `latent` the commit loss `diff`.  -> (loss, {term: unweighted value})"""
    unknown = set(lams) - set(SINGLE_LAMS[stream])
    if unknown:
        raise TypeError(f"the {stream} stage has no loss weight {sorted(unknown)} (it takes {sorted(SINGLE_LAMS[stream])})")
    lam = {**SINGLE_LAMS[stream], **lams}
    if stream == "rgb" and d_gen is None:
        raise ValueError("the rgb stage's loss has an adversarial term: it needs the discriminator's output")
    if _fused(pred, target):
        from . import losses
        l_int, l_gdl = losses.prediction_terms(pred, target, stream == "rgb")
        t = {"int": l_int, "latent": diff.sum()}
    else:
        l_gdl = None
        t = {"int": torch.norm(pred - target, p=2, dim=1).mean(), "latent": diff.sum()}
    if stream == "rgb":
        t["adv"], t["gdl"] = adversarial_loss(d_gen), (l_gdl if l_gdl is not None else gradient_loss(pred, target))
        loss = lam["lam_adv"] * t["adv"] + lam["lam_gdl"] * t["gdl"]
        if flow_pred is not None:
            t["flow"] = _flow_term(flow_pred, flow_gt)
            loss = loss + lam["lam_flow"] * t["flow"]
        loss = loss + lam["lam_lp"] * t["int"]
    else:
        loss = lam["lam_lp_op"] * t["int"]
        if d_gen is not None:
            t["adv"] = adversarial_loss(d_gen)
            loss = loss + lam["lam_adv_op"] * t["adv"]
    return loss + lam["lam_latent"] * t["latent"], t


def train_step_single_gan(generator: torch.nn.Module, discriminator: torch.nn.Module, optimizer_G, optimizer_D,
                          clips: torch.Tensor, flow_fn: Optional[Callable] = None, outputs: Optional[dict] = None, **lams):
    """One iteration of a single-stream stage with its discriminator (`inference_v3` / `inference_v4`,
    train_helper.py:1592-1766): `generator` a `UNetMem_v7`, `clips` [B, T, c, H, W] with the target last - frames (the
    rgb stage, c = 3, `rgb_vq_Loss`; `flow_fn` stands in for FlowNet2-SD as in `train_step_gan`, both pairs starting
    from the target) or flows (the op stage with lam_adv_op > 0, c = 2, `op_vq_Loss`; no flow term).  The same
    schedule as `train_step_gan`: D(real || fake) as one call, D updated first (on the `AMMC_GAN_OVERLAP` lane), G
    through D with the pre-step filters, then the G update; the verdict of `_FiniteWatch` covers both losses and the S16
    range flags of D and of the flow network.  Returns the detached (g_loss, d_loss); `outputs` receives the detached
    prediction ("pred") and the loss terms ("terms", unweighted) - read them before the next iteration is enqueued."""
    b = clips.shape[0]
    stream = clip_stream(clips)
    if flow_fn is not None and stream != "rgb":
        raise ValueError("the flow term belongs to the rgb stage")
    x = clips[:, :-1].reshape(b, -1, *clips.shape[-2:])
    target = clips[:, -1]
    pred, diff, _ = generator(x)
    kept = {}

    def g_loss_fn(d_gen, flow_pred, flow_gt):
        g_loss, kept["terms"] = single_stream_loss(stream, pred, target, diff, d_gen, flow_pred, flow_gt, **lams)
        return g_loss
    losses = _adversarial_iteration(generator, discriminator, optimizer_G, optimizer_D, pred, target, flow_fn, g_loss_fn)
    if outputs is not None:
        outputs["pred"], outputs["terms"] = pred.detach(), {k: v.detach() for k, v in kept["terms"].items()}
    return losses


def train_step_single(generator: torch.nn.Module, optimizer_G, clips: torch.Tensor, outputs: Optional[dict] = None,
                      **lams) -> torch.Tensor:
    """One iteration of the op stage without a discriminator (lam_adv_op = 0: the README's stage 1, prediction + commit
    loss, `inference_v4_1` / `op_vq_Loss_v1`, loss_zoo.py:232-262): `clips` flows [B, T, 2, H, W], target last.
    Returns the detached loss; `outputs` as `train_step_single_gan`'s."""
    b = clips.shape[0]
    if clip_stream(clips) != "op":
        raise ValueError("train_step_single is the discriminator-less op stage: the rgb stage is train_step_single_gan")
    if lams.get("lam_adv_op", 0.0):
        raise ValueError("lam_adv_op > 0 needs a discriminator: train_step_single_gan")
    lams = {k: v for k, v in lams.items() if k != "lam_adv_op"}
    x = clips[:, :-1].reshape(b, -1, *clips.shape[-2:])
    target = clips[:, -1]

    def forward():
        pred, diff, _ = generator(x)
        loss, terms = single_stream_loss("op", pred, target, diff, **lams)
        return loss, (pred, terms)
    loss, (pred, terms) = _generator_iteration(generator, optimizer_G, forward)
    if outputs is not None:
        outputs["pred"], outputs["terms"] = pred.detach(), {k: v.detach() for k, v in terms.items()}
    return loss


# ---- score fusion and frame-level AUC (the step after the records) ------------------------------

LAM_MAP = {"avenue": (0.04, 0.65), "ped2": (0.01, 0.55), "shanghaitech": (0.13, 0.60)}   # test_helper.py:565-569
DECIDABLE_IDX = 4                                                                          # eval_metric.py:17


def _minmax_concat(records: Sequence[np.ndarray]) -> np.ndarray:
    """per-video min-max normalisation, drop the first DECIDABLE_IDX frames, global min-max
    (`norm_score`, main/eval_metric.py:405-417)"""
    parts = []
    for r in records:
        r = np.array(r, dtype=np.float32)
        r = r - r.min()
        r = r / r.max()
        parts.append(r[DECIDABLE_IDX:])
    s = np.concatenate(parts)
    s = s - s.min()
    return s / s.max()


def roc_auc(labels: np.ndarray, scores: np.ndarray, pos_label: int = 0) -> float:
    """area under the ROC curve by the trapezoid rule over distinct thresholds (what
    sklearn.metrics.roc_curve + auc compute; ties share one threshold)"""
    y = (np.asarray(labels) == pos_label)
    s = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-s, kind="mergesort")
    y, s = y[order], s[order]
    distinct = np.where(np.diff(s))[0]
    idx = np.r_[distinct, y.size - 1]
    tps = np.cumsum(y)[idx].astype(np.float64)
    fps = (1 + idx - tps).astype(np.float64)
    tps, fps = np.r_[0.0, tps], np.r_[0.0, fps]
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    return float(trapezoid(tps / tps[-1], fps / fps[-1]))


def fuse_scores_auc(records: dict, gt: Sequence[np.ndarray], lam=None) -> dict:
    """`img_pred_fea_comm_single_auc` (main/eval_metric.py:382-439): normality score
    (1-l1)*psnr_n + l1*(1 - commit_n), one-tap smoothing s'_i = (1-l2) s_{i-1} + l2 s_i (from the
    UNSMOOTHED neighbour), ROC with the normal class (label 0) positive, AUC rounded to 3 d.p.
    `records` is the dict of `evaluate_dataset`; `gt[i]` the per-frame labels of video i (1 = anomalous)."""
    l1, l2 = lam if lam is not None else LAM_MAP[records["dataset"]]
    labels = np.concatenate([np.asarray(g)[DECIDABLE_IDX:] for g in gt])
    img = _minmax_concat(records["rgb_img_pred_records"])
    fea = _minmax_concat(records["rgb_fea_comm_records"])
    scores = (1 - l1) * img + l1 * (1.0 - fea)
    smooth = scores.copy()
    smooth[1:] = (1 - l2) * scores[:-1] + l2 * scores[1:]
    auc = roc_auc(labels, smooth, pos_label=0)
    return {"auc": round(auc, 3), "auc_raw": auc, "lam": (l1, l2), "scores": smooth}


# ---- score-fusion sweep: the AUC over a grid of channel weights and smoothings ----

# channel name -> (key of the records dict, orientation).  Every channel enters the fusion as "higher = more normal":
#   "img":  a quality of the prediction (PSNR, SSIM), used as `_minmax_concat` returns it
#   "comm": a distance to the memory (commit records), used as 1.0f - n, as `fuse_scores_auc` uses the commit records
#   "mse":  an error, negated BEFORE the normalisation (as run_quality's auc_mse), then as "img"
FUSION_CHANNELS = {
    "rgb_img_pred": ("rgb_img_pred_records", "img"), "op_img_pred": ("op_img_pred_records", "img"),
    "rgb_fea_comm": ("rgb_fea_comm_records", "comm"), "op_fea_comm": ("op_fea_comm_records", "comm"),
    "rgb_ssim": ("rgb_ssim_records", "img"), "op_ssim": ("op_ssim_records", "img"),
    "rgb_mse": ("rgb_mse_records", "mse"), "op_mse": ("op_mse_records", "mse"),
    "rgb_clip_comm": ("rgb_clip_comm_records", "comm"), "op_clip_comm": ("op_clip_comm_records", "comm"),
    "rgb_patch_psnr": ("rgb_patch_psnr_records", "img"),
}
FUSION_LAM_FEA = [x * 0.01 for x in range(0, 100)]       # lam_rgb_fea_comm_list, main/eval_metric.py:422
FUSION_LAM_SMOOTH = [x * 0.05 for x in range(0, 20)]     # lam_smooth_list, main/eval_metric.py:423


def smoothing_pairs(lam_smooth: Sequence[float]) -> np.ndarray:
    """[S, 2] fp32 pairs (a, b) = (float32(1 - l2), float32(l2)): the constants `fuse_scores_auc`'s fp32 arrays are
    multiplied by"""
    return np.array([[1 - l2, l2] for l2 in lam_smooth], dtype=np.float32).reshape(-1, 2)


def fusion_grid(k: int = 2, step: Optional[float] = None) -> dict:
    """The grid of a sweep over `k` channels: `weights` fp32 [G, k], `lam_smooth` (the reference's 20 values) and
    `smooth`, their fp32 pairs.  k = 2 without a step: the reference's grid, `lam_fea` = x * 0.01 for x < 100 with the
    weights (float32(1 - l1), float32(l1)).  Otherwise every vector whose entries are multiples of `step` (default 0.1)
    and sum to 1, in lexicographic order, each entry float32(m / M) with M = round(1 / step)."""
    if k < 1:
        raise ValueError("fusion_grid: k >= 1")
    out = {"lam_smooth": list(FUSION_LAM_SMOOTH), "smooth": smoothing_pairs(FUSION_LAM_SMOOTH)}
    if k == 2 and step is None:
        out["lam_fea"] = list(FUSION_LAM_FEA)
        out["weights"] = np.array([[1 - l1, l1] for l1 in FUSION_LAM_FEA], dtype=np.float32)
        return out
    M = int(round(1.0 / (0.1 if step is None else step)))
    if M < 1:
        raise ValueError("fusion_grid: 0 < step <= 1")

    def parts(left: int, slots: int):
        if slots == 1:
            yield (left,)
            return
        for m in range(left + 1):
            for rest in parts(left - m, slots - 1):
                yield (m,) + rest
    out["weights"] = np.array([[m / M for m in v] for v in parts(M, k)], dtype=np.float32)
    return out


def fusion_channels(records: dict, channels: Sequence[str]) -> np.ndarray:
    """fp32 [K, N]: the named channels of `records`, normalised (`_minmax_concat`: the first DECIDABLE_IDX frames of each
    video dropped) and oriented so that higher = more normal (FUSION_CHANNELS)"""
    rows = []
    for name in channels:
        if name not in FUSION_CHANNELS:
            raise ValueError(f"unknown fusion channel {name!r}: one of {sorted(FUSION_CHANNELS)}")
        key, kind = FUSION_CHANNELS[name]
        if key not in records:
            raise ValueError(f"fusion channel {name!r} needs records[{key!r}]: this evaluation did not compute it")
        rec = records[key]
        if kind == "mse":
            rec = [-np.asarray(r, dtype=np.float32) for r in rec]
        n = _minmax_concat(rec)
        rows.append(1.0 - n if kind == "comm" else n)
    return np.stack(rows).astype(np.float32, copy=False)


def sweep_fusion(records: dict, gt: Sequence[np.ndarray], channels: Sequence[str] = ("rgb_img_pred", "rgb_fea_comm"),
                 weights=None, smooth: Optional[Sequence[float]] = None, device=None) -> dict:
    """The frame-level AUC of the fused score at every point of a grid, from one device launch (`ops.fusion_sweep`).
    `records` / `gt` as `fuse_scores_auc` takes them; `channels`: names of FUSION_CHANNELS (at most 8); `weights`:
    [G, K] (default `fusion_grid(K)`'s); `smooth`: lam_smooth values (default the reference's 20).  Returns `two_u`
    (int64 [G, S]), `auc` (float64 [G, S] = two_u / (2 P Q)), `n_pos`, `n_neg`, `weights`, `lam_smooth`, `sweep_ms`
    (the launch between device events), `best` = {weights, lam_smooth, auc, index} - on equal AUC the first in grid
    order - and, for two channels of a dataset in LAM_MAP, `auc_at_lam_map`: the AUC at the published pair, which for
    the default channels is `fuse_scores_auc`'s.  The HIP pass is the only implementation: a GPU is required."""
    from . import ops
    channels = tuple(channels)
    chan = fusion_channels(records, channels)
    labels = np.concatenate([np.asarray(g)[DECIDABLE_IDX:] for g in gt])
    K, N = chan.shape
    if labels.shape[0] != N:
        raise ValueError(f"sweep_fusion: {labels.shape[0]} labels for {N} scored frames")
    if not np.isfinite(chan).all():
        bad = [c for c, row in zip(channels, chan) if not np.isfinite(row).all()]
        raise ValueError(f"sweep_fusion: non-finite normalised scores in {bad} (a constant record, or a NaN / inf in it)")
    pos, neg = np.flatnonzero(labels == 0), np.flatnonzero(labels != 0)
    if pos.size == 0 or neg.size == 0:
        raise ValueError("sweep_fusion: the labels hold one class only: the AUC is undefined")
    grid = fusion_grid(K)
    w = grid["weights"] if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1, K))
    lam_smooth = list(grid["lam_smooth"] if smooth is None else smooth)
    sm = smoothing_pairs(lam_smooth)
    lam = LAM_MAP.get(records.get("dataset")) if K == 2 else None
    if lam is not None:                                   # one more grid point of a second, 1 x 1 launch
        w_lam, sm_lam = np.array([[1 - lam[0], lam[0]]], dtype=np.float32), smoothing_pairs([lam[1]])
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)
    d_chan, d_pos, d_neg = up(chan, torch.float32), up(pos, torch.int32), up(neg, torch.int32)
    d_w, d_sm = up(w, torch.float32), up(sm, torch.float32)
    with torch.cuda.device(dev):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        d_u = ops.fusion_sweep(d_chan, d_pos, d_neg, d_w, d_sm)
        t1.record()
        d_lam = ops.fusion_sweep(d_chan, d_pos, d_neg, up(w_lam, torch.float32), up(sm_lam, torch.float32)) if lam else None
        two_u = d_u.cpu().numpy()
        ms = t0.elapsed_time(t1)
    denom = 2.0 * float(pos.size) * float(neg.size)
    auc = two_u.astype(np.float64) / denom
    gi, si = np.unravel_index(int(np.argmax(auc)), auc.shape)
    out = {"two_u": two_u, "auc": auc, "n_pos": int(pos.size), "n_neg": int(neg.size), "channels": channels, "weights": w,
           "lam_smooth": lam_smooth, "sweep_ms": float(ms),
           "best": {"weights": [float(x) for x in w[gi]], "lam_smooth": float(lam_smooth[si]), "auc": float(auc[gi, si]),
                    "index": (int(gi), int(si))}}
    if d_lam is not None:
        out["auc_at_lam_map"] = float(int(d_lam.cpu()[0, 0]) / denom)
        out["lam_map"] = tuple(lam)
    return out


# ---- curve sweep: EER, average precision and precision-recall area over the same grid ----
# The reference's other two evaluation types (`compute_eer`, `precision_recall_auc`: main/eval_metric.py:442-446) from a
# device pass of its own (`ops.curve_sweep`); `sweep_fusion` above is untouched.

def roc_eer(labels: np.ndarray, scores: np.ndarray, pos_label: int = 0, drop_intermediate: bool = True) -> float:
    """`cal_eer(*roc_curve(labels, scores, pos_label))` (main/eval_metric.py:315-318) restated: the false-positive rate at
    the vertex where |fpr + tpr - 1| is smallest, the first one on a tie.  The vertices are sklearn's: one per distinct
    score, of which `drop_intermediate` keeps those where the second difference of the false- or of the true-positive
    count is non-zero, and both ends; then the origin in front.  The rates are the float64 quotients sklearn forms."""
    y = np.asarray(labels) == pos_label
    s = np.asarray(scores)
    order = np.argsort(s, kind="mergesort")[::-1]
    y, s = y[order], s[order]
    idx = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y)[idx]
    fps = 1 + idx - tps
    if drop_intermediate and len(fps) > 2:
        keep = np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True]
        fps, tps = fps[keep], tps[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    return float(fpr[np.nanargmin(np.absolute(fpr + tpr - 1))])


def fused_keys(chan: np.ndarray, w, pair) -> np.ndarray:
    """key[i] of one grid point on the host, as include/ammc_hip.h defines it: every product and sum one rounded fp32
    numpy operation, left to right; `pair` = (a, b)"""
    chan, w = np.asarray(chan, dtype=np.float32), np.asarray(w, dtype=np.float32)
    f = w[0] * chan[0]
    for k in range(1, chan.shape[0]):
        f = f + w[k] * chan[k]
    t = f.copy()
    t[1:] = np.float32(pair[0]) * f[:-1] + np.float32(pair[1]) * f[1:]
    return t + np.float32(0.0)


CURVE_KEYS = ("auc", "eer", "eer_vertex", "ap", "pr_auc")


def curve_metrics(two_u, pts, thr, sums, n_pos: int, n_neg: int) -> dict:
    """what include/ammc_hip.h derives from `ops.curve_sweep`'s outputs, in float64 and any leading shape: `auc`, `eer`
    (the crossing of segment a-b with fpr + tpr = 1), `eer_vertex` (`cal_eer` on the full curve), `ap`, `pr_auc`, and
    `threshold_eer`: the key value of `eer_vertex`'s vertex (a frame is called positive iff its key >= it)"""
    pts = np.asarray(pts, dtype=np.int64)
    P, Q = np.int64(n_pos), np.int64(n_neg)
    tpa, fpa, tpb, fpb = (pts[..., i] for i in range(4))
    ga, gb = P * fpa + Q * tpa - P * Q, P * fpb + Q * tpb - P * Q
    first = np.abs(ga) <= np.abs(gb)
    lam = -ga / (gb - ga).astype(np.float64)
    sums, thr = np.asarray(sums, dtype=np.float64), np.asarray(thr)
    return {"auc": np.asarray(two_u) / (2.0 * float(P) * float(Q)), "eer": (fpa + lam * (fpb - fpa)) / float(Q),
            "eer_vertex": np.where(first, fpa, fpb) / float(Q), "ap": sums[..., 0] / float(P), "pr_auc": sums[..., 1] / float(P),
            "threshold_eer": np.where(first, thr[..., 0], thr[..., 1])}


def sweep_curves(records: dict, gt: Sequence[np.ndarray], channels: Sequence[str] = ("rgb_img_pred", "rgb_fea_comm"),
                 weights=None, smooth: Optional[Sequence[float]] = None, positive: str = "normal", device=None) -> dict:
    """AUC, equal error rate, average precision and precision-recall area of the fused score at every point of a grid
    (`ops.curve_sweep`); inputs as `sweep_fusion` takes them.  `positive`: "normal" (the reference's pos_label = 0) or
    "anomalous" - what a detection paper's AP means: the two classes change places and the weights their sign, which
    negates every key exactly.  Returns float64 [G, S] arrays `auc`, `eer`, `eer_vertex`, `ap`, `pr_auc`, `threshold_eer`
    (`curve_metrics`), the device's `pts` and `two_u`, `n_pos`, `n_neg`, `weights` (as given, before the sign),
    `lam_smooth`, `sweep_ms` (the launches of the grid between device events) and `best` = {"auc": argmax, "eer": argmin of
    `eer`, "ap": argmax}, each {weights, lam_smooth, index, the five values, threshold_eer, eer_reference} - on equal values
    the first in grid order.  `eer_reference` is the reference's literal call, `roc_eer` with sklearn's default vertex
    dropping, on the host.  For two channels of a dataset in LAM_MAP, `at_lam_map` holds the same at the published pair.
    The HIP pass is the only implementation: a GPU is required."""
    from . import ops
    if positive not in ("normal", "anomalous"):
        raise ValueError(f"sweep_curves: positive must be 'normal' or 'anomalous', got {positive!r}")
    channels = tuple(channels)
    chan = fusion_channels(records, channels)
    labels = np.concatenate([np.asarray(g)[DECIDABLE_IDX:] for g in gt])
    K, N = chan.shape
    if labels.shape[0] != N:
        raise ValueError(f"sweep_curves: {labels.shape[0]} labels for {N} scored frames")
    if not np.isfinite(chan).all():
        bad = [c for c, row in zip(channels, chan) if not np.isfinite(row).all()]
        raise ValueError(f"sweep_curves: non-finite normalised scores in {bad} (a constant record, or a NaN / inf in it)")
    is_pos = (labels == 0) if positive == "normal" else (labels != 0)
    pos, neg = np.flatnonzero(is_pos), np.flatnonzero(~is_pos)
    if pos.size == 0 or neg.size == 0:
        raise ValueError("sweep_curves: the labels hold one class only: the curves are undefined")
    sign = np.float32(1.0 if positive == "normal" else -1.0)
    grid = fusion_grid(K)
    w = grid["weights"] if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1, K))
    lam_smooth = list(grid["lam_smooth"] if smooth is None else smooth)
    sm = smoothing_pairs(lam_smooth)
    lam = LAM_MAP.get(records.get("dataset")) if K == 2 else None
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)
    d_chan, d_pos, d_neg = up(chan, torch.float32), up(pos, torch.int32), up(neg, torch.int32)
    with torch.cuda.device(dev):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d_w, d_sm = up(sign * w, torch.float32), up(sm, torch.float32)
        t0.record()
        d_grid = ops.curve_sweep(d_chan, d_pos, d_neg, d_w, d_sm)
        t1.record()
        if lam is not None:                               # one more grid point of a second, 1 x 1 launch
            w_lam, sm_lam = np.array([[1 - lam[0], lam[0]]], dtype=np.float32), smoothing_pairs([lam[1]])
            d_lam = ops.curve_sweep(d_chan, d_pos, d_neg, up(sign * w_lam, torch.float32), up(sm_lam, torch.float32))
        res = {k: v.cpu().numpy() for k, v in d_grid.items()}
        ms = t0.elapsed_time(t1)
    P, Q = int(pos.size), int(neg.size)
    m = curve_metrics(res["two_u"], res["pts"], res["thr"], res["sums"], P, Q)

    def point(values, at, wv, pair, l2):
        out = {"weights": [float(x) for x in wv], "lam_smooth": float(l2)}
        out.update({k: float(values[k][at]) for k in CURVE_KEYS + ("threshold_eer",)})
        out["eer_reference"] = roc_eer(is_pos, fused_keys(chan, sign * np.asarray(wv, dtype=np.float32), pair), pos_label=True)
        return out
    best = {}
    for name, flat in (("auc", np.argmax(m["auc"])), ("eer", np.argmin(m["eer"])), ("ap", np.argmax(m["ap"]))):
        gi, si = (int(x) for x in np.unravel_index(int(flat), m["auc"].shape))
        best[name] = dict(point(m, (gi, si), w[gi], sm[si], lam_smooth[si]), index=(gi, si))
    out = dict(m, two_u=res["two_u"], pts=res["pts"], n_pos=P, n_neg=Q, channels=channels, positive=positive, weights=w,
               lam_smooth=lam_smooth, sweep_ms=float(ms), best=best)
    if lam is not None:
        r = {k: v.cpu().numpy() for k, v in d_lam.items()}
        out["at_lam_map"] = point(curve_metrics(r["two_u"], r["pts"], r["thr"], r["sums"], P, Q), (0, 0), w_lam[0], sm_lam[0], lam[1])
        out["lam_map"] = tuple(lam)
    return out


# ---- macro AUC and video-bootstrap confidence intervals from per-video pair counts ----
# Frames of one video are correlated, so the sampling unit of an error bar is the video.  `ops.video_pairs` splits the
# sweep's count by the video of either frame (a V x V integer block per grid point); its diagonal gives the per-video and
# the macro AUC, and `ops.bootstrap_pairs` - a bilinear form in the replica's multiplicities - the AUC of every bootstrap
# replica without resampling a frame.  Passes of their own: `sweep_fusion` and `sweep_curves` above are untouched.

def video_offsets(gt: Sequence[np.ndarray], labels_positive: int = 0) -> dict:
    """Where each video's frames stand in the class index lists of a sweep: `n_pos`, `n_neg` (int64 [V], the video's
    scored frames of either class) and `pos_off`, `neg_off` (int64 [V + 1], their running sums from 0).  `gt[v]`: the
    per-frame labels of video v; a frame is positive iff its label equals `labels_positive` (0: the normal class).  The
    first DECIDABLE_IDX frames of each video are not scored, as `sweep_fusion` drops them: a shorter video has none."""
    n_pos = np.array([int((np.asarray(g)[DECIDABLE_IDX:] == labels_positive).sum()) for g in gt], dtype=np.int64)
    n_neg = np.array([int((np.asarray(g)[DECIDABLE_IDX:] != labels_positive).sum()) for g in gt], dtype=np.int64)
    return {"n_pos": n_pos, "n_neg": n_neg, "pos_off": np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int64),
            "neg_off": np.concatenate([[0], np.cumsum(n_neg)]).astype(np.int64)}


def bootstrap_multiplicities(V: int, replicas: int, seed: int) -> np.ndarray:
    """int32 [replicas, V]: how often each of V videos is drawn in each replica of a bootstrap of V draws with
    replacement - one multinomial row per replica from PCG64(seed): the same seed gives the same table"""
    if V < 1 or replicas < 1:
        raise ValueError(f"bootstrap_multiplicities: V >= 1 and replicas >= 1, got {V} and {replicas}")
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.multinomial(V, np.full(V, 1 / V), size=replicas).astype(np.int32)


def _interval(x: np.ndarray, level: float) -> np.ndarray:
    """percentiles (1 - level) / 2 and (1 + level) / 2 over axis 0, numpy's default linear rule, float64 -> [..., 2]"""
    q = np.percentile(np.asarray(x, dtype=np.float64), [50.0 * (1.0 - level), 50.0 * (1.0 + level)], axis=0)
    return np.moveaxis(q, 0, -1)


def replica_statistics(two_u_r, diag, mult, n_pos, n_neg, level: float = 0.95, grid_points: Optional[int] = None,
                       best: Optional[int] = None) -> dict:
    """What a video bootstrap says about M points, on the host in float64 - a pure function of its arguments:
    `two_u_r` int64 [B, M] (`ops.bootstrap_pairs`' table), `diag` int64 [M, V] (the diagonals of the pair blocks), `mult`
    [B, V], `n_pos` / `n_neg` [V] (P_a, Q_a).  Replica r has P_r = sum m[a] P_a, Q_r = sum m[b] Q_b, the AUC
    two_u_r / (2 P_r Q_r) and the macro AUC sum m[a] auc_a / sum m[a] over the scored videos (both classes present).  A
    replica with P_r = 0, Q_r = 0 or no scored video has neither: it is dropped from every statistic and counted; more
    than half of them dropped is a ValueError.  Returns `usable` (bool [B]), `replicas_dropped`, `per_video_auc` [M, V]
    (NaN where a class is missing), `macro_auc` [M], `auc_r` and `macro_auc_r` [usable, M], `auc_ci` and `macro_auc_ci`
    [M, 2] (`level`), and - with `best`, an index below `grid_points` (default M) - `best_share`: the share of usable
    replicas whose own first argmax over the first `grid_points` points is `best`."""
    two_u_r, diag = np.asarray(two_u_r, dtype=np.int64), np.asarray(diag, dtype=np.int64)
    mult, n_pos, n_neg = np.asarray(mult, dtype=np.int64), np.asarray(n_pos, dtype=np.int64), np.asarray(n_neg, dtype=np.int64)
    if not 0.0 < level < 1.0:
        raise ValueError(f"replica_statistics: 0 < level < 1, got {level}")
    scored = (n_pos > 0) & (n_neg > 0)
    p_r, q_r, s_r = mult @ n_pos, mult @ n_neg, mult[:, scored].sum(1)
    usable = (p_r > 0) & (q_r > 0) & (s_r > 0)
    dropped = int((~usable).sum())
    if 2 * dropped > mult.shape[0]:
        raise ValueError(f"replica_statistics: {dropped} of {mult.shape[0]} replicas have no AUC (a class or every scored "
                         f"video missing): too few videos hold both classes for a bootstrap over videos")
    with np.errstate(divide="ignore", invalid="ignore"):
        per_video = np.where(scored, diag / (2.0 * n_pos * n_neg), np.nan)
    auc_r = two_u_r[usable] / (2.0 * p_r[usable] * q_r[usable])[:, None]
    m_s = mult[usable][:, scored].astype(np.float64)
    macro_r = (m_s @ per_video[:, scored].T) / m_s.sum(1)[:, None]
    out = {"usable": usable, "replicas_dropped": dropped, "per_video_auc": per_video,
           "macro_auc": per_video[:, scored].mean(1) if scored.any() else np.full(diag.shape[0], np.nan),
           "auc_r": auc_r, "macro_auc_r": macro_r, "auc_ci": _interval(auc_r, level), "macro_auc_ci": _interval(macro_r, level)}
    if best is not None:
        n_grid = auc_r.shape[1] if grid_points is None else grid_points
        out["best_share"] = float((np.argmax(auc_r[:, :n_grid], axis=1) == best).mean())
    return out


def bootstrap_delta(res: dict, i, j) -> dict:
    """mean and confidence interval (`res["level"]`) of the paired difference auc_r[i] - auc_r[j] over the usable replicas
    of a `sweep_videos` result; `i`, `j`: grid indices (g, s), flat indices in grid order, or "lam_map" """
    S = res["auc"].shape[1]

    def flat(x):
        if isinstance(x, str):
            if x != "lam_map" or "at_lam_map" not in res:
                raise ValueError(f"bootstrap_delta: no point {x!r} in this result")
            return res["auc"].size
        return int(x[0]) * S + int(x[1]) if isinstance(x, (tuple, list)) else int(x)
    d = res["replica_auc"][:, flat(i)] - res["replica_auc"][:, flat(j)]
    return {"mean": float(d.mean()), "ci": [float(x) for x in _interval(d, res["level"])]}


def sweep_videos(records: dict, gt: Sequence[np.ndarray], channels: Sequence[str] = ("rgb_img_pred", "rgb_fea_comm"),
                 weights=None, smooth: Optional[Sequence[float]] = None, replicas: int = 1000, seed: int = 0, level: float = 0.95,
                 max_workspace_bytes: int = 256 << 20, device=None) -> dict:
    """The micro and the macro frame-level AUC of the fused score at every point of a grid, with percentile confidence
    intervals from a bootstrap over VIDEOS (`ops.video_pairs`, then `ops.bootstrap_pairs`).  Inputs, channel handling and
    refusals as `sweep_fusion`; for two channels of a dataset in LAM_MAP the published pair is one more point behind the
    grid, so it sees the same `replicas` multiplicity rows (`bootstrap_multiplicities(V, replicas, seed)`).  The grid runs
    in chunks of points whose V x V blocks fit `max_workspace_bytes`; the values do not depend on the chunking.  Returns
    `auc` (float64 [G, S], `sweep_fusion`'s: `two_u`, the block sums, are its integers), `macro_auc` [G, S] (the mean of
    the per-video AUCs over the videos with both classes), `auc_ci`, `macro_auc_ci` [G, S, 2], `videos`, `videos_scored`,
    `n_pos`, `n_neg`, `video_n_pos`, `video_n_neg`, `weights`, `lam_smooth`, `best` (first maximum of `auc` in grid order:
    {weights, lam_smooth, index, auc, macro_auc, auc_ci, macro_auc_ci, per_video_auc [V] - NaN where a class is missing
    -, pairs [V, V]}), `best_macro` (the same at the first maximum of `macro_auc`, without the block), `best_share` (the
    share of usable replicas whose own first argmax over the grid is `best`'s index), `replicas`, `replicas_dropped`,
    `seed`, `level`, `replica_auc` (float64 [usable, G * S (+ 1)]: what `bootstrap_delta` reads), `video_ms` (the
    launches between device events) and, with a published pair, `at_lam_map` (as `best`, without index) and
    `delta_best_vs_lam_map` = {mean, ci}.  The HIP passes are the only implementation: a GPU is required."""
    from . import ops
    channels = tuple(channels)
    chan = fusion_channels(records, channels)
    labels = np.concatenate([np.asarray(g)[DECIDABLE_IDX:] for g in gt])
    K, N = chan.shape
    if labels.shape[0] != N:
        raise ValueError(f"sweep_videos: {labels.shape[0]} labels for {N} scored frames")
    if not np.isfinite(chan).all():
        bad = [c for c, row in zip(channels, chan) if not np.isfinite(row).all()]
        raise ValueError(f"sweep_videos: non-finite normalised scores in {bad} (a constant record, or a NaN / inf in it)")
    pos, neg = np.flatnonzero(labels == 0), np.flatnonzero(labels != 0)
    if pos.size == 0 or neg.size == 0:
        raise ValueError("sweep_videos: the labels hold one class only: the AUC is undefined")
    if replicas < 1 or not 0.0 < level < 1.0:
        raise ValueError(f"sweep_videos: replicas >= 1 and 0 < level < 1, got {replicas} and {level}")
    vo = video_offsets(gt, 0)
    V = len(gt)
    if V > ops.VIDEO_PAIRS_MAX_VIDEOS:
        raise ValueError(f"sweep_videos: {V} videos, ops.video_pairs takes at most {ops.VIDEO_PAIRS_MAX_VIDEOS}")
    grid = fusion_grid(K)
    w = grid["weights"] if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1, K))
    lam_smooth = list(grid["lam_smooth"] if smooth is None else smooth)
    sm = smoothing_pairs(lam_smooth)
    G, S = len(w), len(sm)
    lam = LAM_MAP.get(records.get("dataset")) if K == 2 else None
    block = V * V * 8
    fit = max_workspace_bytes // block
    if fit < 1:
        raise ValueError(f"sweep_videos: max_workspace_bytes = {max_workspace_bytes} is below one grid point's block of {block} bytes")
    mult = bootstrap_multiplicities(V, replicas, seed)
    for m in mult:                                        # the precondition of ammc_bootstrap_pairs_i64, in Python integers
        if 2 * int(m @ vo["n_pos"]) * int(m @ vo["n_neg"]) >= 1 << 63:
            raise ValueError("sweep_videos: a replica's 2 P_r Q_r does not fit int64")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)
    d_chan, d_pos, d_neg = up(chan, torch.float32), up(pos, torch.int32), up(neg, torch.int32)
    d_poff, d_noff = up(vo["pos_off"], torch.int32), up(vo["neg_off"], torch.int32)
    d_w, d_sm = up(w, torch.float32), up(sm, torch.float32)
    d_mult = up(np.concatenate([mult, np.ones((1, V), dtype=np.int32)]), torch.int32)       # last row: the block sum itself
    chunks = [(g0, min(g0 + fit // S, G), 0, S) for g0 in range(0, G, fit // S)] if fit >= S else \
        [(g0, g0 + 1, s0, min(s0 + fit, S)) for g0 in range(G) for s0 in range(0, S, fit)]
    points = G * S + (1 if lam is not None else 0)
    diag, table = np.empty((points, V), dtype=np.int64), np.empty((replicas + 1, points), dtype=np.int64)

    def launch(dw, dsm):
        """(diagonals [points, V], replica table [B + 1, points], the blocks on the device, ms) of a sub-grid"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        d_c = ops.video_pairs(d_chan, d_pos, d_neg, d_poff, d_noff, dw, dsm)
        d_t = ops.bootstrap_pairs(d_c.view(-1, V, V), d_mult)
        t1.record()
        dg, tb = d_c.view(-1, V, V).diagonal(dim1=1, dim2=2).cpu().numpy(), d_t.cpu().numpy()
        return dg, tb, d_c, t0.elapsed_time(t1)
    ms = 0.0
    with torch.cuda.device(dev):
        for g0, g1, s0, s1 in chunks:
            dg, tb, _, t = launch(d_w[g0:g1], d_sm[s0:s1])
            at = (np.arange(g0, g1)[:, None] * S + np.arange(s0, s1)[None, :]).reshape(-1)
            diag[at], table[:, at] = dg, tb
            ms += t
        two_u = table[replicas, :G * S].reshape(G, S).copy()
        denom = 2.0 * float(pos.size) * float(neg.size)
        auc = two_u.astype(np.float64) / denom
        gi, si = (int(x) for x in np.unravel_index(int(np.argmax(auc)), auc.shape))
        kept = {"best": launch(d_w[gi:gi + 1], d_sm[si:si + 1])[2].cpu().numpy()[0, 0]}       # the block kept at `best`
        if lam is not None:
            w_lam, sm_lam = np.array([[1 - lam[0], lam[0]]], dtype=np.float32), smoothing_pairs([lam[1]])
            dg, tb, d_c, t = launch(up(w_lam, torch.float32), up(sm_lam, torch.float32))
            diag[G * S], table[:, G * S], kept["lam_map"] = dg[0], tb[:, 0], d_c.cpu().numpy()[0, 0]
            ms += t
    st = replica_statistics(table[:replicas], diag, mult, vo["n_pos"], vo["n_neg"], level, grid_points=G * S, best=gi * S + si)

    def point(at, wv, l2, block=None):
        out = {"weights": [float(x) for x in wv], "lam_smooth": float(l2), "auc": float(table[replicas, at] / denom),
               "macro_auc": float(st["macro_auc"][at]), "auc_ci": [float(x) for x in st["auc_ci"][at]],
               "macro_auc_ci": [float(x) for x in st["macro_auc_ci"][at]], "per_video_auc": st["per_video_auc"][at].copy()}
        if block is not None:
            out["pairs"] = block
        return out
    macro = st["macro_auc"][:G * S].reshape(G, S)
    mg, msi = (int(x) for x in np.unravel_index(int(np.argmax(macro)), macro.shape))
    out = {"two_u": two_u, "auc": auc, "macro_auc": macro, "auc_ci": st["auc_ci"][:G * S].reshape(G, S, 2),
           "macro_auc_ci": st["macro_auc_ci"][:G * S].reshape(G, S, 2), "videos": V,
           "videos_scored": int(((vo["n_pos"] > 0) & (vo["n_neg"] > 0)).sum()), "n_pos": int(pos.size), "n_neg": int(neg.size),
           "video_n_pos": vo["n_pos"], "video_n_neg": vo["n_neg"], "channels": channels, "weights": w, "lam_smooth": lam_smooth,
           "best": dict(point(gi * S + si, w[gi], lam_smooth[si], kept["best"]), index=(gi, si)),
           "best_macro": dict(point(mg * S + msi, w[mg], lam_smooth[msi]), index=(mg, msi)),
           "best_share": st["best_share"], "replicas": int(replicas), "replicas_dropped": st["replicas_dropped"], "seed": int(seed),
           "level": float(level), "replica_auc": st["auc_r"], "video_ms": float(ms)}
    if lam is not None:
        out["at_lam_map"] = point(G * S, w_lam[0], lam[1], kept["lam_map"])
        out["lam_map"] = tuple(lam)
        out["delta_best_vs_lam_map"] = bootstrap_delta(out, (gi, si), "lam_map")
    return out


# ---- pixel-level evaluation: mask-aware frame scores from the error maps ----
# A pass of its own behind the evaluation forward and `ops.error_maps` (`ops.pixel_scores`, csrc/pixel_scores.hip): nothing
# above is touched.  The pixel-level criterion (Mahadevan et al.) at the fraction num / den: a frame with ground-truth
# pixels M is a true positive at threshold t iff at least num / den of M is detected (map >= t), a frame without ground
# truth a false positive iff any pixel is.  With k = ceil(num |M| / den), "at least k of M are >= t" is "the k-th largest
# value inside M is >= t", so the criterion's ROC over all thresholds is the frame-level ROC of ONE number per frame.

def pixel_criterion_scores(m, kth, max_all):
    """(scores, labels) of the pixel-level criterion, one per frame: `kth` and label 1 where the frame has ground-truth
    pixels (m > 0), `max_all` and label 0 elsewhere.  numpy arrays; `roc_auc(labels, scores, pos_label=1)` is the area
    under the criterion's ROC."""
    m = np.asarray(m)
    pos = m > 0
    scores = np.where(pos, np.asarray(kth, dtype=np.float64), np.asarray(max_all, dtype=np.float64))
    return scores, pos.astype(np.int8)


def resize_mask(mask: torch.Tensor, size) -> torch.Tensor:
    """Nearest-neighbour resize of a mask [..., h0, w0] to size = (H, W), any dtype, on the mask's device.  The rule,
    in integers: target pixel (y, x) takes source pixel (floor((y + 0.5) * h0 / H), floor((x + 0.5) * w0 / W)) =
    (((2 y + 1) * h0) // (2 H), ((2 x + 1) * w0) // (2 W)) - the pixel under the target pixel's centre.  Plain indexing:
    a value of the result is a value of the source."""
    if mask.dim() < 2:
        raise ValueError("resize_mask: a mask [..., h0, w0]")
    H, W = (int(v) for v in size)
    h0, w0 = mask.shape[-2:]
    if min(H, W, h0, w0) < 1:
        raise ValueError(f"resize_mask: empty size {(h0, w0)} -> {(H, W)}")
    ys = ((2 * torch.arange(H, device=mask.device) + 1) * h0) // (2 * H)
    xs = ((2 * torch.arange(W, device=mask.device) + 1) * w0) // (2 * W)
    return mask.index_select(-2, ys).index_select(-1, xs)


def pool_mask(mask: torch.Tensor, patch: int) -> torch.Tensor:
    """uint8 [..., ceil(H / patch), ceil(W / patch)] from a mask [..., H, W]: 1 where ANY pixel of the patch is nonzero,
    over `ops.error_maps`' patch grid - patch x patch pixels anchored at (0, 0), the last row / column ragged."""
    if mask.dim() < 2 or patch < 1:
        raise ValueError("pool_mask: a mask [..., H, W] and a patch size >= 1")
    lead, (h, w) = mask.shape[:-2], mask.shape[-2:]
    any_px = (mask != 0).to(torch.float32).reshape(-1, 1, h, w)
    pooled = torch.nn.functional.max_pool2d(any_px, kernel_size=patch, stride=patch, ceil_mode=True)
    return pooled.to(torch.uint8).reshape(*lead, *pooled.shape[-2:])


_PIXEL_KEYS = ("m", "kth", "max_in", "max_out")


def _checked_mask(who: str, mask: torch.Tensor, t: int, h: int, w: int, dev) -> torch.Tensor:
    """the ground truth of a mask-aware pass: uint8 (a bool is viewed as uint8: the same memory) [t, h, w] on `dev`,
    returned contiguous"""
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (t, h, w) or mask.device != dev:
        raise ValueError(f"{who}: mask must be uint8 {(t, h, w)} on {dev}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
    return mask.contiguous()


def _frame_mask(who: str, masks, v: int, rgb: torch.Tensor) -> Optional[torch.Tensor]:
    """masks[v] (a uint8 / bool / numeric [T, h0, w0] array or tensor, or None) on rgb's device at its frame size"""
    t, (h, w) = int(rgb.shape[0]), rgb.shape[2:]
    if v >= len(masks):
        raise ValueError(f"{who}: {len(masks)} masks for more than {v} sub-videos (None marks one without)")
    mk = masks[v]
    if mk is None:
        return None
    mk = torch.as_tensor(np.asarray(mk) if not isinstance(mk, torch.Tensor) else mk)
    if mk.dim() != 3 or mk.shape[0] != t:
        raise ValueError(f"{who}: mask {v} is {tuple(mk.shape)}, its sub-video has {t} frames")
    if mk.dtype not in (torch.uint8, torch.bool):
        mk = mk != 0
    mk = mk.to(rgb.device)
    return resize_mask(mk.view(torch.uint8) if mk.dtype == torch.bool else mk, (h, w)).contiguous()


def _masked_subvideos(who: str, model, videos, masks, out: dict, score: Callable, keep_maps: bool, device=None):
    """`_scored_subvideos` for the mask-aware loops: `score(v, rgb, op, mask)` receives `_frame_mask` of masks[v] (None
    for a sub-video without one), `out["mask_videos"]` grows by the sub-videos that have one; yields (v, rec, whether v
    has a mask, and under `keep_maps` its resized mask on the host - else None)"""
    held = {}

    def scored(v, rgb, op):
        held["mask"] = _frame_mask(who, masks, v, rgb)
        return score(v, rgb, op, held["mask"])

    for v, _, _, rec in _scored_subvideos(model, videos, out, scored, device):
        has = held["mask"] is not None
        if has:
            out["mask_videos"].append(v)
        yield v, rec, has, held["mask"].cpu().numpy() if has and keep_maps else None


def _evaluate_masked(who: str, model, videos, masks, dataset_name: str, keys, subvideo: Callable, keep_maps: bool, device) -> dict:
    """the loop `evaluate_dataset_pixel` and `evaluate_dataset_region` share: `subvideo(v, rgb, op, mask, keep_maps)` scores
    one sub-video - one without a mask against a zero mask, for its frame records - and the arrays it returns by `keys`
    (`mask`: the resized mask) become lists over the sub-videos, None at one without a mask"""
    out = _new_records(dataset_name, "n_frames", "mask_videos", *keys)

    def score(v, rgb, op, dm):
        if dm is None:
            return subvideo(v, rgb, op, torch.zeros((rgb.shape[0],) + tuple(rgb.shape[2:]), device=rgb.device, dtype=torch.uint8), False)
        return subvideo(v, rgb, op, dm, keep_maps)

    for v, rec, has, host_mask in _masked_subvideos(who, model, videos, masks, out, score, keep_maps, device):
        for k in keys:
            out[k].append((host_mask if k == "mask" else rec[k]) if has else None)
    return out


def pixel_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, mask: torch.Tensor, patch: int = 16,
                   frac=(2, 5), batch: int = EVAL_BATCH, keep_maps: bool = False) -> Dict[str, np.ndarray]:
    """Is the error where the anomaly is: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W] and mask uint8 (or bool) [T,H,W]
    (nonzero = anomalous, already at the frame size), contiguous and on the model's device -> per-frame numpy arrays of
    the sub-video.  Behind every forward `ops.error_maps(rgb_pred, rgb_target, patch, pixel=True)` writes into one
    per-batch buffer that every batch reuses, and `ops.pixel_scores` runs on its pixel map with the frames' masks and on
    its patch means with `pool_mask(mask, patch)`: frame t's prediction meets mask[t].  Returned: `pix_m` (int32),
    `pix_kth`, `pix_max_in`, `pix_max_out`, the same four with the prefix `patch_`, `rgb_psnr` (the fixed-order one of
    `ops.error_maps`), `rgb_comm`, and for the record lists of the reference `op_psnr` (the output layer's epilogue) and
    `op_comm`.  Only the rgb stream's maps are scored.  Clips, targets, batches, `defer_guard` and the `exact` re-run of
    a flagged batch are `localise_subvideo`'s; frame indexing and fills are `assemble_records`' (`assemble_localised`):
    the first RGB_LEN_CLIP - 1 frames repeat frame RGB_LEN_CLIP - 1's numbers.  The per-frame results lie in one flat
    device buffer: one device-to-host copy per sub-video, and the frame-sized maps never leave the device - unless
    `keep_maps`, a testing hook in the spirit of `predictions=`, asks for `pixel_map` [T,H,W] and `patch_map` [T,ph,pw]
    as they were scored."""
    from . import ops
    batches = _checked_batches("pixel_subvideo", rgb_frames, op_frames, batch)
    t, (h, w) = rgb_frames.shape[0], rgb_frames.shape[2:]
    dev = rgb_frames.device
    mask = _checked_mask("pixel_subvideo", mask, t, h, w, dev)
    pooled = pool_mask(mask, patch)
    ph, pw = pooled.shape[1:]
    sections = [(f"rgb_{g}_{key}", ()) for g in ("pix", "patch") for key in _PIXEL_KEYS] + [("rgb_psnr", ()), ("op_psnr", ())]
    if keep_maps:
        sections += [("rgb_pixel_map", (h, w)), ("rgb_patch_map", (ph, pw))]
    bmax = max(e - s for s, e in batches)
    buf = {"patch_sum": torch.empty((bmax, ph, pw), device=dev), "patch_mean": torch.empty((bmax, ph, pw), device=dev),
           "pixel": torch.empty((bmax, h, w), device=dev), "frame_sq": torch.empty(bmax, device=dev),
           "worst": torch.empty(bmax, device=dev), "worst_idx": torch.empty(bmax, device=dev, dtype=torch.int32)}

    def on_batch(slots, s, e, k, fwd):
        em = ops.error_maps(fwd.rgb_pred, fwd.targets[0], patch, True, {key: v[:e - s] for key, v in buf.items()})
        slots.view("rgb_psnr")[s:e] = em["psnr"]
        slots.view("op_psnr")[s:e] = fwd.fused[1]
        f0, f1 = s + RGB_LEN_CLIP - 1, e + RGB_LEN_CLIP - 1              # the frames these clips predict
        for g, mp, mk in (("pix", em["pixel"], mask[f0:f1]), ("patch", em["patch_mean"], pooled[f0:f1])):
            ops.pixel_scores(mp, mk, frac, {key: slots.view(f"rgb_{g}_{key}")[s:e] for key in _PIXEL_KEYS})
        if keep_maps:
            slots.view("rgb_pixel_map")[s:e] = em["pixel"]
            slots.view("rgb_patch_map")[s:e] = em["patch_mean"]

    rec = _run_pass(model, rgb_frames, op_frames, batches, sections, ("rgb_pix_m", "rgb_patch_m"), on_batch)
    # (the rgb_ prefix chose the rgb stream's clip length in `assemble_localised`; the pixel figures carry none)
    return {(k[4:] if k[4:].startswith(("pix", "patch_")) else k): v for k, v in rec.items()}


def evaluate_dataset_pixel(model, videos, masks, dataset_name: str = "synthetic", patch: int = 16, frac=(2, 5), device=None,
                           keep_maps: bool = False) -> dict:
    """`evaluate_dataset` with `pixel_subvideo` in place of the scoring loop (one rank).  `videos`: as
    `evaluate_dataset_localised` takes them.  `masks[v]`: the pixel ground truth of sub-video v, a uint8 / bool
    [T, h0, w0] array or tensor at any resolution (uploaded and brought to the frame size with `resize_mask`, one
    sub-video at a time), or None: such a sub-video is evaluated for the frame records and left out of every pixel
    figure (the reference's `pixel_video_ids` subset).  A mask whose T differs from its video's raises ValueError.
    Returns the four record lists of the reference (`rgb_img_pred_records` from the fixed-order PSNR), `n_frames`,
    `mask_videos` (the indices of the sub-videos that have a mask) and per sub-video the per-frame arrays of
    `pixel_subvideo` as lists by their names (`pix_m`, ..., `patch_max_out`; with `keep_maps` `pixel_map`, `patch_map`
    and the resized `mask`), None at a sub-video without a mask."""
    keys = [f"{g}_{key}" for g in ("pix", "patch") for key in _PIXEL_KEYS] + (["pixel_map", "patch_map", "mask"] if keep_maps else [])
    return _evaluate_masked("evaluate_dataset_pixel", model, videos, masks, dataset_name, keys,
                            lambda v, rgb, op, dm, keep: pixel_subvideo(model, rgb, op, dm, patch, frac, keep_maps=keep), keep_maps, device)


def pixel_level_auc(rec: dict, normalise: str = "none") -> dict:
    """The pixel-level figures of `evaluate_dataset_pixel`'s result over its `mask_videos`, the first DECIDABLE_IDX
    frames of each dropped, anomalous (a frame with ground-truth pixels) the positive class:
      `auc_pixel`        the area under the pixel-level criterion's ROC on the pixel map: `roc_auc` of
                         `pixel_criterion_scores` (exactly the criterion evaluated at every threshold)
      `auc_pixel_patch`  the same on the patch map with the pooled masks
      `auc_frame_max`    every frame scored by the largest value of its pixel map, wherever it lies
      `pointing`         the share of anomalous frames whose largest value lies inside the mask (max_in >= max_out)
      `n_anomalous`, `n_normal`
    `normalise`: "none", or "video" - a sub-video's scores divided by its largest `max_all` (per map).  Selecting the
    k-th largest commutes with a positive scale, so this is exactly the criterion on maps normalised per sub-video.
    With an empty class the AUCs are None and `note` says why.  Non-finite scores raise ValueError: the kernel orders
    bit patterns and leaves NaN to its caller."""
    if normalise not in ("none", "video"):
        raise ValueError(f"pixel_level_auc: normalise must be 'none' or 'video', got {normalise!r}")
    cols = {"pix": ([], []), "patch": ([], []), "frame": ([], [])}
    hits = []
    for v in rec["mask_videos"]:
        for g in ("pix", "patch"):
            m = np.asarray(rec[f"{g}_m"][v])[DECIDABLE_IDX:]
            kth, max_in, max_out = (np.asarray(rec[f"{g}_{key}"][v], dtype=np.float64)[DECIDABLE_IDX:]
                                    for key in ("kth", "max_in", "max_out"))
            max_all = np.maximum(max_in, max_out)
            if g == "pix":
                hits.append((max_in >= max_out)[m > 0])
            if normalise == "video" and max_all.size and max_all.max() > 0:
                c = max_all.max()
                kth, max_all = kth / c, max_all / c
            scores, labels = pixel_criterion_scores(m, kth, max_all)
            cols[g][0].append(scores)
            cols[g][1].append(labels)
            if g == "pix":
                cols["frame"][0].append(max_all)
                cols["frame"][1].append(labels)
    out = {"normalise": normalise}
    cat = {g: (np.concatenate(s) if s else np.zeros(0), np.concatenate(lab) if lab else np.zeros(0, np.int8))
           for g, (s, lab) in cols.items()}
    labels = cat["pix"][1]
    n_pos, n_neg = int((labels == 1).sum()), int((labels == 0).sum())
    out["n_anomalous"], out["n_normal"] = n_pos, n_neg
    for g, (scores, _) in cat.items():
        if not np.isfinite(scores).all():
            raise ValueError(f"pixel_level_auc: non-finite {g} scores (a NaN or an infinity in an error map)")
    names = {"pix": "auc_pixel", "patch": "auc_pixel_patch", "frame": "auc_frame_max"}
    if n_pos == 0 or n_neg == 0:
        out.update({name: None for name in names.values()})
        out["note"] = f"no {'anomalous' if n_pos == 0 else 'normal'} frame among the scored ones: the ROC has no area"
    else:
        for g, name in names.items():
            out[name] = roc_auc(cat[g][1], cat[g][0], pos_label=1)
    out["pointing"] = float(np.concatenate(hits).mean()) if n_pos else None
    return out


# ---- region-based evaluation: detected regions against ground-truth regions -----------------
# A pass of its own behind the evaluation forward and `ops.error_maps` (`ops.label_regions`, `ops.region_scores`,
# csrc/region_scores.hip): nothing above is touched.  The region-based detection criterion (RBDC, Ramachandra and Jones):
# at threshold t the detected regions are the connected components of {map >= t}; a ground-truth region is detected when
# some detected region meets it with IoU >= num / den, and every detected region that matches no ground-truth region is
# a false positive.  The track-based criterion (TBDC) counts a track as detected when at least alpha of its regions are.

REGION_MAX_REGIONS = 32
REGION_FRAME_CHUNK = 16      # frames per `ops.region_scores` call of `region_subvideo`
REGION_TRACK_NOTE = ("tracks are derived, not annotated: ground-truth regions of consecutive frames that share a pixel "
                     "belong to one track (transitive closure)")
_REGION_KEYS = ("n_px", "n_comp", "n_fp", "hit")


def region_thresholds(T: int = 64, spacing: str = "linear", floor: float = 1e-3) -> np.ndarray:
    """T threshold values in (0, 1], increasing, fp32: "linear" i / T, "log" floor ** ((T - i) / T), i = 1..T - computed
    in float64 and rounded to fp32 once.  A sub-video's thresholds are these values times its largest map value
    (`normalise="video"`) or times `t_max` ("none")."""
    if not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError(f"region_thresholds: T must be an integer >= 1, got {T!r}")
    i = np.arange(1, T + 1, dtype=np.float64)
    if spacing == "linear":
        v = i / float(T)
    elif spacing == "log":
        if not 0.0 < floor < 1.0:
            raise ValueError(f"region_thresholds: the log floor must lie in (0, 1), got {floor!r}")
        v = np.float64(floor) ** ((float(T) - i) / float(T))
    else:
        raise ValueError(f"region_thresholds: spacing must be 'linear' or 'log', got {spacing!r}")
    return v.astype(np.float32)


def region_tracks(labels_per_frame):
    """Track ids from the overlap of consecutive label images.  `labels_per_frame`: [T, h, w] integers (or a sequence of
    [h, w] images), 0 = background, r = region r of that frame (1..the frame's largest label).  Regions of frames f and
    f + 1 belong to one track iff they share a pixel; tracks are the transitive closure, numbered from 0 in order of
    their first region (frame, then label).  -> (tracks, n_tracks): tracks[f] an int array with the track id of region r
    at [r - 1].  A frame without regions ends every track."""
    frames = [np.asarray(f) for f in labels_per_frame]
    counts = [int(f.max()) if f.size else 0 for f in frames]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parent = list(range(int(start[-1])))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for f in range(len(frames) - 1):
        a, b = frames[f], frames[f + 1]
        both = (a > 0) & (b > 0)
        if both.any():
            for ra, rb in sorted(set(zip(a[both].tolist(), b[both].tolist()))):
                x, y = find(int(start[f]) + ra - 1), find(int(start[f + 1]) + rb - 1)
                if x != y:
                    parent[max(x, y)] = min(x, y)
    ids, out = {}, []
    for f, c in enumerate(counts):
        row = np.empty(c, dtype=np.int64)
        for r in range(c):
            row[r] = ids.setdefault(find(int(start[f]) + r), len(ids))
        out.append(row)
    return out, len(ids)


def region_curve_area(fpr, rate) -> float:
    """The area under a detection-rate curve that need not be monotone: the points (fpr, rate) of all thresholds; where
    several share an fpr the largest rate stays; (0, r0) is added with r0 the largest rate at fpr 0 (0 if there is no
    such point); sorted by fpr; a curve that ends below fpr 1 is extended flat to 1, one that passes 1 is cut there by
    linear interpolation; the trapezoid area over [0, 1]."""
    best = {0.0: 0.0}
    for x, y in zip(np.asarray(fpr, dtype=np.float64).tolist(), np.asarray(rate, dtype=np.float64).tolist()):
        if not (x >= 0.0 and y >= 0.0):
            raise ValueError(f"region_curve_area: a point ({x}, {y}) outside the quadrant")
        best[x] = max(best.get(x, 0.0), y)
    xs = sorted(best)
    pts = [(x, best[x]) for x in xs if x <= 1.0]
    if xs[-1] > 1.0:
        x1 = next(x for x in xs if x > 1.0)
        (x0, y0), y1 = pts[-1], best[x1]
        if x0 < 1.0:
            pts.append((1.0, y0 + (y1 - y0) * (1.0 - x0) / (x1 - x0)))
    elif pts[-1][0] < 1.0:
        pts.append((1.0, pts[-1][1]))
    return float(sum((b[0] - a[0]) * (a[1] + b[1]) / 2.0 for a, b in zip(pts, pts[1:])))


def _frames_of(a: np.ndarray) -> np.ndarray:
    """clip rows -> frame rows of the rgb stream, with `assemble_localised`'s head fill"""
    return np.concatenate([np.repeat(a[:1], RGB_LEN_CLIP - 1, axis=0), a])


# The region tail `region_subvideo` and `fused_subvideo` share, over `_Slots` sections: per map g ("pix", "patch") the
# ground truth - `{g}_gt_count` [n_clip], `{g}_labels` [n_clip, h_g, w_g] - and per scored map `{p}{g}` (p: "" or a
# setting's prefix) the four figures [n_clip, K] and `{p}{g}_thresholds` [K] as used.

def _region_sections(grids: dict, n_clip: int, K: int, prefixes=("",)) -> list:
    """`grids`: {g: (h_g, w_g)}"""
    sections = []
    for p in prefixes:
        for g in grids:
            sections += [(f"{p}{g}_{key}", (n_clip, K), torch.int32) for key in _REGION_KEYS]
            sections.append((f"{p}{g}_thresholds", (K,), torch.float32))
    for g, grid in grids.items():
        sections += [(f"{g}_gt_count", (n_clip,), torch.int32), (f"{g}_labels", (n_clip,) + tuple(grid), torch.uint8)]
    return sections


def _label_truth(slots: _Slots, g: str, mask: torch.Tensor, chunk: int, min_gt_area: int, connectivity: int) -> None:
    """`ops.label_regions` of the clips' masks [n_clip, h_g, w_g], `chunk` frames at a time"""
    from . import ops
    for s in range(0, mask.shape[0], chunk):
        ops.label_regions(mask[s:s + chunk], min_gt_area, connectivity,
                          {"labels": slots.view(f"{g}_labels")[s:s + chunk], "count": slots.view(f"{g}_gt_count")[s:s + chunk]})


def _score_regions(slots: _Slots, p: str, g: str, mp: torch.Tensor, values: torch.Tensor, t_max, chunk: int, iou, min_area: int,
                   connectivity: int) -> None:
    """the thresholds `values` times the largest value of the map `mp` [n_clip, h_g, w_g] (one fp32 multiply on the
    device) or times `t_max` where given, then `ops.region_scores` against g's label images, `chunk` frames at a time"""
    from . import ops
    used = slots.view(f"{p}{g}_thresholds")
    used.copy_(values * (mp.max() if t_max is None else torch.tensor(float(t_max), device=mp.device, dtype=torch.float32)))
    for s in range(0, mp.shape[0], chunk):
        ops.region_scores(mp[s:s + chunk], slots.view(f"{g}_labels")[s:s + chunk], used, iou, min_area, connectivity,
                          {key: slots.view(f"{p}{g}_{key}")[s:s + chunk] for key in _REGION_KEYS})


def _check_regions(who: str, slots: _Slots, host: np.ndarray, prefixes, groups, video: str) -> None:
    """the counts, once they are on the host: a labelling that hit its round bound (RuntimeError), a frame with more
    ground-truth regions than are scored (ValueError)"""
    for g in groups:
        count = slots.view(f"{g}_gt_count", host)
        if (count < 0).any() or any((slots.view(f"{p}{g}_n_comp", host) < 0).any() for p in prefixes):
            raise RuntimeError(f"{who}: the labelling of sub-video {video!r} hit its round bound ({g} map)")
        if (count > REGION_MAX_REGIONS).any():
            f = int(np.argmax(count > REGION_MAX_REGIONS))
            raise ValueError(f"sub-video {video!r}, frame {f + RGB_LEN_CLIP - 1}: {int(count[f])} ground-truth regions on the "
                             f"{'frame' if g == 'pix' else 'patch grid'}, at most {REGION_MAX_REGIONS} are scored: drop "
                             f"the specks with --min_gt_area")


def _region_arrays(slots: _Slots, host: np.ndarray, p: str, g: str) -> Dict[str, np.ndarray]:
    """the per-frame arrays of one scored map, by `region_subvideo`'s names"""
    one = {f"{g}_{key}": _frames_of(slots.view(f"{p}{g}_{key}", host)) for key in _REGION_KEYS}
    one[f"{g}_gt_count"] = _frames_of(slots.view(f"{g}_gt_count", host))
    one[f"{g}_labels"] = _frames_of(slots.view(f"{g}_labels", host))
    one[f"{g}_thresholds"] = slots.view(f"{p}{g}_thresholds", host).copy()
    return one


def region_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, mask: torch.Tensor, thresholds, patch: int = 16,
                    iou=(1, 10), min_area: int = 1, connectivity: int = 8, normalise: str = "video", t_max=None,
                    keep_maps: bool = False, min_gt_area: int = 1, batch: int = EVAL_BATCH,
                    video: str = "") -> Dict[str, np.ndarray]:
    """Are the detected regions the anomalous ones: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W] and mask uint8 (or bool)
    [T,H,W] (nonzero = anomalous, at the frame size), contiguous and on the model's device, `thresholds` the fp32 [K]
    values of `region_thresholds` -> per-frame numpy arrays of the sub-video.  Behind every forward
    `ops.error_maps(rgb_pred, rgb_target, patch, pixel=True)` writes the batch's pixel map and patch means straight into
    two per-sub-video device buffers.  After the last batch `ops.label_regions` numbers the ground-truth regions of
    `mask` and of `pool_mask(mask, patch)` (`min_gt_area`), the thresholds become the values times the buffers' largest
    value (`normalise="video"`: one fp32 multiply on the device, per map) or times `t_max` ("none"), and
    `ops.region_scores` runs over the stored maps, REGION_FRAME_CHUNK frames at a time: frame t's prediction meets
    mask[t].  Returned: `pix_n_px`, `pix_n_comp`, `pix_n_fp`, `pix_hit` (int32 [T, K]), `pix_gt_count` (int32 [T]),
    `pix_labels` (uint8 [T,H,W]: the label images, which the tracks are derived from), `pix_thresholds` (fp32 [K], as
    used), the same with the prefix `patch_`, and `rgb_psnr`, `rgb_comm`, `op_psnr`, `op_comm` as `pixel_subvideo` gives
    them.  The first RGB_LEN_CLIP - 1 frames repeat frame RGB_LEN_CLIP - 1's numbers.  The region figures come to the
    host in one copy per sub-video behind the driver's own; the maps leave the device only under `keep_maps`
    (`pixel_map`, `patch_map`).  A frame with more than 32 ground-truth regions raises ValueError."""
    from . import ops
    if normalise not in ("video", "none"):
        raise ValueError(f"region_subvideo: normalise must be 'video' or 'none', got {normalise!r}")
    if normalise == "none" and (t_max is None or not np.isfinite(t_max) or t_max <= 0):
        raise ValueError(f"region_subvideo: normalise='none' needs a finite t_max > 0, got {t_max!r}")
    batches = _checked_batches("region_subvideo", rgb_frames, op_frames, batch)
    t, (h, w) = rgb_frames.shape[0], rgb_frames.shape[2:]
    dev, lc, n_clip = rgb_frames.device, RGB_LEN_CLIP, batches[-1][1]
    mask = _checked_mask("region_subvideo", mask, t, h, w, dev)
    values = torch.as_tensor(np.asarray(thresholds, dtype=np.float32).reshape(-1)).to(dev)
    K = int(values.numel())
    if K < 1:
        raise ValueError("region_subvideo: no thresholds")
    masks = {"pix": mask[lc - 1:], "patch": pool_mask(mask, patch).contiguous()[lc - 1:]}
    ph, pw = masks["patch"].shape[1:]
    maps = {"pix": torch.empty((n_clip, h, w), device=dev), "patch": torch.empty((n_clip, ph, pw), device=dev)}
    bmax = max(e - s for s, e in batches)
    buf = {"patch_sum": torch.empty((bmax, ph, pw), device=dev), "frame_sq": torch.empty(bmax, device=dev),
           "worst": torch.empty(bmax, device=dev), "worst_idx": torch.empty(bmax, device=dev, dtype=torch.int32)}

    def on_batch(slots, s, e, k, fwd):
        out = {key: v[:e - s] for key, v in buf.items()}
        out.update(pixel=maps["pix"][s:e], patch_mean=maps["patch"][s:e])
        em = ops.error_maps(fwd.rgb_pred, fwd.targets[0], patch, True, out)
        slots.view("rgb_psnr")[s:e] = em["psnr"]
        slots.view("op_psnr")[s:e] = fwd.fused[1]

    rec = _run_pass(model, rgb_frames, op_frames, batches, [("rgb_psnr", ()), ("op_psnr", ())], (), on_batch)
    with torch.no_grad():
        res = _Slots(_region_sections({"pix": (h, w), "patch": (ph, pw)}, n_clip, K), dev)
        for g in maps:
            _label_truth(res, g, masks[g], REGION_FRAME_CHUNK, min_gt_area, connectivity)
            _score_regions(res, "", g, maps[g], values, None if normalise == "video" else t_max, REGION_FRAME_CHUNK, iou, min_area,
                           connectivity)
        host = res.flat.cpu().numpy()                    # the region figures' one copy
    _check_regions("region_subvideo", res, host, ("",), maps, video)
    for g in maps:
        rec.update(_region_arrays(res, host, "", g))
    if keep_maps:
        rec["pixel_map"], rec["patch_map"] = _frames_of(maps["pix"].cpu().numpy()), _frames_of(maps["patch"].cpu().numpy())
    return rec


_REGION_REC_KEYS = tuple(f"{g}_{key}" for g in ("pix", "patch") for key in _REGION_KEYS + ("gt_count", "labels", "thresholds"))


def evaluate_dataset_region(model, videos, masks, dataset_name: str = "synthetic", patch: int = 16, thresholds=None,
                            iou=(1, 10), min_area: int = 1, connectivity: int = 8, normalise: str = "video", t_max=None,
                            min_gt_area: int = 1, device=None, keep_maps: bool = False) -> dict:
    """`evaluate_dataset` with `region_subvideo` in place of the scoring loop (one rank).  `videos` and `masks` as
    `evaluate_dataset_pixel` takes them: masks[v] a uint8 / bool [T, h0, w0] array or tensor at any resolution (brought to
    the frame size with `resize_mask`), or None - such a sub-video is evaluated for the frame records only and left out
    of every region figure.  `thresholds`: fp32 values in (0, 1] (default `region_thresholds(64)`).  Returns the four
    record lists of the reference, `n_frames`, `mask_videos` and per sub-video the arrays of `region_subvideo` as lists
    by their names (with `keep_maps` also `pixel_map`, `patch_map` and the resized `mask`), None at a sub-video without
    a mask."""
    values = region_thresholds(64) if thresholds is None else np.asarray(thresholds, dtype=np.float32)
    keys = list(_REGION_REC_KEYS) + (["pixel_map", "patch_map", "mask"] if keep_maps else [])
    return _evaluate_masked("evaluate_dataset_region", model, videos, masks, dataset_name, keys,
                            lambda v, rgb, op, dm, keep: region_subvideo(model, rgb, op, dm, values, patch, iou, min_area, connectivity,
                                                                         normalise, t_max, keep, min_gt_area, video=str(v)),
                            keep_maps, device)


def region_level_auc(rec: dict, alpha=(1, 10)) -> dict:
    """The region- and track-based figures of `evaluate_dataset_region`'s result over its `mask_videos`, the first
    DECIDABLE_IDX frames of each dropped.  Per threshold index: RBDR = detected ground-truth regions / all of them, FPR =
    false-positive regions / frames, TBDR = tracks with at least alpha = (num, den) of their regions detected / all
    tracks (`region_tracks` over each sub-video's kept frames).  `rbdc`, `tbdc`: `region_curve_area` of (FPR, RBDR) and
    (FPR, TBDR) on the pixel map; `rbdc_patch`, `tbdc_patch` on the patch map; `curves`: the arrays `fpr`, `rbdr`, `tbdr`
    and their `_patch` forms; `n_gt_regions`, `n_tracks` (and `_patch`), `n_frames`, `track_note`.  Without a
    ground-truth region the areas are None and `note` says why."""
    a_num, a_den = (int(v) for v in alpha)
    if not 1 <= a_num <= a_den:
        raise ValueError(f"region_level_auc: alpha = (num, den) with 1 <= num <= den, got {alpha!r}")
    out = {"track_note": REGION_TRACK_NOTE, "curves": {}}
    d = DECIDABLE_IDX
    for g, suffix in (("pix", ""), ("patch", "_patch")):
        n_frames = n_gt = n_tracks = 0
        fp = det = trk = None
        for v in rec["mask_videos"]:
            n_comp, n_fp, hit = (np.asarray(rec[f"{g}_{key}"][v])[d:].astype(np.int64) for key in ("n_comp", "n_fp", "hit"))
            count = np.asarray(rec[f"{g}_gt_count"][v])[d:].astype(np.int64)
            if (n_comp < 0).any():
                raise ValueError(f"region_level_auc: sub-video {v} carries a failed labelling (n_comp = -1)")
            if (count > REGION_MAX_REGIONS).any():
                raise ValueError(f"region_level_auc: sub-video {v} has a frame with more than {REGION_MAX_REGIONS} regions")
            K = n_fp.shape[1]
            if fp is None:
                fp, det, trk = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
            n_frames += n_fp.shape[0]
            fp += n_fp.sum(axis=0)
            tracks, nt = region_tracks(np.asarray(rec[f"{g}_labels"][v])[d:])
            hits = np.zeros((nt, K), np.int64)
            size = np.zeros(nt, np.int64)
            for f in range(count.shape[0]):
                for r in range(int(count[f])):
                    bit = (hit[f] >> r) & 1
                    det += bit
                    hits[tracks[f][r]] += bit
                    size[tracks[f][r]] += 1
            n_gt += int(count.sum())
            n_tracks += nt
            trk += (hits * a_den >= a_num * size[:, None]).sum(axis=0)
        out["n_frames"] = n_frames
        out["n_gt_regions" + suffix], out["n_tracks" + suffix] = n_gt, n_tracks
        if n_gt == 0 or n_frames == 0:
            out["rbdc" + suffix] = out["tbdc" + suffix] = None
            out["note"] = "no ground-truth region among the scored frames: the curves have no rate"
            continue
        fpr, rbdr, tbdr = fp / float(n_frames), det / float(n_gt), trk / float(n_tracks)
        out["curves"].update({"fpr" + suffix: fpr, "rbdr" + suffix: rbdr, "tbdr" + suffix: tbdr})
        out["rbdc" + suffix], out["tbdc" + suffix] = region_curve_area(fpr, rbdr), region_curve_area(fpr, tbdr)
    return out


# ---- fused localisation maps: flow error and memory commit beside the rgb error --------------
# A pass of its own behind the evaluation forward (`ops.fuse_maps`, csrc/fuse_maps.hip): the rgb and flow error maps and
# the two memory blocks' commit maps are kept on the device for a sub-video, then weighted, summed, smoothed by a box
# window and scored by the pixel-level and region-based criteria above, once per weight vector.  Nothing above is touched.

FUSE_CHANNELS = ("rgb_err", "op_err", "rgb_commit", "op_commit")
FUSE_CELLS = (1, 1, 8, 8)    # frame pixels per value: the error maps are per pixel, the commit maps on the H/8 x W/8 bottleneck grid
FUSE_MAX_SETTINGS = 8
FUSE_FRAME_CHUNK = 16        # frames per `ops.fuse_maps` call of `fused_subvideo`
FUSE_BUFFER_BUDGET = 4 << 30   # bytes of per-sub-video device buffers `fused_subvideo` accepts


def _fuse_frame_size(sources, cells):
    ref = next((c for c, cell in enumerate(cells) if cell == 1), None)
    if ref is not None:
        return tuple(int(v) for v in sources[ref].shape[1:])
    return int(sources[0].shape[1]) * cells[0], int(sources[0].shape[2]) * cells[0]


def fuse_maps_reference(sources, cells, coef, radius: int, patch: int) -> Dict[str, torch.Tensor]:
    """the quantities of `ops.fuse_maps` in float64 with plain torch (any device; the reference of the tests).  `sources`:
    [B, gh_c, gw_c] tensors, `cells` their cell sizes, `coef` [n_ch].  Source c is expanded blockily - frame pixel (y, x)
    reads cell (min(y // cell, gh - 1), min(x // cell, gw - 1)) - `raw` is the coefficient-weighted sum, `pixel` its mean
    over the in-frame part of the (2 radius + 1)^2 window, `patch_mean` the mean of `pixel` over each patch's true pixel
    count, `frame_max` the largest `pixel` of a sample.  The frame size is that of the first source with cell 1 (else
    grid * cell of source 0)."""
    cells = [int(c) for c in cells]
    h, w = _fuse_frame_size(sources, cells)
    dev = sources[0].device
    cf = torch.as_tensor(coef, dtype=torch.float64, device=dev) if not isinstance(coef, torch.Tensor) else coef.to(dev, torch.float64)
    raw = None
    for c, (s, cell) in enumerate(zip(sources, cells)):
        ys = torch.clamp(torch.arange(h, device=dev) // cell, max=s.shape[1] - 1)
        xs = torch.clamp(torch.arange(w, device=dev) // cell, max=s.shape[2] - 1)
        term = cf[c] * s.to(torch.float64).index_select(1, ys).index_select(2, xs)
        raw = term if raw is None else raw + term
    ones = torch.ones((1, 1, h, w), dtype=torch.float64, device=dev)
    r = int(radius)
    padded = torch.nn.functional.pad(raw, (r, r, 0, 0))                      # sums of shifted slices: additions only
    rows = sum(padded[:, :, d:d + w] for d in range(2 * r + 1))
    padded = torch.nn.functional.pad(rows, (0, 0, r, r))
    box = sum(padded[:, d:d + h, :] for d in range(2 * r + 1))
    ys, xs = torch.arange(h, device=dev), torch.arange(w, device=dev)
    ny = torch.clamp(ys + r, max=h - 1) - torch.clamp(ys - r, min=0) + 1
    nx = torch.clamp(xs + r, max=w - 1) - torch.clamp(xs - r, min=0) + 1
    pixel = box / (ny[:, None] * nx[None, :]).to(torch.float64)
    ph, pw = -(-h // patch), -(-w // patch)
    pad = (0, pw * patch - w, 0, ph * patch - h)
    sums = torch.nn.functional.pad(pixel, pad).reshape(-1, ph, patch, pw, patch).sum(dim=(2, 4))
    count = torch.nn.functional.pad(ones[0], pad).reshape(1, ph, patch, pw, patch).sum(dim=(2, 4))
    return {"raw": raw, "pixel": pixel, "patch_mean": sums / count, "frame_max": pixel.amax(dim=(1, 2))}


def check_fusion_weights(weights) -> List[List[float]]:
    """`weights` as a list of 1..FUSE_MAX_SETTINGS settings of one length n_ch in 1..4, each value finite and >= 0 and not
    all 0 (ValueError otherwise)"""
    try:
        rows = [[float(v) for v in r] for r in weights]
    except (TypeError, ValueError):
        raise ValueError(f"fusion weights: a list of weight vectors, got {weights!r}") from None
    if not 1 <= len(rows) <= FUSE_MAX_SETTINGS:
        raise ValueError(f"fusion weights: 1..{FUSE_MAX_SETTINGS} settings, got {len(rows)}")
    n_ch = len(rows[0])
    if not 1 <= n_ch <= len(FUSE_CHANNELS):
        raise ValueError(f"fusion weights: 1..{len(FUSE_CHANNELS)} values per setting {FUSE_CHANNELS}, got {n_ch}")
    for r in rows:
        if len(r) != n_ch:
            raise ValueError(f"fusion weights: every setting needs {n_ch} values, got {r}")
        if not all(np.isfinite(v) and v >= 0 for v in r):
            raise ValueError(f"fusion weights: finite values >= 0, got {r}")
        if not any(v > 0 for v in r):
            raise ValueError(f"fusion weights: a setting of all zeros scores nothing, got {r}")
    return rows


def fuse_coefficients(weights, maxima=None, normalise: str = "video", scales=None) -> torch.Tensor:
    """The coefficients of one weight vector, fp32 [n_ch], computed on the device of `maxima` (a tensor: nothing waits for
    it) or on the host.  "video": coef_c = fp32(w_c) / max_c with max_c the channel's largest value over the sub-video -
    one fp32 division - and 0 where max_c == 0 (a channel that is zero everywhere adds nothing).  "none": coef_c =
    fp32(w_c) * fp32(scale_c), `scales` defaulting to ones."""
    w = (weights.to(torch.float32).reshape(-1) if isinstance(weights, torch.Tensor)
         else torch.as_tensor(np.asarray(weights, dtype=np.float32).reshape(-1)))
    if normalise == "video":
        if maxima is None:
            raise ValueError("fuse_coefficients: normalise='video' needs the channel maxima")
        mx = torch.as_tensor(maxima, dtype=torch.float32).reshape(-1)
        if mx.numel() != w.numel():
            raise ValueError(f"fuse_coefficients: {w.numel()} weights for {mx.numel()} maxima")
        w = w.to(mx.device)
        return torch.where(mx == 0, torch.zeros_like(w), w / mx)
    if normalise == "none":
        sc = (torch.ones_like(w) if scales is None else scales.to(torch.float32).reshape(-1) if isinstance(scales, torch.Tensor)
              else torch.as_tensor(np.asarray(scales, dtype=np.float32).reshape(-1)))
        if sc.numel() != w.numel():
            raise ValueError(f"fuse_coefficients: {w.numel()} weights for {sc.numel()} scales")
        return w * sc.to(w.device)
    raise ValueError(f"fuse_coefficients: normalise must be 'video' or 'none', got {normalise!r}")


def fused_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, mask: Optional[torch.Tensor], weights, radius: int = 2,
                   patch: int = 16, frac=(2, 5), thresholds=None, region: bool = True, normalise: str = "video", scales=None,
                   iou=(1, 10), min_area: int = 1, connectivity: int = 8, t_max=None, keep_maps: bool = False,
                   min_gt_area: int = 1, batch: int = EVAL_BATCH, video: str = "", budget: int = FUSE_BUFFER_BUDGET) -> dict:
    """Do appearance, motion and the memories together find the anomaly: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W] and
    mask uint8 (or bool) [T,H,W] (nonzero = anomalous, at the frame size), contiguous and on the model's device, `weights`
    up to FUSE_MAX_SETTINGS weight vectors over the first n_ch of FUSE_CHANNELS.  One pass of the driver: behind every
    forward `ops.error_maps(pixel=True)` writes the rgb pair's and the flow pair's per-pixel error and `ops.memory_scores`
    both streams' commit maps (H/8 x W/8) straight into per-sub-video device buffers.  After the last batch (and the
    driver's re-run of range-flagged batches) the channel maxima are taken on the device; then, per weight vector,
    `fuse_coefficients` (on the device), `ops.fuse_maps` FUSE_FRAME_CHUNK frames at a time into ONE fused buffer that
    every setting reuses, `ops.pixel_scores` on the fused pixel map with the masks and on its patch means with
    `pool_mask(mask, patch)`, and with `region` `ops.region_scores` at `thresholds` (values in (0, 1], default
    `region_thresholds(64)`) times the fused map's largest value - or times `t_max` where given - against the label
    images `ops.label_regions` made once.  Frame t's prediction meets mask[t].  Returns `rgb_psnr`, `rgb_comm`,
    `op_psnr`, `op_comm` (as `pixel_subvideo` gives them), `channel_max` (fp32 [n_ch]), `coef` (fp32 [G, n_ch]) and
    `settings`: per weight vector the per-frame arrays `pix_m`, `pix_kth`, `pix_max_in`, `pix_max_out`, `patch_*`,
    `frame_max`, and with `region` the arrays of `region_subvideo`.  The first RGB_LEN_CLIP - 1 frames repeat frame
    RGB_LEN_CLIP - 1's numbers.  One device-to-host copy behind the driver's own; maps leave the device only under
    `keep_maps` (`pixel_map`, `patch_map` per setting, `channel_maps` by channel name).  `mask=None`: only the four
    records.  The buffers - three [clips, H, W] fp32 maps, the commit grids, the fused patch grid and the label images -
    must fit in `budget` bytes (ValueError names the size)."""
    from . import ops
    rows = check_fusion_weights(weights)
    n_ch, G = len(rows[0]), len(rows)
    if normalise not in ("video", "none"):
        raise ValueError(f"fused_subvideo: normalise must be 'video' or 'none', got {normalise!r}")
    if t_max is not None and (not np.isfinite(t_max) or t_max <= 0):
        raise ValueError(f"fused_subvideo: t_max must be finite and > 0, got {t_max!r}")
    batches = _checked_batches("fused_subvideo", rgb_frames, op_frames, batch)
    t, (h, w) = rgb_frames.shape[0], rgb_frames.shape[2:]
    dev, lc, n_clip = rgb_frames.device, RGB_LEN_CLIP, batches[-1][1]
    if h < 8 or w < 8:
        raise ValueError(f"fused_subvideo: frames of at least 8 x 8 (the commit maps live on the H/8 x W/8 grid), got {h} x {w}")
    scored = mask is not None
    if scored:
        mask = _checked_mask("fused_subvideo", mask, t, h, w, dev)
    values = torch.as_tensor(np.asarray(region_thresholds(64) if thresholds is None else thresholds, dtype=np.float32).reshape(-1)).to(dev)
    K = int(values.numel())
    if region and K < 1:
        raise ValueError("fused_subvideo: no thresholds")
    ph, pw, gh, gw = -(-h // patch), -(-w // patch), h // 8, w // 8
    bmax = max(e - s for s, e in batches)
    n_buf = n_clip if scored else bmax                   # without a mask nothing is kept: every batch reuses its slots
    need = 4 * n_buf * (3 * h * w + 2 * gh * gw + ph * pw) + (n_buf * (h * w + ph * pw) if scored and region else 0)
    if need > budget:
        raise ValueError(f"fused_subvideo: sub-video {video!r} needs {need} bytes ({need / 2 ** 20:.1f} MiB) of device buffers "
                         f"for {n_buf} clips of {h} x {w}, the budget is {budget} bytes: split the sub-video")
    shapes = {"rgb_err": (h, w), "op_err": (h, w), "rgb_commit": (gh, gw), "op_commit": (gh, gw)}
    maps = {name: torch.empty((n_buf,) + shapes[name], device=dev) for name in FUSE_CHANNELS}
    buf = {"patch_sum": torch.empty((bmax, ph, pw), device=dev), "patch_mean": torch.empty((bmax, ph, pw), device=dev),
           "frame_sq": torch.empty(bmax, device=dev), "worst": torch.empty(bmax, device=dev),
           "worst_idx": torch.empty(bmax, device=dev, dtype=torch.int32)}
    mbuf = {"commit": torch.empty(bmax, device=dev), "worst": torch.empty(bmax, device=dev),
            "worst_idx": torch.empty(bmax, device=dev, dtype=torch.int32)}
    quans = (model.rgb.vq_down3, model.op.vq_down3)
    wdev = torch.tensor(rows, dtype=torch.float32).to(dev)                   # uploaded before the pass: nothing waits later
    sdev = None if scales is None else torch.as_tensor(np.asarray(scales, dtype=np.float32).reshape(-1)).to(dev)
    if sdev is not None and sdev.numel() != n_ch:
        raise ValueError(f"fused_subvideo: {n_ch} weights per setting for {sdev.numel()} scales")

    def on_batch(slots, s, e, k, fwd):
        rows_ = slice(s, e) if scored else slice(0, e - s)
        scratch = {key: v[:e - s] for key, v in buf.items()}
        em = ops.error_maps(fwd.rgb_pred, fwd.targets[0], patch, True, dict(scratch, pixel=maps["rgb_err"][rows_]))
        slots.view("rgb_psnr")[s:e] = em["psnr"]
        slots.view("op_psnr")[s:e] = fwd.fused[1]
        ops.error_maps(fwd.op_pred, fwd.targets[1], patch, True, dict(scratch, pixel=maps["op_err"][rows_]))
        for name, quan, x4 in zip(("rgb_commit", "op_commit"), quans, model.bottleneck_inputs()):
            ops.memory_scores(quan, x4.permute(0, 3, 1, 2), False, dict({key: v[:e - s] for key, v in mbuf.items()}, map=maps[name][rows_]))

    rec = _run_pass(model, rgb_frames, op_frames, batches, [("rgb_psnr", ()), ("op_psnr", ())], (), on_batch)
    if not scored:
        return rec
    names = FUSE_CHANNELS[:n_ch]
    masks = {"pix": mask[lc - 1:], "patch": pool_mask(mask, patch).contiguous()[lc - 1:]}
    grids = {"pix": (h, w), "patch": (ph, pw)}
    prefixes = [f"{gi}_" for gi in range(G)]
    sections = [("channel_max", (n_ch,), torch.float32), ("coef", (G, n_ch), torch.float32)]
    for p in prefixes:
        sections.append((f"{p}frame_max", (n_clip,), torch.float32))
        sections += [(f"{p}{g}_{key}", (n_clip,), torch.int32 if key == "m" else torch.float32) for g in grids for key in _PIXEL_KEYS]
    if region:
        sections += _region_sections(grids, n_clip, K, prefixes)
    with torch.no_grad():
        res = _Slots(sections, dev)
        fused = {g: torch.empty((n_clip,) + grid, device=dev) for g, grid in grids.items()}
        maxima = res.view("channel_max")
        for c, name in enumerate(names):
            maxima[c] = maps[name].amax()
        if region:
            for g in grids:
                _label_truth(res, g, masks[g], FUSE_FRAME_CHUNK, min_gt_area, connectivity)
        kept = []
        for gi, p in enumerate(prefixes):
            coef = res.view("coef")[gi]
            coef.copy_(fuse_coefficients(wdev[gi], maxima, normalise, sdev))
            for s in range(0, n_clip, FUSE_FRAME_CHUNK):
                e = min(s + FUSE_FRAME_CHUNK, n_clip)
                ops.fuse_maps([maps[name][s:e] for name in names], FUSE_CELLS[:n_ch], coef, radius, patch,
                              {"pixel": fused["pix"][s:e], "patch_mean": fused["patch"][s:e], "frame_max": res.view(f"{p}frame_max")[s:e]})
                for g in grids:
                    ops.pixel_scores(fused[g][s:e], masks[g][s:e], frac, {key: res.view(f"{p}{g}_{key}")[s:e] for key in _PIXEL_KEYS})
            if region:
                for g in grids:
                    _score_regions(res, p, g, fused[g], values, t_max, FUSE_FRAME_CHUNK, iou, min_area, connectivity)
            if keep_maps:
                kept.append((fused["pix"].cpu().numpy(), fused["patch"].cpu().numpy()))
        host = res.flat.cpu().numpy()                    # the fused figures' one copy
    if region:
        _check_regions("fused_subvideo", res, host, prefixes, grids, video)
    rec["channel_max"], rec["coef"] = res.view("channel_max", host).copy(), res.view("coef", host).copy()
    rec["settings"] = []
    for gi, p in enumerate(prefixes):
        one = {"frame_max": _frames_of(res.view(f"{p}frame_max", host))}
        for g in grids:
            for key in _PIXEL_KEYS:
                one[f"{g}_{key}"] = _frames_of(res.view(f"{p}{g}_{key}", host))
            if region:
                one.update(_region_arrays(res, host, p, g))
        if keep_maps:
            one["pixel_map"], one["patch_map"] = _frames_of(kept[gi][0]), _frames_of(kept[gi][1])
        rec["settings"].append(one)
    if keep_maps:
        rec["channel_maps"] = {name: _frames_of(maps[name].cpu().numpy()) for name in names}
    return rec


def evaluate_dataset_fused(model, videos, masks, weights, dataset_name: str = "synthetic", radius: int = 2, patch: int = 16,
                           frac=(2, 5), thresholds=None, region: bool = True, normalise: str = "video", scales=None,
                           iou=(1, 10), min_area: int = 1, connectivity: int = 8, t_max=None, min_gt_area: int = 1, device=None,
                           keep_maps: bool = False, budget: int = FUSE_BUFFER_BUDGET) -> dict:
    """`evaluate_dataset` with `fused_subvideo` in place of the scoring loop (one rank): ONE forward of the data set
    scores every weight vector of `weights`.  `videos` and `masks` as `evaluate_dataset_pixel` takes them (a None mask:
    the sub-video is evaluated for the frame records only and left out of every figure).  Returns {"weights": the
    settings as lists, "settings": [rec_0, ...]}: rec_g carries the keys of `evaluate_dataset_pixel`'s result and, with
    `region`, of `evaluate_dataset_region`'s - so `pixel_level_auc(rec_g)` and `region_level_auc(rec_g)` work unchanged -
    plus `frame_max`; the four reference record lists, `n_frames` and `mask_videos` are the SAME list objects in every
    rec_g.  With `keep_maps` rec_g also holds `pixel_map`, `patch_map` and `mask`, and the result `channel_maps` (per
    sub-video a dict by channel name, None without a mask), `channel_max` and `coef`."""
    rows = check_fusion_weights(weights)
    keys = ["frame_max"] + [f"{g}_{key}" for g in ("pix", "patch") for key in _PIXEL_KEYS] + (list(_REGION_REC_KEYS) if region else [])
    keys += ["pixel_map", "patch_map", "mask"] if keep_maps else []
    base = _new_records(dataset_name, "n_frames", "mask_videos")
    recs = [dict(base, **{k: [] for k in keys}) for _ in rows]      # (a shallow copy: the lists of `base` are shared)
    out = {"weights": rows, "settings": recs, "channel_max": [], "coef": []}
    if keep_maps:
        out["channel_maps"] = []

    def score(v, rgb, op, dm):
        return fused_subvideo(model, rgb, op, dm, rows, radius, patch, frac, thresholds, region, normalise, scales, iou, min_area,
                              connectivity, t_max, keep_maps and dm is not None, min_gt_area, video=str(v), budget=budget)

    for v, rec, has, host_mask in _masked_subvideos("evaluate_dataset_fused", model, videos, masks, base, score, keep_maps, device):
        for gi, one in enumerate(recs):
            for k in keys:
                one[k].append((host_mask if k == "mask" else rec["settings"][gi][k]) if has else None)
        out["channel_max"].append(rec["channel_max"] if has else None)
        out["coef"].append(rec["coef"] if has else None)
        if keep_maps:
            out["channel_maps"].append(rec["channel_maps"] if has else None)
    return out


# ---- qualitative evaluation: prediction, flow and error panels ------------------------------
# A pass of its own behind the evaluation forward (`ops.render_panels`, csrc/render.hip): finished uint8 pictures of the
# frames, the colour-coded flows and the error heat maps.  The scoring loops above are not touched.

RENDER_TILES = ("rgb_target", "rgb_pred", "rgb_heat", "op_target", "op_pred", "op_heat")       # the C ABI's tile ids
RENDER_DEFAULT_TILES = (RENDER_TILES[:3], RENDER_TILES[3:])
FLOW_UNKNOWN = 1e7           # a flow component above it (or a NaN) marks a pixel without a flow (Middlebury's convention)


def panel_layout(tiles) -> List[List[str]]:
    """`tiles` as rows of tile names: a sequence of names is one row, a sequence of sequences the rows (equal lengths).
    An ordered subset of RENDER_TILES - at most six, none twice.  ValueError otherwise."""
    if isinstance(tiles, str):
        tiles = [tiles]
    rows = [list(tiles)] if all(isinstance(t, str) for t in tiles) else [[t for t in row] for row in tiles]
    flat = [t for row in rows for t in row]
    if not flat or any(len(row) != len(rows[0]) for row in rows):
        raise ValueError(f"render: tiles must be a non-empty row of names or rows of equal length, got {tiles!r}")
    for t in flat:
        if t not in RENDER_TILES:
            raise ValueError(f"render: unknown tile {t!r}; the tiles are {', '.join(RENDER_TILES)}")
    if len(set(flat)) != len(flat):
        raise ValueError(f"render: every tile at most once, got {flat}")
    return rows


def colour_wheel() -> np.ndarray:
    """the Middlebury colour wheel [55, 3] as fp32 values / 255, from its published segment lengths: along a segment of
    length n one channel holds 255 and one ramps floor(255 i / n) - up in the 1st, 3rd and 5th segment, down from 255 in
    the others"""
    wheel, k = np.zeros((55, 3), dtype=np.float32), 0
    for s, (n, full, ramp) in enumerate(((15, 0, 1), (6, 1, 0), (4, 1, 2), (11, 2, 1), (13, 2, 0), (6, 0, 2))):
        for i in range(n):
            r = 255 * i // n
            wheel[k, full] = 255
            wheel[k, ramp] = r if s % 2 == 0 else 255 - r
            k += 1
    return wheel / np.float32(255)


def _flow_parts(flow: np.ndarray, scale):
    """fp32: the scaled components with the unknown pixels zeroed, the radius, the known mask; flow [B,2,H,W]"""
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = f32(scale[0]) * flow[:, 0].astype(f32), f32(scale[1]) * flow[:, 1].astype(f32)
        known = (np.abs(u) <= f32(FLOW_UNKNOWN)) & (np.abs(v) <= f32(FLOW_UNKNOWN))         # False for a NaN
    u, v = np.where(known, u, f32(0)), np.where(known, v, f32(0))
    return u, v, np.sqrt(u * u + v * v), known


def flow_colour_reference(flow, scale=(1.0, 1.0), max_rad=None) -> Dict[str, np.ndarray]:
    """The Middlebury colour code of flows [B,2,H,W] (tensor or array, any device) in fp32 numpy, as include/ammc_hip.h
    defines it: `rgb` uint8 [B,H,W,3], `raw` [B,H,W] (the radius), `max_rad` [B] (each sample's largest radius, or the
    supplied per-sample values), `inside` and `known` [B,H,W].  The reference's `flow_to_image` up to one deliberate
    difference: a pixel is inside when raw <= max_rad and its normalised radius is clamped to 1 (the reference re-derives
    the radius from the normalised components in float64, which lands on either side of 1 for the pixels that attain the
    maximum)."""
    f32 = np.float32
    flow = flow.detach().cpu().numpy() if isinstance(flow, torch.Tensor) else np.asarray(flow)
    u, v, raw, known = _flow_parts(flow, scale)
    own = raw.reshape(raw.shape[0], -1).max(axis=1)
    if max_rad is None:
        mr = own
    else:
        mr = (max_rad.detach().cpu().numpy() if isinstance(max_rad, torch.Tensor) else np.asarray(max_rad)).astype(f32)
    mr3 = mr.astype(f32)[:, None, None]
    with np.errstate(over="ignore"):
        inv = f32(1) / (mr3 + f32(2.0 ** -52))
        inside = raw <= mr3
        rad = np.minimum(raw * inv, f32(1))
    a = np.arctan2(-v, -u) / f32(np.pi)
    fk = (a + f32(1)) / f32(2) * f32(54) + f32(1)
    k0f = np.clip(np.floor(fk), f32(1), f32(55))
    k0 = k0f.astype(np.int64)
    k1 = np.where(k0 == 55, 1, k0 + 1)
    f = fk - k0f
    wheel = colour_wheel()
    out = np.zeros(raw.shape + (3,), dtype=np.uint8)
    for ch in range(3):
        col = (f32(1) - f) * wheel[k0 - 1, ch] + f * wheel[k1 - 1, ch]
        col = np.where(inside, f32(1) - rad * (f32(1) - col), col * f32(0.75))
        out[..., ch] = np.where(known, np.clip(np.floor(f32(255) * col), 0, 255), 0).astype(np.uint8)
    return {"rgb": out, "raw": raw, "max_rad": mr.astype(f32), "own_max": own, "inside": inside, "known": known}


def _err32(pred: np.ndarray, target: np.ndarray) -> np.ndarray:
    """fp32 `ops.error_maps` pixel: ((d_0^2 + d_1^2) + ...) / c with d = 0.5 (target - pred); a NaN counts as 0"""
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        acc = None
        for ch in range(pred.shape[1]):
            d = f32(0.5) * (target[:, ch] - pred[:, ch])
            acc = d * d if acc is None else acc + d * d
        e = acc / f32(pred.shape[1])
    return np.where(np.isnan(e), f32(0), e)


def frame_tile_reference(x: np.ndarray) -> np.ndarray:
    """float64: u8 = floor(clamp((x + 1) * 127.5, 0, 255) + 0.5) per channel, [B,3,H,W] -> uint8 [B,H,W,3]; NaN -> 0"""
    x = np.where(np.isnan(x), -1.0, x.astype(np.float64))
    return np.floor(np.clip((x + 1.0) * 127.5, 0.0, 255.0) + 0.5).astype(np.uint8).transpose(0, 2, 3, 1)


def heat_tile_reference(e: np.ndarray, heat_max: np.ndarray, grey: np.ndarray, alpha: float) -> np.ndarray:
    """float64: t = min(e / heat_max, 1) (0 where heat_max <= 0), colour = clamp(1.5 - |4 t - (3, 2, 1)|, 0, 1),
    u8 = floor((1 - alpha) * grey + alpha * 255 * colour + 0.5); e [B,H,W], heat_max [B], grey [B,H,W] or a number"""
    hm = np.asarray(heat_max, dtype=np.float64)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(hm > 0, np.minimum(np.nan_to_num(e.astype(np.float64) / hm, nan=1.0), 1.0), 0.0)
    a = float(np.float32(alpha))
    grey = np.broadcast_to(np.asarray(grey, dtype=np.float64), e.shape)
    out = np.empty(e.shape + (3,), dtype=np.uint8)
    for ch in range(3):
        c = np.clip(1.5 - np.abs(4.0 * t - (3 - ch)), 0.0, 1.0)
        out[..., ch] = np.clip(np.floor((1.0 - a) * grey + a * 255.0 * c + 0.5), 0, 255).astype(np.uint8)
    return out


def render_reference(rgb_pred, rgb_target, op_pred, op_target, tiles=RENDER_DEFAULT_TILES, flow_scale=(1.0, 1.0),
                     flow_norm="target", heat_max="frame", alpha: float = 0.6) -> Dict[str, np.ndarray]:
    """The quantities of `ops.render_panels` in plain numpy (tensors of any device or arrays; the witness of the tests):
    the colour code in fp32 (`flow_colour_reference`), the frame and heat tiles in float64.  The normalising maxima
    (`stats` [B,4] fp32: the largest radius of the target and of the predicted flow, the largest per-pixel error of the
    frame pair and of the flow pair) are the fp32 restatement the kernel must reproduce bit for bit.  Returns `panels`
    uint8 [B, rows*H, cols*W, 3], `stats`, and every tile by its name [B,H,W,3]."""
    f32 = np.float32
    arr = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (rgb_pred, rgb_target, op_pred, op_target)]
    rp, rt, fp, ft = (a.astype(f32) for a in arr)
    rows = panel_layout(tiles)
    b = rp.shape[0]
    ct, cp = flow_colour_reference(ft, flow_scale), flow_colour_reference(fp, flow_scale)
    e_rgb64 = (((rt.astype(np.float64) - rp.astype(np.float64)) * 0.5) ** 2).mean(axis=1)
    e_op64 = (((ft.astype(np.float64) - fp.astype(np.float64)) * 0.5) ** 2).mean(axis=1)
    both = ct["known"] & cp["known"]
    e_rgb64 = np.where(np.isnan(e_rgb64), 0.0, e_rgb64)
    e_op64 = np.where(both & ~np.isnan(e_op64), e_op64, 0.0)
    e_op32 = np.where(both, _err32(fp, ft), f32(0))
    stats = np.stack([ct["own_max"], cp["own_max"], _err32(rp, rt).reshape(b, -1).max(axis=1),
                      e_op32.reshape(b, -1).max(axis=1)], axis=1).astype(f32)

    def vec(v):
        return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(f32).reshape(b)
    if isinstance(flow_norm, str):
        if flow_norm not in ("target", "each"):
            raise ValueError(f"render: flow_norm must be 'target', 'each' or a tensor [B], got {flow_norm!r}")
        mr_t, mr_p = stats[:, 0], (stats[:, 0] if flow_norm == "target" else stats[:, 1])
    else:
        mr_t = mr_p = vec(flow_norm)
    if isinstance(heat_max, str):
        if heat_max != "frame":
            raise ValueError(f"render: heat_max must be 'frame', a tensor [B] or a pair of them, got {heat_max!r}")
        hm_rgb, hm_op = stats[:, 2], stats[:, 3]
    elif isinstance(heat_max, (tuple, list)):
        hm_rgb, hm_op = vec(heat_max[0]), vec(heat_max[1])
    else:
        hm_rgb = hm_op = vec(heat_max)
    out = {"stats": stats}
    out["rgb_target"], out["rgb_pred"] = frame_tile_reference(rt), frame_tile_reference(rp)
    out["rgb_heat"] = heat_tile_reference(e_rgb64, hm_rgb, out["rgb_target"].astype(np.float64).sum(axis=3) / 3.0, alpha)
    out["op_target"] = flow_colour_reference(ft, flow_scale, mr_t)["rgb"]
    out["op_pred"] = flow_colour_reference(fp, flow_scale, mr_p)["rgb"]
    out["op_heat"] = heat_tile_reference(e_op64, hm_op, 128.0, alpha)
    out["panels"] = np.concatenate([np.concatenate([out[t] for t in row], axis=2) for row in rows], axis=1)
    return out


def render_subvideo(model, rgb_frames: torch.Tensor, op_frames: torch.Tensor, select=None, tiles=RENDER_DEFAULT_TILES,
                    flow_scale=None, flow_norm="target", heat_max="frame", alpha: float = 0.6, batch: int = EVAL_BATCH,
                    ring: int = 2, stats: Optional[dict] = None):
    """Pictures of a sub-video: rgb_frames [T,3,H,W], op_frames [T-1,2,H,W], contiguous and on the model's device ->
    a generator of (frame index, panel uint8 [rows*H, cols*W, 3]) in frame order.  Frame f >= RGB_LEN_CLIP - 1 is the
    target of clip f - (RGB_LEN_CLIP - 1), with flow f - 1 the target of the flow stream: `localise_subvideo`'s clips,
    targets, batches (`batch` clips at a time), `defer_guard` and `exact` re-run of a batch whose S16 range flag is set.
    `select`: the frame indices to render (any iterable; default every predicted frame) - only the batches that hold one
    run, and of such a batch only the span of clips between its first and last selected one is rendered and copied.
    Behind the forward `ops.render_panels` writes the span's panels into a device buffer, whose last word receives the
    range flag; ONE device-to-host copy per batch on a side stream brings both into a pinned ring of `ring` buffers
    while the next batch runs.  The yielded panel is the caller's own array (a copy out of the ring).
    `flow_scale`: default (H, W), the reference's `get_vis_tensor` re-scaling.  The other options are `ops.render_panels`'.
    `stats` (optional dict) receives `render_ms` (the render launches between events, summed), `render_batches`,
    `copies`, `rerun_batches`."""
    from . import ops
    batches = _checked_batches("render_subvideo", rgb_frames, op_frames, batch)
    t, lc = rgb_frames.shape[0], RGB_LEN_CLIP - 1
    if select is None:
        clips = list(range(batches[-1][1]))
    else:
        frames = sorted(set(int(f) for f in select))
        if frames and (frames[0] < lc or frames[-1] >= t):
            raise ValueError(f"render_subvideo: the predicted frames are {lc} .. {t - 1}, got {frames[0]} .. {frames[-1]}")
        clips = [f - lc for f in frames]
    rows = panel_layout(tiles)
    h, w = rgb_frames.shape[2:]
    if flow_scale is None:
        flow_scale = (float(h), float(w))
    ph, pw = len(rows) * h, len(rows[0]) * w
    per = ph * pw * 3
    dev = rgb_frames.device
    work = []                                                       # (batch index, first clip, last clip + 1, wanted clips)
    for k, (s, e) in enumerate(batches):
        mine = [c for c in clips if s <= c < e]
        if mine:
            work.append((k, mine[0], mine[-1] + 1, mine))
    if not work:
        return
    head = 16                                                       # the range flag's word, in front of the panels
    cap = head + max(hi - lo for _, lo, hi, _ in work) * per
    ring = max(int(ring), 2)
    dbuf = [torch.empty(cap, device=dev, dtype=torch.uint8) for _ in range(ring)]
    hbuf = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(ring)]
    side = torch.cuda.Stream(device=dev)
    timed, copies, reruns = [], 0, 0
    # a number in place of a mode: the same value for every frame (pictures of different frames are then comparable)
    fixed = {key: torch.full((batch,), float(v), device=dev, dtype=torch.float32)
             for key, v in (("flow_norm", flow_norm), ("heat_max", heat_max)) if isinstance(v, (int, float))}

    def launch(j: int, exact: bool):
        k, lo, hi, _ = work[j]
        s, e = batches[k]
        slot = j % ring
        fwd = _forward_batch(model, rgb_frames, op_frames, s, e, exact)
        rgb_out, op_out, targets, flag = fwd.rgb_pred, fwd.op_pred, fwd.targets, fwd.overflow
        with torch.no_grad():
            n = hi - lo
            out = dbuf[slot][head:head + n * per].view(n, ph, pw, 3)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            ops.render_panels(rgb_out[lo - s:hi - s], targets[0][lo - s:hi - s], op_out[lo - s:hi - s], targets[1][lo - s:hi - s],
                              tiles=rows, flow_scale=flow_scale, alpha=alpha, out=out,
                              flow_norm=fixed["flow_norm"][:n] if "flow_norm" in fixed else flow_norm,
                              heat_max=fixed["heat_max"][:n] if "heat_max" in fixed else heat_max)
            ev1.record()
            timed.append((ev0, ev1))
            word = dbuf[slot][:4].view(torch.float32)
            if flag is not None:
                word.copy_(flag.reshape(1).to(torch.float32))
            else:
                word.zero_()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            hbuf[slot][:head + n * per].copy_(dbuf[slot][:head + n * per], non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        return done

    def finish(j: int, done):
        nonlocal reruns, copies
        k, lo, hi, mine = work[j]
        slot = j % ring
        done.synchronize()
        copies += 1
        host = hbuf[slot].numpy()
        if host[:4].view(np.float32)[0] != 0:                        # S16 range guard: this batch again on the exact-fp32 kernels
            launch(j, True).synchronize()
            copies += 1
            reruns += 1
            _count_fallback(model)
        panels = host[head:head + (hi - lo) * per].reshape(hi - lo, ph, pw, 3)
        return [(c + lc, panels[c - lo].copy()) for c in mine]

    try:
        pending = None
        for j in range(len(work)):
            # batch j runs while the copy of batch j - 1 is in flight; buffer j % ring is free: the copy of batch
            # j - ring (<= j - 2) was awaited when that batch was handed out
            done = launch(j, False)
            if pending is not None:
                yield from finish(*pending)
            pending = (j, done)
        if pending is not None:
            yield from finish(*pending)
    finally:
        torch.cuda.current_stream(dev).wait_stream(side)
        if stats is not None:
            torch.cuda.synchronize(dev)
            stats["render_ms"] = stats.get("render_ms", 0.0) + sum(a.elapsed_time(b) for a, b in timed)
            stats["render_batches"] = stats.get("render_batches", 0) + len(timed)
            stats["copies"] = stats.get("copies", 0) + copies
            stats["rerun_batches"] = stats.get("rerun_batches", 0) + reruns


class OrderedWriterPool:
    """A bounded pool of writer threads: `submit(fn, *args)` queues a job (it blocks while 2 x workers jobs are waiting:
    the producer cannot run ahead of the disk), `close()` hands the return values back in SUBMISSION order.
    The first exception of a job is raised by the next `submit` or by `close` - never lost - and the jobs queued behind it
    are dropped."""

    MAX_WORKERS = 16

    def __init__(self, workers: int = 8):
        from concurrent.futures import ThreadPoolExecutor
        import threading
        if workers < 1:
            raise ValueError(f"OrderedWriterPool: at least one worker, got {workers}")
        self.workers = min(int(workers), self.MAX_WORKERS)
        self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="panel-writer")
        self._room = threading.BoundedSemaphore(2 * self.workers)
        self._futures = []
        self._checked = 0
        self.busy_s = 0.0                                           # seconds the jobs ran, summed over the threads
        self._lock = threading.Lock()

    def _run(self, fn, args):
        import time
        t0 = time.perf_counter()
        try:
            return fn(*args)
        finally:
            with self._lock:
                self.busy_s += time.perf_counter() - t0
            self._room.release()

    def _raise_finished(self):
        while self._checked < len(self._futures) and self._futures[self._checked].done():
            self._futures[self._checked].result()                   # raises the job's exception
            self._checked += 1

    def submit(self, fn, *args) -> None:
        try:
            self._raise_finished()
        except BaseException:
            self._abort()
            raise
        self._room.acquire()
        self._futures.append(self._pool.submit(self._run, fn, args))

    def _abort(self):
        for f in self._futures:
            f.cancel()
        self._pool.shutdown(wait=True)

    def close(self) -> list:
        """wait for every job; the results in submission order, or the first exception in that order"""
        try:
            return [f.result() for f in self._futures]
        except BaseException:
            self._abort()
            raise
        finally:
            self._pool.shutdown(wait=True)


def write_panel(path: str, panel: np.ndarray, fmt: str = "png") -> str:
    """one panel [h, w, 3] uint8 to `path`: PNG through PIL at compress_level 1 (the writers are the slow side: a low
    level keeps them near the device's pace), or .npy"""
    if fmt == "png":
        from PIL import Image
        Image.fromarray(panel, "RGB").save(path, format="PNG", compress_level=1)
    elif fmt == "npy":
        np.save(path, panel)
    else:
        raise ValueError(f"write_panel: format must be 'png' or 'npy', got {fmt!r}")
    return path


def select_frames(psnr: np.ndarray, every: int = 1, top: Optional[int] = None) -> List[int]:
    """which frames of a sub-video get a picture: of the predicted frames RGB_LEN_CLIP - 1 .. T - 1 every `every`-th,
    and of those - with `top` - the `top` with the lowest `psnr` (the per-frame record; equal values: the earlier
    frame first).  Ascending frame indices."""
    if every < 1 or (top is not None and top < 1):
        raise ValueError(f"select_frames: every >= 1 and top >= 1, got {every} and {top}")
    frames = np.arange(RGB_LEN_CLIP - 1, len(psnr), every)
    if top is not None and top < len(frames):
        frames = frames[np.argsort(np.asarray(psnr)[frames], kind="stable")[:top]]
    return sorted(int(f) for f in frames)


def evaluate_dataset_panels(model, videos, dataset_name: str = "synthetic", panels_dir: Optional[str] = None, fmt: str = "png",
                            every: int = 1, top: Optional[int] = None, workers: int = 8, device=None,
                            stats: Optional[dict] = None, **render) -> dict:
    """`evaluate_dataset_localised` (patch 16, no maps: its records are returned as they are) with pictures: every
    sub-video is scored with `localise_subvideo`, `select_frames` picks its frames from the rgb PSNR record, and
    `render_subvideo` re-runs the batches that hold one (`render`: its options).  `panels_dir`: the pictures go to
    `panels_dir/NNNN/FFFFFF.<fmt>` (sub-video, frame) through an `OrderedWriterPool` of `workers` threads; None renders
    and drops them (a warm-up).  Returns the record dict plus `panel_files` (in sub-video and frame order) and
    `panel_frames` (per sub-video, the frames chosen).  `stats` receives `render_subvideo`'s counters, `write_s` (the
    writers' busy seconds, summed over the threads) and `write_wait_s` (the seconds this thread waited for them)."""
    import time
    if fmt not in ("png", "npy"):
        raise ValueError(f"evaluate_dataset_panels: format must be 'png' or 'npy', got {fmt!r}")
    out = _new_records(dataset_name, "rgb_patch_psnr_records", "n_frames", "panel_frames", "panel_files")
    pool = OrderedWriterPool(workers) if panels_dir else None
    counters: dict = {}
    waited = 0.0
    try:
        for v, rgb, op, rec in _scored_subvideos(model, videos, out, lambda v, rgb, op: localise_subvideo(model, rgb, op), device):
            out["rgb_patch_psnr_records"].append(_worst_patch_psnr(rec["rgb_worst"]))
            frames = select_frames(rec["rgb_psnr"], every, top)
            out["panel_frames"].append(frames)
            if panels_dir:
                os.makedirs(os.path.join(panels_dir, f"{v:04d}"), exist_ok=True)
            for f, panel in render_subvideo(model, rgb, op, select=frames, stats=counters, **render):
                if pool is not None:
                    t0 = time.perf_counter()
                    pool.submit(write_panel, os.path.join(panels_dir, f"{v:04d}", f"{f:06d}.{fmt}"), panel, fmt)
                    waited += time.perf_counter() - t0
    except BaseException:
        if pool is not None:
            pool._abort()
        raise
    if pool is not None:
        t0 = time.perf_counter()
        out["panel_files"] = pool.close()
        waited += time.perf_counter() - t0
    if stats is not None:
        stats.update(counters)
        stats.update(write_s=pool.busy_s if pool is not None else 0.0, write_wait_s=waited)
    return out


def weights_init_normal(model: torch.nn.Module) -> None:
    """the reference's training-from-scratch init (utils/utils.py:328-334): Conv* ~ N(0, 0.02),
    BatchNorm2d gamma ~ N(1, 0.02), beta = 0; applied by class name exactly as there"""
    for m in model.modules():
        cn = m.__class__.__name__
        if cn.find("Conv") != -1 and hasattr(m, "weight") and isinstance(m.weight, torch.nn.Parameter):
            torch.nn.init.normal_(m.weight.data, 0.0, 0.02)
        elif cn.find("BatchNorm2d") != -1:
            torch.nn.init.normal_(m.weight.data, 1.0, 0.02)
            torch.nn.init.constant_(m.bias.data, 0.0)
    if hasattr(model, "_param_epoch"):
        model._param_epoch += 1


# ---- checkpoint tooling (utils/utils.py:182-263): same file names and key conventions as the reference ------------

def save_checkpoint(state_dict: dict, model_dir: str, step: int) -> str:
    """`saver` (utils.py:182-189): <model_dir>/step_<step+1, 6 digits>.pth"""
    import os
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, "step_{}.pth".format(str(step + 1).zfill(6)))
    torch.save(state_dict, path)
    return path


def load_latest_checkpoint(model: torch.nn.Module, model_dir: str, map_location="cpu"):
    """`loader` (utils.py:192-203): the lexicographically last file of the directory; returns (model, step)"""
    import os
    names = sorted(os.listdir(model_dir))
    if not names:
        raise FileNotFoundError(f"no checkpoint in {model_dir}")
    path = os.path.join(model_dir, names[-1])
    model.load_state_dict(torch.load(path, map_location=map_location))
    return model, int(path.split("_")[-1].split(".")[0])


def load_pretrained_branches(model: torch.nn.Module, rgb_ckpt, op_ckpt, map_location="cpu"):
    """`loader_rgb_op_branch` (utils.py:236-263): the two-stage recipe of the reference README - single-stream
    `UNetMem_v7` checkpoints (paths or state dicts) go into the `rgb.` / `op.` branches of `twostream`, keys the joint
    model does not have are dropped, the bridge keeps its initialisation.  Returns (model, 0) like the reference."""
    def as_dict(c):
        return torch.load(c, map_location=map_location) if isinstance(c, (str, bytes)) or hasattr(c, "__fspath__") else c
    own = model.state_dict()
    for prefix, ck in (("rgb", as_dict(rgb_ckpt)), ("op", as_dict(op_ckpt))):
        own.update({f"{prefix}.{k}": v for k, v in ck.items() if f"{prefix}.{k}" in own})
    model.load_state_dict(own)
    return model, 0


def flownet_flow_fn(flownet: torch.nn.Module) -> Callable:
    """`flow_fn` for `train_step_gan` from a (frozen, eval-mode) FlowNet2-SD: frames in [-1, 1] -> flow / 255, as
    train_helper.py:309-316 feeds it (`(pair * 0.5 + 0.5) * 255`, then `/ 255`, detached)"""
    def fn(prev: torch.Tensor, cur: torch.Tensor) -> torch.Tensor:
        pair = torch.cat([prev.unsqueeze(2), cur.unsqueeze(2)], 2)
        with torch.no_grad():
            return flownet((pair * 0.5 + 0.5) * 255.0) / 255.0
    return fn
