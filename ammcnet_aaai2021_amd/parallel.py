"""One process per GPU: what the path needs from `torch.distributed` (RCCL over xGMI), nothing more.

The reference is single-GPU (no DP/DDP anywhere); these are the builder's
choices for BASELINE.json's multi-GPU configs:

* **Inference** (configs 2, 5) shards by WHOLE harness batches (16 consecutive clips of one
  sub-video): the commit score is a per-batch mean (reference unet.py:310), so a batch is
  never split across GPUs and never re-batched.  No data-path collective; per-frame records
  are gathered at the end (`gather_records`).
* **Training** (configs 3, 4) is plain data parallelism: every rank holds the full 25 M-parameter
  generator, runs the HIP forward/backward on its local clips and averages the gradients with
  a bucketed all-reduce.  `BucketedGradReducer` is driven by the training engine as each stage
  of the hand-scheduled backward finishes (decoders -> bridge -> memory -> encoders), so the
  RCCL traffic of early buckets overlaps the remaining backward kernels.  100 MB of fp32
  gradients per step is ~1.2 ms on one xGMI link; buckets of ~25 MB keep RCCL's ring/tree
  protocols in their bandwidth regime without delaying the first launch.
  BatchNorm statistics and the EMA codebook stay per-rank (stock DDP semantics); buffers are
  made identical across ranks with `broadcast_state` (rank 0 wins) at start and on demand.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import _lib


def init_distributed(backend: Optional[str] = None) -> Tuple[int, int, torch.device]:
    """RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment (torchrun); backend
    "nccl" (= RCCL on ROCm) when a GPU is visible, else "gloo"."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_gpu = torch.cuda.is_available()
    dev = torch.device("cuda", local) if use_gpu else torch.device("cpu")
    if use_gpu:
        torch.cuda.set_device(dev)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        backend = backend or ("nccl" if use_gpu else "gloo")
        kw = {"device_id": dev} if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    return rank, world, dev


def shard_batches(n_batches: int, rank: int, world: int) -> List[int]:
    """indices of the harness batches this rank evaluates (contiguous blocks, so that a
    sub-video's batches mostly stay on one GPU); every batch is owned by exactly one rank"""
    base, extra = divmod(n_batches, world)
    start = rank * base + min(rank, extra)
    return list(range(start, start + base + (1 if rank < extra else 0)))


def gather_records(local: Dict[int, object], world: int) -> Dict[int, object]:
    """merge {batch index: per-frame records} from all ranks (a few KB; object all-gather)"""
    if world == 1 or not dist.is_initialized():
        return dict(local)
    parts: List[Optional[dict]] = [None] * world
    dist.all_gather_object(parts, local)
    out: Dict[int, object] = {}
    for p in parts:
        out.update(p)
    return out


def broadcast_state(module: torch.nn.Module, src: int = 0) -> None:
    """make parameters and buffers (BN running stats, codebook) identical on every rank"""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            dist.broadcast(t.data, src)
    if hasattr(module, "_param_epoch"):
        module._param_epoch += 1


class BucketedGradReducer:
    """Average gradients across ranks in ~`bucket_mb` MiB buckets, launched as they become ready.

    `push(tensors)` may be called many times during one backward; a bucket is flattened and
    all-reduced asynchronously as soon as it is full.  `finish()` flushes the tail, waits and
    scatters the averaged values back IN PLACE into the pushed tensors.  `force`: take the collective path with ONE
    rank too (an initialised process group is then required) - the one-GPU proof that the communicator, the
    asynchronous all-reduce and its ordering against the raw-pointer kernels on torch's current stream work.

    Buckets of contiguous fp32 GPU tensors are gathered by `ammc_bucket_pack_f32` and come back through
    `ammc_bucket_unpack_scale_f32` (csrc/bucket.hip: one launch per 128 members, the 1 / world multiply folded into the
    scatter) on torch's current stream, ordered against the asynchronous all-reduce exactly as the `torch._foreach_*`
    calls that remain the path for everything else (CPU tensors over gloo); `hip=False` takes that path for GPU buckets
    too (the A/B of DESIGN.md section 6).  Both give the same bits: `x * (1 / world)` is one fp32 multiply in either."""

    def __init__(self, bucket_mb: float = 25.0, group=None, force: bool = False, hip: bool = True):
        self.bucket_bytes = int(bucket_mb * (1 << 20))
        self.group = group
        self.force = bool(force)
        self.hip = bool(hip)
        self._flats: Dict[int, torch.Tensor] = {}
        self._layouts: Dict[int, tuple] = {}
        self._pending: List[torch.Tensor] = []
        self._pending_bytes = 0
        # (flat buffer, its member views or None where the HIP kernels move the bucket, members, all-reduce handle)
        self._inflight: List[Tuple[torch.Tensor, Optional[List[torch.Tensor]], List[torch.Tensor], object]] = []
        self.buckets_launched = 0
        # measurement (bench.py --mode train --gpus N): with `time_finish` every `finish()` is bracketed by HIP events on
        # the compute stream - what the step pays for the collectives that did NOT hide behind the backward (the wait
        # for the last buckets, the averaging and the scatter back) - collected in `finish_events`
        self.time_finish = False
        self.finish_events: List[Tuple[torch.cuda.Event, torch.cuda.Event]] = []
        self.last_step_buckets = 0

    @property
    def world(self) -> int:
        return dist.get_world_size(self.group) if dist.is_initialized() else 1

    @property
    def active(self) -> bool:
        return self.world > 1 or (self.force and dist.is_initialized())

    def push(self, tensors: Iterable[torch.Tensor]) -> None:
        if not self.active:
            return
        for t in tensors:
            self._pending.append(t)
            self._pending_bytes += t.numel() * t.element_size()
            if self._pending_bytes >= self.bucket_bytes:
                self._launch()

    def _flat_for(self, slot: int, members: List[torch.Tensor], n: Optional[int] = None) -> torch.Tensor:
        """the persistent flat buffer of the `slot`-th bucket of a step: the bucket composition is the same every step
        (the backward pushes the same tensors in the same order), so the buffer is allocated once and only re-made
        when the total size or dtype / device changes - no `torch.cat` allocation per bucket per step.  Allocated
        zeroed: the HIP path pads every member's start to 16 bytes, and the all-reduce sums zeros in the padding."""
        n = sum(t.numel() for t in members) if n is None else n
        flat = self._flats.get(slot)
        if flat is None or flat.numel() != n or flat.dtype != members[0].dtype or flat.device != members[0].device:
            flat = torch.zeros(n, dtype=members[0].dtype, device=members[0].device)
            self._flats[slot] = flat
        return flat

    def _hip_ok(self, members: List[torch.Tensor]) -> bool:
        """the bucket kernels (csrc/bucket.hip) move non-empty contiguous fp32 tensors of one GPU; anything else (CPU
        tensors over gloo, other dtypes) takes torch's multi-tensor ops"""
        dev = members[0].device
        return self.hip and dev.type == "cuda" and all(
            t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.numel() > 0 for t in members)

    def _tables(self, slot: int, members: List[torch.Tensor]):
        """[(table, members in it, flat offset of its first member)], one entry per launch, and the padded length of
        the bucket.  Only the layout is kept between steps; the pointers are read every step (`.grad` tensors are re-made
        after `zero_grad(set_to_none=True)`) and travel in the kernel arguments."""
        sizes = tuple(t.numel() for t in members)
        cached = self._layouts.get(slot)
        if cached is None or cached[0] != sizes:
            launches, off = [], 0
            for i in range(0, len(sizes), _lib.AMMC_BUCKET_MAX):
                part, base, ends = sizes[i:i + _lib.AMMC_BUCKET_MAX], off, []
                for n in part:
                    off = (off + 3) & ~3
                    off += n
                    ends.append(off - base)
                table = _lib.AmmcBucketTable()
                table.end[:len(ends)] = ends
                launches.append((table, i, len(part), base))
                off = (off + 3) & ~3               # the next launch's `flat` stays 16-byte aligned
            cached = (sizes, launches, off)
            self._layouts[slot] = cached
        for table, i, n, _ in cached[1]:
            table.ptr[:n] = [t.data_ptr() for t in members[i:i + n]]
        return cached[1], cached[2]

    def _launch(self) -> None:
        if not self._pending:
            return
        members = self._pending
        slot = len(self._inflight)
        if self._hip_ok(members):
            lib = _lib.load()
            launches, total = self._tables(slot, members)
            flat = self._flat_for(slot, members, total)
            stream = torch.cuda.current_stream(flat.device).cuda_stream
            for table, _, n, base in launches:                               # one gather launch per 128 members
                _lib.check(lib.ammc_bucket_pack_f32(ctypes.byref(table), n, 4, flat.data_ptr() + 4 * base, stream),
                           "bucket_pack")
            views = None
        else:
            flat = self._flat_for(slot, members)
            views, off = [], 0
            for t in members:
                n = t.numel()
                views.append(flat[off:off + n].view_as(t))
                off += n
            torch._foreach_copy_(views, [t.detach() for t in members])      # one fused gather into the bucket
        work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._inflight.append((flat, views, members, work))
        self._pending, self._pending_bytes = [], 0
        self.buckets_launched += 1

    def finish(self) -> None:
        if not self.active:
            return
        self._launch()
        inv = 1.0 / self.world
        self.last_step_buckets = len(self._inflight)
        ev = None
        if self.time_finish and self._inflight and self._inflight[0][0].is_cuda:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        for slot, (flat, views, members, work) in enumerate(self._inflight):
            work.wait()
            if views is None:                                                # the average and the scatter in one pass
                lib = _lib.load()
                launches, _ = self._tables(slot, members)
                stream = torch.cuda.current_stream(flat.device).cuda_stream
                for table, _, n, base in launches:
                    _lib.check(lib.ammc_bucket_unpack_scale_f32(ctypes.byref(table), n, 4, flat.data_ptr() + 4 * base,
                                                                inv, stream), "bucket_unpack_scale")
            else:
                torch._foreach_mul_(views, inv)                              # average in the bucket ...
                torch._foreach_copy_([t.detach() for t in members], views)   # ... and scatter back in place
        if ev is not None:
            ev[1].record()
            self.finish_events.append(ev)
        self._inflight = []


def attach_reducer(module: torch.nn.Module, reducer: Optional[BucketedGradReducer]) -> None:
    """let the model's training engine feed `reducer` stage by stage during backward"""
    object.__setattr__(module, "_grad_reducer", reducer)


def sync_statistics(module: torch.nn.Module, enabled: bool = True, group=None, force: bool = False) -> None:
    """Large-batch-exact data parallelism: BatchNorm batch statistics (forward sums and the
    two backward sums per layer, [2C] floats each) and the per-slot counts / feature sums of the EMA codebook
    update are all-reduced across ranks, so N ranks x B clips reproduce ONE step on N*B clips (running statistics
    and codebook identical on every rank).  Ranks must hold equal batch sizes.  Off by default: the stock
    behaviour keeps statistics per rank.  `force`: take the collective path with a world of one as well (one-GPU test of
    the 33 collectives of a step over RCCL)."""
    object.__setattr__(module, "_sync_stats", (bool(enabled), group, bool(force)))
