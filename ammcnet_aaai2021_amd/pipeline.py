"""Input pipeline for the path: decoded frames / `.flo` files -> device-resident, normalised
sub-videos, one upload per frame.

The reference's `test_dataset` (Code/dataset/two_stream_dataset.py:491-539) decodes, resizes and normalises every
frame once per clip that contains it (5x for rgb, 4x for flow) on DataLoader workers, and ships fp32 clips
(3.4 MB per clip) through `.cuda()`.  Here a frame crosses PCIe once, as the raw decoded bytes (uint8 RGB at the
native resolution; the `.flo` payload as stored), and the resize / ToTensor / Normalize arithmetic runs on the GPU
(`csrc/pipeline.hip`).  Clips are then slices of the resident `[T, c, 256, 256]` tensors (`harness.score_batch`).

`SubVideoStager` overlaps the next sub-video's host read + H2D copy (pinned staging buffers, a side HIP stream, one
event per sub-video) with the scoring of the current one.  One stager per process = one loader shard per GPU.

Host-side decoding: `.flo` is parsed here (numpy); JPEG/PNG frames go through PIL when it is installed (the reference
uses TurboJPEG, `utils/img_process.py:6-19`); `.npy` frame stacks need nothing.
"""
from __future__ import annotations

import glob
import os
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

FLO_MAGIC = np.float32(202021.25)


def read_flo(path: str) -> np.ndarray:
    """Middlebury .flo -> float32 [h, w, 2] (the reference's `readFlow`, utils/flowlib.py:589-611); raises on a bad
    magic number instead of returning None"""
    with open(path, "rb") as f:
        head = np.fromfile(f, np.float32, count=1)
        if head.size != 1 or head[0] != FLO_MAGIC:
            raise ValueError(f"{path}: magic number incorrect, not a .flo file")
        wh = np.fromfile(f, np.int32, count=2)
        if wh.size != 2 or wh[0] <= 0 or wh[1] <= 0:
            raise ValueError(f"{path}: bad .flo header")
        w, h = int(wh[0]), int(wh[1])
        data = np.fromfile(f, np.float32, count=2 * w * h)
    if data.size != 2 * w * h:
        raise ValueError(f"{path}: truncated .flo payload")
    return data.reshape(h, w, 2)


def read_image(path: str) -> np.ndarray:
    """decoded RGB uint8 [h, w, 3]"""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{path}: expected uint8 [h, w, 3]")
        return a
    try:
        from PIL import Image
    except ImportError as e:                                    # pragma: no cover
        raise RuntimeError("decoding image files needs PIL; store frames as uint8 .npy instead") from e
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def list_subvideos(rgb_root: Optional[str], op_root: Optional[str]) -> List[Tuple[List[str], List[str]]]:
    """sorted sub-video folders, sorted files inside (test_helper.py:404-411, two_stream_dataset.py:515-518).  One root
    may be None (a single-stream set): the folders are those of the other root, and the missing kind's lists are empty."""
    out = []
    for name in sorted(os.listdir(rgb_root if rgb_root is not None else op_root)):
        frames = sorted(glob.glob(os.path.join(rgb_root, name, "*"))) if rgb_root is not None else []
        flows = sorted(glob.glob(os.path.join(op_root, name, "*"))) if op_root is not None else []
        out.append((frames, flows))
    return out


def frames_to_device(frames_u8: torch.Tensor, size: Tuple[int, int] = (256, 256), bgr: bool = False) -> torch.Tensor:
    """uint8 [T, h, w, 3] on the GPU -> float32 [T, 3, H, W] in [-1, 1] (`_load_frame` + ToTensor + Normalize)"""
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise _lib.AmmcHipError("frames_to_device: expected a uint8 [T, h, w, 3] GPU tensor (no CPU path)")
    frames_u8 = frames_u8.contiguous()
    t, h, w, _ = frames_u8.shape
    ow, oh = size
    out = torch.empty(t, 3, oh, ow, device=frames_u8.device, dtype=torch.float32)
    s = torch.cuda.current_stream(frames_u8.device).cuda_stream
    _lib.check(_lib.load().ammc_frames_u8_to_f32(frames_u8.data_ptr(), t, h, w, out.data_ptr(), oh, ow, int(bgr), s),
               "frames_u8_to_f32")
    return out


def flows_to_device(flows: torch.Tensor, size: Tuple[int, int] = (256, 256)) -> torch.Tensor:
    """float32 [T, h, w, 2] on the GPU -> float32 [T, 2, H, W] (`_load_op`)"""
    if not flows.is_cuda or flows.dtype != torch.float32 or flows.dim() != 4 or flows.shape[3] != 2:
        raise _lib.AmmcHipError("flows_to_device: expected a float32 [T, h, w, 2] GPU tensor (no CPU path)")
    flows = flows.contiguous()
    t, h, w, _ = flows.shape
    ow, oh = size
    out = torch.empty(t, 2, oh, ow, device=flows.device, dtype=torch.float32)
    s = torch.cuda.current_stream(flows.device).cuda_stream
    _lib.check(_lib.load().ammc_flows_to_f32(flows.data_ptr(), t, h, w, out.data_ptr(), oh, ow, s), "flows_to_f32")
    return out


def load_subvideo_host(frame_files: Sequence[str], flow_files: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """host side of one sub-video: decoded frames uint8 [T, h, w, 3], flows float32 [T', h, w, 2]"""
    frames = np.stack([read_image(p) for p in frame_files])
    flows = np.stack([read_flo(p) if p.endswith(".flo") else np.load(p).astype(np.float32) for p in flow_files])
    return frames, flows


class SubVideoStager:
    """Iterate device-resident (rgb [T,3,H,W], flow [T',2,H,W]) pairs; sub-video i+1 is read and copied to the GPU on a
    side stream while the caller works on sub-video i.

    `sources`: a sequence of callables returning (frames uint8 [T,h,w,3], flows float32 [T',h,w,2]) numpy arrays (or a
    list of (frame_files, flow_files) from `list_subvideos`); pinned uint8 / float32 tensors are uploaded from where they
    are.  `shard=(rank, world)` keeps every world-th sub-video; `ahead`: sub-videos staged beyond the current one.
    """

    def __init__(self, sources: Sequence, device, size: Tuple[int, int] = (256, 256), bgr: bool = False,
                 shard: Tuple[int, int] = (0, 1), ahead: int = 1, timed: bool = False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmmcHipError("SubVideoStager stages onto a GPU; there is no CPU pipeline")
        rank, world = shard
        self.sources = [s for i, s in enumerate(sources) if i % world == rank]
        self.size, self.bgr = size, bgr
        self.ahead = max(1, int(ahead))        # sub-videos staged beyond the one being scored
        self.timed, self.stage_events = bool(timed), []
        self.stream = torch.cuda.Stream(self.device)
        self.bytes_uploaded = 0
        self.host_seconds = 0.0        # file reads / decoding / pinning in the reader thread (overlapped with the GPU)

    def _host(self, src):
        import time
        t0 = time.perf_counter()
        frames, flows = src() if callable(src) else load_subvideo_host(*src)
        pf, po = self._pinned(frames, torch.uint8), self._pinned(flows, torch.float32)
        self.host_seconds += time.perf_counter() - t0
        return pf, po

    @staticmethod
    def _pinned(a, dtype) -> torch.Tensor:
        """page-locked host tensor of `a` (numpy array or tensor); a source that already hands out pinned tensors of the
        right type - a decoder writing into its own staging buffers - is taken as it is"""
        if isinstance(a, torch.Tensor):
            if a.dtype == dtype and a.is_contiguous() and a.is_pinned():
                return a
            return a.to(dtype).contiguous().pin_memory()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8 if dtype == torch.uint8 else np.float32)).pin_memory()

    def _reader(self, q):
        """background thread: file reads, decoding and pinning, one sub-video ahead of the GPU staging"""
        try:
            for src in self.sources:
                q.put(self._host(src))
        except BaseException as e:                               # surfaced in the consumer
            q.put(e)

    def _stage(self, host):
        """pinned buffers -> async H2D + the device kernels, all on the side stream"""
        pf, po = host
        self.bytes_uploaded += pf.numel() + 4 * po.numel()
        with torch.cuda.stream(self.stream):
            if self.timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.stream)
            df = pf.to(self.device, non_blocking=True)
            do = po.to(self.device, non_blocking=True)
            if self.timed:
                e1.record(self.stream)
            rgb = frames_to_device(df, self.size, self.bgr)
            op = flows_to_device(do, self.size)
            ev = torch.cuda.Event(enable_timing=self.timed)
            ev.record(self.stream)
            if self.timed:
                self.stage_events.append((e0, e1, ev))
        return rgb, op, ev, (pf, po, df, do)

    def stage_ms(self) -> Tuple[float, float]:
        """(copy, kernels) milliseconds summed over the staged sub-videos (`timed=True`; call after a device sync)"""
        return (sum(a.elapsed_time(b) for a, b, _ in self.stage_events), sum(b.elapsed_time(c) for _, b, c in self.stage_events))

    def __len__(self) -> int:
        return len(self.sources)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        import collections
        import queue
        import threading
        if not self.sources:
            return
        q: "queue.Queue" = queue.Queue(maxsize=1 + self.ahead)
        th = threading.Thread(target=self._reader, args=(q,), daemon=True)
        th.start()

        def take():
            item = q.get()
            if isinstance(item, BaseException):
                raise item
            return self._stage(item)

        # `ahead` sub-videos are staged (H2D + conversion kernels on the side stream) beyond the one handed out
        staged = collections.deque()
        taken = 0
        for i in range(len(self.sources)):
            while taken < len(self.sources) and len(staged) < 1 + self.ahead:
                staged.append(take())
                taken += 1
            rgb, op, ev, keep = staged.popleft()
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)                                    # the consumer's stream waits, not the host
            rgb.record_stream(cur)
            op.record_stream(cur)
            yield rgb, op
            del keep
        th.join()


# ---- training: the device-resident clip bank and the reference's draw rule ------------------------------------------

class ClipSampler:
    """The reference's training draw (`TwoStream_Train_DS.__getitem__`, two_stream_dataset.py:467-468, over
    `clip_Train_DS.__getitem__`, :289-292) as it runs with `num_workers=0`: one `np.random.RandomState(seed)` (the
    module-level `rng = RandomState(2017)` of :31) and, per sample, in this order:

      1. rgb: `vid = randint(0, n_rgb_videos)`, then `start = randint(0, len(vid) - rgb_len)`;
      2. op:  `vid = randint(0, n_op_videos)`,  then `start = randint(0, len(vid) - op_len)`.

    Two quirks of the reference are kept as it runs them: the rgb and op clips of a sample are drawn INDEPENDENTLY (other
    videos, other starts), and the upper bound of `randint` is exclusive, so a video's last clip (start len - clip_len) is
    never drawn.  One artefact is NOT reproduced: the reference trains with 16 DataLoader workers, each a fork that copies
    the module-level RNG, so the workers' draw streams repeat each other; here one stream feeds every sample.

    `rgb_lens` / `op_lens`: frames per sub-video of each folder (sorted order).  `draw(b)` returns the four int arrays
    (rgb video, rgb start, op video, op start)."""

    def __init__(self, rgb_lens: Sequence[int], op_lens: Sequence[int], rgb_len: int = 5, op_len: int = 4,
                 seed: int = 2017):
        self.rgb_lens, self.op_lens = [int(n) for n in rgb_lens], [int(n) for n in op_lens]
        self.rgb_len, self.op_len = int(rgb_len), int(op_len)
        if not self.rgb_lens or not self.op_lens:
            raise ValueError("ClipSampler: no sub-videos")
        for what, lens, clip in (("rgb", self.rgb_lens, self.rgb_len), ("op", self.op_lens, self.op_len)):
            short = [i for i, n in enumerate(lens) if n <= clip]
            if short:
                raise ValueError(f"ClipSampler: {what} sub-videos {short} have <= {clip} frames: the draw rule needs "
                                 f"at least {clip + 1}")
        self.rng = np.random.RandomState(seed)

    def draw(self, batch: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        out = np.empty((4, batch), np.int64)
        r = self.rng
        for i in range(batch):
            v = r.randint(0, len(self.rgb_lens))
            out[0, i], out[1, i] = v, r.randint(0, self.rgb_lens[v] - self.rgb_len)
            v = r.randint(0, len(self.op_lens))
            out[2, i], out[3, i] = v, r.randint(0, self.op_lens[v] - self.op_len)
        return out[0], out[1], out[2], out[3]

    def get_state(self) -> dict:
        """the RNG state as plain values and a tensor (loadable with `torch.load(weights_only=True)`)"""
        name, keys, pos, has_gauss, cached = self.rng.get_state()
        return {"name": name, "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}

    def set_state(self, st: dict) -> None:
        keys = st["keys"].numpy() if isinstance(st["keys"], torch.Tensor) else np.asarray(st["keys"])
        self.rng.set_state((st["name"], keys.astype(np.uint32), int(st["pos"]), int(st["has_gauss"]),
                            float(st["cached_gaussian"])))


class SingleClipSampler:
    """The draw of one stream trained on its own (stage 1 of the reference's recipe: `clip_Train_DS.__getitem__`,
    two_stream_dataset.py:287-333, behind `train_single_Helper`): one `np.random.RandomState(seed)` and, per sample,
    `vid = randint(0, n_videos)`, then `start = randint(0, len(vid) - clip_len)` - the exclusive upper bound kept, as in
    `ClipSampler`.  `draw(b)` returns (video, start) int arrays; `get_state` / `set_state` as `ClipSampler`'s."""

    def __init__(self, lens: Sequence[int], clip_len: int, seed: int = 2017, what: str = "clip"):
        self.lens, self.clip_len = [int(n) for n in lens], int(clip_len)
        if not self.lens:
            raise ValueError("SingleClipSampler: no sub-videos")
        short = [i for i, n in enumerate(self.lens) if n <= self.clip_len]
        if short:
            raise ValueError(f"SingleClipSampler: {what} sub-videos {short} have <= {self.clip_len} frames: the draw rule "
                             f"needs at least {self.clip_len + 1}")
        self.rng = np.random.RandomState(seed)

    def draw(self, batch: int) -> Tuple[np.ndarray, np.ndarray]:
        out = np.empty((2, batch), np.int64)
        r = self.rng
        for i in range(batch):
            v = r.randint(0, len(self.lens))
            out[0, i], out[1, i] = v, r.randint(0, self.lens[v] - self.clip_len)
        return out[0], out[1]

    get_state = ClipSampler.get_state
    set_state = ClipSampler.set_state


def _size_wh(size) -> Tuple[int, int]:
    """`size` as (width, height): an int is a square"""
    if isinstance(size, int):
        return size, size
    w, h = size
    return int(w), int(h)


def bank_bytes(n_rgb_frames: int, n_op_frames: int, size) -> int:
    """device bytes of a ClipBank: uint8 [N][3][H][W] + float32 [N'][H][W]"""
    w, h = _size_wh(size)
    return n_rgb_frames * 3 * h * w + n_op_frames * 4 * h * w


def bank_tiers(n_rgb: int, n_op: int, size, device_bytes: float, host_bytes: float) -> Tuple[int, int]:
    """(n_rgb_dev, n_op_dev): how many leading frames of each kind of a two-tier ClipBank live in device memory, the
    rest in pinned host memory.  Both kinds keep the same fraction on the device (a clip of either kind is then as likely
    to come from the host tier), and the split is the largest that fits: the proportional share rounded down, then
    single frames added - to the kind whose device fraction is the lower - while one still fits `device_bytes`.
    Raises AmmcHipError when what is left over exceeds `host_bytes`."""
    w, h = _size_wh(size)
    cost = {"rgb": 3 * h * w, "op": 4 * h * w}
    total = {"rgb": int(n_rgb), "op": int(n_op)}
    all_bytes = bank_bytes(n_rgb, n_op, size)
    if all_bytes <= device_bytes:
        return total["rgb"], total["op"]
    frac = max(0.0, float(device_bytes)) / all_bytes
    dev = {k: min(total[k], int(total[k] * frac)) for k in total}
    used = sum(dev[k] * cost[k] for k in dev)
    while used > device_bytes:                                # (float rounding of the share: never more than a frame)
        k = max(dev, key=lambda k: dev[k])
        dev[k] -= 1
        used -= cost[k]
    while True:
        open_ = sorted((k for k in dev if dev[k] < total[k] and used + cost[k] <= device_bytes),
                       key=lambda k: dev[k] / total[k])
        if not open_:
            break
        dev[open_[0]] += 1
        used += cost[open_[0]]
    rest = all_bytes - used
    if rest > host_bytes:
        raise _lib.AmmcHipError(
            f"ClipBank: {n_rgb} frames + {n_op} flows at {w}x{h} need {all_bytes / 1e9:.2f} GB; {used / 1e9:.2f} GB fit the "
            f"device budget of {device_bytes / 1e9:.2f} GB and the remaining {rest / 1e9:.2f} GB exceed the host budget of "
            f"{host_bytes / 1e9:.2f} GB")
    return dev["rgb"], dev["op"]


class ClipBank:
    """Every frame of a training set, decoded once and resized once into device memory; each iteration's clips gathered
    from it by one launch (`csrc/clip_bank.hip`), bit-identical to `frames_to_device` / `flows_to_device`.

    Layout: `rgb` uint8 [N][3][H][W] holds the 8-bit resize result (the normalised float is a function of it alone, a
    quarter of the bytes); `op` float32 [N'][H][W] holds channel 0 of `_load_op` (`u / H`), channel 1 (`c0 / W`) is
    derived at gather time.  Sub-video v occupies frames [rgb_start[v], rgb_start[v] + rgb_count[v]) (op likewise);
    `gather` takes GLOBAL first-frame indices and validates every one of them on the host (a clip never crosses a
    sub-video) before anything is launched.

    Filling: sub-videos from `list_subvideos` (sorted); the bank size is estimated from the file counts and the fill
    refused BEFORE anything is decoded when it exceeds `budget_gb` (default: 80 % of the device's free memory).  Frames
    are decoded by a pool of `workers` threads (PIL releases the GIL) into pinned staging buffers (two, alternating,
    each guarded by an event so it is not rewritten before its copy ran), copied to the device at their native
    resolution (which may differ between sub-videos) and resized into the sub-video's slice on a side stream.
    `fill_seconds`: wall time of the whole fill.

    One kind (a single-stream training stage): `rgb_root=None` or `op_root=None`.  Such a bank decodes, uploads and
    budgets only its kind (the other bank is None), `global_index(vid, start)` and `gather(first)` take and return that
    kind alone, and the gather is one launch of `ammc_gather_clips_one`, bit-identical to the matching half of the
    two-kind gather.  `kinds`: ("rgb", "op"), ("rgb",) or ("op",).

    Two tiers: with `host_budget_gb` > 0 a set that exceeds the device budget is not refused; `bank_tiers` keeps the
    leading `n_rgb_dev` / `n_op_dev` frames in device memory (`rgb`, `op`) and the rest goes to ONE pinned host tensor
    per kind (`rgb_host`, `op_host`), both tiers budgeted before anything is decoded.  A sub-video that reaches the host
    tier is resized on the device into a bounce buffer (sized for the largest sub-video, released after the fill) and
    copied from there into its slices on the fill stream; it may straddle the split.  Indices stay global, and the gather
    is one launch of `ammc_gather_clips_tiered`, which reads the host tier through the host link and is bit-identical
    to the all-device gather.  `device_nbytes` / `host_nbytes` (`nbytes` stays their sum); with `host_budget_gb=0`, or
    when everything fits the device, nothing changes: no host tier, the same two kernels.

    `prefetch(*first)` enqueues a gather on a stream the bank owns, behind everything already enqueued on the current
    stream; the next `gather` with the same indices hands out its tensors (the current stream waits on the prefetch's
    event, the host does not); a `gather` with other indices drops it."""

    def __init__(self, rgb_root: Optional[str], op_root: Optional[str], size, device, workers: int = 8,
                 budget_gb: Optional[float] = None, rgb_len: int = 5, op_len: int = 4, bgr: bool = False,
                 host_budget_gb: float = 0.0):
        import time
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmmcHipError("ClipBank lives on a GPU; there is no CPU pipeline")
        self.width, self.height = _size_wh(size)
        if (self.width * self.height) % 4:
            raise _lib.AmmcHipError(f"ClipBank: {self.width}x{self.height} frames: the gather needs H * W % 4 == 0")
        self.rgb_len, self.op_len, self.bgr, self.workers = int(rgb_len), int(op_len), bool(bgr), max(1, int(workers))
        if rgb_root is None and op_root is None:
            raise ValueError("ClipBank: needs rgb_root, op_root or both")
        self.kinds = tuple(k for k, root in (("rgb", rgb_root), ("op", op_root)) if root is not None)
        self.videos = list_subvideos(rgb_root, op_root)
        if not self.videos:
            raise ValueError(f"ClipBank: no sub-video folders under {rgb_root if rgb_root is not None else op_root}")
        self.rgb_count = np.array([len(f) for f, _ in self.videos], np.int64)
        self.op_count = np.array([len(o) for _, o in self.videos], np.int64)
        self.rgb_start = np.concatenate([[0], np.cumsum(self.rgb_count)[:-1]]).astype(np.int64)
        self.op_start = np.concatenate([[0], np.cumsum(self.op_count)[:-1]]).astype(np.int64)
        self.n_rgb, self.n_op = int(self.rgb_count.sum()), int(self.op_count.sum())
        self.nbytes = bank_bytes(self.n_rgb, self.n_op, (self.width, self.height))
        if budget_gb is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            budget, whose = 0.8 * free, f"80 % of the {free / 1e9:.2f} GB free on {self.device}"
        else:
            budget, whose = float(budget_gb) * 1e9, f"the budget of {float(budget_gb):.2f} GB"
        self.n_rgb_dev, self.n_op_dev = self.n_rgb, self.n_op
        if self.nbytes > budget and float(host_budget_gb) > 0:
            self.n_rgb_dev, self.n_op_dev = bank_tiers(self.n_rgb, self.n_op, (self.width, self.height), budget,
                                                       float(host_budget_gb) * 1e9)
        elif self.nbytes > budget:
            raise _lib.AmmcHipError(
                f"ClipBank: {self.n_rgb} frames + {self.n_op} flows at {self.width}x{self.height} need "
                f"{self.nbytes / 1e9:.2f} GB of device memory, more than {whose}")
        if max(self.n_rgb, self.n_op) >= 2**31:
            raise _lib.AmmcHipError("ClipBank: more than 2^31 frames (the gather's indices are int32)")
        self.device_nbytes = bank_bytes(self.n_rgb_dev, self.n_op_dev, (self.width, self.height))
        self.host_nbytes = self.nbytes - self.device_nbytes
        t0 = time.perf_counter()
        self.rgb = self.op = self.rgb_host = self.op_host = None
        if self.host_nbytes == 0:
            if "rgb" in self.kinds:
                self.rgb = torch.empty(self.n_rgb, 3, self.height, self.width, dtype=torch.uint8, device=self.device)
            if "op" in self.kinds:
                self.op = torch.empty(max(self.n_op, 1), self.height, self.width, dtype=torch.float32, device=self.device)
        else:
            if "rgb" in self.kinds:
                self.rgb = torch.empty(self.n_rgb_dev, 3, self.height, self.width, dtype=torch.uint8, device=self.device)
                self.rgb_host = torch.empty(self.n_rgb - self.n_rgb_dev, 3, self.height, self.width, dtype=torch.uint8,
                                            pin_memory=True)
            if "op" in self.kinds:
                self.op = torch.empty(self.n_op_dev, self.height, self.width, dtype=torch.float32, device=self.device)
                self.op_host = torch.empty(self.n_op - self.n_op_dev, self.height, self.width, dtype=torch.float32,
                                           pin_memory=True)
        self._fill()
        self.fill_seconds = time.perf_counter() - t0
        self._prefetch_stream = None                          # made by the first `prefetch`
        self._prefetched = None                               # (index rows, output tensors, event)
        self._idx_pinned = [torch.empty(0, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._idx_events = [None, None]
        self._idx_turn = 0

    # -- fill ----------------------------------------------------------------------------------------------------------

    def _fill(self) -> None:
        from concurrent.futures import ThreadPoolExecutor
        stream = torch.cuda.Stream(self.device)
        staging = {}                                          # (kind, slot) -> (pinned tensor, event of its last copy)
        lib = _lib.load()

        def stage(kind, slot, shape, dtype):
            buf, ev = staging.get((kind, slot), (None, None))
            if ev is not None:
                ev.synchronize()                              # its previous copy has run: the buffer may be rewritten
            n = int(np.prod(shape))
            if buf is None or buf.numel() < n:
                buf = torch.empty(n, dtype=dtype).pin_memory()
            staging[(kind, slot)] = (buf, None)
            return buf[:n].view(*shape)

        def upload(kind, slot, host):
            with torch.cuda.stream(stream):
                dev = host.to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
            staging[(kind, slot)] = (staging[(kind, slot)][0], ev)
            return dev

        # the resize's destination: the sub-video's slice of the device tier, or - for a sub-video that reaches the host
        # tier - a device bounce buffer whose parts then go to their tiers (`settle`), all in the fill stream's order
        n_dev = {"rgb": self.n_rgb_dev, "op": self.n_op_dev}
        tiers = {"rgb": (self.rgb, self.rgb_host), "op": (self.op, self.op_host)}
        bounce = {}
        for kind, starts, counts in (("rgb", self.rgb_start, self.rgb_count), ("op", self.op_start, self.op_count)):
            reach = counts[starts + counts > n_dev[kind]] if self.host_nbytes and kind in self.kinds else []
            if len(reach):
                bounce[kind] = torch.empty(int(max(reach)), *tiers[kind][0].shape[1:], dtype=tiers[kind][0].dtype,
                                           device=self.device)

        def dest(kind, s0, cnt):
            return tiers[kind][0][s0] if s0 + cnt <= n_dev[kind] else bounce[kind]

        def settle(kind, s0, cnt):
            split = n_dev[kind]
            if s0 + cnt <= split:
                return
            dev, host = tiers[kind]
            k = max(0, split - s0)                            # leading frames of the sub-video that stay on the device
            with torch.cuda.stream(stream):
                if k:
                    dev[s0:split].copy_(bounce[kind][:k], non_blocking=True)
                host[s0 + k - split:s0 + cnt - split].copy_(bounce[kind][k:cnt], non_blocking=True)

        with ThreadPoolExecutor(self.workers) as pool:
            for v, (frames, flows) in enumerate(self.videos):
                slot = v % 2
                if frames:
                    imgs = list(pool.map(read_image, frames))
                    h, w = imgs[0].shape[:2]
                    if any(im.shape != (h, w, 3) for im in imgs):
                        raise ValueError(f"ClipBank: frames of different sizes in {os.path.dirname(frames[0])}")
                    host = stage("rgb", slot, (len(imgs), h, w, 3), torch.uint8)
                    pool_np = host.numpy()
                    for i, im in enumerate(imgs):
                        pool_np[i] = im
                    dev = upload("rgb", slot, host)
                    s0 = int(self.rgb_start[v])
                    with torch.cuda.stream(stream):
                        _lib.check(lib.ammc_frames_u8_resize_u8(dev.data_ptr(), len(imgs), h, w,
                                                                dest("rgb", s0, len(imgs)).data_ptr(),
                                                                self.height, self.width, int(self.bgr), stream.cuda_stream),
                                   "frames_u8_resize_u8")
                        dev.record_stream(stream)
                    settle("rgb", s0, len(imgs))
                if flows:
                    fls = list(pool.map(_read_flow_file, flows))
                    h, w = fls[0].shape[:2]
                    if any(f.shape != (h, w, 2) for f in fls):
                        raise ValueError(f"ClipBank: flows of different sizes in {os.path.dirname(flows[0])}")
                    host = stage("op", slot, (len(fls), h, w, 2), torch.float32)
                    pool_np = host.numpy()
                    for i, f in enumerate(fls):
                        pool_np[i] = f
                    dev = upload("op", slot, host)
                    s0 = int(self.op_start[v])
                    with torch.cuda.stream(stream):
                        _lib.check(lib.ammc_flows_resize_c0(dev.data_ptr(), len(fls), h, w,
                                                            dest("op", s0, len(fls)).data_ptr(),
                                                            self.height, self.width, stream.cuda_stream), "flows_resize_c0")
                        dev.record_stream(stream)
                    settle("op", s0, len(fls))
        stream.synchronize()
        torch.cuda.current_stream(self.device).wait_stream(stream)
        bounce.clear()                                        # the fill is over (synchronised): the buffers go back

    # -- gather --------------------------------------------------------------------------------------------------------

    def _single(self) -> Optional[str]:
        return self.kinds[0] if len(self.kinds) == 1 else None

    def global_index(self, *pairs):
        """(sub-video, start) pairs (`ClipSampler.draw`) -> global first-frame indices of the banks; a one-kind bank takes
        the (video, start) of `SingleClipSampler.draw` and returns one array"""
        one = self._single()
        if one is not None:
            vid, start = pairs
            return (self.rgb_start if one == "rgb" else self.op_start)[np.asarray(vid)] + np.asarray(start)
        rgb_vid, rgb_start, op_vid, op_start = pairs
        return (self.rgb_start[np.asarray(rgb_vid)] + np.asarray(rgb_start),
                self.op_start[np.asarray(op_vid)] + np.asarray(op_start))

    def validate(self, rgb_first, op_first) -> Tuple[np.ndarray, np.ndarray]:
        """host check of every index (`check_clip_indices`); raises AmmcHipError"""
        if self._single() is not None:
            raise _lib.AmmcHipError(f"ClipBank: a {self._single()}-only bank has no clips of the other kind")
        rf = check_clip_indices("rgb", rgb_first, self.rgb_start, self.rgb_count, self.rgb_len)
        of = check_clip_indices("op", op_first, self.op_start, self.op_count, self.op_len)
        if rf.size != of.size or rf.size == 0:
            raise _lib.AmmcHipError("ClipBank.gather: need as many (>= 1) rgb as op indices")
        return rf, of

    def _indices_to_device(self, rows) -> torch.Tensor:
        """validated host index rows -> device int32 [len(rows), B] on the current stream, through one of two pinned
        buffers (event-guarded)"""
        n, b = len(rows), rows[0].size
        k = self._idx_turn
        self._idx_turn ^= 1
        if self._idx_events[k] is not None:
            self._idx_events[k].synchronize()                 # the copy that last read this buffer has run
        if self._idx_pinned[k].numel() < n * b:
            self._idx_pinned[k] = torch.empty(n * b, dtype=torch.int32).pin_memory()
        host = self._idx_pinned[k][:n * b].view(n, b)
        hn = host.numpy()
        for i, r in enumerate(rows):
            hn[i] = r
        stream = torch.cuda.current_stream(self.device)
        idx = torch.empty(n, b, dtype=torch.int32, device=self.device)
        idx.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        self._idx_events[k] = ev
        return idx

    def _checked(self, first) -> Tuple[np.ndarray, ...]:
        """the validated int64 index rows of a gather: (rgb, op), or the one row of a one-kind bank"""
        one = self._single()
        if one is None:
            return self.validate(*first)
        if len(first) != 1:
            raise TypeError(f"ClipBank.gather: a {one}-only bank takes one index array, got {len(first)}")
        first = first[0]
        starts, counts, clip = (self.rgb_start, self.rgb_count, self.rgb_len) if one == "rgb" else \
            (self.op_start, self.op_count, self.op_len)
        f = check_clip_indices(one, first, starts, counts, clip)
        if f.size == 0:
            raise _lib.AmmcHipError("ClipBank.gather: need >= 1 index")
        return (f,)

    def _gather_tiered(self, rows):
        """one launch of `ammc_gather_clips_tiered` on the current stream; returns what `gather` returns"""
        one = self._single()
        b = rows[0].size
        idx = self._indices_to_device(rows)
        stream = torch.cuda.current_stream(self.device)
        rgb = op = None
        if one != "op":
            rgb = torch.empty(b, self.rgb_len, 3, self.height, self.width, dtype=torch.float32, device=self.device)
        if one != "rgb":
            op = torch.empty(b, self.op_len, 2, self.height, self.width, dtype=torch.float32, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        _lib.check(_lib.load().ammc_gather_clips_tiered(
            ptr(self.rgb), ptr(self.rgb_host), self.n_rgb_dev, self.n_rgb, ptr(self.op), ptr(self.op_host), self.n_op_dev,
            self.n_op, idx[0].data_ptr() if rgb is not None else None, idx[-1].data_ptr() if op is not None else None, b,
            self.rgb_len, self.op_len, self.height, self.width, ptr(rgb), ptr(op), stream.cuda_stream), "gather_clips_tiered")
        return (rgb, op) if one is None else (rgb if one == "rgb" else op)

    def _gather_rows(self, rows):
        if self.host_nbytes:
            return self._gather_tiered(rows)
        return self._gather_one(self._single(), rows[0]) if self._single() is not None else self._gather_two(*rows)

    def prefetch(self, *first) -> None:
        """Enqueue the gather of `first` (as `gather` takes them, validated here) on the bank's own stream, which first
        waits for everything already enqueued on the current stream, and record an event behind it.  The next `gather`
        with the same indices returns these tensors.  They are fresh tensors of the bank's stream, handed to the
        consumer's stream with `record_stream`: nothing a consumer may still read is ever rewritten."""
        rows = self._checked(first)
        if self._prefetch_stream is None:
            self._prefetch_stream = torch.cuda.Stream(self.device)
        side = self._prefetch_stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            out = self._gather_rows(rows)
            ev = torch.cuda.Event()
            ev.record(side)
        self._prefetched = (rows, out, ev)

    def gather(self, *first):
        """host int arrays of global first frames -> (rgb float32 [B, rgb_len, 3, H, W], op float32 [B, op_len, 2, H, W])
        on the current stream: the indices go H2D through one of two pinned buffers (event-guarded), then one launch.
        A one-kind bank: `gather(first)` -> that kind's clips alone (`ammc_gather_clips_one`).  After a `prefetch` of
        the same indices: its tensors, once the current stream has waited on its event."""
        rows = self._checked(first)
        pre, self._prefetched = self._prefetched, None
        if pre is not None and len(pre[0]) == len(rows) and all(np.array_equal(a, b) for a, b in zip(pre[0], rows)):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(pre[2])
            for t in (pre[1] if isinstance(pre[1], tuple) else (pre[1],)):
                t.record_stream(cur)
            return pre[1]
        return self._gather_rows(rows)

    def _gather_two(self, rf, of):
        b = rf.size
        idx = self._indices_to_device((rf, of))
        stream = torch.cuda.current_stream(self.device)
        rgb = torch.empty(b, self.rgb_len, 3, self.height, self.width, dtype=torch.float32, device=self.device)
        op = torch.empty(b, self.op_len, 2, self.height, self.width, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ammc_gather_clips(self.rgb.data_ptr(), self.n_rgb, self.op.data_ptr(), self.n_op,
                                                 idx[0].data_ptr(), idx[1].data_ptr(), b, self.rgb_len, self.op_len,
                                                 self.height, self.width, rgb.data_ptr(), op.data_ptr(), stream.cuda_stream),
                   "gather_clips")
        return rgb, op

    def _gather_one(self, kind: str, f: np.ndarray) -> torch.Tensor:
        rgb = kind == "rgb"
        clip, n, bank = (self.rgb_len, self.n_rgb, self.rgb) if rgb else (self.op_len, self.n_op, self.op)
        idx = self._indices_to_device((f,))
        stream = torch.cuda.current_stream(self.device)
        out = torch.empty(f.size, clip, 3 if rgb else 2, self.height, self.width, dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().ammc_gather_clips_one(bank.data_ptr(), n, 0 if rgb else 1, idx[0].data_ptr(), f.size, clip,
                                                     self.height, self.width, out.data_ptr(), stream.cuda_stream),
                   "gather_clips_one")
        return out


def check_clip_indices(what: str, first, starts: np.ndarray, counts: np.ndarray, clip: int) -> np.ndarray:
    """global first-frame indices of clips of `clip` frames in a bank whose sub-video v holds frames
    [starts[v], starts[v] + counts[v]): every clip must start inside a sub-video and end inside THE SAME one; returns
    them as int64, raises AmmcHipError naming the first bad clip"""
    a = np.asarray(first).reshape(-1)
    if a.dtype.kind not in "iu":
        raise _lib.AmmcHipError(f"ClipBank.gather: {what} indices must be integers, got {a.dtype}")
    a = a.astype(np.int64)
    v = np.searchsorted(starts, a, side="right") - 1
    vc = np.clip(v, 0, len(starts) - 1)
    ok = (a >= 0) & (v >= 0) & (a + clip <= starts[vc] + counts[vc])
    if not ok.all():
        bad = int(np.flatnonzero(~ok)[0])
        raise _lib.AmmcHipError(f"ClipBank.gather: {what} clip {bad} (first frame {int(a[bad])}, {clip} frames) does not "
                                f"lie inside one sub-video of the bank")
    return a


def _read_flow_file(p: str) -> np.ndarray:
    return read_flo(p) if p.endswith(".flo") else np.load(p).astype(np.float32)
