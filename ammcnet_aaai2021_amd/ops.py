"""Stand-alone forwards of the path's building blocks (NCHW in, NCHW out).

The whole-model forwards run on the cached plans of `engine.EvalEngine`; these
functions run ONE block on freshly allocated buffers through the same C-ABI
kernels, so that `double_conv(...)`, `down(...)`, `up(...)`, `bridge(...)`,
`Quantize_topk(...)` and the vq block work when called on their own, exactly
as the reference's sub-modules do, and so that every kernel has a per-op
parity test (tests/test_gpu_parity.py, tests/test_gpu_s16.py).  No ATen compute here either.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import ACT_NONE
from .engine import Act, Plan, _Builder, _DoubleConvPack, _Packer, _ptr


def _need_cuda(x: torch.Tensor):
    if not x.is_cuda:
        raise _lib.AmmcHipError("the HIP path needs tensors on the GPU; there is no CPU fallback")


def _stream(x) -> int:
    return torch.cuda.current_stream(x.device).cuda_stream


# ---- what the ops with an `out=` table, a workspace or a (num, den) pair share ----------------

_workspaces: dict = {}       # (name, device index, stream handle) -> the cached workspace


def _workspace(name: str, dev: torch.device, n: int, dtype, stream: int) -> torch.Tensor:
    """at least `n` elements of `dtype` for the op family `name`, cached per (name, device index, stream): launches on
    one stream run in order, so two calls never use it at once; it only grows"""
    key = (name, dev.index if dev.index is not None else torch.cuda.current_device(), stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < n:
        _workspaces.pop(key, None)                            # (let the smaller one go before its successor is allocated)
        ws = _workspaces[key] = torch.empty(n, device=dev, dtype=dtype)
    return ws


def _bs(t: torch.Tensor, n: int) -> int:
    """the batch stride of [B, ...] with samples of n elements: a dimension of size 1 may carry any stride in torch"""
    return max(t.stride(0), n) if t.shape[0] == 1 else t.stride(0)


def _slots(what: str, out, dev, B: int, want: dict, strided=(), single: bool = False):
    """The `out=` table of an op.  `want` = {key: (shape, dtype)}, every shape [B, ...]; `out`: the caller's tensors by
    those keys, or None (`single`: the op's one `out` tensor, which stands for a table of `want`'s one entry).  An unknown
    key is refused, an absent slot allocated, a given one must be `dtype` `shape` on `dev` and contiguous - or, for the
    slots `strided` names (those whose batch stride the kernel takes), have contiguous samples and with B > 1 a batch
    stride of at least the sample's size.
    -> ({key: tensor} in `want`'s order, {key: batch stride in elements} of the strided slots)"""
    if single:
        out = None if out is None else dict.fromkeys(want, out)
    elif out and not out.keys() <= want.keys():
        raise ValueError(f"{what}: `out` has no slot {sorted(set(out) - set(want))}")
    res, bs = {}, {}
    for key, (shape, dtype) in want.items():
        t, why = out.get(key) if out else None, None
        if t is None:
            t = torch.empty(shape, device=dev, dtype=dtype)
        elif not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev:
            why = f"must be {dtype} {shape} on {dev}"
        elif not t.is_contiguous() and (key not in strided or not t[0].is_contiguous()
                                        or (B > 1 and t.stride(0) < math.prod(shape[1:]))):
            why = "must be contiguous" if key not in strided else "must have contiguous samples and a batch stride >= a sample's size"
        if why:
            raise ValueError(f"{what}: {'out' if single else f'out[{key!r}]'} {why}")
        res[key] = t
        if key in strided:
            bs[key] = _bs(t, math.prod(shape[1:]))
    return res, bs


def _pair(what: str, name: str, v, top: int):
    """(num, den) with 1 <= num <= den <= top"""
    try:
        num, den = (int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a pair (num, den), got {v!r}") from None
    if not 1 <= num <= den <= top:
        raise ValueError(f"{what}: 1 <= num <= den <= {top}, got {v!r}")
    return num, den


def _to_halo(bld: _Builder, x: torch.Tensor, cp: int | None = None, into: Act | None = None) -> Act:
    """NCHW tensor -> halo-padded NHWC activation (optionally a channel slice of a wider buffer)"""
    B, C, H, W = x.shape
    cp = cp or (C + 3) // 4 * 4
    a = into if into is not None else bld.act(B, H, W, cp)
    x = x.detach().float().contiguous()
    bld.plan.keep.append(x)
    bld.plan.add(bld.lib.ammc_nchw_to_nhwc_f32, _ptr(x), B, C, H, W, a.pix0(), *a.strides, cp, name="to_nhwc")
    return a


def _to_nchw(bld: _Builder, a: Act) -> torch.Tensor:
    y = torch.empty((a.B, a.c, a.H, a.W), device=a.buf.device, dtype=torch.float32)
    bld.plan.add(bld.lib.ammc_nhwc_to_nchw_f32, a.pix0(), *a.strides, a.B, a.c, a.H, a.W, _ptr(y), name="to_nchw")
    return y


def double_conv_eval(dc, x: torch.Tensor, pool_first: bool = False, residual: torch.Tensor | None = None):
    """`double_conv.forward` / `down.forward` / one half of `bridge.forward` in eval mode"""
    _need_cuda(x)
    plan = Plan()
    bld = _Builder(plan, x.device)
    pack = _DoubleConvPack(_Packer(x.device), dc)
    a = _to_halo(bld, x, pack.cin_p)
    if pool_first:
        p = bld.act(a.B, a.H // 2, a.W // 2, a.c)
        bld.maxpool(a, p)
        a = p
    mid = bld.act(a.B, a.H, a.W, pack.cout)
    out = bld.act(a.B, a.H, a.W, pack.cout)
    res = _to_halo(bld, residual) if residual is not None else None
    bld.double_conv(a, pack, mid, out, res=res)
    y = _to_nchw(bld, out)
    plan.run(_stream(x))
    return y


def up_eval(upm, x1: torch.Tensor, x2: torch.Tensor):
    """`up.forward`: ConvTranspose into the second half of the concat buffer, skip into the first"""
    _need_cuda(x1)
    dy, dx = x2.shape[2] - 2 * x1.shape[2], x2.shape[3] - 2 * x1.shape[3]
    if dy not in (0, 1) or dx not in (0, 1):
        raise ValueError("up: the skip tensor must be 2x the upsampled one, or one row / column more (what MaxPool2d(2) "
                         "leaves of an odd level; `up.forward` pads that row / column with zeros, unet.py:53-56)")
    plan = Plan()
    bld = _Builder(plan, x1.device)
    pk = _Packer(x1.device)
    c = x2.shape[1]
    B, _, H, W = x2.shape
    cat = bld.act(B, H, W, 2 * c)
    _to_halo(bld, x2, into=cat.slice(0, c))          # the skip tensor: channels [0, c)
    a = _to_halo(bld, x1)
    bld.convt(a, pk.convt(upm.up.weight), upm.up.bias.detach(), cat.slice(c, c))
    pack = _DoubleConvPack(pk, upm.conv)
    mid = bld.act(B, H, W, pack.cout)
    out = bld.act(B, H, W, pack.cout)
    bld.double_conv(cat, pack, mid, out)
    y = _to_nchw(bld, out)
    plan.run(_stream(x1))
    return y


def quantize_topk_eval(qmod, x: torch.Tensor):
    """`Quantize_topk.forward` in eval mode on an NHWC tensor [B,h,w,D]"""
    _need_cuda(x)
    lib = _lib.load()
    B, h, w, d = x.shape
    n, m, k = B * h * w, qmod.n_embed, qmod.k
    x = x.detach().float().contiguous()
    e_md, enorm = _Packer(x.device).codebook(qmod.embed)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    qk = torch.empty((B, h, w, k * d), device=x.device, dtype=torch.float32)
    q1 = torch.empty((B, h, w, d), device=x.device, dtype=torch.float32)
    nblk = lib.ammc_memory_topk_blocks(n)
    part = torch.empty(nblk, device=x.device, dtype=torch.float32)
    diff = torch.empty(1, device=x.device, dtype=torch.float32)
    s = _stream(x)
    _lib.check(lib.ammc_memory_topk_fwd_f32(_ptr(x), _ptr(qmod.embed), _ptr(e_md), _ptr(enorm), n, d, m, k,
                                            idx.data_ptr(), _ptr(qk), _ptr(q1), _ptr(part), s), "memory_topk")
    _lib.check(lib.ammc_sum_partials_f32(_ptr(part), nblk, 1.0 / float(n * d), _ptr(diff), s), "sum_partials")
    qmod.last_indices = idx.view(B, h, w, k)
    return qk, diff[0], q1


def vq_block_eval(quan, x: torch.Tensor, residual: bool):
    """`enc_quan_dec_topk.forward` (+ `out += x` of enc_quan_dec_res_topk) in eval mode"""
    _need_cuda(x)
    plan = Plan()
    bld = _Builder(plan, x.device)
    pk = _Packer(x.device)
    lib = bld.lib
    a = _to_halo(bld, x)
    B, H, W = a.B, a.H, a.W
    q = quan.quantize
    d, m, k = q.dim, q.n_embed, q.k
    n = B * H * W
    enc_w, _ = pk.conv(quan.enc.weight, 1)
    dec_w, _ = pk.conv(quan.dec.weight, 1)
    e_md, enorm = pk.codebook(q.embed)
    z = bld.act(B, H, W, d, halo=0)
    bld.conv(a, enc_w, z, ntaps=1, cin=a.c, n=d, shift=quan.enc.bias.detach(), name="enc")
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    qk = bld.act(B, H, W, k * d, halo=0)
    q1 = bld.buf(B, H, W, d)
    nblk = lib.ammc_memory_topk_blocks(n)
    part = bld.buf(nblk)
    diff = bld.buf(1)
    plan.keep.extend([idx, e_md, enorm])
    plan.add(lib.ammc_memory_topk_fwd_f32, _ptr(z.buf), _ptr(q.embed), _ptr(e_md), _ptr(enorm), n, d, m, k,
             idx.data_ptr(), _ptr(qk.buf), _ptr(q1), _ptr(part), name="memory_topk")
    plan.add(lib.ammc_sum_partials_f32, _ptr(part), nblk, 1.0 / float(n * d), _ptr(diff), name="diff")
    out = bld.act(B, H, W, a.c)
    bld.conv(qk, dec_w, out, ntaps=1, cin=k * d, n=a.c, shift=quan.dec.bias.detach(),
             res=a if residual else None, act=ACT_NONE, name="dec")
    y = _to_nchw(bld, out)
    plan.run(_stream(x))
    return y, diff, q1


ERROR_MAP_PATCHES = (8, 16, 32)


def _nchw_strides(t: torch.Tensor):
    """(batch, channel, row) strides of an NCHW view for `ammc_error_maps_f32`; a dimension of size 1 may carry any
    stride in torch - it is given the extent below it instead"""
    _, c, h, w = t.shape
    bs, cs, rs, _ = t.stride()
    if h == 1:
        rs = max(rs, w)
    plane = (h - 1) * rs + w
    if c == 1:
        cs = max(cs, plane)
    if t.shape[0] == 1:
        bs = max(bs, (c - 1) * cs + plane)
    return bs, cs, rs


def error_maps(pred: torch.Tensor, target: torch.Tensor, patch: int = 16, pixel: bool = False, out: dict | None = None) -> dict:
    """Where the prediction error sits (csrc/error_maps.hip; definitions in include/ammc_hip.h): `pred`, `target` fp32
    [B, C, H, W] on the GPU, pixel stride 1, any batch / channel / row strides (nothing is copied).  Returns
    `patch_sum`, `patch_mean` [B, ph, pw], `frame_sq`, `worst` [B], `worst_idx` [B] int32, `pixel` [B, H, W] when asked,
    and `psnr` = 10 log10(C H W / frame_sq) as `EvalEngine.forward` forms it.  Two launches on torch's current stream;
    every sum is taken in a fixed order, so equal inputs give equal bits.  `out`: tensors to write into, by the same
    keys (views of per-sub-video buffers: a batch then fills its frames' slots) - a sample's map contiguous, any batch
    stride of at least its size (samples may not overlap), the [B] slots contiguous."""
    _need_cuda(pred)
    _need_cuda(target)
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"error_maps: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be equal [B, C, H, W] shapes")
    if pred.dtype != torch.float32 or target.dtype != torch.float32 or pred.device != target.device:
        raise ValueError("error_maps: fp32 tensors on one device")
    if pred.stride(3) != 1 or target.stride(3) != 1:
        raise ValueError("error_maps: pixel stride 1 (NCHW views; make channels-last tensors contiguous first)")
    if patch not in ERROR_MAP_PATCHES:
        raise ValueError(f"error_maps: patch must be one of {ERROR_MAP_PATCHES}")
    lib = _lib.load()
    B, C, H, W = pred.shape
    ph, pw = (H + patch - 1) // patch, (W + patch - 1) // patch
    dev = pred.device
    want = {"patch_sum": ((B, ph, pw), torch.float32), "patch_mean": ((B, ph, pw), torch.float32),
            "frame_sq": ((B,), torch.float32), "worst": ((B,), torch.float32), "worst_idx": ((B,), torch.int32)}
    if pixel:
        want["pixel"] = ((B, H, W), torch.float32)
    res, bs = _slots("error_maps", out, dev, B, want, ("patch_sum", "patch_mean", "pixel"))
    if B > 1 and bs["patch_mean"] != bs["patch_sum"]:
        raise ValueError("error_maps: out['patch_sum'] and out['patch_mean'] must share one batch stride")
    px = res.get("pixel")
    _lib.check(lib.ammc_error_maps_f32(_ptr(pred), *_nchw_strides(pred), _ptr(target), *_nchw_strides(target), B, C, H, W, patch,
                                       _ptr(res["patch_sum"]), bs["patch_sum"], _ptr(res["patch_mean"]),
                                       _ptr(px) if px is not None else None, bs.get("pixel", 0),
                                       _ptr(res["frame_sq"]), _ptr(res["worst"]), res["worst_idx"].data_ptr(), _stream(pred)),
               "error_maps")
    res["psnr"] = 10.0 * torch.log10(float(C * H * W) / res["frame_sq"])
    return res


SSIM_TILE = 32               # tile edge of csrc/ssim.hip (`ammc_ssim_tile()`): where a frame is cut for its fixed-order sums
SSIM_MAX_CHANNELS = 4
_ssim_window_c = None


def ssim_window() -> torch.Tensor:
    """the reference's 1-D window (utils/pytorch_ssim.py:8-10): exp(-(x - 5)^2 / (2 * 1.5^2)) taken in double, rounded to
    fp32, divided by the fp32 sum; [11] fp32 on the CPU"""
    import math
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


def ssim(pred: torch.Tensor, target: torch.Tensor, map: bool = False, out: dict | None = None) -> dict:
    """The reference's SSIM and MSE frame scores (csrc/ssim.hip; definitions in include/ammc_hip.h): `pred`, `target` fp32
    [B, C, H, W] on the GPU, C <= 4, pixel stride 1, any batch / channel / row strides (nothing is copied), values as they
    are (the reference scores its [-1, 1] frames).  Returns `ssim` [B] (the reference's `ssim_error` of each sample),
    `ssim_c` [B, C], `sq` [B] (the sum of (target - pred)^2), `map` [B, H, W] when asked (the channel mean of the SSIM
    map), and derived from `sq`: `mse` = 256 sq / (C H W) (the reference's `mse_error`) and `psnr` = 10 log10(4 C H W / sq).
    Two launches on torch's current stream; every sum is taken in a fixed order, so equal inputs give equal bits wherever
    the sample stands in a batch.  `out`: tensors to write into, by the keys `ssim`, `ssim_c`, `sq`, `map` (views of
    per-sub-video buffers) - the map of a sample contiguous with any batch stride, the others contiguous."""
    global _ssim_window_c
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"ssim: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be equal [B, C, H, W] shapes")
    if pred.dtype != torch.float32 or target.dtype != torch.float32 or pred.device != target.device:
        raise ValueError("ssim: fp32 tensors on one device")
    if pred.stride(3) != 1 or target.stride(3) != 1:
        raise ValueError("ssim: pixel stride 1 (NCHW views; make channels-last tensors contiguous first)")
    B, C, H, W = pred.shape
    dev = pred.device
    want = {"ssim": ((B,), torch.float32), "ssim_c": ((B, C), torch.float32), "sq": ((B,), torch.float32)}
    if map:
        want["map"] = ((B, H, W), torch.float32)
    res, bs = _slots("ssim", out, dev, B, want, ("map",))
    _need_cuda(pred)
    lib = _lib.load()
    if _ssim_window_c is None:
        _ssim_window_c = (ctypes.c_float * 11)(*ssim_window().tolist())
    mp = res.get("map")
    stream = _stream(pred)
    ws = _workspace("ssim", dev, max(int(lib.ammc_ssim_workspace_floats(B, C, H, W)), 4096), torch.float32, stream)
    _lib.check(lib.ammc_ssim_f32(_ptr(pred), *_nchw_strides(pred), _ptr(target), *_nchw_strides(target), B, C, H, W,
                                 _ssim_window_c, _ptr(res["ssim"]), _ptr(res["ssim_c"]), _ptr(res["sq"]),
                                 _ptr(mp) if mp is not None else None, bs.get("map", 0), _ptr(ws), ws.numel(), stream), "ssim")
    n = float(C * H * W)
    res["mse"] = 256.0 * res["sq"] / n
    res["psnr"] = 10.0 * torch.log10(4.0 * n / res["sq"])
    return res


# ---- score-fusion sweep (csrc/fusion_sweep.hip) -----------------------------------------------

FUSION_MAX_CHANNELS = 8
FUSION_MAX_SORTED = 32768    # `ammc_fusion_sweep_max_sorted()`: the smaller class is sorted in one workgroup's LDS
VIDEO_PAIRS_MAX_SEGMENT = 32768   # `ammc_video_pairs_max_segment()`: one video's frames of the smaller class, sorted in LDS
VIDEO_PAIRS_MAX_VIDEOS = 1024     # `ammc_video_pairs_max_videos()`: a workgroup keeps one int64 total per video in LDS


def _sweep_args(what: str, chan, pos_idx, neg_idx, weights, smooth):
    """the argument checks the two sweeps share -> (K, N, P, Q, G, S, row stride of chan)"""
    if chan.dim() != 2 or chan.dtype != torch.float32:
        raise ValueError(f"{what}: chan must be fp32 [K, N], got {chan.dtype} {tuple(chan.shape)}")
    K, N = chan.shape
    if not 1 <= K <= FUSION_MAX_CHANNELS or N < 2:
        raise ValueError(f"{what}: 1 <= K <= {FUSION_MAX_CHANNELS} channels over N >= 2 frames, got K = {K}, N = {N}")
    if chan.stride(1) != 1 or (K > 1 and chan.stride(0) < N):
        raise ValueError(f"{what}: chan needs frame stride 1 and a row stride >= N")
    dev = chan.device
    for name, t in (("pos_idx", pos_idx), ("neg_idx", neg_idx)):
        if t.dim() != 1 or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous int32 vector on {dev}")
    P, Q = pos_idx.numel(), neg_idx.numel()
    if P < 1 or Q < 1 or P + Q != N:
        raise ValueError(f"{what}: both classes non-empty and P + Q == N, got P = {P}, Q = {Q}, N = {N}")
    if weights.dim() != 2 or weights.shape[1] != K or weights.shape[0] < 1 or smooth.dim() != 2 or smooth.shape[1] != 2 \
            or smooth.shape[0] < 1:
        raise ValueError(f"{what}: weights [G, {K}] and smooth [S, 2], got {tuple(weights.shape)} and {tuple(smooth.shape)}")
    for name, t in (("weights", weights), ("smooth", smooth)):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous fp32 on {dev}")
    return K, N, P, Q, weights.shape[0], smooth.shape[0], chan.stride(0) if K > 1 else max(chan.stride(0), N)


def fusion_sweep(chan: torch.Tensor, pos_idx: torch.Tensor, neg_idx: torch.Tensor, weights: torch.Tensor,
                 smooth: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Twice the Mann-Whitney U statistic - the exact numerator of the frame-level AUC - of the fused, smoothed score at
    every point of a grid (csrc/fusion_sweep.hip; the definition is in include/ammc_hip.h).  `chan` fp32 [K, N] on the
    GPU, K <= 8, frame stride 1, any row stride: K normalised channels, higher = more normal, all finite (the caller
    checks).  `pos_idx` / `neg_idx`: int32 device vectors, the frames of the positive (normal) class and the others, a
    partition of 0 .. N - 1 (not checked here: that would wait for the device; an index outside [0, N) is clamped).
    `weights` fp32 [G, K], `smooth` fp32 [S, 2] (the pairs (a, b)), both on the GPU.  Returns int64 [G, S] (`out`, when
    given: contiguous int64 [G, S]); AUC = two_u / (2 P Q).  One launch on torch's current stream; an integer sum, so
    the same values on every launch.  The smaller class may have at most FUSION_MAX_SORTED frames: ValueError beyond."""
    K, N, P, Q, G, S, rs = _sweep_args("fusion_sweep", chan, pos_idx, neg_idx, weights, smooth)
    dev = chan.device
    if min(P, Q) > FUSION_MAX_SORTED:
        raise ValueError(f"fusion_sweep: the smaller class has {min(P, Q)} frames, the pass sorts at most "
                         f"{FUSION_MAX_SORTED} (ammc_fusion_sweep_max_sorted) in a workgroup's LDS")
    _need_cuda(chan)
    if out is None:
        out = torch.empty((G, S), device=dev, dtype=torch.int64)
    elif tuple(out.shape) != (G, S) or out.dtype != torch.int64 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"fusion_sweep: out must be contiguous torch.int64 {(G, S)} on {dev}")
    lib = _lib.load()
    _lib.check(lib.ammc_fusion_sweep_f32(_ptr(chan), rs, K, N, _ptr(weights), G, _ptr(smooth), S, _ptr(pos_idx), P,
                                         _ptr(neg_idx), Q, _ptr(out), _stream(chan)), "fusion_sweep")
    return out


# ---- curve sweep: EER bracket, average precision and PR area (csrc/curve_sweep.hip) ------------

CURVE_MAX_CLASS = 32768      # `ammc_curve_sweep_max_class()`: both classes are sorted in one workgroup's LDS, one after the other


def curve_sweep(chan: torch.Tensor, pos_idx: torch.Tensor, neg_idx: torch.Tensor, weights: torch.Tensor, smooth: torch.Tensor,
                max_workspace_bytes: int = 64 << 20, out: dict | None = None) -> dict:
    """At every point of a grid: `two_u` int64 [G, S] (`fusion_sweep`'s, bit for bit), `pts` int32 [G, S, 4] - the two ROC
    vertices (TP_a, FP_a, TP_b, FP_b) that bracket fpr + tpr = 1 -, `thr` fp32 [G, S, 2], their thresholds, and `sums`
    fp64 [G, S, 2], P times the average precision and P times the precision-recall area (csrc/curve_sweep.hip; the
    definitions and what the caller derives from them are in include/ammc_hip.h).  Inputs as `fusion_sweep` takes them.
    Each grid point needs a row of max(P, Q) words of workspace: the grid is launched in chunks of points whose rows fit
    `max_workspace_bytes`, on torch's current stream; the values do not depend on the chunking.  `out`: a dict of any of
    the four tensors, contiguous.  Either class may have at most CURVE_MAX_CLASS frames: ValueError beyond."""
    K, N, P, Q, G, S, rs = _sweep_args("curve_sweep", chan, pos_idx, neg_idx, weights, smooth)
    dev = chan.device
    if max(P, Q) > CURVE_MAX_CLASS:
        raise ValueError(f"curve_sweep: the larger class has {max(P, Q)} frames, the pass sorts at most "
                         f"{CURVE_MAX_CLASS} (ammc_curve_sweep_max_class) in a workgroup's LDS")
    lib = _lib.load()
    row = lib.ammc_curve_sweep_workspace_bytes(1, P, Q)
    if max_workspace_bytes < row:
        raise ValueError(f"curve_sweep: max_workspace_bytes = {max_workspace_bytes} is below one grid point's row of {row} bytes")
    _need_cuda(chan)
    res, _ = _slots("curve_sweep", out, dev, G, {"two_u": ((G, S), torch.int64), "pts": ((G, S, 4), torch.int32),
                                                 "thr": ((G, S, 2), torch.float32), "sums": ((G, S, 2), torch.float64)})
    fit = max_workspace_bytes // row                          # grid points per launch: whole weight rows, or parts of one
    chunks = [(g0, min(g0 + fit // S, G), 0, S) for g0 in range(0, G, fit // S)] if fit >= S else \
        [(g0, g0 + 1, s0, min(s0 + fit, S)) for g0 in range(G) for s0 in range(0, S, fit)]
    stream = _stream(chan)
    ws = _workspace("curve_sweep", dev, max((g1 - g0) * (s1 - s0) for g0, g1, s0, s1 in chunks) * row, torch.uint8, stream)
    for g0, g1, s0, s1 in chunks:
        at = g0 * S + s0
        _lib.check(lib.ammc_curve_sweep_f32(
            _ptr(chan), rs, K, N, _ptr(weights[g0:g1]), g1 - g0, _ptr(smooth[s0:s1]), s1 - s0, _ptr(pos_idx), P, _ptr(neg_idx), Q,
            _ptr(res["two_u"].view(-1)[at:]), _ptr(res["pts"].view(-1, 4)[at:]), _ptr(res["thr"].view(-1, 2)[at:]),
            _ptr(res["sums"].view(-1, 2)[at:]), _ptr(ws), ws.numel(), stream), "curve_sweep")
    return res


# ---- per-video pair counts and their bootstrap form (csrc/video_pairs.hip) ----------------------

def _video_offsets(what: str, name: str, off, V, count: int, dev):
    """one offset vector of `video_pairs` -> (V, the vector as given or as a host int64 array, the host array or None).
    A list or a CPU tensor is checked here; a device tensor only for what needs no read-back."""
    if isinstance(off, torch.Tensor) and off.is_cuda:
        if off.dim() != 1 or off.dtype != torch.int32 or off.device != dev or not off.is_contiguous() or off.numel() < 2:
            raise ValueError(f"{what}: {name} must be a contiguous int32 vector of V + 1 >= 2 entries on {dev}")
        host = None
    else:
        if isinstance(off, torch.Tensor):
            if off.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{what}: {name} must hold integers, got {off.dtype}")
            off = off.numpy()
        host = np.asarray(off)
        if host.ndim != 1 or host.size < 2 or host.dtype.kind not in "iu":
            raise ValueError(f"{what}: {name} must be a vector of V + 1 >= 2 integers")
        host = host.astype(np.int64)
        if host[0] != 0 or host[-1] != count or (np.diff(host) < 0).any():
            raise ValueError(f"{what}: {name} must be non-decreasing from 0 to {count}, got {host[0]} .. {host[-1]}")
    n = (off.numel() if host is None else host.size) - 1
    if V is not None and n != V:
        raise ValueError(f"{what}: pos_off and neg_off must both have V + 1 entries, got {V + 1} and {n + 1}")
    return n, off, host


def video_pairs(chan: torch.Tensor, pos_idx: torch.Tensor, neg_idx: torch.Tensor, pos_off, neg_off, weights: torch.Tensor,
                smooth: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """`fusion_sweep`'s count split by the video of either frame (csrc/video_pairs.hip; the definition is in
    include/ammc_hip.h): int64 [G, S, V, V], entry [a, b] the count over the positive frames of video a and the negative
    frames of video b.  `chan`, `pos_idx`, `neg_idx`, `weights`, `smooth` as `fusion_sweep` takes them, the index lists in
    video order.  `pos_off` / `neg_off`: V + 1 offsets into them, non-decreasing from 0 to P (Q) - a list, an array or a
    CPU tensor (checked here, then uploaded) or an int32 device vector (not checked: that would wait for the device; only
    when the smaller class exceeds VIDEO_PAIRS_MAX_SEGMENT is the vector read back, for its longest segment).  The block
    sums are `fusion_sweep`'s integers.  One launch on torch's current stream, every element written once (`out`, when
    given: contiguous int64 [G, S, V, V], nothing to clear).  V <= VIDEO_PAIRS_MAX_VIDEOS and a video's frames of the
    smaller class <= VIDEO_PAIRS_MAX_SEGMENT: ValueError beyond."""
    K, N, P, Q, G, S, rs = _sweep_args("video_pairs", chan, pos_idx, neg_idx, weights, smooth)
    dev = chan.device
    V, pos_off, pos_host = _video_offsets("video_pairs", "pos_off", pos_off, None, P, dev)
    V, neg_off, neg_host = _video_offsets("video_pairs", "neg_off", neg_off, V, Q, dev)
    if V > VIDEO_PAIRS_MAX_VIDEOS:
        raise ValueError(f"video_pairs: {V} videos, the pass keeps at most {VIDEO_PAIRS_MAX_VIDEOS} "
                         f"(ammc_video_pairs_max_videos) totals in a workgroup's LDS")
    sorted_host = neg_host if Q <= P else pos_host         # the class the kernel sorts, video by video
    seg = min(P, Q) if sorted_host is None else int(np.diff(sorted_host).max())
    if seg > VIDEO_PAIRS_MAX_SEGMENT and sorted_host is not None:
        raise ValueError(f"video_pairs: a video has {seg} frames of the smaller class, the pass sorts at most "
                         f"{VIDEO_PAIRS_MAX_SEGMENT} (ammc_video_pairs_max_segment) in a workgroup's LDS")
    _need_cuda(chan)
    if seg > VIDEO_PAIRS_MAX_SEGMENT:                         # device offsets and a large class: its longest segment is needed
        seg = int((neg_off if Q <= P else pos_off).diff().max())
        if seg > VIDEO_PAIRS_MAX_SEGMENT:
            raise ValueError(f"video_pairs: a video has {seg} frames of the smaller class, the pass sorts at most "
                             f"{VIDEO_PAIRS_MAX_SEGMENT} (ammc_video_pairs_max_segment) in a workgroup's LDS")
    if pos_host is not None:
        pos_off = torch.from_numpy(pos_host.astype(np.int32)).to(dev)
    if neg_host is not None:
        neg_off = torch.from_numpy(neg_host.astype(np.int32)).to(dev)
    if out is None:
        out = torch.empty((G, S, V, V), device=dev, dtype=torch.int64)
    elif tuple(out.shape) != (G, S, V, V) or out.dtype != torch.int64 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"video_pairs: out must be contiguous torch.int64 {(G, S, V, V)} on {dev}")
    lib = _lib.load()
    _lib.check(lib.ammc_video_pairs_f32(_ptr(chan), rs, K, N, _ptr(weights), G, _ptr(smooth), S, _ptr(pos_idx), P, _ptr(neg_idx),
                                        Q, _ptr(pos_off), _ptr(neg_off), V, max(seg, 1), _ptr(out), _stream(chan)), "video_pairs")
    return out


def bootstrap_pairs(pairs: torch.Tensor, mult: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[r, j] = sum over a, b of mult[r, a] * mult[r, b] * pairs[j, a, b] in exact int64 (csrc/video_pairs.hip,
    `ammc_bootstrap_pairs_i64`): what `video_pairs`' blocks give for replicas that draw video x mult[r, x] times.  `pairs`
    int64 [M, V, V] and `mult` int32 [B, V], contiguous, on the GPU, entries >= 0.  The caller keeps the precondition
    of include/ammc_hip.h: 2 P_r Q_r < 2^63 per replica.  Returns int64 [B, M] (`out`, when given, contiguous).  One
    launch on torch's current stream."""
    if not isinstance(pairs, torch.Tensor) or not isinstance(mult, torch.Tensor):
        raise ValueError("bootstrap_pairs: pairs and mult must be tensors")
    if pairs.dim() != 3 or pairs.shape[1] != pairs.shape[2] or pairs.dtype != torch.int64 or pairs.shape[0] < 1 or pairs.shape[1] < 1:
        raise ValueError(f"bootstrap_pairs: pairs must be int64 [M, V, V], got {pairs.dtype} {tuple(pairs.shape)}")
    M, V = pairs.shape[0], pairs.shape[1]
    if mult.dim() != 2 or mult.shape[1] != V or mult.shape[0] < 1 or mult.dtype != torch.int32:
        raise ValueError(f"bootstrap_pairs: mult must be int32 [B, {V}], got {mult.dtype} {tuple(mult.shape)}")
    if V > VIDEO_PAIRS_MAX_VIDEOS:
        raise ValueError(f"bootstrap_pairs: {V} videos, at most {VIDEO_PAIRS_MAX_VIDEOS} (ammc_video_pairs_max_videos)")
    dev = pairs.device
    if mult.device != dev or not pairs.is_contiguous() or not mult.is_contiguous():
        raise ValueError(f"bootstrap_pairs: pairs and mult must be contiguous and both on {dev}")
    B = mult.shape[0]
    _need_cuda(pairs)
    if out is None:
        out = torch.empty((B, M), device=dev, dtype=torch.int64)
    elif tuple(out.shape) != (B, M) or out.dtype != torch.int64 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"bootstrap_pairs: out must be contiguous torch.int64 {(B, M)} on {dev}")
    _lib.check(_lib.load().ammc_bootstrap_pairs_i64(_ptr(pairs), M, V, _ptr(mult), B, _ptr(out), _stream(pairs)), "bootstrap_pairs")
    return out


# ---- pixel-level evaluation (csrc/pixel_scores.hip) -------------------------------------------

PIXEL_MAX_PIXELS = 1 << 24   # h * w of one sample
PIXEL_MAX_DEN = 4096


def pixel_scores(map: torch.Tensor, mask: torch.Tensor, frac=(2, 5), out: dict | None = None) -> dict:
    """What the pixel-level criterion needs of a score map and a ground-truth mask (csrc/pixel_scores.hip; definitions
    in include/ammc_hip.h).  `map` fp32 [B, H, W] on the GPU, higher = more anomalous; `mask` uint8 or bool [B, H, W] on
    the same device, nonzero = anomalous; each with contiguous samples and any batch stride >= H * W (nothing is copied).
    `frac` = (num, den), 1 <= num <= den <= 4096.  Returns per sample `m` int32 [B] (mask pixels), `kth` (the k-th largest
    map value inside the mask, k = ceil(num * m / den) in integers), `max_in`, `max_out` (the largest value inside /
    outside the mask) - an empty set gives -inf - and the derived `max_all` = maximum(max_in, max_out).  The kernel does
    no floating-point arithmetic: the floats are stored map values bit for bit, the same for a sample wherever it stands
    in a batch.  NaN in the map is the caller's to keep out.  One launch on torch's current stream.  `out`: contiguous
    [B] tensors to write into, by the keys `m`, `kth`, `max_in`, `max_out` (views of per-sub-video buffers)."""
    if not isinstance(map, torch.Tensor) or not isinstance(mask, torch.Tensor) or map.dim() != 3 or mask.shape != map.shape:
        raise ValueError("pixel_scores: map and mask must be [B, H, W] tensors of one shape")
    if map.dtype != torch.float32 or mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"pixel_scores: map must be fp32 and mask uint8 or bool, got {map.dtype} and {mask.dtype}")
    B, H, W = map.shape
    if B < 1 or H < 1 or W < 1 or H * W > PIXEL_MAX_PIXELS:
        raise ValueError(f"pixel_scores: B, H, W >= 1 and H * W <= {PIXEL_MAX_PIXELS}, got {tuple(map.shape)}")
    num, den = _pair("pixel_scores", "frac", frac, PIXEL_MAX_DEN)
    for name, t in (("map", map), ("mask", mask)):
        if not t[0].is_contiguous() or (B > 1 and t.stride(0) < H * W):
            raise ValueError(f"pixel_scores: {name}: a sample must be contiguous, with a batch stride >= H * W")
    if not map.is_cuda or mask.device != map.device:
        raise ValueError("pixel_scores: map and mask must be on one GPU; there is no CPU fallback")
    res, _ = _slots("pixel_scores", out, map.device, B, {"m": ((B,), torch.int32), "kth": ((B,), torch.float32),
                                                         "max_in": ((B,), torch.float32), "max_out": ((B,), torch.float32)})
    lib = _lib.load()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)                         # a bool is one byte, 0 or 1: the same memory
    _lib.check(lib.ammc_pixel_scores_f32(_ptr(map), _bs(map, H * W), mask.data_ptr(), _bs(mask, H * W), B, H, W, num, den,
                                         res["m"].data_ptr(), _ptr(res["kth"]), _ptr(res["max_in"]), _ptr(res["max_out"]),
                                         _stream(map)), "pixel_scores")
    res["max_all"] = torch.maximum(res["max_in"], res["max_out"])
    return res


# ---- region-based evaluation (csrc/region_scores.hip) -----------------------------------------

REGION_MAX_PIXELS = 1 << 22  # h * w of one sample
REGION_MAX_REGIONS = 32      # ground-truth regions of one frame
REGION_MAX_DEN = 4096
REGION_WORKSPACE_BUDGET = 256 << 20   # bytes: `region_scores` splits its thresholds into launches that stay below it
_REGION_KEYS = ("n_px", "n_comp", "n_fp", "hit")


def _region_sample_checks(what: str, tensors, min_area, connectivity):
    """the [B, H, W] checks `label_regions` and `region_scores` share; tensors: [(name, tensor, dtypes)]"""
    first = tensors[0][1]
    for name, t, dtypes in tensors:
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype not in dtypes:
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} must be a [B, H, W] tensor of {' or '.join(str(d) for d in dtypes)}, got {got}")
        if t.shape != first.shape:
            raise ValueError(f"{what}: {name} is {tuple(t.shape)}, {tensors[0][0]} is {tuple(first.shape)}")
    B, H, W = first.shape
    if B < 1 or H < 1 or W < 1 or H * W > REGION_MAX_PIXELS:
        raise ValueError(f"{what}: B, H, W >= 1 and H * W <= {REGION_MAX_PIXELS}, got {tuple(first.shape)}")
    if not isinstance(min_area, int) or min_area < 1:
        raise ValueError(f"{what}: min_area must be an integer >= 1, got {min_area!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    for name, t, _ in tensors:
        if not t[0].is_contiguous() or (B > 1 and t.stride(0) < H * W):
            raise ValueError(f"{what}: {name}: a sample must be contiguous, with a batch stride >= H * W")
    return B, H, W


def label_regions(mask: torch.Tensor, min_area: int = 1, connectivity: int = 8, out: dict | None = None) -> dict:
    """The ground-truth regions of masks (csrc/region_scores.hip; definitions in include/ammc_hip.h).  `mask` uint8 or
    bool [B, H, W] on the GPU, nonzero = anomalous, contiguous samples with any batch stride >= H * W.  Returns `labels`
    uint8 [B, H, W] - 0 for the background, r = 1..32 for the r-th connected component (8- or 4-connectivity) with at
    least `min_area` pixels, in raster order of the components' first pixels - and `count` int32 [B], the TRUE number
    of kept components: components ranked beyond 32 are written as 0 and it is the caller's to refuse them.  One launch
    on torch's current stream.  `out`: tensors to write into by those two keys (`labels` with contiguous samples)."""
    B, H, W = _region_sample_checks("label_regions", [("mask", mask, (torch.uint8, torch.bool))], min_area, connectivity)
    if not mask.is_cuda:
        raise ValueError("label_regions: mask must be on the GPU; there is no CPU fallback")
    dev = mask.device
    res, bs = _slots("label_regions", out, dev, B, {"labels": ((B, H, W), torch.uint8), "count": ((B,), torch.int32)}, ("labels",))
    lib = _lib.load()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    stream = _stream(mask)
    ws = _workspace("region", dev, (lib.ammc_region_workspace_bytes(B, 1, H, W) + 3) // 4, torch.int32, stream)
    _lib.check(lib.ammc_label_regions_u8(mask.data_ptr(), _bs(mask, H * W), B, H, W, min_area, connectivity, res["labels"].data_ptr(),
                                         bs["labels"], res["count"].data_ptr(), ws.data_ptr(), ws.numel() * 4, stream),
               "label_regions")
    return res


def region_scores(map: torch.Tensor, labels: torch.Tensor, thresholds: torch.Tensor, iou=(1, 10), min_area: int = 1,
                  connectivity: int = 8, out: dict | None = None) -> dict:
    """What the region-based detection criterion needs of score maps and label images (csrc/region_scores.hip;
    definitions in include/ammc_hip.h).  `map` fp32 [B, H, W] on the GPU, higher = more anomalous; `labels` uint8
    [B, H, W] as `label_regions` writes them (values above 32 count as background); each with contiguous samples and any
    batch stride >= H * W.  `thresholds` fp32 [T] on the same device, any values in any order.  `iou` = (num, den),
    1 <= num <= den <= 4096.  Per sample and threshold, int32 [B, T]: `n_px` (pixels with map >= t), `n_comp` (connected
    components of them with at least `min_area` pixels), `n_fp` (those that match no region: |C n G| den >= num |C u G|
    in 64-bit integers), `hit` (bit r - 1: some component matches region r).  Integers that depend on the sample's
    values, its labels and the threshold alone.  One launch on torch's current stream per chunk of thresholds: the
    workspace (12 bytes per pixel, sample and threshold) is cached per device and stays below REGION_WORKSPACE_BUDGET =
    256 MiB (or one threshold's need, if that is more).  `n_comp` = -1 would report a labelling that hit its round
    bound.  `out`: contiguous [B, T] int32 tensors to write into by the four keys."""
    B, H, W = _region_sample_checks("region_scores", [("map", map, (torch.float32,)), ("labels", labels, (torch.uint8,))],
                                    min_area, connectivity)
    if not isinstance(thresholds, torch.Tensor) or thresholds.dim() != 1 or thresholds.dtype != torch.float32 or thresholds.numel() < 1:
        raise ValueError("region_scores: thresholds must be a non-empty fp32 [T] tensor")
    if not thresholds.is_contiguous():
        raise ValueError("region_scores: thresholds must be contiguous")
    num, den = _pair("region_scores", "iou", iou, REGION_MAX_DEN)
    if not map.is_cuda or labels.device != map.device or thresholds.device != map.device:
        raise ValueError("region_scores: map, labels and thresholds must be on one GPU; there is no CPU fallback")
    dev, T = map.device, thresholds.numel()
    res, _ = _slots("region_scores", out, dev, B, {key: ((B, T), torch.int32) for key in _REGION_KEYS})
    lib = _lib.load()
    per_t = lib.ammc_region_workspace_bytes(B, 1, H, W)
    chunk = max(1, min(T, REGION_WORKSPACE_BUDGET // per_t))
    stream = _stream(map)
    ws = _workspace("region", dev, (per_t * chunk + 3) // 4, torch.int32, stream)
    for t0 in range(0, T, chunk):
        tc = min(chunk, T - t0)
        _lib.check(lib.ammc_region_scores_f32(_ptr(map), _bs(map, H * W), labels.data_ptr(), _bs(labels, H * W), B, H, W,
                                              _ptr(thresholds[t0:]), tc, num, den, min_area, connectivity,
                                              *(res[key][:, t0:].data_ptr() for key in _REGION_KEYS), T, ws.data_ptr(),
                                              ws.numel() * 4, stream), "region_scores")
    return res


# ---- fused localisation maps (csrc/fuse_maps.hip) ----------------------------------------------

FUSE_MAX_CHANNELS = 4
FUSE_MAX_RADIUS = 8
FUSE_MAX_PIXELS = 1 << 28    # h * w of one sample
FUSE_TILE = (32, 64)         # the tile of csrc/fuse_maps.hip: the workspace holds one float per tile and sample


def fuse_maps(sources, cells, coef: torch.Tensor, radius: int = 0, patch: int = 16, out: dict | None = None) -> dict:
    """Several score maps of different resolution -> one smoothed map (csrc/fuse_maps.hip; definitions in
    include/ammc_hip.h).  `sources`: 1..4 fp32 [B, gh_c, gw_c] tensors on one GPU, higher = more anomalous, a sample's rows
    and columns contiguous, any batch stride (nothing is copied); `cells`: per source the integer edge >= 1 of the square
    of frame pixels one value covers.  The frame size is that of the first source with cell 1, or, without one,
    (gh_0 * cell_0, gw_0 * cell_0); every gh_c must be H // cell_c or ceil(H / cell_c) and >= 1, gw_c alike.  `coef`: fp32
    [n_ch] on the same device (computed there: no host wait).  `radius` 0..8: a count-normalised (2 radius + 1)^2 box mean
    without padding; `patch` 8, 16 or 32.  Returns `pixel` [B, H, W] (the weighted sum of the blockily expanded sources,
    smoothed), `patch_mean` [B, ph, pw] (its means over `error_maps`' patch grid, true pixel counts) and `frame_max` [B]
    (its largest value, bit for bit).  fp32 without contraction, sums that only add, no atomics: a sample's outputs do
    not depend on the batch it is in, equal inputs give equal bits.  Two launches on torch's current stream.  `out`:
    tensors to write into by the same keys (views of per-sub-video buffers) - maps with contiguous samples and any batch
    stride, `frame_max` contiguous."""
    if not isinstance(sources, (list, tuple)) or not 1 <= len(sources) <= FUSE_MAX_CHANNELS:
        raise ValueError(f"fuse_maps: 1..{FUSE_MAX_CHANNELS} source maps, got "
                         f"{len(sources) if isinstance(sources, (list, tuple)) else type(sources).__name__}")
    n_ch = len(sources)
    try:
        cells = [int(c) for c in cells]
    except (TypeError, ValueError):
        raise ValueError(f"fuse_maps: cells must be {n_ch} integers, got {cells!r}") from None
    if len(cells) != n_ch or min(cells) < 1:
        raise ValueError(f"fuse_maps: one cell size >= 1 per source, got {cells!r} for {n_ch} sources")
    for c, s in enumerate(sources):
        if not isinstance(s, torch.Tensor) or s.dim() != 3 or s.dtype != torch.float32:
            got = f"{s.dtype} {tuple(s.shape)}" if isinstance(s, torch.Tensor) else type(s).__name__
            raise ValueError(f"fuse_maps: source {c} must be an fp32 [B, gh, gw] tensor, got {got}")
    B = sources[0].shape[0]
    ref = next((c for c in range(n_ch) if cells[c] == 1), None)
    H, W = sources[ref].shape[1:] if ref is not None else (sources[0].shape[1] * cells[0], sources[0].shape[2] * cells[0])
    H, W = int(H), int(W)
    if B < 1 or H < 1 or W < 1 or H * W > FUSE_MAX_PIXELS:
        raise ValueError(f"fuse_maps: B, H, W >= 1 and H * W <= {FUSE_MAX_PIXELS}, got B = {B}, a {H} x {W} frame")
    for c, s in enumerate(sources):
        _, gh, gw = s.shape
        if s.shape[0] != B:
            raise ValueError(f"fuse_maps: source {c} has batch {s.shape[0]}, source 0 has {B}")
        if gh < 1 or gw < 1 or gh not in (H // cells[c], -(-H // cells[c])) or gw not in (W // cells[c], -(-W // cells[c])):
            raise ValueError(f"fuse_maps: source {c} is a {gh} x {gw} grid: a {H} x {W} frame in cells of {cells[c]} has "
                             f"{H // cells[c]} or {-(-H // cells[c])} rows and {W // cells[c]} or {-(-W // cells[c])} columns (>= 1)")
        if not s[0].is_contiguous() or (B > 1 and s.stride(0) < gh * gw):
            raise ValueError(f"fuse_maps: source {c}: a sample must be contiguous, with a batch stride >= gh * gw")
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= FUSE_MAX_RADIUS:
        raise ValueError(f"fuse_maps: radius must be an integer in 0..{FUSE_MAX_RADIUS}, got {radius!r}")
    if patch not in ERROR_MAP_PATCHES:
        raise ValueError(f"fuse_maps: patch must be one of {ERROR_MAP_PATCHES}, got {patch!r}")
    if not isinstance(coef, torch.Tensor) or coef.dtype != torch.float32 or tuple(coef.shape) != (n_ch,) or not coef.is_contiguous():
        raise ValueError(f"fuse_maps: coef must be a contiguous fp32 [{n_ch}] tensor")
    dev = sources[0].device
    if coef.device != dev or any(s.device != dev for s in sources):
        raise ValueError("fuse_maps: the sources and coef must be on one device")
    ph, pw = (H + patch - 1) // patch, (W + patch - 1) // patch
    res, bs = _slots("fuse_maps", out, dev, B, {"pixel": ((B, H, W), torch.float32), "patch_mean": ((B, ph, pw), torch.float32),
                                                "frame_max": ((B,), torch.float32)}, ("pixel", "patch_mean"))
    if dev.type != "cuda":
        raise ValueError("fuse_maps: the sources and coef must be on the GPU; there is no CPU fallback")
    lib = _lib.load()
    stream = _stream(sources[0])
    ws = _workspace("fuse", dev, B * (-(-H // FUSE_TILE[0])) * (-(-W // FUSE_TILE[1])), torch.float32, stream)
    ptrs = (ctypes.c_void_p * n_ch)(*(s.data_ptr() for s in sources))
    strides = (ctypes.c_int64 * n_ch)(*(_bs(s, s.shape[1] * s.shape[2]) for s in sources))
    ghs = (ctypes.c_int32 * n_ch)(*(s.shape[1] for s in sources))
    gws = (ctypes.c_int32 * n_ch)(*(s.shape[2] for s in sources))
    cls = (ctypes.c_int32 * n_ch)(*cells)
    _lib.check(lib.ammc_fuse_maps_f32(ctypes.addressof(ptrs), ctypes.addressof(strides), ctypes.addressof(ghs), ctypes.addressof(gws), ctypes.addressof(cls),
                                      n_ch, _ptr(coef), B, H, W, radius, patch, _ptr(res["pixel"]), bs["pixel"], _ptr(res["patch_mean"]),
                                      bs["patch_mean"], _ptr(res["frame_max"]), _ptr(ws), stream), "fuse_maps")
    return res


# ---- qualitative evaluation: panels of frames, colour-coded flows and error heat maps (csrc/render.hip) ----------

RENDER_MAX_BATCH = 65535
RENDER_MAX_PIXELS = 1 << 28  # h * w of one sample


def _render_input(what: str, name: str, t, c: int, like=None) -> int:
    """checks one fp32 [B, c, H, W] input of the render ops (a sample contiguous, any batch stride >= its size);
    returns the batch stride in floats"""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != c or t.dtype != torch.float32:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be an fp32 [B, {c}, H, W] tensor, got {got}")
    B, _, H, W = t.shape
    if B < 1 or H < 1 or W < 1 or B > RENDER_MAX_BATCH or H * W > RENDER_MAX_PIXELS:
        raise ValueError(f"{what}: 1 <= B <= {RENDER_MAX_BATCH}, H, W >= 1 and H * W <= {RENDER_MAX_PIXELS}, got {name} {tuple(t.shape)}")
    if like is not None and (t.shape[0] != like.shape[0] or t.shape[2:] != like.shape[2:] or t.device != like.device):
        raise ValueError(f"{what}: {name} {tuple(t.shape)} on {t.device} does not match the batch, frame size and device of "
                         f"{tuple(like.shape)} on {like.device}")
    if not t[0].is_contiguous() or (B > 1 and t.stride(0) < c * H * W):
        raise ValueError(f"{what}: {name}: a sample must be contiguous, with a batch stride >= C * H * W")
    return _bs(t, c * H * W)


def _render_vector(what: str, name: str, v, B: int, dev) -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (B,) or v.device != dev or not v.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor [{B}] on {dev}")
    return v


def _render_scale(what: str, scale):
    try:
        su, sv = (float(s) for s in scale)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the flow scale must be a pair (su, sv), got {scale!r}") from None
    if not (abs(su) < float("inf") and abs(sv) < float("inf")):
        raise ValueError(f"{what}: the flow scale must be finite, got {scale!r}")
    return su, sv


def _render_out(what: str, out, shape, dev) -> tuple:
    """the uint8 [B, h, w, 3] output (allocated when None) and its batch stride in bytes"""
    res, bs = _slots(what, out, dev, shape[0], {"out": (shape, torch.uint8)}, ("out",), single=True)
    return res["out"], bs["out"]


def flow_to_rgb(flow: torch.Tensor, scale=(1.0, 1.0), max_rad: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The Middlebury colour code of a flow batch (csrc/render.hip; the definition is in include/ammc_hip.h): `flow` fp32
    [B, 2, H, W] on the GPU, a sample contiguous, any batch stride (nothing is copied) -> uint8 [B, H, W, 3].  `scale` =
    (su, sv) multiplies the two components first.  A pixel with a component beyond 1e7 or a NaN is unknown: black, and
    outside the maximum.  `max_rad` fp32 [B]: the radius that maps to full saturation, per sample (pixels beyond it are
    dimmed by a quarter); default each sample's own largest radius, taken by a launch of its own on the same stream.
    The reference's `flow_to_image` but for the pixels that attain the maximum, which are always inside here.  `out`:
    uint8 [B, H, W, 3] to write into, a sample's picture contiguous, any batch stride."""
    what = "flow_to_rgb"
    bs = _render_input(what, "flow", flow, 2)
    su, sv = _render_scale(what, scale)
    B, _, H, W = flow.shape
    dev = flow.device
    if max_rad is not None:
        _render_vector(what, "max_rad", max_rad, B, dev)
    out, out_bs = _render_out(what, out, (B, H, W, 3), dev)
    _render_need_gpu(what, flow)
    lib = _lib.load()
    ws = torch.empty((B, 4), device=dev, dtype=torch.float32) if max_rad is None else None
    _lib.check(lib.ammc_flow_colour_u8(_ptr(flow), bs, B, H, W, su, sv, _ptr(max_rad) if max_rad is not None else None,
                                       _ptr(ws) if ws is not None else None, out.data_ptr(), out_bs, _stream(flow)), what)
    return out


def _render_inputs(what: str, rgb_pred, rgb_target, op_pred, op_target):
    strides = [_render_input(what, "rgb_pred", rgb_pred, 3)]
    strides.append(_render_input(what, "rgb_target", rgb_target, 3, rgb_pred))
    strides.append(_render_input(what, "op_pred", op_pred, 2, rgb_pred))
    strides.append(_render_input(what, "op_target", op_target, 2, rgb_pred))
    return strides


def _render_need_gpu(what: str, t: torch.Tensor):
    if not t.is_cuda:
        raise ValueError(f"{what}: the tensors must be on one GPU; there is no CPU fallback")


def render_stats(rgb_pred: torch.Tensor, rgb_target: torch.Tensor, op_pred: torch.Tensor, op_target: torch.Tensor,
                 flow_scale=(1.0, 1.0), out: torch.Tensor | None = None) -> torch.Tensor:
    """The maxima the tiles of `render_panels` are normalised by, fp32 [B, 4]: the largest flow radius of the target and
    of the predicted flow (components scaled by `flow_scale`, unknown pixels left out), the largest per-pixel error of
    the frame pair and of the flow pair (`error_maps`' `pixel`; a NaN and an unknown flow pixel count as 0).  One launch
    behind a memset of `out` on torch's current stream; exact maxima: the same bits on every launch."""
    what = "render_stats"
    strides = _render_inputs(what, rgb_pred, rgb_target, op_pred, op_target)
    su, sv = _render_scale(what, flow_scale)
    B, _, H, W = rgb_pred.shape
    dev = rgb_pred.device
    out = _slots(what, out, dev, B, {"out": ((B, 4), torch.float32)}, single=True)[0]["out"]
    _render_need_gpu(what, rgb_pred)
    lib = _lib.load()
    _lib.check(lib.ammc_render_stats_f32(_ptr(rgb_pred), strides[0], _ptr(rgb_target), strides[1], _ptr(op_pred), strides[2],
                                         _ptr(op_target), strides[3], B, H, W, su, sv, _ptr(out), _stream(rgb_pred)), what)
    return out


def render_panels(rgb_pred: torch.Tensor, rgb_target: torch.Tensor, op_pred: torch.Tensor, op_target: torch.Tensor,
                  tiles=None, flow_scale=(1.0, 1.0), flow_norm="target", heat_max="frame", alpha: float = 0.6,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Pictures of a batch of predictions (csrc/render.hip; definitions in include/ammc_hip.h): `rgb_pred`, `rgb_target`
    fp32 [B, 3, H, W] on the model's [-1, 1] range, `op_pred`, `op_target` fp32 [B, 2, H, W], on one GPU, a sample
    contiguous, any batch strides (nothing is copied) -> uint8 [B, rows * H, cols * W, 3]: per sample a panel of tiles.
    `tiles`: a row of names or rows of equal length, an ordered subset of `harness.RENDER_TILES` - `rgb_target`,
    `rgb_pred` (the frames), `rgb_heat` (the per-pixel error of the frame pair as a heat map over the grey target),
    `op_target`, `op_pred` (the Middlebury colour code, components scaled by `flow_scale` first), `op_heat`; default
    all six, 2 x 3.  `flow_norm`: "target" colours both flows by the target's largest radius (the two tiles are
    comparable), "each" every flow by its own (the reference's per-image behaviour), a tensor [B] by the given radius.
    `heat_max`: "frame" scales a heat tile by its sample's largest error, a tensor [B] (both streams) or a pair of them
    (frame pair, flow pair) by fixed values: pictures of different frames are then comparable.  `alpha`: the weight of
    the heat colour over the grey.  Two launches on torch's current stream (one where every normalisation is given).
    `out`: uint8 [B, rows * H, cols * W, 3] to write into, a sample's panel contiguous, any batch stride."""
    from .harness import RENDER_DEFAULT_TILES, RENDER_TILES, panel_layout
    what = "render_panels"
    strides = _render_inputs(what, rgb_pred, rgb_target, op_pred, op_target)
    su, sv = _render_scale(what, flow_scale)
    rows = panel_layout(RENDER_DEFAULT_TILES if tiles is None else tiles)
    ids = [RENDER_TILES.index(t) for row in rows for t in row]
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: alpha must be a number in [0, 1], got {alpha!r}") from None
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{what}: alpha must be a number in [0, 1], got {alpha!r}")
    B, _, H, W = rgb_pred.shape
    dev = rgb_pred.device
    max_rad, each = None, 0
    if isinstance(flow_norm, str):
        if flow_norm not in ("target", "each"):
            raise ValueError(f"{what}: flow_norm must be 'target', 'each' or a tensor [B], got {flow_norm!r}")
        each = int(flow_norm == "each")
    else:
        max_rad = _render_vector(what, "flow_norm", flow_norm, B, dev)
    heat_rgb = heat_op = None
    if isinstance(heat_max, str):
        if heat_max != "frame":
            raise ValueError(f"{what}: heat_max must be 'frame', a tensor [B] or a pair of them, got {heat_max!r}")
    elif isinstance(heat_max, (tuple, list)):
        if len(heat_max) != 2:
            raise ValueError(f"{what}: heat_max must be 'frame', a tensor [B] or a pair of them, got {len(heat_max)} values")
        heat_rgb = _render_vector(what, "heat_max[0]", heat_max[0], B, dev)
        heat_op = _render_vector(what, "heat_max[1]", heat_max[1], B, dev)
    else:
        heat_rgb = heat_op = _render_vector(what, "heat_max", heat_max, B, dev)
    out, out_bs = _render_out(what, out, (B, len(rows) * H, len(rows[0]) * W, 3), dev)
    _render_need_gpu(what, rgb_pred)
    lib = _lib.load()
    need = (max_rad is None and (3 in ids or 4 in ids)) or (heat_rgb is None and 2 in ids) or (heat_op is None and 5 in ids)
    stream = _stream(rgb_pred)
    ptrs = [_ptr(rgb_pred), strides[0], _ptr(rgb_target), strides[1], _ptr(op_pred), strides[2], _ptr(op_target), strides[3]]
    stats = None
    if need:
        stats = torch.empty((B, 4), device=dev, dtype=torch.float32)
        _lib.check(lib.ammc_render_stats_f32(*ptrs, B, H, W, su, sv, _ptr(stats), stream), "render_panels (stats)")
    opt = [_ptr(t) if t is not None else None for t in (stats, max_rad, heat_rgb, heat_op)]
    _lib.check(lib.ammc_render_panels_u8(*ptrs, B, H, W, su, sv, (ctypes.c_int32 * len(ids))(*ids), len(rows), len(rows[0]),
                                         opt[0], each, opt[1], opt[2], opt[3], alpha, out.data_ptr(), out_bs, stream), what)
    return out


def _nhwc_strides(t: torch.Tensor):
    """(batch, row, pixel) strides of an NHWC view [B, h, w, C] for `ammc_memory_scores_f32`; a dimension of size 1 may
    carry any stride in torch - it is given the extent below it instead"""
    b, h, w, c = t.shape
    bs, rs, ps, _ = t.stride()
    if w == 1:
        ps = max(ps, c)
    row = (w - 1) * ps + c
    if h == 1:
        rs = max(rs, row)
    if b == 1:
        bs = max(bs, (h - 1) * rs + row)
    return bs, rs, ps


def memory_scores(quan, x: torch.Tensor, indices: bool = False, out: dict | None = None) -> dict:
    """Per-clip memory-commit scores (csrc/memory_scores.hip; definitions in include/ammc_hip.h).  `quan`: an
    `enc_quan_dec_topk` / `enc_quan_dec_res_topk` module - its `enc.weight`, `enc.bias`, `quantize.embed` and
    `quantize.k` are read.  `x`: the bottleneck in front of it, fp32 [B, C, h, w] NCHW-SHAPED on the GPU with any strides;
    the kernel reads its NHWC view in place when that view's channel stride is 1 (a permuted NHWC tensor, a workspace
    view); otherwise - a plain contiguous NCHW tensor - ONE channels-last copy is made first.  Returns `map` [B, h, w]
    (the squared distance to the nearest slot / d per position), `commit` [B] (its fixed-order mean), `worst` [B],
    `worst_idx` [B] int32 (the largest map value and the lowest y * w + x attaining it) and, with `indices`, `idx`
    [B, h, w, k] int32 (the k nearest slots, nearest first).  A clip's outputs do not depend on the batch it is in.  Two
    launches on torch's current stream behind the codebook pack.  `out`: tensors to write into, by the same keys (views of
    per-sub-video buffers) - `map` with contiguous clips and any batch stride, the others contiguous."""
    _need_cuda(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("memory_scores: x must be an fp32 [B, C, h, w] tensor")
    quan = getattr(quan, "quan", quan)                        # enc_quan_dec_res_topk wraps the block it adds `x` to
    q = quan.quantize
    enc_w, enc_b, embed = quan.enc.weight.detach(), quan.enc.bias.detach(), q.embed.detach()
    d, m, k = int(embed.shape[0]), int(embed.shape[1]), int(q.k)
    B, c, h, w = x.shape
    if tuple(enc_w.shape) != (d, c, 1, 1):
        raise ValueError(f"memory_scores: enc.weight {tuple(enc_w.shape)} does not map {c} channels to the codebook's {d}")
    dev = x.device
    if enc_w.device != dev or embed.device != dev:
        raise ValueError("memory_scores: the module and x must be on one device")
    lib = _lib.load()
    xv = x.detach().permute(0, 2, 3, 1)
    if xv.stride(3) != 1:
        xv = xv.contiguous()                                  # the one copy: NCHW-contiguous input -> channels last
    enc_w, enc_b, embed = enc_w.float().contiguous(), enc_b.float().contiguous(), embed.float().contiguous()
    e_md, enorm = _Packer(dev).codebook(embed)
    want = {"map": ((B, h, w), torch.float32), "commit": ((B,), torch.float32), "worst": ((B,), torch.float32),
            "worst_idx": ((B,), torch.int32)}
    if indices:
        want["idx"] = ((B, h, w, k), torch.int32)
    res, bs = _slots("memory_scores", out, dev, B, want, ("map",))
    idx = res.get("idx")
    _lib.check(lib.ammc_memory_scores_f32(_ptr(xv), *_nhwc_strides(xv), B, h, w, c, _ptr(enc_w), _ptr(enc_b), _ptr(embed),
                                          _ptr(e_md), _ptr(enorm), d, m, k, _ptr(res["map"]), bs["map"],
                                          idx.data_ptr() if idx is not None else None, _ptr(res["commit"]), _ptr(res["worst"]),
                                          res["worst_idx"].data_ptr(), _stream(x)), "memory_scores")
    return res


def embed_rows(embed: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """`Quantize_topk.embed_code` (unet.py:315-316): rows of the transposed codebook"""
    return embed.t()[ids]


# which kernel `quantize_topk_f16` / `workload.MemoryStress` launch: 1 (default) = rows resident in registers
# (csrc/memory_topk_f16r.hip, round 5), 0 = the round-2 form (csrc/memory_topk_f16.hip: rows in LDS, codebook L2 -> registers)
F16_ROWS_IN_REGISTERS = os.environ.get("AMMC_MEMORY_F16_FORM", "1") != "0"


def quantize_topk_f16(embed: torch.Tensor, x: torch.Tensor, k: int):
    """Stress form of the memory addressing (BASELINE.json config 5): fp16 MFMA operands, fp32
    accumulation.  embed [D,M] fp32, x [..., D] fp32 -> (q_topk [..., k*D], diff, q_one, idx [..., k]).
    Not the parity path (the slot ranking sees fp16-rounded operands)."""
    _need_cuda(x)
    lib = _lib.load()
    d, m = embed.shape
    lead = x.shape[:-1]
    x2 = x.detach().float().contiguous().view(-1, d)
    n = x2.shape[0]
    dev = x.device
    s = _stream(x)
    idx = torch.empty((n, k), device=dev, dtype=torch.int32)
    qk = torch.empty((n, k * d), device=dev, dtype=torch.float32)
    q1 = torch.empty((n, d), device=dev, dtype=torch.float32)
    diff = torch.empty(1, device=dev, dtype=torch.float32)
    e_md, _ = _Packer(dev).codebook(embed)
    if F16_ROWS_IN_REGISTERS:
        # round 5: feature rows resident in registers, codebook tiles through LDS (csrc/memory_topk_f16r.hip)
        tiles = torch.empty(lib.ammc_codebook_f16_tiles_bytes(d, m), device=dev, dtype=torch.uint8)
        _lib.check(lib.ammc_pack_codebook_f16_tiles(_ptr(embed), d, m, tiles.data_ptr(), s), "pack_codebook_f16_tiles")
        nblk = lib.ammc_memory_topk_f16r_blocks(n)
        part = torch.empty(nblk, device=dev, dtype=torch.float32)
        _lib.check(lib.ammc_memory_topk_fwd_f16r(_ptr(x2), tiles.data_ptr(), _ptr(e_md), n, d, m, k, idx.data_ptr(), _ptr(qk),
                                                 _ptr(q1), _ptr(part), s), "memory_topk_f16r")
    else:
        mpad = (m + 31) // 32 * 32
        e_kblk = torch.empty((d // 8, mpad, 8), device=dev, dtype=torch.float16)
        enorm16 = torch.empty(m, device=dev, dtype=torch.float32)
        _lib.check(lib.ammc_pack_codebook_f16(_ptr(embed), d, m, e_kblk.data_ptr(), _ptr(enorm16), s), "pack_codebook_f16")
        nblk = lib.ammc_memory_topk_f16_blocks(n)
        part = torch.empty(nblk, device=dev, dtype=torch.float32)
        _lib.check(lib.ammc_memory_topk_fwd_f16(_ptr(x2), e_kblk.data_ptr(), _ptr(e_md), _ptr(enorm16), n, d, m, k,
                                                idx.data_ptr(), _ptr(qk), _ptr(q1), _ptr(part), s), "memory_topk_f16")
    _lib.check(lib.ammc_sum_partials_f32(_ptr(part), nblk, 1.0 / float(n * d), _ptr(diff), s), "sum_partials")
    return qk.view(*lead, k * d), diff[0], q1.view(*lead, d), idx.view(*lead, k)
