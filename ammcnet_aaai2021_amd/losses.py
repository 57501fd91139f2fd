"""The per-pixel terms of the generator's objective on the library's own kernels (csrc/loss.hip): what
`harness.generator_loss` / `generator_loss_full` / `single_stream_loss` compute with chains of ATen elementwise and
reduction launches - and autograd with the mirror image of them - as ONE forward and ONE backward launch per
(prediction, target) pair.  `harness.FUSED_LOSS` (AMMC_FUSED_LOSS=1, `run_train --fused_loss`) routes the harness here;
it is off by default.

* `prediction_terms(pred, target, gdl)` -> (int_mean, gdl_mean | None): the channel-L2 intensity term (`L2`,
  losses_utils.py:124-129) and, when asked, the gradient-difference term (`Gradient_Loss`, :30-61, alpha = 1) of one
  pair; differentiable in `pred` only.  The weights of the objective stay torch scalar arithmetic on the 0-d results.
* `l1_mean(a, b)`: `Flow_Loss` (:10-15), value only - both flows come out of a `no_grad` block.

The LSGAN terms (`adversarial_loss`, `discriminate_loss`, :100-110) act on [B, 1, 34, 34] patch maps - 37 k elements at
batch 32 - and stay in torch: there is no sweep to save.

HIP only: anything but CUDA fp32 dense tensors with 2 or 3 channels raises `AmmcHipError`; nothing here falls back to
torch.  Kernels run on `torch.cuda.current_stream()`; the partial-sum workspaces are cached per device, stream and size.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import AmmcHipError

_WS: Dict[tuple, torch.Tensor] = {}


def _workspace(dev: torch.device, stream: int, floats: int) -> torch.Tensor:
    key = (dev.index, stream, floats)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(floats, device=dev, dtype=torch.float32)
    return ws


def _need(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise AmmcHipError(f"losses: {name} must be a CUDA float32 tensor (HIP kernels only; there is no torch fallback here)")


def _batch_stride(target: torch.Tensor) -> int:
    """a target is contiguous, or the last frame of a contiguous clip batch (`clips[:, -1]`): dense samples, own batch stride"""
    b, c, h, w = target.shape
    if target.is_contiguous():
        return c * h * w
    if target.stride()[1:] == (h * w, w, 1) and target.stride(0) >= c * h * w:
        return target.stride(0)
    raise AmmcHipError("losses: target must be contiguous NCHW (or a batch-strided view with dense [C, H, W] samples)")


def _check_pair(pred: torch.Tensor, target: torch.Tensor) -> int:
    _need(pred, "pred")
    _need(target, "target")
    if pred.dim() != 4 or pred.shape != target.shape or pred.device != target.device:
        raise AmmcHipError(f"losses: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be equal [B, C, H, W] on one device")
    if pred.shape[1] not in (2, 3):
        raise AmmcHipError(f"losses: {pred.shape[1]} channels (the kernels take the frame's 3 and the flow's 2)")
    if not pred.is_contiguous():
        raise AmmcHipError("losses: pred must be contiguous NCHW")
    if pred.numel() == 0:
        raise AmmcHipError("losses: empty tensors")
    return _batch_stride(target)


class _PredictionTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, gdl):
        t_bs = _check_pair(pred, target)
        lib = _lib.load()
        b, c, h, w = pred.shape
        stream = torch.cuda.current_stream(pred.device).cuda_stream
        rows = lib.ammc_pred_loss_partial_rows(b, h, w)
        if rows <= 0:
            raise AmmcHipError(f"losses: shape {tuple(pred.shape)} is out of range")
        part = _workspace(pred.device, stream, 2 * rows)
        out = torch.empty(2, device=pred.device, dtype=torch.float32)
        _lib.check(lib.ammc_pred_loss_fwd_f32(pred.data_ptr(), target.data_ptr(), t_bs, b, c, h, w, int(gdl), part.data_ptr(),
                                              stream), "pred_loss_fwd")
        _lib.check(lib.ammc_reduce_partials_f32(part.data_ptr(), rows, 2, 1.0 / float(b * h * w), out.data_ptr(), stream),
                   "pred_loss combine")
        ctx.save_for_backward(pred, target)
        ctx.gdl = bool(gdl)
        ctx.set_materialize_grads(False)
        o_int, o_gdl = out[0], out[1]
        if not gdl:
            ctx.mark_non_differentiable(o_gdl)
        return o_int, o_gdl

    @staticmethod
    def backward(ctx, g_int, g_gdl):
        pred, target = ctx.saved_tensors
        if not ctx.gdl:
            g_gdl = None
        lib = _lib.load()
        b, c, h, w = pred.shape
        d_pred = torch.empty_like(pred)
        ptrs = []
        for g in (g_int, g_gdl):                        # upstream 0-d tensors are read on the device: no .item(), no sync
            if g is not None:
                g = g.to(device=pred.device, dtype=torch.float32).contiguous()
            ptrs.append(g)
        _lib.check(lib.ammc_pred_loss_bwd_f32(pred.data_ptr(), target.data_ptr(), _batch_stride(target),
                                              ptrs[0].data_ptr() if ptrs[0] is not None else None,
                                              ptrs[1].data_ptr() if ptrs[1] is not None else None, b, c, h, w,
                                              d_pred.data_ptr(), torch.cuda.current_stream(pred.device).cuda_stream),
                   "pred_loss_bwd")
        return d_pred, None, None


def prediction_terms(pred: torch.Tensor, target: torch.Tensor, gdl: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(mean channel-L2 norm of pred - target, mean gradient difference | None): 0-d tensors, differentiable in `pred`"""
    if isinstance(target, torch.Tensor) and target.requires_grad:
        raise AmmcHipError("losses: prediction_terms is differentiable in pred only (detach the target)")
    i, g = _PredictionTerms.apply(pred, target, bool(gdl))
    return i, (g if gdl else None)


def l1_mean(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """mean |a - b| as a 0-d tensor; value only (no gradient reaches a or b)"""
    _need(a, "a")
    _need(b, "b")
    if a.shape != b.shape or a.device != b.device or a.numel() == 0:
        raise AmmcHipError(f"losses: l1_mean needs two equal non-empty shapes on one device, got {tuple(a.shape)} / {tuple(b.shape)}")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise AmmcHipError("losses: l1_mean needs contiguous tensors")
    lib = _lib.load()
    n = a.numel()
    stream = torch.cuda.current_stream(a.device).cuda_stream
    nparts = (n + _lib.AMMC_L1_CHUNK - 1) // _lib.AMMC_L1_CHUNK
    part = _workspace(a.device, stream, nparts)
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    _lib.check(lib.ammc_l1_partials_f32(a.data_ptr(), b.data_ptr(), n, part.data_ptr(), stream), "l1_partials")
    _lib.check(lib.ammc_sum_partials_f32(part.data_ptr(), nparts, 1.0 / float(n), out.data_ptr(), stream), "l1 combine")
    return out[0]
