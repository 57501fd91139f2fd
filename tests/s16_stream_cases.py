"""Shapes and deterministic inputs of tests/test_gpu_s16_stream_kernels.py, shared with tests/test_s16_stream_refs_host.py
(which checks without a device that the grid references fit fp32 and that the codec facts hold on the cont inputs).

(B, H, W, C) of the S16 apply passes.  Row forms: one workgroup per image row of n = W * C/8 items, 256 threads, a trip =
1024 items (512 windows in the pool form); they need C/8 = 2^csh, else the one-item forms run:
  (1,1,1,8) the smallest case; (2,3,5,8) csh 0, dpx 256; (3,9,13,16) odd sizes; (2,16,24,64) the common case;
  (1,2,128,64) n = 1024 exactly; (1,2,130,64) n = 1040: a second trip that is mostly the re-load-item-0 path;
  (2,5,7,1024) csh 7, dpx 2, odd W; (1,4,9,1024) n = 1152; (2,4,6,24) and (2,10,12,72): C/8 = 3 and 9, the one-item forms"""
import numpy as np
import torch

from ammcnet_aaai2021_amd import synthetic as S

import stream_cases as K
import stream_refs as R

SHAPES = [(1, 1, 1, 8), (2, 3, 5, 8), (3, 9, 13, 16), (2, 16, 24, 64), (1, 2, 128, 64), (1, 2, 130, 64), (2, 5, 7, 1024),
          (1, 4, 9, 1024), (2, 4, 6, 24), (2, 10, 12, 72)]
POOL_SHAPES = [(1, 2, 2, 8), (2, 4, 6, 16), (1, 2, 130, 64), (1, 4, 18, 1024)]      # (1,2,130,64): 520 windows, a second trip
SEG_CASES = [(100, 128), (256, 128), (1000, 128), (1, 1)]                          # (rows, seg) of ammc_reduce_partials_seg_f32
SEG_QC = [16, 48, 136]
FINALIZE_CASES = [(1, 4), (129, 12), (1030, 1024), (1030, 12), (129, 1024)]          # (nblocks, C): RP_SLICES / RP_COLS tails
# the scale cases of the power-of-two factor: name -> (max |x|, its sign, where it is planted: "first" | "last")
SCALE_CASES = {"one": (1.0, 1, "first"), "below_one": (float(np.nextafter(np.float32(1), np.float32(0))), 1, "first"),
               "2^-30": (2.0 ** -30, 1, "first"), "subnormal": (2.0 ** -140, 1, "first"), "zero": (0.0, 1, "first"),
               "negative": (3.7, -1, "first"), "last_group": (5.0, 1, "last")}


def rows_form(c: int) -> bool:
    """C/8 a power of two <= 256 (`rows_csh` of train_kernels.hip, strides permitting)"""
    return c % 8 == 0 and K.is_pow2(c // 8) and c // 8 <= 256


def ssa_case(kind, shape):
    """x, res [B,H,W,C]; scale, shift [C].  grid: all on the 1/8 grid (x scale + shift is a multiple of 1/64 below 2: an
    exact fp16, so the twin has lo == 0)"""
    b, h, w, c = shape
    tag = f"ssa-{kind}-{b}-{h}-{w}-{c}"
    x, res = K.values(kind, tag + "x", shape), K.values(kind, tag + "r", shape)
    if kind == "grid":
        scale, shift = R.grid(tag + "s", (c,)), R.grid(tag + "h", (c,))
    else:
        scale = S.hashed_uniform(tag + "s", (c,), 0.5, 1.5) * K.pick(tag + "n", (c,), [-1.0, 1.0, 1.0])
        shift = S.hashed_normal(tag + "h", (c,), 0.5)
    return x, scale, shift, res


def pool_case(kind, shape):
    """x, scale, shift of the apply pass with a pooled output.  grid: the planted pairs of `pool_bwd_case` (the value 2 at
    the two positions of pair n % 6 in channels 0, 1 of window n) under scale 1, shift 0 in those two channels: y = x there,
    every other activation of the window is at most 1, and the pair ties at the window's maximum with or without ReLU"""
    b, h, w, c = shape
    tag = f"ssp-{kind}-{b}-{h}-{w}-{c}"
    x, _, _ = K.pool_bwd_case(kind, b, h, w, c)
    if kind == "grid":
        scale, shift = R.grid(tag + "s", (c,)), R.grid(tag + "h", (c,))
        scale[0:2], shift[0:2] = 1.0, 0.0
    else:
        scale = S.hashed_uniform(tag + "s", (c,), 0.5, 1.5) * K.pick(tag + "n", (c,), [-1.0, 1.0, 1.0])
        shift = S.hashed_normal(tag + "h", (c,), 0.5)
    return x, scale, shift


def unpool_case(kind, shape):
    """add [B,H,W,C], dpo [B,H/2,W/2,C], idx uint8 [B,H/2,W/2,C] hashed over {0,1,2,3}: with an odd H or W the windows of the
    last pooled row / column carry every position, the last full row / column included"""
    b, h, w, c = shape
    tag = f"unp-{kind}-{b}-{h}-{w}-{c}"
    ph, pw = h // 2, w // 2
    add, dpo = K.values(kind, tag + "a", shape), K.values(kind, tag + "p", (b, max(ph, 1), max(pw, 1), c))
    idx = torch.floor(S.hashed_uniform(tag + "i", (b, max(ph, 1), max(pw, 1), c), 0.0, 4.0).double()).clamp(max=3).to(torch.uint8)
    return add, dpo[:, :ph, :pw].contiguous(), idx[:, :ph, :pw].contiguous()


def unpool_grad(add, dpo, idx):
    """the gradient the unpool forms read, float64: add + scatter(dpo by idx)"""
    b, h, w, c = add.shape
    return R.d(add) + R.unpool2x2(dpo, idx, h, w)


def scale_values(name, shape, tag="sc"):
    """an fp32 tensor whose largest magnitude is exactly SCALE_CASES[name][0], planted with its sign in the first or the
    last group of 8; every other element is at most 0.9 of it"""
    amax, sign, where = SCALE_CASES[name]
    base = S.hashed_uniform(f"{tag}-{name}", shape, -0.9, 0.9).double()
    x = (base * amax).float()
    flat = x.view(-1)
    flat[3 if where == "first" else flat.numel() - 2] = sign * amax
    assert float(x.abs().max()) == float(np.float32(amax))
    return x


def codec_values(tag, n):
    """hashed fp32 values with |t| log-uniform over [1e-17, 65504] and a hashed sign"""
    u = S.hashed_uniform(tag + "m", (n,), 0.0, 1.0).double().numpy()
    s = np.where(S.hashed_uniform(tag + "s", (n,), -1.0, 1.0).numpy() < 0, -1.0, 1.0)
    lo, hi = np.log(1e-17), np.log(65504.0)
    return np.minimum(np.exp(lo + (hi - lo) * u), 65504.0).astype(np.float32) * s.astype(np.float32)
