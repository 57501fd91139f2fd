"""Shapes and deterministic inputs of tests/test_gpu_stream_kernels.py, shared with tests/test_stream_refs_host.py (which
checks, without a device, that the grid inputs make every reference result exactly representable in fp32 - the
condition under which the GPU test may ask for bit equality).

kind "grid": values on a coarse dyadic grid (hashed integers in [-8, 8] / 8) and parameters that are powers of two or
grid values, so every fp32 operation of the kernels is exact.  kind "cont": `synthetic.hashed_normal`."""
import torch

from ammcnet_aaai2021_amd import synthetic as S

import stream_refs as R

# (B, H, W, C) of the per-channel reductions (chan_reduce_kernel: thread = (C/4 channel groups, PY = 256 / (C/4) pixel lanes),
# U = 8 (4 in the backward) pixel streams per thread, a trip = gridDim * U * PY pixels):
#   (1,1,1,4) one pixel; (1,3,3,12) C/4 = 3 leaves thread 255 idle; (2,16,24,64) the common case; (3,9,13,512) four trips,
#   both carries, a guarded last trip; (2,5,7,1024) PY = 1; W = 1 / H = 1; (1,8,8,1024) M = 64 = a whole number of trips (no
#   guarded trip, U = 8 and U = 4 alike); (4,4,8,12) and (2,16,32,64): power-of-two pixel counts (1/M exact)
CHAN_SHAPES = [(1, 1, 1, 4), (1, 3, 3, 12), (2, 16, 24, 64), (3, 9, 13, 512), (2, 5, 7, 1024), (1, 1, 70, 16), (1, 70, 1, 16),
               (1, 8, 8, 1024), (4, 4, 8, 12), (2, 16, 32, 64)]

# (N, D, M, k, index pattern) of the EMA accumulation (ema_accumulate_kernel: 16 waves, a wave's rows = a chunk rounded to 64,
# four 64-row index streams per trip, hits drained four at a time, features lane + 64 j < D)
EMA_CASES = [(1, 64, 7, 1, "uniform"), (128, 64, 256, 2, "half"), (1030, 100, 40, 2, "one"), (1030, 100, 40, 2, "uniform"),
             (4200, 256, 33, 3, "last"), (4200, 256, 33, 3, "one"), (2048, 20, 256, 2, "uniform")]

COMMIT_CASES = [(1, 4, 1), (130, 64, 2), (257, 100, 3)]
POOL_BWD_SIZES = [(4, 6), (5, 7), (2, 3), (3, 2)]           # full sizes with at least one window
PREP_SHAPES = [(1, 3, 3), (2, 8, 16), (3, 17, 23)]
UP_SHAPES = [(1, 1), (1, 5), (4, 1), (6, 7)]


def is_pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


def values(kind, tag, shape, std=1.0):
    return R.grid(tag, shape) if kind == "grid" else S.hashed_normal(tag, shape, std)


def pick(tag, shape, choices):
    """hashed choice among a few fp32 values"""
    i = torch.floor(S.hashed_uniform(tag, shape, 0.0, float(len(choices))).double()).clamp(max=len(choices) - 1).long()
    return torch.tensor(choices, dtype=torch.float32)[i]


def bn_bwd_case(kind, shape, relu):
    """x, dy [B,H,W,C]; mean, invstd, scale, shift [C].  grid: mean a multiple of 1/8, invstd in {0.5, 1, 2}, scale and
    shift on the grid, and (relu) element (0,0,0,0) has pre == 0 exactly with a non-zero gradient: masked, as pre > 0 asks"""
    b, h, w, c = shape
    tag = f"bnb-{kind}-{b}-{h}-{w}-{c}"
    x, dy = values(kind, tag + "x", shape), values(kind, tag + "g", shape)
    if kind == "grid":
        mean, invstd = R.grid(tag + "m", (c,)), pick(tag + "i", (c,), [0.5, 1.0, 2.0])
        scale, shift = R.grid(tag + "s", (c,)), R.grid(tag + "h", (c,))
        x[0, 0, 0, 0], shift[0], dy[0, 0, 0, 0] = 0.0, 0.0, 1.0
    else:
        mean, invstd = S.hashed_normal(tag + "m", (c,), 0.5), S.hashed_uniform(tag + "i", (c,), 0.5, 2.0)
        scale = S.hashed_uniform(tag + "s", (c,), 0.5, 1.5) * invstd * pick(tag + "n", (c,), [-1.0, 1.0, 1.0])
        shift = S.hashed_normal(tag + "h", (c,), 0.5)
    return x, dy, mean, invstd, scale, shift


def bn_apply_sums(kind, shape):
    """the [2][C] sums `ammc_bn_bwd_apply_f32` is given (an input of that kernel: any values serve)"""
    b, h, w, c = shape
    tag = f"bna-{kind}-{b}-{h}-{w}-{c}"
    if kind == "grid":
        return R.grid(tag + "sg", (c,)), R.grid(tag + "sx", (c,))
    m = b * h * w
    return S.hashed_normal(tag + "sg", (c,), m ** 0.5), S.hashed_normal(tag + "sx", (c,), m ** 0.5)


def pool_bwd_case(kind, b, fh, fw, c):
    """x, dp, add.  grid: besides the ties the grid itself has, window n of the batch holds the value 2 (above the grid) at
    the two positions of pair n % 6 of ((0,1),(0,2),(0,3),(1,2),(1,3),(2,3)) in channels 0, 1: the first of the two wins.
    cont: no ties (distinct hashed values)"""
    tag = f"mpb-{kind}-{b}-{fh}-{fw}-{c}"
    h, w = fh // 2, fw // 2
    x = values(kind, tag + "x", (b, fh, fw, c))
    if kind == "grid":
        pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
        n = 0
        for bb in range(b):
            for yy in range(h):
                for xx in range(w):
                    for p in pairs[n % 6]:
                        x[bb, 2 * yy + (p >> 1), 2 * xx + (p & 1), 0:2] = 2.0
                    n += 1
    return x, values(kind, tag + "p", (b, h, w, c)), values(kind, tag + "a", (b, fh, fw, c))


def ema_indices(n, m, k, pattern, chunk):
    """idx [N, k] int32: column 0 = the nearest slot the kernels read, the other columns other slots (never read).
    "uniform": hashed over all slots; "half": even slots only; "one": every row on slot m // 2 (64 hits per ballot, the
    four-at-a-time drain all the way); "last": slot m - 1 is hit only by rows of the last 64 of a wave's chunk."""
    tag = f"emai-{n}-{m}-{k}-{pattern}"
    u = torch.floor(S.hashed_uniform(tag, (n,), 0.0, float(m)).double()).clamp(max=m - 1).long()
    if pattern == "half":
        u = (u // 2) * 2
    elif pattern == "one":
        u = torch.full((n,), m // 2, dtype=torch.int64)
    elif pattern == "last":
        rows = torch.arange(n)
        u = u % (m - 1)
        u[((rows % chunk) >= chunk - 64) & (rows % 3 == 0)] = m - 1
    cols = [(u + 1 + j) % m for j in range(k)]
    cols[0] = u
    return torch.stack(cols, 1).to(torch.int32).contiguous()


def ema_chunk(n):
    return ((n + 15) // 16 + 63) // 64 * 64            # rows per wave (EMA_NW = 16)


def ema_case(kind, n, dim, m, k, pattern):
    tag = f"ema-{kind}-{n}-{dim}-{m}-{pattern}"
    x = values(kind, tag + "x", (n, dim))
    idx = ema_indices(n, m, k, pattern, ema_chunk(n))
    if kind == "grid":
        cs = torch.floor(S.hashed_uniform(tag + "c", (m,), 0.0, 9.0)).float()          # integers 0..8
        ea = R.grid(tag + "a", (dim, m))
        decay = 0.5
    else:
        cs = S.hashed_uniform(tag + "c", (m,), 0.5, 4.0)
        ea = S.hashed_normal(tag + "a", (dim, m), 0.9)
        decay = 0.99
    return x, idx, cs, ea, decay


def commit_case(kind, n, dim, k, m=16):
    tag = f"cmt-{kind}-{n}-{dim}-{k}"
    z, e, dq = values(kind, tag + "z", (n, dim)), values(kind, tag + "e", (m, dim)), values(kind, tag + "q", (n, dim))
    idx = ema_indices(n, m, k, "uniform", 64)
    ddiff = torch.tensor([0.5 if kind == "grid" else 0.7310586])
    return z, e, idx, ddiff, dq


def prep_case(kind, b, h, w):
    """inputs [B, 3, 2, H, W] in 0..255.  grid: integers whose sum over each (sample, colour) is a multiple of 2HW (element 0
    absorbs the remainder), so the mean is an integer and (x - mean) / 256 exact"""
    tag = f"prep-{kind}-{b}-{h}-{w}"
    if kind == "cont":
        return S.hashed_uniform(tag, (b, 3, 2, h, w), 0.0, 255.0)
    x = torch.floor(S.hashed_uniform(tag, (b, 3, 2, h, w), 0.0, 256.0).double()).clamp(max=255)
    flat = x.view(b, 3, -1)
    n = 2 * h * w
    flat[:, :, 0] += (n - flat.sum(-1) % n) % n
    return x.float()
