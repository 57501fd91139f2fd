"""Shapes and deterministic inputs of tests/test_gpu_memory_kernels.py, shared with tests/test_memory_refs_host.py (which
proves, without a device, that the grid inputs make every intermediate value exactly representable in fp32 - the condition
under which the GPU test asks for bit equality - and that the cont inputs keep the share of ambiguous rows under 2 %).

kind "grid": features and codebook are hashed integers in [-8, 8] / 8 (`stream_refs.grid`): exact in half, lo = 0 in the S16
  split; distances, ranking keys and commit partials are small dyadic rationals.  Exact ties between slots are frequent on
  this grid, and that is intended: the kernels must break them exactly as the reference does (lower slot first).
kind "planted": grid, n >= m rows with x_r = E_(r mod m): every slot is the nearest neighbour of some row at distance 0, so
  every (slot tile, wave, lane half, accumulator register) position, slot m - 1 included, must be found.
kind "twins": planted, and a few slots duplicated (`twins`): each pair must come back as (lower slot, higher slot).
kind "cont": `synthetic.hashed_normal` (codebook std 0.9, features std 0.8, as in the existing parity tests)."""
from typing import NamedTuple

import torch

from ammcnet_aaai2021_amd import synthetic as S

import memory_refs as R

OPERAND = {"f32": "f32", "s16": "s16", "f16": "f16", "f16r": "f16"}
BLOCK = {"f32": 32, "s16": 32, "f16": 128, "f16r": 32}            # rows per commit partial
TILE_ROWS = 4099                                                   # large inputs repeat a block of this many rows (a prime)
MI355X_CUS = 256


class Case(NamedTuple):
    kernel: str
    kind: str
    n: int                       # 0: from the device's CU count (`sweeps`)
    d: int
    m: int
    k: int
    opt: tuple = ()              # (ammc_set_option key, value) in force for the launch
    sweeps: int = 0              # f16r: row tiles per wave (pw) the case must reach

    @property
    def id(self):
        o = "".join(f"-{key}{val}" for key, val in self.opt) + (f"-pw{self.sweeps}" if self.sweeps else "")
        return f"{self.kernel}-{self.kind}-n{self.n}-d{self.d}-m{self.m}-k{self.k}{o}"


def is_pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


def f16r_rt(case: Case) -> int:
    """row tiles a wave of memory_topk_f16r_kernel sweeps at a time: 2 in the packed-key form (K = 2, d = 512), else 3"""
    return 2 if (case.k == 2 and case.d == 512) else 3


def packed_keys(case: Case) -> bool:
    """memory_topk_f16r_kernel ranks on packed keys for K = 2, d >= 288 (`PACKED = K == 2 && NSTEP >= 18` in `r_sweep`, in
    the two- and the three-row-tile form alike; include/ammc_hip.h says the same): the winner among exactly tied candidates
    for the last place is open there.  Not to be confused with `f16r_rt`: the two-row-tile form with its pipelined
    write-out is built for d = 512 only, but d = 384 still ranks on packed keys"""
    return case.kernel == "f16r" and case.k == 2 and case.d >= 288


def rows(case: Case, cus: int = MI355X_CUS) -> int:
    """n of the case.  sweeps = pw: the smallest number of 32-row tiles with ceil(t32 / min(4 CUs, t32)) = pw, i.e.
    4 CUs (pw - 1) + 1 tiles, the last of them ragged (17 rows)"""
    if not case.sweeps:
        return case.n
    t32 = 4 * cus * (case.sweeps - 1) + 1
    return (t32 - 1) * 32 + 17


def twins(m: int):
    """(s, t), s < t: slot t is a copy of slot s.  In the same lane (s + 1), across the lane halves of a tile (s + 4), across
    a wave's tile pair (s + 32), across waves (s + 128), and with t = m - 1 in the last, ragged tile"""
    pairs = [(2, 3), (8, 12), (40, 72), (17, 145)]
    last = m - 1
    pairs.append((last - 1, last) if last % 32 >= 1 else (5, last))
    used, out = set(), []
    for s, t in pairs:
        if 0 <= s < t < m and s not in used and t not in used:
            used |= {s, t}
            out.append((s, t))
    return out


def inputs(case: Case, n: int = None):
    """x [n, d], E [d, m] fp32"""
    n = rows(case) if n is None else n
    tag = f"mem-{case.kernel}-{case.kind}-{case.d}-{case.m}-{case.k}-{case.n}"
    if case.kind == "cont":
        e = S.hashed_normal(tag + "e", (case.d, case.m), 0.9)
        nb = min(n, TILE_ROWS)
        x = S.hashed_normal(tag + "x", (nb, case.d), 0.8)
    else:
        e = R.grid(tag + "e", (case.d, case.m))
        if case.kind == "twins":
            for s, t in twins(case.m):
                e[:, t] = e[:, s]
        if case.kind == "grid":
            nb = min(n, TILE_ROWS)
            x = R.grid(tag + "x", (nb, case.d))
        else:
            nb = n
            x = e.t()[torch.arange(n) % case.m].contiguous()
    if nb < n:
        x = x[torch.arange(n) % nb].contiguous()
    return x, e


# ---- fp32: memory_topk_kernel<K> (32 rows per workgroup; wave w contracts slot tiles w, w + 4, ...; d = 64: double-buffered) ----
#   m = 1, 2, 31, 32: one tile, waves 1-3 idle; 33: two tiles (ragged); 128: four whole tiles, one per wave; 129, 160: wave 0
#   takes a second tile (the odd half of the d = 64 loop's unroll), ragged / whole; 257: nine tiles, wave 0 a third one
#   (back in the even half); 2000: the model's memory, 63 tiles.  n = 1, 31, 32, 33, 130: a ragged only / last workgroup.
#   d = 128, 192, 256 take the generic loop (d = 192: an odd number of 16-feature pairs does not exist: 24 groups, 12 trips)
_M = (1, 2, 31, 32, 33, 128, 129, 160, 257, 2000)
F32_CASES = (
    [Case("f32", "grid", 33, 64, m, min(2, m)) for m in _M] +
    [Case("f32", "grid", n, 64, 129, 4) for n in (1, 31, 32, 130)] +
    [Case("f32", "grid", 130, 128, 160, 3), Case("f32", "grid", 33, 192, 257, 1), Case("f32", "grid", 33, 256, 33, 4),
     Case("f32", "grid", 31, 64, 257, 3),
     Case("f32", "planted", 260, 64, 257, 2), Case("f32", "twins", 300, 64, 257, 2), Case("f32", "twins", 300, 64, 257, 3),
     Case("f32", "twins", 200, 128, 160, 4), Case("f32", "planted", 2000, 64, 2000, 1), Case("f32", "twins", 180, 192, 161, 2),
     Case("f32", "cont", 130, 64, 2000, 2), Case("f32", "cont", 33, 192, 257, 3), Case("f32", "cont", 130, 256, 160, 4),
     Case("f32", "cont", 32, 128, 33, 1)])

# ---- S16: memory_topk_s16_kernel<K, NL, RT> (d = 64) ---------------------------------------------------------------------
#   RT = 1: wave w contracts tile PAIRS (2 w, 2 w + 1), (2 w + 8, ...): m = 257 (9 tiles) gives wave 0 a second, half-empty
#   step; RT = 2 ("memory_rt" = 2; K <= 2, m <= 2048): 8 waves, one tile per step, 64 rows per workgroup, two commit
#   partials.  m = 4096: the norm cache full; m = 4100 (NL = false: norms from global memory) with K = 3
_RT1, _RT2 = (("memory_rt", 1),), (("memory_rt", 2),)
S16_CASES = (
    [Case("s16", "grid", 33, 64, m, min(2, m), _RT1) for m in _M] +
    [Case("s16", "grid", 130, 64, m, min(2, m), _RT2) for m in (1, 33, 129, 257, 2000)] +
    [Case("s16", "grid", n, 64, 129, 2, _RT2) for n in (1, 31, 33, 64, 65)] +
    [Case("s16", "grid", n, 64, 129, 4, _RT1) for n in (1, 31, 32, 130)] +
    [Case("s16", "grid", 33, 64, 4096, 3), Case("s16", "grid", 33, 64, 4100, 3),
     Case("s16", "twins", 300, 64, 257, 2, _RT1), Case("s16", "twins", 300, 64, 257, 2, _RT2), Case("s16", "twins", 300, 64, 257, 3),
     Case("s16", "planted", 2000, 64, 2000, 2, _RT2), Case("s16", "twins", 4100, 64, 4100, 4),
     Case("s16", "cont", 130, 64, 2000, 2, _RT1), Case("s16", "cont", 130, 64, 2000, 2, _RT2), Case("s16", "cont", 33, 64, 4100, 3),
     Case("s16", "cont", 96, 64, 129, 4)])

# ---- f16: memory_topk_f16_kernel / _split_kernel + memory_gather_f16_kernel (128 rows per workgroup, 8 waves, wave w
#   contracts tile pairs (2 w, 2 w + 1), (2 w + 16, ...)) ---------------------------------------------------------------------
#   slot tiles 1, 2, 3 (m = 20, 64, 70: waves idle, a pair half empty), 16, 17, 18 (m = 512, 540, 570: every wave one pair,
#   wave 0 a second), 33 (m = 1050: a third trip); n = 1, 127, 128, 129, 300; "memory_split" = 1 at 1024 rows (one chunk)
#   and at 32768 + 130 rows (258 workgroups: chunks are whole rounds of 256, so a second chunk of two workgroups, the last
#   of them with 2 rows)
_SPLIT = (("memory_split", 1),)
F16_CASES = [
    Case("f16", "grid", 129, 128, 20, 2), Case("f16", "grid", 1, 128, 64, 1), Case("f16", "grid", 127, 256, 70, 3),
    Case("f16", "grid", 128, 384, 512, 2), Case("f16", "grid", 300, 512, 540, 2), Case("f16", "grid", 129, 128, 570, 4),
    Case("f16", "grid", 130, 256, 1050, 2),
    Case("f16", "twins", 600, 128, 570, 2), Case("f16", "twins", 300, 512, 161, 3), Case("f16", "planted", 1050, 384, 1050, 1),
    Case("f16", "grid", 1024, 512, 70, 2, _SPLIT), Case("f16", "twins", 1024, 128, 570, 2, _SPLIT),
    Case("f16", "grid", 32768 + 130, 128, 40, 2, _SPLIT),
    Case("f16", "cont", 300, 512, 1050, 2), Case("f16", "cont", 129, 128, 570, 3), Case("f16", "cont", 128, 384, 70, 1),
    Case("f16", "cont", 1024, 256, 540, 2, _SPLIT)]

# ---- f16r: memory_topk_f16r_kernel (a wave keeps RT row tiles in registers, codebook tiles through a ring of 4 in LDS) -----
#   slot tiles 1, 2, 3, 4 (the ring exactly), 5 (the first re-used buffer), 8, 9 (m = 20, 64, 70, 128, 150, 256, 270);
#   n = 1, 31, 33 (one wave), 96, 97 (three / four waves of one workgroup), 129, 300 (two and three workgroups);
#   K = 2 at d = 512: the packed-key form (two row tiles per wave, write-out pipelined behind the next sweep); K = 3 at
#   d = 128: the compare-and-branch form.  sweeps = RT + 1: more than one sweep per wave
F16R_CASES = [
    Case("f16r", "grid", 1, 128, 20, 1), Case("f16r", "grid", 31, 128, 64, 3), Case("f16r", "grid", 33, 256, 70, 2),
    Case("f16r", "grid", 96, 384, 128, 2), Case("f16r", "grid", 97, 512, 150, 2), Case("f16r", "grid", 129, 512, 256, 4),
    Case("f16r", "grid", 300, 128, 270, 3), Case("f16r", "grid", 300, 512, 270, 2), Case("f16r", "grid", 97, 384, 270, 3),
    Case("f16r", "twins", 300, 128, 270, 3), Case("f16r", "twins", 300, 512, 270, 2), Case("f16r", "twins", 300, 256, 270, 2),
    Case("f16r", "planted", 300, 384, 150, 1),
    Case("f16r", "grid", 0, 128, 160, 3, (), 4), Case("f16r", "grid", 0, 512, 160, 2, (), 3),
    # ... and the write-out that rides along with the next sweep's slot tiles (`TAIL_INLINE`: K = 2, d = 512, a unit per
    # slot tile, so 64 slot tiles per carried row tile: m >= 4065 for two); m = 4100: 129 tiles, the last with 4 slots.
    # With m = 160 above the carried rows are written by `r_tail_tile` at the start of the next sweep instead
    Case("f16r", "grid", 0, 512, 4100, 2, (), 3),
    Case("f16r", "cont", 300, 512, 270, 2), Case("f16r", "cont", 129, 128, 256, 3), Case("f16r", "cont", 97, 384, 150, 4),
    Case("f16r", "cont", 33, 256, 70, 1)]

TOPK_CASES = F32_CASES + S16_CASES + F16_CASES + F16R_CASES

# ---- the packers: (d, m) -------------------------------------------------------------------------------------------------
PACK_SHAPES = [(64, 1), (64, 33), (64, 2000), (128, 64), (192, 257), (512, 270)]

# ---- ammc_sum_partials_f32: number of partials (one thread, a ragged stride, several strides) ------------------------------
SUM_COUNTS = [1, 255, 256, 257, 2049]

# ---- ammc_memory_block_s16: c = 512, d = 64, k = 2; (B, H, W): a whole 64-pixel tile, one ragged tile, ragged tiles across
#   images; m = 33 (two slot tiles: six waves idle in the sweep), 256 (one tile per wave), 2048 (the norm cache full) --------
BLOCK_AMBIGUOUS_CAP = 0.25     # the cont block case: z's bound rides on every distance (tests/test_memory_refs_host.py)
BLOCK_CASES = [("grid", (1, 8, 8), 33), ("grid", (1, 9, 7), 256), ("grid", (2, 18, 18), 2048), ("planted", (2, 18, 18), 256),
               ("cont", (1, 9, 7), 256)]


def block_inputs(kind, bhw, m, c=512, dim=64, k=2):
    """x [B, H, W, c], enc_w [d, c], enc_b [d], E [d, m], dec_w [c, k d], dec_b [c].
    grid / planted: signed-selection filters - enc row j holds one +-1 (j even) or two +-1/2 (j odd), dec row likewise -
    with grid activations, codebook and biases: z = x enc^T + b and y stay on a grid fp32 holds exactly (multiples of 1/16
    below 4).  planted: pixel p's features are built so that z_p = E_(p mod m): the selected channels carry E - b.
    cont: hashed uniform filters of the model's own scale"""
    b, h, w = bhw
    n = b * h * w
    tag = f"mblk-{kind}-{b}-{h}-{w}-{m}"
    if kind == "cont":
        x = S.hashed_normal(tag + "x", (b, h, w, c), 0.7)
        enc_w = S.hashed_uniform(tag + "ew", (dim, c), -(3.0 / c) ** 0.5, (3.0 / c) ** 0.5)
        dec_w = S.hashed_uniform(tag + "dw", (c, k * dim), -(3.0 / (k * dim)) ** 0.5, (3.0 / (k * dim)) ** 0.5)
        enc_b, dec_b = S.hashed_uniform(tag + "eb", (dim,), -0.1, 0.1), S.hashed_uniform(tag + "db", (c,), -0.1, 0.1)
        e = S.hashed_normal(tag + "e", (dim, m), 0.9)
        return x, enc_w, enc_b, e, dec_w, dec_b

    def selection(rows_, cols, t, single_cols=None):
        wsel = torch.zeros(rows_, cols)
        r = torch.arange(rows_)
        c0 = torch.floor(S.hashed_uniform(t + "c0", (rows_,), 0.0, float(cols))).long().clamp(max=cols - 1)
        if single_cols is not None:
            c0 = single_cols
        c1 = (c0 + 1 + torch.floor(S.hashed_uniform(t + "c1", (rows_,), 0.0, float(cols - 1))).long().clamp(max=cols - 2)) % cols
        sg0 = torch.where(S.hashed_uniform(t + "s0", (rows_,)) < 0, -1.0, 1.0)
        sg1 = torch.where(S.hashed_uniform(t + "s1", (rows_,)) < 0, -1.0, 1.0)
        two = (r % 2 == 1) if single_cols is None else torch.zeros(rows_, dtype=torch.bool)
        wsel[r, c0] = torch.where(two, 0.5 * sg0, sg0)
        wsel[r[two], c1[two]] = 0.5 * sg1[two]
        return wsel, c0, sg0

    x = R.grid(tag + "x", (b, h, w, c))
    e = R.grid(tag + "e", (dim, m))
    enc_b, dec_b = R.grid(tag + "eb", (dim,)), R.grid(tag + "db", (c,))
    dec_w, _, _ = selection(c, k * dim, tag + "dw")
    if kind == "planted":
        # one +-1 per enc row, on DISTINCT channels 8 j + 3: z_j = sg_j x[8 j + 3] + b_j, so x[8 j + 3] = sg_j (E_j - b_j)
        enc_w, c0, sg = selection(dim, c, tag + "ew", single_cols=8 * torch.arange(dim) + 3)
        want = e.t()[torch.arange(n) % m]                                      # [n, d]
        x.view(n, c)[:, c0] = sg[None, :] * (want - enc_b[None, :])
    else:
        enc_w, _, _ = selection(dim, c, tag + "ew")
    return x, enc_w, enc_b, e, dec_w, dec_b
