"""Plain fp64 references of the memory-addressing kernels (csrc/memory_topk.hip, memory_topk_s16.hip, memory_topk_f16.hip,
memory_topk_f16r.hip, the codebook packers and `ammc_sum_partials_f32` of layout_pool.hip).

torch float64 on CPU tensors, written with indexing, matrix products and sorts only.  tests/test_memory_refs_host.py checks
them against torch.topk / the oracle and proves the representability the GPU test's bit equalities rest on;
tests/test_gpu_memory_kernels.py checks the HIP kernels against them.  x is [n, d] (feature rows), E is the module's own
codebook buffer [d, m]; semantics are those of the kernel comments and include/ammc_hip.h."""
import math

import torch

from stream_refs import F64, d as _d, fits_f32, grid  # noqa: F401  (re-exported: one set of helpers for both families)

U = 2.0 ** -24                    # unit roundoff of fp32
S_LO = 2048.0                     # the S16 split: v ~ hi + lo / 2048, hi = half(v), lo = half((v - hi) 2048)


def gamma(n: int) -> float:
    """n u / (1 - n u): the factor of a value that passed through at most n fp32 roundings (Higham, Accuracy and Stability,
    lemma 3.1)"""
    return n * U / (1.0 - n * U)


def half(t):
    """round to nearest-even half, as fp64 (what `(_Float16)v` does to an fp32 v)"""
    return torch.as_tensor(t).detach().to("cpu", torch.float32).half().double()


def s16_split(t):
    """(hi, lo) of the documented split, as fp64.  v - hi is exact in fp32 (hi is v rounded to 11 bits) and so is the
    product with 2048; the one rounding is the conversion of that product to half"""
    v = torch.as_tensor(t).detach().to("cpu", torch.float32)
    hi = v.half()
    lo = ((v.double() - hi.double()) * S_LO).half()
    return hi.double(), lo.double()


def s16_value(t):
    hi, lo = s16_split(t)
    return hi + lo / S_LO


# ---- ranking -----------------------------------------------------------------------------------------------------------

def operands(x, e_dm, operand):
    """(x for the dot product, E for the dot product, |x|^2, |E|^2) as the kernel's contract rounds them"""
    x, e = _d(x), _d(e_dm)
    if operand == "f32":
        return x, e, (x * x).sum(1), (e * e).sum(0)
    if operand == "s16":                       # rounded operands in the dot product only: the norms are the fp32 data's
        return s16_value(x), s16_value(e), (x * x).sum(1), (e * e).sum(0)
    if operand == "f16":                       # the ranking sees half(x), half(E) and |half(E)|^2
        xh, eh = half(x), half(e)
        return xh, eh, (xh * xh).sum(1), (eh * eh).sum(0)
    raise ValueError(operand)


def topk_ref(x, e_dm, k, operand="f32"):
    """dist = (|x|^2 - 2 x.E) + |E|^2 in float64 from the rounded operands, ranked lexicographically on (distance, slot).
    Returns idx [n, k] int64, the sorted distances [n, m] and the distance matrix [n, m]"""
    xo, eo, xx, ee = operands(x, e_dm, operand)
    dist = (xx[:, None] - 2.0 * (xo @ eo)) + ee[None, :]
    srt, order = torch.sort(dist, dim=1, stable=True)            # stable: equal distances stay in slot order
    return order[:, :k].contiguous(), srt, dist


def gather_ref(e_dm, idx):
    """q_topk [n, k d]: the codebook rows of the returned slots, nearest first"""
    e_md = _d(e_dm).t().contiguous()
    n, k = idx.shape
    return e_md[idx.long().reshape(-1)].reshape(n, k * e_md.shape[1])


def commit_ref(x, e_dm, idx, block):
    """q_one = x + (E_i0 - x), the per-`block`-rows partial sums of (E_i0 - x)^2, diff = their sum / (n d)"""
    x = _d(x)
    n, dim = x.shape
    df = _d(e_dm).t()[idx[:, 0].long()] - x
    sq = (df * df).sum(1)
    nb = (n + block - 1) // block
    part = torch.zeros(nb * block, dtype=F64)
    part[:n] = sq
    part = part.view(nb, block).sum(1)
    return x + df, part, part.sum() / (n * dim)


def block_ref(x, enc_w, enc_b, e_dm, dec_w, dec_b, k, round_z=True):
    """The whole memory block on NHWC activations x [B, H, W, c]: z = x enc_w^T + enc_b (enc_w [d, c]), the S16 lookup of z,
    y = [E_i0 | E_i1 | ...] dec_w^T + dec_b + x (dec_w [c, k d]).  round_z: z is an fp32 tensor in the kernel's contract -
    the lookup, q_one and the commit distance see it rounded to fp32"""
    x = _d(x)
    b, h, w, c = x.shape
    z = x.reshape(-1, c) @ _d(enc_w).t() + _d(enc_b)
    if round_z:
        z = z.float().double()
    idx, srt, dist = topk_ref(z, e_dm, k, "s16")
    qk = gather_ref(e_dm, idx)
    q1, part, diff = commit_ref(z, e_dm, idx, 32)
    y = (qk @ _d(dec_w).t() + _d(dec_b)).reshape(b, h, w, c) + x
    return {"z": z, "idx": idx, "srt": srt, "dist": dist, "q_topk": qk, "q_one": q1, "diff_partial": part, "diff": diff, "y": y}


# ---- error bounds ------------------------------------------------------------------------------------------------------

def dist_error_bound(operand, dim, x, e_dm, packed=False):
    """Forward error bound [n, m] of the kernel's distance of row r to slot s against `topk_ref(..., operand)`.

    Every kernel evaluates a sum of terms in fp32; a term that passes through at most c roundings on its way into the
    result carries a relative error of at most gamma(c), whatever the order of the additions.  With A = sum_i |x_i E_i|
    over the operands the dot product sees:

    "f32" (memory_topk.hip): |x|^2 and |E|^2 are sequential sums of d rounded squares (d roundings per term: the square and
      d - 1 additions, counted as d), x.E is an MFMA accumulation of d products (d roundings), then (|x|^2 - 2 x.E) + |E|^2
      adds two roundings (the factor 2 is exact):             B = gamma(d + 2) (|x|^2 + 2 A + |E|^2)
    "s16" (memory_topk_s16.hip): the norms as above.  x.E is the accumulation of the 3 d products hi hi, lo (hi 2^-11),
      hi (lo 2^-11) - products of halfs, exact in fp32 - so 3 d + 2 roundings per term; the reference's lo lo 2^-22 term is
      dropped: 2^-22 sum |lo_x lo_E| exactly; and the operands hi_x 2^-11, lo_x 2^-11 are formed in HALF precision: exact
      unless the result is subnormal (below 2^-14), then off by at most half a subnormal spacing, 2^-25, times the other
      factor:  B = gamma(d + 2) (|x|^2 + |E|^2) + 2 [gamma(3 d + 2) A3 + 2^-22 sum |lo_x lo_E| + 2^-25 sum (|lo_E| + |hi_E|)]
      with A3 = sum |hi_x hi_E| + 2^-11 (|hi_x lo_E| + |lo_x hi_E|).
    "f16" (memory_topk_f16.hip ranks fma(acc, -2, |half E|^2); memory_topk_f16r.hip ranks the key acc that starts at
      -|half E|^2 / 2): products of halfs are exact; |half E|^2 is a sequential fp32 sum of d exact squares; the d
      products join by MFMA accumulation; one more rounding (the fma, or the halving's - exact - plus the start value's
      trip through the accumulator).  |half x|^2 is a constant of the row, added exactly by the test:
                                                              B = gamma(d + 1) (2 A + |half E|^2)
      packed = True (memory_topk_f16r.hip, K = 2 at d >= 288): the four lowest mantissa bits of the key are replaced by a
      register tag: at most 15 ulp = 15 2^-23 of |key| = |x.E - |E|^2 / 2|, twice that in the distance."""
    x, e = _d(x), _d(e_dm)
    if operand == "f32":
        a = x.abs() @ e.abs()
        return gamma(dim + 2) * ((x * x).sum(1)[:, None] + 2.0 * a + (e * e).sum(0)[None, :])
    if operand == "s16":
        hx, lx = s16_split(x)
        he, le = s16_split(e)
        hx, lx, he, le = hx.abs(), lx.abs(), he.abs(), le.abs()
        a3 = hx @ he + (hx @ le + lx @ he) / S_LO
        extra = 2.0 ** -22 * (lx @ le) + 2.0 ** -25 * (le.sum(0) + he.sum(0))[None, :]
        return gamma(dim + 2) * ((x * x).sum(1)[:, None] + (e * e).sum(0)[None, :]) + 2.0 * (gamma(3 * dim + 2) * a3 + extra)
    if operand == "f16":
        xh, eh = half(x), half(e)
        ee = (eh * eh).sum(0)[None, :]
        b = gamma(dim + 1) * (2.0 * (xh.abs() @ eh.abs()) + ee)
        if packed:
            b = b + 2.0 * 15.0 * 2.0 ** -23 * (xh @ eh - 0.5 * ee).abs()
        return b
    raise ValueError(operand)


def ambiguous_rows(k, m, srt, bound):
    """rows whose first k + 1 sorted distances hold a gap of at most 2 B: the kernel may legitimately order or choose
    differently there.  B is the row's LARGEST bound, not that of the two slots next to the gap: the kernel's k-th place
    can go to any slot whose computed distance falls below, so the slot that displaces the reference's choice need not be
    the reference's (k + 1)-th, and only a bound that holds for every slot of the row makes `gap > 2 B` imply the same
    order (order statistics move by at most the largest perturbation).  Any gap among the first k + 1 counts, since the
    test then asks for the same ORDER of the k slots; where only the gap behind the k-th exceeds 2 B the test still asks
    for the same set."""
    gaps = srt[:, 1:k] - srt[:, :k - 1] if m == k else srt[:, 1:k + 1] - srt[:, :k]
    if gaps.shape[1] == 0:
        return torch.zeros(srt.shape[0], dtype=torch.bool)
    return gaps.min(1).values <= 2.0 * bound.max(1).values


def commit_chain(kernel, dim, k):
    """roundings a term (E_i0 - x)^2 passes through on its way into a commit partial: the difference, the square, the
    thread's own additions (4 per loop trip) and the levels of the reduction tree - read off each kernel's gather loop"""
    if kernel in ("f32", "s16", "block"):                 # 256 threads per 32 rows walk 32 K d/4 pieces; 8 tree levels
        trips, levels = -(-32 * k * (dim // 4) // 256), 8
    elif kernel == "f16":                                 # 512 threads per 128 rows; 9 levels
        trips, levels = -(-128 * k * (dim // 4) // 512), 9
    elif kernel == "f16_split":                           # memory_gather_f16_kernel: 256 threads per 128 rows; 8 levels
        trips, levels = -(-128 * k * (dim // 4) // 256), 8
    elif kernel == "f16r":                                # a wave per 32 rows: 32 ceil(d / 256) units per lane; 6 shuffles
        trips, levels = 32 * (-(-dim // 256)), 6
    else:
        raise ValueError(kernel)
    return 2 + 4 * trips + levels


def block_z_bound(xv, enc_w, enc_b):
    """`ammc_memory_block_s16`, enc 1x1: forward error bound [n, d] of the kernel's fp32 z against x enc_w^T + enc_b in
    float64, both from the S16 operands' VALUES xv [n, c], enc_w [d, c] (hi + lo / 2048: what the kernel is given).
    Per output the kernel accumulates the 3 c products hi hi, lo hi, hi lo (products of halfs: exact) in two fp32 MFMA
    accumulators that are joined (3 c + 1 roundings), then adds the bias (one more): gamma(3 c + 2) on sum |x| |w| + |b|;
    the lo lo products are dropped: 2^-22 sum |lo_x lo_w| exactly."""
    c = xv.shape[1]
    lx, lw = s16_split(xv.float())[1].abs(), s16_split(enc_w.float())[1].abs()
    return gamma(3 * c + 2) * (xv.abs() @ enc_w.abs().t() + _d(enc_b).abs()) + 2.0 ** -22 * (lx @ lw.t())


def block_dist_bound(z, e_dm, bz):
    """bound [n, m] of the block's distance of pixel r to slot s against `topk_ref(z, E, "s16")` on the float64 z: the
    distance is sum_i (z_i - E_i)^2 up to what `dist_error_bound` covers; moving z_i by at most bz_i moves it by at most
    2 sum_i bz_i |z_i - E_i| + sum_i bz_i^2, on top of `dist_error_bound("s16")` at z"""
    dim = z.shape[1]
    shift = 2.0 * torch.einsum("ni,nim->nm", bz, (z[:, :, None] - _d(e_dm)[None]).abs()) + (bz * bz).sum(1, keepdim=True)
    return dist_error_bound("s16", dim, z, e_dm) + shift


def block_q_one_bound(z, e0, bz):
    """q_one = fl(z~ + fl(E - z~)) on the kernel's z~ (|z~ - z| <= bz) against z + (E - z): E - z~ is off by bz, its
    rounding by u (|E| + |z~|), the sum's by u |q_one| <= u (|E| + ...): bz + 3 u (|z| + |E|) covers both and the second
    order terms"""
    return bz + 3 * U * (z.abs() + e0.abs())


def block_partial_bound(z, e0, bz, n_blocks, chain):
    """(exact partials [nb], bound [nb]) of the block's 32-row commit partials: a term (E - z)^2 moves by at most
    (2 |E - z| + bz) bz when z moves by bz (summed: wd); the moved sum then passes through `chain` roundings
    (`commit_chain("block")`): gamma(chain) (partial + wd) + wd"""
    n = z.shape[0]
    df = (e0 - z).abs()
    pad = torch.zeros(n_blocks * 32, dtype=F64)
    wpart, wd = pad.clone(), pad.clone()
    wpart[:n], wd[:n] = (df * df).sum(1), ((2 * df + bz) * bz).sum(1)
    wpart, wd = wpart.view(n_blocks, 32).sum(1), wd.view(n_blocks, 32).sum(1)
    return wpart, gamma(chain) * (wpart + wd) + wd


def block_y_bound(qv, dec_w, dec_b, xres, ywant):
    """dec 1x1 + bias + residual from the RETURNED slots' rows qv [n, k d], dec_w [c, k d] and xres [n, c] (S16 values):
    the gathered rows are split to S16 in the kernel (2^-22 relative per operand, and the dropped lo lo term of the same
    size: 2^-21 on sum |q| |w|), 3 k d + 1 accumulation roundings, the bias, the residual (its hi + lo / 2048 is one
    rounding more): gamma(3 k d + 5) on sum |q| |w| + |b| + |x|; y is stored as an S16 pair: 2^-22 |y|"""
    kd = qv.shape[1]
    mag = qv.abs() @ dec_w.abs().t()
    return gamma(3 * kd + 5) * (mag + _d(dec_b).abs() + xres.abs()) + 2.0 ** -21 * mag + 2.0 ** -22 * ywant.abs()


# ---- pack references ---------------------------------------------------------------------------------------------------

def mpad_of(m):
    return (m + 31) // 32 * 32


def pack_f32_ref(e_dm):
    """`ammc_pack_codebook_f32`: rows [m][d] and |E_s|^2 (fp64)"""
    e = _d(e_dm)
    return e.t().contiguous(), (e * e).sum(0)


def pack_s16_ref(e_dm):
    """`ammc_pack_codebook_s16`: [d/8][hi | lo][mpad][8] halfs, slots >= m zero"""
    dim, m = e_dm.shape
    hi, lo = s16_split(e_dm)
    out = torch.zeros(dim // 8, 2, mpad_of(m), 8, dtype=torch.float16)
    out[:, 0, :m] = hi.half().view(dim // 8, 8, m).permute(0, 2, 1)
    out[:, 1, :m] = lo.half().view(dim // 8, 8, m).permute(0, 2, 1)
    return out


def pack_f16_ref(e_dm):
    """`ammc_pack_codebook_f16`: [d/8][mpad][8] halfs (slots >= m zero) and |half(E_s)|^2 (fp64, [m])"""
    dim, m = e_dm.shape
    eh = half(e_dm)
    out = torch.zeros(dim // 8, mpad_of(m), 8, dtype=torch.float16)
    out[:, :m] = eh.half().view(dim // 8, 8, m).permute(0, 2, 1)
    return out, (eh * eh).sum(0)


def pack_f16_tiles_ref(e_dm):
    """`ammc_pack_codebook_f16_tiles`: per tile of 32 slots, d/16 KB of fragments - KB t, lane (l31, h): the 8 halfs of slot
    32 T + l31, features 16 t + 8 h .. + 7 - and one KB of constants: float i < 32 = -|half(E_{32 T + i})|^2 / 2 (-3e38 for
    slots >= m), zeros after float 32.  Returns (halfs [T][d/16][64][8], constants [T][256] fp64)"""
    dim, m = e_dm.shape
    nt, ns = mpad_of(m) // 32, dim // 16
    eh = torch.zeros(dim, nt * 32, dtype=F64)
    eh[:, :m] = half(e_dm)
    # feature f = 16 t + 8 h + i, slot s = 32 T + l31 -> [T][t][h][l31][i]
    frag = eh.view(ns, 2, 8, nt, 32).permute(3, 0, 1, 4, 2).reshape(nt, ns, 64, 8).half()
    kb = torch.zeros(nt, 256, dtype=F64)
    nrm = torch.full((nt * 32,), float("nan"), dtype=F64)
    nrm[:m] = -0.5 * (eh[:, :m] * eh[:, :m]).sum(0)
    nrm[m:] = float(torch.tensor(-3.0e38, dtype=torch.float32))
    kb[:, :32] = nrm.view(nt, 32)
    return frag, kb


def frag_row_source(r):
    """MFMA order inside every 32-row tile: row l of a tile holds filter pi(l), bits 2 and 3 of l swapped"""
    l = r & 31
    return (r & ~31) | (l & 19) | ((l & 4) << 1) | ((l & 8) >> 1)


def pack_frag_rows_ref(w_s16, n, k):
    """`ammc_pack_frag_rows_s16`: S16 filter rows [n][k] (k/8 groups of [8 hi | 8 lo] halfs = 8 floats) -> [k/8][hi | lo][n][8
    halfs].  w_s16: the S16 image as a float tensor of n k elements (bit patterns are moved, not values)"""
    w = w_s16.detach().cpu().contiguous().view(torch.int32).view(n, k // 8, 2, 4)
    src = torch.tensor([frag_row_source(r) for r in range(n)])
    return w[src].permute(1, 2, 0, 3).contiguous().view(-1)


def sum_partials_ref(part, n_elems):
    """`ammc_sum_partials_f32`: sum / count"""
    return _d(part).sum() / n_elems


def ulp_of(v: float) -> float:
    """spacing of fp32 at |v|"""
    v = abs(float(v))
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149
