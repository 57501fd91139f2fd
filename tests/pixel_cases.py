"""A numpy restatement of the pixel-level evaluation that imports nothing of the package, and
the seeded cases tests/test_pixel_scores_host.py and tests/test_gpu_pixel_scores.py share.

  kth_largest        what `ammc_pixel_scores_f32` returns for one sample, via np.sort
  criterion_literal  the pixel-level criterion of Mahadevan et al. AS WRITTEN: at every candidate threshold count the
                     detected ground-truth pixels of every anomalous frame and test any detected pixel of every normal
                     one, form the ROC points, take the trapezoid area
  resize_nearest, pool_any   the mask rules of `harness.resize_mask` / `harness.pool_mask` with explicit loops
"""
import functools

import numpy as np

NINF = np.float32(-np.inf)


def rank_k(m: int, num: int, den: int) -> int:
    """k = ceil(num * m / den) in integers"""
    return (m * num + den - 1) // den


def kth_largest(values, mask, num, den):
    """one sample: (m, kth, max_in, max_out); an empty set gives -inf.  values: any float array, mask: same shape"""
    v = np.asarray(values).ravel()
    inside = np.asarray(mask).ravel() != 0
    vin, vout = v[inside], v[~inside]
    m = int(vin.size)
    kth = np.sort(vin)[::-1][rank_k(m, num, den) - 1] if m else NINF
    return m, kth, (vin.max() if m else NINF), (vout.max() if vout.size else NINF)


def batch_scores(maps, masks, num, den):
    """`kth_largest` per sample -> dict of arrays [B]; floats keep the maps' dtype"""
    rows = [kth_largest(a, k, num, den) for a, k in zip(maps, masks)]
    dt = np.asarray(maps[0]).dtype
    return {"m": np.array([r[0] for r in rows], dtype=np.int32), "kth": np.array([r[1] for r in rows], dtype=dt),
            "max_in": np.array([r[2] for r in rows], dtype=dt), "max_out": np.array([r[3] for r in rows], dtype=dt)}


def criterion_literal(maps, masks, num, den):
    """the area under the pixel-level criterion's ROC, anomalous frames positive.  For every distinct map value t (and
    +inf, where nothing is detected): an anomalous frame with m ground-truth pixels of which `count` are detected
    (map >= t) is a true positive iff den * count >= num * m; a normal frame is a false positive iff any pixel is
    detected.  Returns None when a class is empty."""
    maps = [np.asarray(a, dtype=np.float64) for a in maps]
    masks = [np.asarray(k) != 0 for k in masks]
    anom = [i for i, k in enumerate(masks) if k.any()]
    norm = [i for i, k in enumerate(masks) if not k.any()]
    if not anom or not norm:
        return None
    cand = np.unique(np.concatenate([a.ravel() for a in maps]))[::-1]          # descending

    def detected(values):
        """the number of `values` >= t at every candidate t (a count of a sorted array; all candidates at once)"""
        s = np.sort(values.ravel())
        return s.size - np.searchsorted(s, cand, side="left")
    tp = np.zeros(cand.size, dtype=np.int64)
    for i in anom:
        tp += den * detected(maps[i][masks[i]]) >= num * int(masks[i].sum())
    fp = np.zeros(cand.size, dtype=np.int64)
    for i in norm:
        fp += detected(maps[i]) > 0
    fpr = np.r_[0.0, fp / len(norm)]                                           # in front: t = +inf, nothing detected
    tpr = np.r_[0.0, tp / len(anom)]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def resize_nearest(mask, H, W):
    """target (y, x) <- source (floor((y + 0.5) * h0 / H), floor((x + 0.5) * w0 / W)); mask [T, h0, w0]"""
    mask = np.asarray(mask)
    t, h0, w0 = mask.shape
    out = np.empty((t, H, W), dtype=mask.dtype)
    for y in range(H):
        sy = ((2 * y + 1) * h0) // (2 * H)
        for x in range(W):
            out[:, y, x] = mask[:, sy, ((2 * x + 1) * w0) // (2 * W)]
    return out


def pool_any(mask, patch):
    """uint8 [T, ceil(H / patch), ceil(W / patch)]: any nonzero pixel of the patch (anchored at (0, 0), ragged edges)"""
    mask = np.asarray(mask)
    t, h, w = mask.shape
    ph, pw = -(-h // patch), -(-w // patch)
    out = np.zeros((t, ph, pw), dtype=np.uint8)
    for i in range(ph):
        for j in range(pw):
            out[:, i, j] = (mask[:, i * patch:(i + 1) * patch, j * patch:(j + 1) * patch] != 0).reshape(t, -1).any(axis=1)
    return out


# ---- seeded cases ----------------------------------------------------------------------------------------------------

VALUE_KINDS = ("uniform", "equal", "decimal", "low_bits", "signs", "range", "zeros")
MASK_KINDS = ("empty", "full", "one", "rect", "p05", "p50", "m1", "m2", "m3", "m5")


def make_values(kind, shape, seed=0):
    """fp32 maps of one kind (no NaN):
      uniform   random in [0, 1)
      equal     one value everywhere
      decimal   rounded to one decimal: eleven distinct values, heavy ties that straddle rank k
      low_bits  equal in the upper 24 bits, different only in the lowest 8 mantissa bits: the last radix pass decides
      signs     normal deviates, both signs, with -0.0 and +0.0 planted
      range     magnitudes from the smallest denormal to 1e30, both signs
      zeros     mostly exact zeros among a few positive values"""
    rng = np.random.default_rng(1000 + seed)
    n = int(np.prod(shape))
    if kind == "uniform":
        v = rng.random(n, dtype=np.float32)
    elif kind == "equal":
        v = np.full(n, 0.37, dtype=np.float32)
    elif kind == "decimal":
        v = np.round(rng.random(n), 1).astype(np.float32)
    elif kind == "low_bits":
        base = np.float32(0.7123456).view(np.uint32) & np.uint32(0xFFFFFF00)
        v = (base | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    elif kind == "signs":
        v = rng.standard_normal(n).astype(np.float32)
        v[::7] = 0.0
        v[3::11] = -0.0
    elif kind == "range":
        mag = np.exp(rng.uniform(np.log(1.5e-45), np.log(1e30), n)).astype(np.float32)
        mag[::13] = np.float32(1.4e-45)                                       # the smallest denormal
        v = mag * rng.choice(np.array([-1, 1], dtype=np.float32), n)
    elif kind == "zeros":
        v = np.where(rng.random(n) < 0.9, 0.0, rng.random(n)).astype(np.float32)
    else:
        raise KeyError(kind)
    assert v.dtype == np.float32 and not np.isnan(v).any()
    return v.reshape(shape)


def make_masks(kind, shape, seed=0):
    """uint8 masks [B, H, W] of one kind; nonzero values vary (1, 2, 255): nonzero means anomalous"""
    rng = np.random.default_rng(2000 + seed)
    b, h, w = shape
    n = h * w
    mk = np.zeros((b, n), dtype=np.uint8)
    fixed = {"one": 1, "m1": 1, "m2": 2, "m3": 3, "m5": 5}
    for i in range(b):
        if kind == "empty":
            pass
        elif kind == "full":
            mk[i] = 1
        elif kind in fixed:
            mk[i, rng.choice(n, size=min(fixed[kind], n), replace=False)] = 1
        elif kind == "rect":
            m2 = mk[i].reshape(h, w)
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            m2[y0:y0 + max(1, h // 3), x0:x0 + max(1, w // 2)] = 1
        elif kind in ("p05", "p50"):
            mk[i] = rng.random(n) < (0.05 if kind == "p05" else 0.5)
        else:
            raise KeyError(kind)
    mk = mk.reshape(b, h, w)
    mk[mk != 0] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), int((mk != 0).sum()))
    return mk


@functools.lru_cache(maxsize=None)
def case(values, masks, shape, seed=0):
    """(maps fp32 [B,H,W], masks uint8 [B,H,W]) - cached and shared: treat as read-only"""
    a, k = make_values(values, shape, seed), make_masks(masks, shape, seed)
    a.setflags(write=False)
    k.setflags(write=False)
    return a, k


@functools.lru_cache(maxsize=None)
def reference(values, masks, shape, frac=(2, 5), seed=0):
    a, k = case(values, masks, shape, seed)
    return batch_scores(a, k, *frac)


def criterion_cases():
    """small (maps, masks) sets for the equivalence of the criterion as written and the per-frame numbers: ties within
    and across frames, normal and anomalous frames, one-pixel and full masks"""
    out = []
    for seed, (t, h, w, kind) in enumerate([(9, 5, 7, "decimal"), (12, 4, 4, "uniform"), (8, 6, 5, "decimal"), (10, 3, 3, "zeros"),
                                            (7, 5, 5, "signs")]):
        rng = np.random.default_rng(300 + seed)
        maps = make_values(kind, (t, h, w), seed)
        masks = np.zeros((t, h, w), dtype=np.uint8)
        for f in range(t):
            if f % 3 == 0:
                continue                                                       # a normal frame
            if f % 5 == 1:
                masks[f] = 1                                                   # a full mask
            elif f % 5 == 2:
                masks[f, rng.integers(0, h), rng.integers(0, w)] = 1           # one pixel
            else:
                masks[f] = rng.random((h, w)) < 0.4
                masks[f, 0, 0] = 1
        out.append((maps, masks))
    return out
