"""The score-fusion sweep restated in numpy, independent of the package (nothing of it is imported here): the fp32
scores exactly as include/ammc_hip.h defines them, and two_u from np.sort and np.searchsorted in int64.  Plus the
inputs the host and the GPU tests share: the committed ped2 fixture and seeded synthetic cases."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECIDABLE_IDX = 4            # main/eval_metric.py:17
F32 = np.float32


def scores(chan, w, a, b, raw=False):
    """key[i] of one grid point: chan fp32 [K, N], w fp32 [K], (a, b) fp32.  Every product and sum is one rounded fp32
    numpy operation (numpy does not fuse), left to right.  `raw`: t[i], before the zeros lose their sign."""
    chan = np.asarray(chan, dtype=F32)
    w = np.asarray(w, dtype=F32)
    f = w[0] * chan[0]
    for k in range(1, chan.shape[0]):
        f = f + w[k] * chan[k]
    t = f.copy()
    t[1:] = F32(a) * f[:-1] + F32(b) * f[1:]
    assert t.dtype == F32
    return t if raw else t + F32(0.0)


def two_u_point(key, pos_idx, neg_idx):
    """sum over positive p, negative q of 2 [key_p > key_q] + [key_p == key_q], int64"""
    kp, kn = key[pos_idx], np.sort(key[neg_idx])
    lb = np.searchsorted(kn, kp, side="left").astype(np.int64)
    ub = np.searchsorted(kn, kp, side="right").astype(np.int64)
    return int((lb + ub).sum())


def two_u_grid(chan, weights, smooth, pos_idx, neg_idx):
    """int64 [G, S] over weights fp32 [G, K] and smoothing pairs fp32 [S, 2]"""
    out = np.zeros((len(weights), len(smooth)), dtype=np.int64)
    for g, w in enumerate(weights):
        for s, (a, b) in enumerate(smooth):
            out[g, s] = two_u_point(scores(chan, w, a, b), pos_idx, neg_idx)
    return out


def two_u_brute(key, pos_idx, neg_idx):
    """the definition itself, pair by pair (small cases: the check of the searchsorted form)"""
    kp, kn = key[pos_idx][:, None], key[neg_idx][None, :]
    return int((2 * (kp > kn) + (kp == kn)).sum())


def pairs(lam_smooth):
    return np.array([[1 - l2, l2] for l2 in lam_smooth], dtype=F32).reshape(-1, 2)


def minmax_concat(records):
    """`norm_score` (main/eval_metric.py:405-417) restated: per-video min-max, drop the first frames, global min-max"""
    parts = []
    for r in records:
        r = np.array(r, dtype=F32)
        r = r - r.min()
        r = r / r.max()
        parts.append(r[DECIDABLE_IDX:])
    s = np.concatenate(parts)
    s = s - s.min()
    return s / s.max()


_fixture = None


def fixture():
    """the ped2 fixture: records dict, gt list, the two reference channels oriented (img_n, 1 - fea_n) as fp32 [2, N],
    the class index lists, the reference's 100 x 20 grid, and the golden (lam, auc) pairs.  Loaded once, never modified."""
    global _fixture
    if _fixture is None:
        d = np.load(os.path.join(GOLDEN, "score_fusion_ped2.npz"))
        cuts = np.cumsum(d["lens"])[:-1]
        rec = {"dataset": "ped2", "rgb_img_pred_records": np.split(d["rgb_img_pred_records"], cuts),
               "rgb_fea_comm_records": np.split(d["rgb_fea_comm_records"], cuts)}
        gt = np.split(d["gt"], cuts)
        labels = np.concatenate([g[DECIDABLE_IDX:] for g in gt])
        chan = np.stack([minmax_concat(rec["rgb_img_pred_records"]), F32(1.0) - minmax_concat(rec["rgb_fea_comm_records"])])
        lam_fea = [x * 0.01 for x in range(0, 100)]
        lam_smooth = [x * 0.05 for x in range(0, 20)]
        _fixture = {
            "records": rec, "gt": gt, "labels": labels, "chan": chan.astype(F32),
            "pos": np.flatnonzero(labels == 0).astype(np.int32), "neg": np.flatnonzero(labels != 0).astype(np.int32),
            "lam_fea": lam_fea, "lam_smooth": lam_smooth,
            "weights": np.array([[1 - l1, l1] for l1 in lam_fea], dtype=F32), "smooth": pairs(lam_smooth),
            "golden": {k: (tuple(float(x) for x in d[f"lam.{k}"]), float(d[f"auc.{k}"])) for k in ("avenue", "ped2", "shanghaitech")},
        }
        for v in _fixture.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _fixture


_fixture_grid = None


def fixture_grid():
    """the restatement's two_u over the fixture's whole 100 x 20 grid (computed once)"""
    global _fixture_grid
    if _fixture_grid is None:
        fx = fixture()
        _fixture_grid = two_u_grid(fx["chan"], fx["weights"], fx["smooth"], fx["pos"], fx["neg"])
        _fixture_grid.setflags(write=False)
    return _fixture_grid


def synthetic(n, k, m=None, small="neg", seed=0, decimals=None, g=5, s=3):
    """a seeded case: chan fp32 [k, n] in [0, 1] (rounded to `decimals` when given: ties), a class of exactly `m` frames
    (default about n / 3, at least 1) that is the negative or the positive one, g weight vectors (signed) and s smoothing
    pairs whose first two are the pure shift (l2 = 0) and no smoothing (l2 = 1)"""
    rng = np.random.default_rng([seed, n, k, 0 if m is None else m])
    chan = rng.random((k, n), dtype=F32)
    if decimals is not None:
        chan = np.round(chan, decimals).astype(F32)
    if m is None:
        m = min(max(1, n // 3), n - 1)
    assert 1 <= m <= n - 1
    chosen = np.sort(rng.choice(n, size=m, replace=False))
    rest = np.setdiff1d(np.arange(n), chosen)
    pos, neg = (rest, chosen) if small == "neg" else (chosen, rest)
    weights = rng.normal(size=(g, k)).astype(F32)
    weights[0] = F32(1.0) / F32(k)
    lam = [0.0, 1.0] + list(rng.random(max(s - 2, 0)))
    return {"chan": chan, "pos": pos.astype(np.int32), "neg": neg.astype(np.int32), "weights": weights,
            "smooth": pairs(lam[:s])}
