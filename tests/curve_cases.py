"""The curve sweep restated in numpy, independent of the package (nothing of it is imported here): the definitions of
include/ammc_hip.h from np.sort and np.searchsorted in int64, the sums in float64.  Keys and inputs come from
tests/fusion_cases.py; the scikit-learn values recorded by tests/golden/make_curve_golden.py are loaded here."""
import os

import numpy as np

import fusion_cases as FC

F32 = np.float32


def counts(key, pos_idx, neg_idx, v):
    """(TP, FP, TPgt, FPgt) at the values v (int64 arrays): positives / negatives with key >= v and with key > v"""
    kp, kn = np.sort(key[pos_idx]), np.sort(key[neg_idx])
    P, Q = np.int64(len(kp)), np.int64(len(kn))
    v = np.atleast_1d(v)
    return (P - np.searchsorted(kp, v, side="left"), Q - np.searchsorted(kn, v, side="left"),
            P - np.searchsorted(kp, v, side="right"), Q - np.searchsorted(kn, v, side="right"))


def curve_point(key, pos_idx, neg_idx):
    """one grid point: two_u (int), pts int64 [4] = (TP_a, FP_a, TP_b, FP_b), thr fp32 [2] = (v_a, v_b), sums float64 [2]"""
    key = np.asarray(key, dtype=F32)
    P, Q = np.int64(len(pos_idx)), np.int64(len(neg_idx))
    v = np.unique(key)[::-1]                                   # v_1 > ... > v_D
    tp, fp, _, _ = counts(key, pos_idx, neg_idx, v)
    tp, fp = np.r_[np.int64(0), tp], np.r_[np.int64(0), fp]    # vertex 0 = (0, 0)
    G = P * fp + Q * tp - P * Q
    assert (np.diff(G) > 0).all() and G[0] == -P * Q and G[-1] == P * Q
    a = int(np.flatnonzero(G <= 0)[-1])
    thr_all = np.r_[F32(np.inf), v]
    u = np.unique(key[pos_idx])
    TP, FP, TPgt, FPgt = counts(key, pos_idx, neg_idx, u)
    prec = TP / (TP + FP)
    with np.errstate(invalid="ignore", divide="ignore"):
        last = np.where(TPgt > 0, TPgt / (TPgt + FPgt), np.where(FPgt > 0, 0.0, 1.0))
    mult = (TP - TPgt).astype(np.float64)
    sums = np.array([(mult * prec).sum(), (0.5 * mult * (last + prec)).sum()], dtype=np.float64)
    return {"two_u": FC.two_u_point(key, pos_idx, neg_idx), "pts": np.array([tp[a], fp[a], tp[a + 1], fp[a + 1]], dtype=np.int64),
            "thr": thr_all[a:a + 2].astype(F32), "sums": sums}


def curve_grid(chan, weights, smooth, pos_idx, neg_idx):
    """two_u int64 [G, S], pts int64 [G, S, 4], thr fp32 [G, S, 2], sums float64 [G, S, 2]"""
    g, s = len(weights), len(smooth)
    out = {"two_u": np.zeros((g, s), np.int64), "pts": np.zeros((g, s, 4), np.int64), "thr": np.zeros((g, s, 2), F32),
           "sums": np.zeros((g, s, 2), np.float64)}
    for gi, w in enumerate(weights):
        for si, (a, b) in enumerate(smooth):
            r = curve_point(FC.scores(chan, w, a, b), pos_idx, neg_idx)
            for k in out:
                out[k][gi, si] = r[k]
    return out


def derived(pts, sums, P, Q):
    """eer_vertex, eer, ap, pr_auc (float64, any leading shape) from the device's outputs, as the header derives them"""
    pts = np.asarray(pts, dtype=np.int64)
    P, Q = np.int64(P), np.int64(Q)
    tpa, fpa, tpb, fpb = (pts[..., i] for i in range(4))
    ga, gb = P * fpa + Q * tpa - P * Q, P * fpb + Q * tpb - P * Q
    eer_vertex = np.where(np.abs(ga) <= np.abs(gb), fpa, fpb) / np.float64(Q)
    lam = -ga / (gb - ga).astype(np.float64)
    return {"eer_vertex": eer_vertex, "eer": (fpa + lam * (fpb - fpa)) / np.float64(Q), "ap": np.asarray(sums)[..., 0] / np.float64(P),
            "pr_auc": np.asarray(sums)[..., 1] / np.float64(P), "tie": np.abs(ga) == np.abs(gb)}


def full_curve(key, pos_idx, neg_idx):
    """every vertex of the ROC curve, vertex 0 included: (tps, fps) int64"""
    v = np.unique(np.asarray(key, dtype=F32))[::-1]
    tp, fp, _, _ = counts(key, pos_idx, neg_idx, v)
    return np.r_[np.int64(0), tp], np.r_[np.int64(0), fp]


def brute(key, pos_idx, neg_idx):
    """the definitions pair by pair, no sort and no search (n <= 12): the same dict as `curve_point`"""
    key = [float(x) for x in np.asarray(key, dtype=F32)]
    pos, neg = [key[i] for i in pos_idx], [key[i] for i in neg_idx]
    P, Q = len(pos), len(neg)
    tp = lambda v, gt=False: sum((x > v) if gt else (x >= v) for x in pos)
    fp = lambda v, gt=False: sum((x > v) if gt else (x >= v) for x in neg)
    verts = [(0, 0, float("inf"))] + [(tp(v), fp(v), v) for v in sorted(set(key), reverse=True)]
    G = [P * f + Q * t - P * Q for t, f, _ in verts]
    a = max(d for d, g in enumerate(G) if g <= 0)
    s0 = s1 = 0.0
    for u in sorted(set(pos), reverse=True):
        T, Fp, Tg, Fg = tp(u), fp(u), tp(u, True), fp(u, True)
        last = Tg / (Tg + Fg) if Tg > 0 else (0.0 if Fg > 0 else 1.0)
        s0 += (T - Tg) * (T / (T + Fp))
        s1 += 0.5 * (T - Tg) * (last + T / (T + Fp))
    two_u = sum(2 * (p > q) + (p == q) for p in pos for q in neg)
    return {"two_u": two_u, "pts": np.array([verts[a][0], verts[a][1], verts[a + 1][0], verts[a + 1][1]], dtype=np.int64),
            "thr": np.array([verts[a][2], verts[a + 1][2]], dtype=F32), "sums": np.array([s0, s1])}


def gate(P):
    """|ap - ap'| and |pr_auc - pr_auc'| between two float64 evaluations of at most P terms: (P + 4) 2^-52"""
    return (int(P) + 4) * 2.0 ** -52


_fixture_curves = None


def fixture_curves():
    """the restatement over the ped2 fixture's whole 100 x 20 grid (computed once, never modified)"""
    global _fixture_curves
    if _fixture_curves is None:
        fx = FC.fixture()
        _fixture_curves = curve_grid(fx["chan"], fx["weights"], fx["smooth"], fx["pos"], fx["neg"])
        for v in _fixture_curves.values():
            v.setflags(write=False)
    return _fixture_curves


_golden = None


def golden():
    """tests/golden/curve_metrics_ped2.npz: scikit-learn's own values at every 10th point of the ped2 grid (`grid_*`,
    `grid_index` = flat indices into the 100 x 20 grid), at ped2's published pair `lam_map` (`lam_*`) and at five synthetic
    cases with ties (`syn_*`, `syn_case` = (n, k, decimals, seed, g, s) rows)"""
    global _golden
    if _golden is None:
        with np.load(os.path.join(FC.GOLDEN, "curve_metrics_ped2.npz")) as d:
            _golden = {k: d[k] for k in d.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def synthetic_tied(row):
    """the synthetic case of one `syn_case` row and its key"""
    n, k, decimals, seed, g, s = (int(x) for x in row)
    c = FC.synthetic(n, k, seed=seed, decimals=decimals)
    return c, FC.scores(c["chan"], c["weights"][g], *c["smooth"][s])
