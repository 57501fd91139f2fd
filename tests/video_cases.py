"""The per-video pair counts and their bootstrap form restated in numpy, independent of the package (nothing of it is
imported here), plus the cases the host and the GPU tests share.  `pairs_brute` is the definition pair by pair - an
O(P Q) comparison, no sort anywhere; `bootstrap_brute` the bilinear form by np.einsum in int64."""
import numpy as np

import fusion_cases as FC

F32 = np.float32


def video_ids(off):
    """the video of every entry of a class list, from its V + 1 offsets"""
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def pairs_brute(keys, pos, neg, pos_off, neg_off):
    """int64 [V, V]: entry [a, b] = sum over the positive frames p of video a and the negative frames q of video b of
    2 [key_p > key_q] + [key_p == key_q].  (IEEE comparisons: -0.0 == +0.0.)  Every pair is compared."""
    V = len(pos_off) - 1
    kp, kn = np.asarray(keys)[np.asarray(pos)][:, None], np.asarray(keys)[np.asarray(neg)][None, :]
    each = 2 * (kp > kn).astype(np.int64) + (kp == kn)
    cell = video_ids(pos_off)[:, None] * V + video_ids(neg_off)[None, :]
    out = np.zeros(V * V, dtype=np.int64)
    np.add.at(out, cell.ravel(), each.ravel())
    return out.reshape(V, V)


def pairs_grid(c):
    """int64 [G, S, V, V] of a case, every block by `pairs_brute`"""
    return np.array([[pairs_brute(FC.scores(c["chan"], w, a, b), c["pos"], c["neg"], c["pos_off"], c["neg_off"])
                      for a, b in c["smooth"]] for w in c["weights"]])


def pairs_searchsorted(keys, pos, neg, pos_off, neg_off):
    """the same blocks from np.sort and np.searchsorted per negative video (large cases)"""
    V = len(pos_off) - 1
    keys, ids = np.asarray(keys), video_ids(pos_off)
    out = np.zeros((V, V), dtype=np.int64)
    kp = keys[np.asarray(pos)]
    for b in range(V):
        kn = np.sort(keys[np.asarray(neg)[neg_off[b]:neg_off[b + 1]]])
        each = np.searchsorted(kn, kp, side="left").astype(np.int64) + np.searchsorted(kn, kp, side="right")
        assert 2 * len(kp) * len(kn) < 1 << 53                             # (bincount adds in float64: exact below 2^53)
        out[:, b] = np.bincount(ids, weights=each, minlength=V).astype(np.int64)
    return out


def bootstrap_brute(pairs, mult):
    """int64 [B, M]: out[r, g] = sum_ab mult[r, a] mult[r, b] pairs[g, a, b]"""
    pairs, mult = np.asarray(pairs, dtype=np.int64), np.asarray(mult, dtype=np.int64)
    out = np.einsum("ra,rb,gab->rg", mult, mult, pairs, optimize=True)
    assert out.dtype == np.int64
    return out


def offsets_from_cuts(idx, cuts, n):
    """offsets of a sorted frame-index list under the split of 0 .. n - 1 into videos at `cuts` (first frames of the
    videos after the first)"""
    edges = np.r_[0, np.asarray(cuts, dtype=np.int64), n]
    return np.searchsorted(np.asarray(idx), edges, side="left").astype(np.int64)


def split(c, cuts):
    """a `FC.synthetic` case plus the offsets of a split of its frames into len(cuts) + 1 videos"""
    n = c["chan"].shape[1]
    return dict(c, pos_off=offsets_from_cuts(c["pos"], cuts, n), neg_off=offsets_from_cuts(c["neg"], cuts, n))


def with_segments(small_counts, other_counts, k, small="neg", seed=0, g=5, s=3, decimals=None):
    """a case whose video v holds exactly small_counts[v] frames of the class `small` and other_counts[v] of the other,
    shuffled inside the video; channels, weights and smoothings are `FC.synthetic`'s for that many frames"""
    rng = np.random.default_rng([seed, len(small_counts), k, sum(small_counts)])
    is_small = np.concatenate([rng.permutation(np.r_[np.ones(a, dtype=bool), np.zeros(b, dtype=bool)])
                               for a, b in zip(small_counts, other_counts)])
    n = is_small.size
    base = FC.synthetic(n, k, seed=seed, g=g, s=s, decimals=decimals)
    small_idx, other_idx = np.flatnonzero(is_small).astype(np.int32), np.flatnonzero(~is_small).astype(np.int32)
    small_off, other_off = np.r_[0, np.cumsum(small_counts)].astype(np.int64), np.r_[0, np.cumsum(other_counts)].astype(np.int64)
    pos, neg, pos_off, neg_off = (other_idx, small_idx, other_off, small_off) if small == "neg" else \
        (small_idx, other_idx, small_off, other_off)
    return {"chan": base["chan"], "pos": pos, "neg": neg, "weights": base["weights"], "smooth": base["smooth"],
            "pos_off": pos_off, "neg_off": neg_off}


def fixture_offsets():
    """(pos_off, neg_off, P_a, Q_a) of the ped2 fixture's 12 videos, restated from its labels"""
    fx = FC.fixture()
    n_pos = np.array([int((g[FC.DECIDABLE_IDX:] == 0).sum()) for g in fx["gt"]], dtype=np.int64)
    n_neg = np.array([int((g[FC.DECIDABLE_IDX:] != 0).sum()) for g in fx["gt"]], dtype=np.int64)
    return np.r_[0, np.cumsum(n_pos)].astype(np.int64), np.r_[0, np.cumsum(n_neg)].astype(np.int64), n_pos, n_neg


def resampled(keys, labels, lens, m):
    """the data set of a replica, literally: video v's keys and labels repeated m[v] times"""
    cuts = np.cumsum(lens)[:-1]
    ks, ls = np.split(np.asarray(keys), cuts), np.split(np.asarray(labels), cuts)
    return (np.concatenate([np.tile(k, int(r)) for k, r in zip(ks, m)]), np.concatenate([np.tile(l, int(r)) for l, r in zip(ls, m)]))
