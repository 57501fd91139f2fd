"""Per-video pair counts and the video bootstrap on the device (csrc/video_pairs.hip, `ops.video_pairs`,
`ops.bootstrap_pairs`, `harness.sweep_videos`, `run_fusion --videos`) against the numpy
restatements of tests/video_cases.py.  The counts are integers: every comparison of them is equality.

Shapes: the smallest at which the pass can go wrong - one video; 2, 3 and 7 videos whose segments of the sorted class
have 0, 1, 2 (no padding), 63 / 64 / 65 (the wave boundary, a pad boundary), 257 and 1025 frames (several rounds per
thread), each class as the smaller one, K = 1, 2, 8; videos with one class or no frame, first, in the middle and last; the
two limits themselves (1024 videos of a few frames; a segment of 32768 among 70 000 frames, where the workgroup has 1024
threads) and one beyond each."""
import functools
import json

import numpy as np
import pytest
import torch

import fusion_cases as FC
import video_cases as VC
from ammcnet_aaai2021_amd import harness as Hn, ops, run_fusion

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID_KEYS = ("chan", "pos", "neg", "weights", "smooth")


def _dev(c):
    return {k: torch.from_numpy(np.array(c[k], order="C")).to(DEV) for k in GRID_KEYS}       # (a copy: the fixture is read-only)


def _run(c, **kw):
    d = _dev(c)
    return ops.video_pairs(d["chan"], d["pos"], d["neg"], c["pos_off"], c["neg_off"], d["weights"], d["smooth"], **kw).cpu().numpy()


def _two_u(c):
    d = _dev(c)
    return ops.fusion_sweep(d["chan"], d["pos"], d["neg"], d["weights"], d["smooth"]).cpu().numpy()


def test_one_video_is_the_fusion_sweep():
    for n, k, small in ((2, 1, "neg"), (65, 2, "pos"), (1025, 8, "neg")):
        c = FC.synthetic(n, k, small=small)
        c.update(pos_off=[0, len(c["pos"])], neg_off=[0, len(c["neg"])])
        got = _run(c)
        assert got.dtype == np.int64 and got.shape == (5, 3, 1, 1)
        assert np.array_equal(got[:, :, 0, 0], _two_u(c)) and np.array_equal(got[:, :, 0, 0], FC.two_u_grid(*[c[x] for x in (
            "chan", "weights", "smooth", "pos", "neg")]))


SEGMENTS = {2: ([1025, 1], [700, 400]), 3: ([63, 0, 65], [100, 50, 30]),
            7: ([2, 64, 0, 257, 1, 65, 63], [100, 0, 130, 90, 77, 1, 120])}


@pytest.mark.parametrize("small", ["neg", "pos"])
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("v", [2, 3, 7])
def test_several_videos(v, k, small):
    seg, other = SEGMENTS[v]
    assert set(sum((s for s, _ in SEGMENTS.values()), [])) == {0, 1, 2, 63, 64, 65, 257, 1025}
    c = VC.with_segments(seg, other, k, small=small, seed=v)
    sorted_off = c["neg_off"] if small == "neg" else c["pos_off"]
    assert np.diff(sorted_off).tolist() == seg and min(len(c["pos"]), len(c["neg"])) == sum(seg)
    got = _run(c)
    assert got.shape == (5, 3, v, v)
    assert np.array_equal(got, VC.pairs_grid(c)), (v, k, small)
    assert np.array_equal(got.sum((2, 3)), _two_u(c))


@pytest.mark.parametrize("where", [0, 1, 3])
def test_empty_and_one_class_videos(where):
    base = VC.with_segments([40, 65, 30], [70, 90, 64], 2, small="neg", seed=21)
    base["smooth"] = FC.pairs([1.0])                    # a = 0: a key is its own frame's alone, whatever stands before it
    want = _run(base)
    assert np.array_equal(want, VC.pairs_grid(base))
    n = base["chan"].shape[1]
    edges = VC.video_ids(np.r_[0, np.cumsum([110, 155, 94])])              # the video of every frame
    cut = int(np.searchsorted(edges, where, side="left"))                  # the new video stands before frame `cut`
    rng = np.random.default_rng(where)
    keep = [x for x in range(4) if x != where]
    for kind, extra in (("positives only", 37), ("negatives only", 37), ("no scored frame", 0)):
        chan = np.concatenate([base["chan"][:, :cut], rng.random((2, extra), dtype=np.float32), base["chan"][:, cut:]], axis=1)
        shift = lambda idx: np.where(idx >= cut, idx + extra, idx).astype(np.int32)
        pos, neg = shift(base["pos"]), shift(base["neg"])
        new = np.arange(cut, cut + extra, dtype=np.int32)
        pos_off, neg_off = np.insert(base["pos_off"], where, base["pos_off"][where]), np.insert(base["neg_off"], where, base["neg_off"][where])
        if kind == "positives only":
            pos = np.insert(pos, base["pos_off"][where], new)
            pos_off[where + 1:] += extra
        elif kind == "negatives only":
            neg = np.insert(neg, base["neg_off"][where], new)
            neg_off[where + 1:] += extra
        c = dict(base, chan=chan, pos=pos, neg=neg, pos_off=pos_off, neg_off=neg_off)
        assert chan.shape[1] == n + extra and len(pos) + len(neg) == n + extra
        got = _run(c)
        assert got.shape == (5, 1, 4, 4)
        assert np.array_equal(got, VC.pairs_grid(c)), kind
        assert np.array_equal(got[:, :, keep][:, :, :, keep], want), kind  # the other blocks are what they were
        if kind != "negatives only":
            assert (got[:, :, :, where] == 0).all()                        # no negative frame: its column is 0
        if kind != "positives only":
            assert (got[:, :, where, :] == 0).all()                        # no positive frame: its row is 0
        if kind == "positives only":
            assert (got[:, :, where, :] != 0).any()
    # with any smoothing a video without a frame changes nothing but its own row and column
    c = dict(VC.with_segments([40, 65, 30], [70, 90, 64], 2, small="pos", seed=22))
    full = _run(c)
    c4 = dict(c, pos_off=np.insert(c["pos_off"], where, c["pos_off"][where]), neg_off=np.insert(c["neg_off"], where, c["neg_off"][where]))
    got = _run(c4)
    assert np.array_equal(got[:, :, keep][:, :, :, keep], full) and (got[:, :, where] == 0).all() and (got[:, :, :, where] == 0).all()


def test_ties_from_coarse_channels_split_into_videos():
    for n, k, cuts in ((65, 2, [1, 30]), (1025, 4, [300, 301, 900]), (3000, 2, [64, 1200, 1300, 2999])):
        c = FC.synthetic(n, k, decimals=1, seed=3)
        c["weights"][1:] = np.round(c["weights"][1:], 1)
        key = FC.scores(c["chan"], c["weights"][0], *c["smooth"][1])
        assert len(np.unique(key)) < n // 2                                # ties are the rule here
        c = VC.split(c, cuts)
        got = _run(c)
        assert np.array_equal(got, VC.pairs_grid(c))
        assert np.array_equal(got.sum((2, 3)), _two_u(c))


def test_negative_and_positive_zeros_tie_across_videos():
    rng = np.random.default_rng(11)
    n = 600
    chan = np.round(rng.normal(size=(1, n)), 1).astype(np.float32)         # signed, many exact zeros
    chan[0, rng.choice(n, size=200, replace=False)] = 0.0
    labels = rng.random(n) < 0.4
    c = {"chan": chan, "pos": np.flatnonzero(~labels).astype(np.int32), "neg": np.flatnonzero(labels).astype(np.int32),
         "weights": np.array([[-1.0]], dtype=np.float32), "smooth": FC.pairs([1.0, 0.0, 0.5])}
    c = VC.split(c, [150, 300, 450])
    raw = FC.scores(chan, c["weights"][0], *c["smooth"][0], raw=True)      # l2 = 1: t = 0 * f[i - 1] + f[i]
    for cls, off in (("pos", c["pos_off"]), ("neg", c["neg_off"])):
        for v in range(4):                                                 # both zeros in every video, in both classes
            z = raw[c[cls][off[v]:off[v + 1]]]
            z = z[z == 0]
            assert np.signbit(z).any() and not np.signbit(z).all(), (cls, v)
    want = np.array([[VC.pairs_brute(FC.scores(chan, c["weights"][0], a, b, raw=True), c["pos"], c["neg"], c["pos_off"], c["neg_off"])
                      for a, b in c["smooth"]]])
    assert np.array_equal(want, VC.pairs_grid(c))
    assert np.array_equal(_run(c), want)


def test_smoothing_reaches_across_a_video_boundary():
    c = VC.split(FC.synthetic(1025, 2, seed=7), [200, 201, 640])
    c["smooth"] = FC.pairs([0.0, 1.0, 0.5])
    got = _run(c)
    assert np.array_equal(got, VC.pairs_grid(c))
    for g, w in enumerate(c["weights"]):
        f = w[0] * c["chan"][0] + w[1] * c["chan"][1]
        shifted = np.concatenate([f[:1], f[:-1]])       # l2 = 0: a frame has its predecessor's score - the previous video's last
        assert np.array_equal(got[g, 0], VC.pairs_brute(shifted + np.float32(0), c["pos"], c["neg"], c["pos_off"], c["neg_off"]))
        assert np.array_equal(got[g, 1], VC.pairs_brute(f + np.float32(0), c["pos"], c["neg"], c["pos_off"], c["neg_off"]))
    restart = np.concatenate([f[:1], f[:-1]])
    restart[[200, 201, 640]] = f[[200, 201, 640]]       # what a smoothing that restarted at the boundaries would give
    assert not np.array_equal(got[-1, 0], VC.pairs_brute(restart + np.float32(0), c["pos"], c["neg"], c["pos_off"], c["neg_off"]))


def test_placement_strides_offsets_out_repeats():
    c = VC.split(FC.synthetic(2000, 4, seed=9), [400, 401, 1333])
    want = VC.pairs_grid(c)
    d = _dev(c)
    off = (c["pos_off"], c["neg_off"])
    base = ops.video_pairs(d["chan"], d["pos"], d["neg"], *off, d["weights"], d["smooth"])
    assert np.array_equal(base.cpu().numpy(), want)
    # the offsets as lists, as CPU tensors and as int32 device vectors
    for form in (lambda o: o.tolist(), lambda o: torch.from_numpy(o), lambda o: torch.from_numpy(o).int(),
                 lambda o: torch.from_numpy(o).int().to(DEV)):
        assert torch.equal(ops.video_pairs(d["chan"], d["pos"], d["neg"], form(off[0]), form(off[1]), d["weights"], d["smooth"]), base)
    # a grid point alone, and a part of the grid = the same points inside the grid
    for g, s in ((0, 0), (3, 2), (4, 1)):
        one = ops.video_pairs(d["chan"], d["pos"], d["neg"], *off, d["weights"][g:g + 1].contiguous(), d["smooth"][s:s + 1].contiguous())
        assert one.shape == (1, 1, 4, 4) and torch.equal(one[0, 0], base[g, s])
    part = ops.video_pairs(d["chan"], d["pos"], d["neg"], *off, d["weights"][1:4], d["smooth"][1:])
    assert torch.equal(part, base[1:4, 1:])
    # a strided view of the channels (rows 2003 floats apart, an odd start)
    wide = torch.full((4, 2003), float("nan"), device=DEV)
    wide[:, 3:] = d["chan"]
    assert not wide[:, 3:].is_contiguous()
    assert torch.equal(ops.video_pairs(wide[:, 3:], d["pos"], d["neg"], *off, d["weights"], d["smooth"]), base)
    # out=: every element written, in place, and returned; a wrong one is refused
    out = torch.full((5, 3, 4, 4), -7, dtype=torch.int64, device=DEV)
    ret = ops.video_pairs(d["chan"], d["pos"], d["neg"], *off, d["weights"], d["smooth"], out=out)
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, base)
    for bad in (torch.zeros(5, 3, 4, 4, device=DEV), torch.zeros(5, 3, 4, 3, dtype=torch.int64, device=DEV),
                torch.zeros(5, 3, 16, dtype=torch.int64, device=DEV), torch.zeros(5, 3, 4, 4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops.video_pairs(d["chan"], d["pos"], d["neg"], *off, d["weights"], d["smooth"], out=bad)
    assert torch.equal(ops.video_pairs(d["chan"], d["pos"], d["neg"], *off, d["weights"], d["smooth"]), base)      # launches repeat


def test_fixture_full_reference_grid_in_chunks():
    fx = FC.fixture()
    pos_off, neg_off, n_pos, n_neg = VC.fixture_offsets()
    assert len(n_pos) == 12 and n_neg[-1] == 1                            # the last video: a single anomalous frame
    c = dict({k: fx[k] for k in GRID_KEYS}, pos_off=pos_off, neg_off=neg_off)
    got = _run(c)
    assert got.shape == (100, 20, 12, 12) and (got >= 0).all()
    assert np.array_equal(got.sum((2, 3)), FC.fixture_grid())
    assert (got <= 2 * n_pos[:, None] * n_neg[None, :]).all()
    for g, s in ((0, 0), (1, 11), (99, 19)):                               # (1, 11): the published pair of LAM_MAP["ped2"]
        key = FC.scores(fx["chan"], fx["weights"][g], *fx["smooth"][s])
        assert np.array_equal(got[g, s], VC.pairs_brute(key, fx["pos"], fx["neg"], pos_off, neg_off)), (g, s)
    assert fx["lam_fea"][1] == Hn.LAM_MAP["ped2"][0] and abs(fx["lam_smooth"][11] - Hn.LAM_MAP["ped2"][1]) < 1e-12
    for g0, g1, s0, s1 in ((0, 37, 0, 20), (37, 100, 0, 20), (5, 6, 0, 7), (5, 6, 7, 20)):
        part = _run(dict(c, weights=fx["weights"][g0:g1], smooth=fx["smooth"][s0:s1]))
        assert np.array_equal(part, got[g0:g1, s0:s1])


def _same(a, b, skip=("video_ms",)):
    assert type(a) is type(b)
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            if k not in skip:
                _same(a[k], b[k], skip)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    else:
        assert a == b


def test_sweep_videos_does_not_depend_on_the_chunking():
    fx = FC.fixture()
    kw = dict(replicas=50, seed=3, device=DEV)
    whole = Hn.sweep_videos(fx["records"], fx["gt"], **kw)
    _same(Hn.sweep_videos(fx["records"], fx["gt"], max_workspace_bytes=12 * 12 * 8, **kw), whole)      # a chunk = one grid point
    _same(Hn.sweep_videos(fx["records"], fx["gt"], max_workspace_bytes=12 * 12 * 8 * 47, **kw), whole)  # two weight rows and a bit
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        Hn.sweep_videos(fx["records"], fx["gt"], max_workspace_bytes=12 * 12 * 8 - 1, **kw)


def test_limit_of_videos():
    V = ops.VIDEO_PAIRS_MAX_VIDEOS
    rng = np.random.default_rng(5)
    seg, other = rng.integers(0, 4, size=V).tolist(), rng.integers(1, 5, size=V).tolist()
    seg[0], seg[-1] = 0, 3
    c = VC.with_segments(seg, other, 2, small="pos", seed=1, g=1, s=2)
    assert len(c["pos"]) < len(c["neg"])
    got = _run(c)
    assert got.shape == (1, 2, V, V)
    assert np.array_equal(got, VC.pairs_grid(c)) and np.array_equal(got.sum((2, 3)), _two_u(c))
    d = _dev(c)
    more = dict(pos_off=np.r_[c["pos_off"], c["pos_off"][-1]], neg_off=np.r_[c["neg_off"], c["neg_off"][-1]])
    out = torch.full((1, 2, V + 1, V + 1), -7, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match=str(V)):
        ops.video_pairs(d["chan"], d["pos"], d["neg"], more["pos_off"], more["neg_off"], d["weights"], d["smooth"], out=out)
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all()                                         # nothing was launched


def test_limit_of_a_segment():
    cap = ops.VIDEO_PAIRS_MAX_SEGMENT
    c = VC.with_segments([0, cap, 0], [20000, 17000, 70000 - cap - 37000], 2, small="neg", seed=2, g=1, s=1)   # (fusion_sweep: the class <= cap)
    assert c["chan"].shape[1] == 70000 and np.diff(c["neg_off"]).max() == cap and len(c["neg"]) < len(c["pos"])
    got = _run(c)
    key = FC.scores(c["chan"], c["weights"][0], *c["smooth"][0])
    assert np.array_equal(got[0, 0], VC.pairs_searchsorted(key, c["pos"], c["neg"], c["pos_off"], c["neg_off"]))
    assert got.sum() == int(_two_u(c)[0, 0])
    c = VC.with_segments([0, cap + 1, 0], [20000, 17000, 70000 - cap - 1 - 37000], 2, small="neg", seed=2, g=1, s=1)
    d = _dev(c)
    out = torch.full((1, 1, 3, 3), -7, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match=str(cap)):
        ops.video_pairs(d["chan"], d["pos"], d["neg"], c["pos_off"], c["neg_off"], d["weights"], d["smooth"], out=out)
    with pytest.raises(ValueError, match=str(cap)):                        # device offsets: read back only in this case
        ops.video_pairs(d["chan"], d["pos"], d["neg"], torch.from_numpy(c["pos_off"]).int().to(DEV),
                        torch.from_numpy(c["neg_off"]).int().to(DEV), d["weights"], d["smooth"], out=out)
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all()                                         # nothing was launched


def _boot(pairs, mult, **kw):
    return ops.bootstrap_pairs(torch.from_numpy(np.ascontiguousarray(pairs)).to(DEV),
                               torch.from_numpy(np.ascontiguousarray(mult, dtype=np.int32)).to(DEV), **kw).cpu().numpy()


def test_bootstrap_pairs_unit_rows():
    rng = np.random.default_rng(3)
    V, M = 5, 4
    pairs = rng.integers(0, 1 << 30, size=(M, V, V), dtype=np.int64)
    eye = np.eye(V, dtype=np.int32)
    assert np.array_equal(_boot(pairs, np.ones((1, V)))[0], pairs.sum((1, 2)))                     # the block sum
    assert np.array_equal(_boot(pairs, eye), np.array([np.diag(p) for p in pairs]).T)              # e_a: C[a][a]
    assert np.array_equal(_boot(pairs, 2 * eye), 4 * np.array([np.diag(p) for p in pairs]).T)      # 2 e_a: 4 C[a][a]
    a, b = 1, 3
    got = _boot(pairs, (eye[a] + eye[b])[None])[0]
    assert np.array_equal(got, pairs[:, a, a] + pairs[:, a, b] + pairs[:, b, a] + pairs[:, b, b])
    assert (_boot(pairs, np.zeros((2, V))) == 0).all()
    out = torch.full((V, M), -7, dtype=torch.int64, device=DEV)
    d_p, d_m = torch.from_numpy(pairs).to(DEV), torch.from_numpy(eye).to(DEV)
    ret = ops.bootstrap_pairs(d_p, d_m, out=out)
    assert ret.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), np.array([np.diag(p) for p in pairs]).T)
    for bad in (torch.zeros(V, M, device=DEV), torch.zeros(M, V, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError):
            ops.bootstrap_pairs(d_p, d_m, out=bad)


@pytest.mark.parametrize("M", [1, 60])
@pytest.mark.parametrize("V", [1, 3, 12, 107])
def test_bootstrap_pairs_random_tables(V, M):
    # P_a = Q_a = 2^20 frames per video would allow entries up to 2 P_a Q_b = 2^41; a replica draws V videos, so its
    # 2 P_r Q_r = 2 (V 2^20)^2 <= 2^55: the documented precondition holds with room
    rng = np.random.default_rng([V, M])
    pairs = rng.integers((1 << 40) - (1 << 36), (1 << 40) + (1 << 36), size=(M, V, V), dtype=np.int64)
    assert 2 * (V << 20) ** 2 < 1 << 63 and pairs.max() <= 1 << 41
    for B in (1, 7, 1000):
        mult = Hn.bootstrap_multiplicities(V, B, seed=B)
        if B == 7:
            mult[0], mult[-1] = 0, 0
            mult[0, 0], mult[-1, -1] = V, V                                # multiplicities up to V
        got = _boot(pairs, mult)
        assert got.shape == (B, M) and np.array_equal(got, VC.bootstrap_brute(pairs, mult)), (B, V, M)


def _witness(keys, labels, lens, blocks, n_pos, n_neg, mult):
    got = _boot(blocks[None], mult)[:, 0]
    worst = 0.0
    for m, two_u in zip(mult, got):
        k, l = VC.resampled(keys, labels, lens, m)
        p_r, q_r = int(m @ n_pos), int(m @ n_neg)
        assert (l == 0).sum() == p_r and (l != 0).sum() == q_r and p_r > 0 and q_r > 0
        worst = max(worst, abs(int(two_u) / (2.0 * p_r * q_r) - Hn.roc_auc(l, k, pos_label=0)))
    print(f"literal witness: worst |device - roc_auc of the resampled set| = {worst:.3e} over {len(mult)} replicas")
    assert worst <= 1e-12


def test_literal_witness_resampled_data_sets():
    # a replica built frame by frame and scored by the project's own roc_auc, against the bilinear form of the blocks
    c = VC.with_segments([40, 30, 50], [60, 80, 45], 2, small="neg", seed=4, g=2, s=2)
    labels = np.zeros(c["chan"].shape[1], dtype=np.int8)
    labels[c["neg"]] = 1
    keys = Hn.fused_keys(c["chan"], c["weights"][1], c["smooth"][1])
    mult = np.array([[1, 1, 1], [3, 0, 0], [0, 2, 1], [1, 0, 2], [0, 0, 3]])
    _witness(keys, labels, [100, 110, 95], _run(c)[1, 1], np.diff(c["pos_off"]), np.diff(c["neg_off"]), mult)

    fx = FC.fixture()
    pos_off, neg_off, n_pos, n_neg = VC.fixture_offsets()
    l1, l2 = Hn.LAM_MAP["ped2"]
    w, sm = np.array([[1 - l1, l1]], dtype=np.float32), Hn.smoothing_pairs([l2])
    blocks = _run(dict({k: fx[k] for k in GRID_KEYS}, weights=w, smooth=sm, pos_off=pos_off, neg_off=neg_off))[0, 0]
    _witness(Hn.fused_keys(fx["chan"], w[0], sm[0]), fx["labels"], n_pos + n_neg, blocks, n_pos, n_neg,
             Hn.bootstrap_multiplicities(12, 5, 0))


@functools.lru_cache(maxsize=None)
def _fixture_sweep():
    fx = FC.fixture()
    return Hn.sweep_videos(fx["records"], fx["gt"], device=DEV)


def test_sweep_videos_on_the_fixture():
    fx = FC.fixture()
    res = _fixture_sweep()
    ref = Hn.sweep_fusion(fx["records"], fx["gt"], device=DEV)
    assert np.array_equal(res["two_u"], ref["two_u"]) and np.array_equal(res["two_u"], FC.fixture_grid())
    assert res["auc"].dtype == np.float64 and np.array_equal(res["auc"], ref["auc"])
    assert res["best"]["index"] == ref["best"]["index"] and res["best"]["auc"] == ref["best"]["auc"]
    assert res["best"]["weights"] == ref["best"]["weights"] and res["best"]["lam_smooth"] == ref["best"]["lam_smooth"]
    assert res["at_lam_map"]["auc"] == ref["auc_at_lam_map"] and res["lam_map"] == Hn.LAM_MAP["ped2"]
    assert (res["videos"], res["videos_scored"], res["replicas"], res["replicas_dropped"], res["seed"], res["level"]) == \
        (12, 12, 1000, 0, 0, 0.95)
    assert res["macro_auc"].shape == (100, 20) and res["auc_ci"].shape == res["macro_auc_ci"].shape == (100, 20, 2)
    assert res["video_ms"] > 0 and 0.0 <= res["best_share"] <= 1.0

    # the macro AUC: the mean of twelve roc_auc calls on the per-video slices of the host keys
    cuts = np.cumsum([len(g) - Hn.DECIDABLE_IDX for g in fx["gt"]])[:-1]
    labels = np.split(fx["labels"], cuts)

    def macro(w, pair):
        keys = np.split(Hn.fused_keys(fx["chan"], w, pair), cuts)
        return [Hn.roc_auc(l, k, pos_label=0) for l, k in zip(labels, keys)]
    points = sorted({res["best"]["index"], res["best_macro"]["index"], (1, 11)} | {(g, (3 * g) % 20) for g in range(0, 100, 7)})
    worst = 0.0
    for g, s in points:
        worst = max(worst, abs(res["macro_auc"][g, s] - np.mean(macro(fx["weights"][g], fx["smooth"][s]))))
    per_video = macro(np.asarray(res["best"]["weights"], dtype=np.float32), Hn.smoothing_pairs([res["best"]["lam_smooth"]])[0])
    worst = max(worst, np.abs(res["best"]["per_video_auc"] - per_video).max())
    l1, l2 = Hn.LAM_MAP["ped2"]
    at_lam = macro(np.array([1 - l1, l1], dtype=np.float32), Hn.smoothing_pairs([l2])[0])
    worst = max(worst, abs(res["at_lam_map"]["macro_auc"] - np.mean(at_lam)))
    print(f"sweep_videos: worst |macro AUC - mean of per-video roc_auc| = {worst:.3e} over {len(points) + 2} points")
    assert worst <= 1e-12
    gm, sm_ = res["best_macro"]["index"]
    assert res["best_macro"]["macro_auc"] == res["macro_auc"].max() == res["macro_auc"][gm, sm_]
    assert (gm, sm_) == tuple(int(x) for x in np.unravel_index(np.argmax(res["macro_auc"]), (100, 20)))

    # the intervals: np.percentile of the replica AUCs recomputed on the host from the kept blocks
    _, _, n_pos, n_neg = VC.fixture_offsets()
    mult = Hn.bootstrap_multiplicities(12, 1000, 0).astype(np.int64)
    p_r, q_r = mult @ n_pos, mult @ n_neg
    q = [100 * (1 - 0.95) / 2, 100 * (1 + 0.95) / 2]
    rep = {}
    for name in ("best", "at_lam_map"):
        blocks = res[name]["pairs"]
        assert blocks.shape == (12, 12) and blocks.sum() / (2.0 * res["n_pos"] * res["n_neg"]) == res[name]["auc"]
        rep[name] = VC.bootstrap_brute(blocks[None], mult)[:, 0] / (2.0 * p_r * q_r)
        assert res[name]["auc_ci"] == [float(x) for x in np.percentile(rep[name], q)], name
        pv = np.diag(blocks) / (2.0 * n_pos * n_neg)
        assert np.array_equal(pv, res[name]["per_video_auc"])
        macro_r = (mult @ pv) / mult.sum(1)
        # (float64 evaluations of the same twelve-term sums in another order: within 12 * 2^-53 of each other)
        assert np.allclose(res[name]["macro_auc_ci"], np.percentile(macro_r, q), rtol=0, atol=1e-14), name
    gi, si = res["best"]["index"]
    assert res["auc_ci"][gi, si].tolist() == res["best"]["auc_ci"]
    assert np.array_equal(res["replica_auc"][:, gi * 20 + si], rep["best"]) and np.array_equal(res["replica_auc"][:, -1], rep["at_lam_map"])
    d = rep["best"] - rep["at_lam_map"]
    assert res["delta_best_vs_lam_map"] == {"mean": float(d.mean()), "ci": [float(x) for x in np.percentile(d, q)]}
    assert Hn.bootstrap_delta(res, (gi, si), "lam_map") == res["delta_best_vs_lam_map"]
    assert Hn.bootstrap_delta(res, "lam_map", gi * 20 + si)["mean"] == -res["delta_best_vs_lam_map"]["mean"]
    assert res["best_share"] == float(np.mean(np.argmax(res["replica_auc"][:, :2000], axis=1) == gi * 20 + si))

    # the same seed gives the same dictionary, another seed other replicas
    fx2 = Hn.sweep_videos(fx["records"], fx["gt"], device=DEV)
    _same(fx2, res)
    other = Hn.sweep_videos(fx["records"], fx["gt"], seed=1, replicas=200, level=0.9, device=DEV)
    assert np.array_equal(other["auc"], res["auc"]) and np.array_equal(other["macro_auc"], res["macro_auc"])
    assert other["replicas_dropped"] == 0 and not np.array_equal(other["auc_ci"], res["auc_ci"])


def test_sweep_videos_refusals():
    fx = FC.fixture()
    with pytest.raises(ValueError, match="one class"):
        Hn.sweep_videos(fx["records"], [np.zeros_like(g) for g in fx["gt"]], device=DEV)
    with pytest.raises(ValueError, match="replicas"):
        Hn.sweep_videos(fx["records"], fx["gt"], replicas=0, device=DEV)
    with pytest.raises(ValueError, match="unknown fusion channel"):
        Hn.sweep_videos(fx["records"], fx["gt"], ("no_such_channel",), device=DEV)
    # every anomalous frame in one video: two replicas in three draw it... not at all with probability (11/12)^12 = 0.35
    gt = [np.zeros_like(g) for g in fx["gt"]]
    gt[3] = fx["gt"][3]
    res = Hn.sweep_videos(fx["records"], gt, weights=fx["weights"][:3], smooth=[0.55, 1.0], replicas=400, device=DEV)
    m = Hn.bootstrap_multiplicities(12, 400, 0)
    assert res["videos_scored"] == 1 and res["replicas_dropped"] == int((m[:, 3] == 0).sum()) > 0
    assert res["replica_auc"].shape == (400 - res["replicas_dropped"], 7)
    assert np.isnan(res["best"]["per_video_auc"]).sum() == 11 and res["best"]["macro_auc"] == res["best"]["per_video_auc"][3]
    # ... and when no video holds both classes (one video all anomalous, the others all normal) no replica has a macro
    # figure: more than half are dropped, and the bootstrap is refused
    gt = [np.zeros_like(g) for g in fx["gt"]]
    gt[3] = np.ones_like(fx["gt"][3])
    with pytest.raises(ValueError, match="replicas have no AUC"):
        Hn.sweep_videos(fx["records"], gt, weights=fx["weights"][:3], smooth=[0.55, 1.0], replicas=400, device=DEV)


def test_run_fusion_videos_entry(tmp_path, capsys):
    fx = FC.fixture()
    rec_file, grid = tmp_path / "rec.npz", tmp_path / "grid.npz"
    np.savez(rec_file, **run_fusion.flatten_records(fx["records"], fx["gt"]))
    run_fusion.main(["--records", str(rec_file)])
    before = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    run_fusion.main(["--records", str(rec_file), "--videos", "--replicas", "200", "--out", str(grid)])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k, v in before.items():
        if k != "sweep_ms":                                                # (a time)
            assert line[k] == v, k
    new = {"macro_auc_best", "macro_auc_at_lam_map", "videos", "videos_scored", "auc_ci_best", "auc_ci_at_lam_map",
           "macro_auc_ci_best", "best_share", "delta_best_vs_lam_map", "replicas", "replicas_dropped", "seed", "level", "video_ms"}
    assert new <= set(line) and not new & set(before)
    assert (line["videos"], line["videos_scored"], line["replicas"], line["replicas_dropped"], line["seed"], line["level"]) == \
        (12, 12, 200, 0, 0, 0.95)
    res = Hn.sweep_videos(fx["records"], fx["gt"], replicas=200, device=DEV)
    assert line["macro_auc_best"] == res["macro_auc"].max() and line["macro_auc_at_lam_map"] == res["at_lam_map"]["macro_auc"]
    assert line["auc_ci_best"] == res["best"]["auc_ci"] and line["auc_ci_at_lam_map"] == res["at_lam_map"]["auc_ci"]
    assert line["macro_auc_ci_best"] == res["best_macro"]["macro_auc_ci"] and line["best_share"] == res["best_share"]
    assert line["delta_best_vs_lam_map"] == res["delta_best_vs_lam_map"] and line["video_ms"] > 0
    a = np.load(grid)
    assert {"auc", "two_u", "weights", "smooth", "macro_auc", "auc_ci", "macro_auc_ci", "per_video_auc", "pairs_best",
            "pairs_at_lam_map", "per_video_auc_at_lam_map"} == set(a.files)
    assert np.array_equal(a["macro_auc"], res["macro_auc"]) and np.array_equal(a["pairs_best"], res["best"]["pairs"])
    assert a["pairs_best"].sum() == a["two_u"].max() and a["auc_ci"].shape == (100, 20, 2)
    # a records file without labels is refused by name
    bare = {k: v for k, v in run_fusion.flatten_records(fx["records"], fx["gt"]).items() if k != "gt"}
    np.savez(tmp_path / "bare.npz", **bare)
    with pytest.raises(SystemExit, match="gt"):
        run_fusion.main(["--records", str(tmp_path / "bare.npz"), "--videos"])
