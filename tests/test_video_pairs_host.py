"""Per-video pair counts and the video bootstrap, the part that needs no GPU: the new C symbols
and their argument errors, the wrappers' refusals, the offsets, the multiplicity table, the replica statistics on a
hand-made block, and the numpy restatement (tests/video_cases.py) against the existing golden grid."""
import numpy as np
import pytest

import fusion_cases as FC
import video_cases as VC
from ammcnet_aaai2021_amd import _lib, harness as Hn


def test_symbols_are_exported_and_reject_argument_errors_without_a_gpu():
    lib = _lib.load()
    seg, vmax = lib.ammc_video_pairs_max_segment(), lib.ammc_video_pairs_max_videos()
    assert 1 <= seg <= 32768 and vmax >= 512
    # fake, aligned, never dereferenced addresses: every refusal below is decided before anything touches the device
    ok = dict(chan=0x100000, rs=100000, k=2, n=100000, w=0x200000, g=3, sm=0x300000, s=2, pos=0x400000, p=70000,
              neg=0x500000, q=30000, poff=0x600000, noff=0x700000, v=12, seg=3000, out=0x800000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ammc_video_pairs_f32(a["chan"], a["rs"], a["k"], a["n"], a["w"], a["g"], a["sm"], a["s"], a["pos"], a["p"],
                                        a["neg"], a["q"], a["poff"], a["noff"], a["v"], a["seg"], a["out"], None)
    for name in ("chan", "w", "sm", "pos", "neg", "poff", "noff", "out"):
        assert call(**{name: None}) == -1, name                            # null pointers
    assert call(k=0) == -1 and call(k=9) == -1                            # K < 1, K > 8
    assert call(v=0) == -1 and call(v=-1) == -1 and call(v=vmax + 1) == -1
    assert call(seg=0) == -1 and call(seg=seg + 1) == -1
    assert call(n=1, p=1, q=0) == -1 and call(p=0, q=100000) == -1 and call(p=70001) == -1
    assert call(g=0) == -1 and call(s=0) == -1 and call(rs=99999) == -1
    assert call(poff=0x600002) == -1 and call(out=0x800004) == -1         # alignment
    assert call(g=1 << 14, s=1 << 14, v=8) == -2                          # the grid's x dimension

    okb = dict(pairs=0x100000, m=5, v=12, mult=0x200000, b=1000, out=0x300000)

    def boot(**kw):
        a = dict(okb, **kw)
        return lib.ammc_bootstrap_pairs_i64(a["pairs"], a["m"], a["v"], a["mult"], a["b"], a["out"], None)
    for name in ("pairs", "mult", "out"):
        assert boot(**{name: None}) == -1, name
    assert boot(b=0) == -1 and boot(v=0) == -1 and boot(v=vmax + 1) == -1 and boot(m=0) == -1
    assert boot(pairs=0x100004) == -1 and boot(mult=0x200002) == -1
    with pytest.raises(_lib.AmmcHipError):
        _lib.check(call(k=9), "video_pairs")


def test_ops_wrappers_refuse_bad_arguments_before_asking_for_a_gpu():
    import torch
    from ammcnet_aaai2021_amd import ops
    lib = _lib.load()
    assert ops.VIDEO_PAIRS_MAX_SEGMENT == lib.ammc_video_pairs_max_segment()
    assert ops.VIDEO_PAIRS_MAX_VIDEOS == lib.ammc_video_pairs_max_videos()
    c = VC.split(FC.synthetic(65, 2), [20, 41])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items()}

    def call(**kw):
        a = dict(t, **kw)
        return ops.video_pairs(a["chan"], a["pos"], a["neg"], a["pos_off"], a["neg_off"], a["weights"], a["smooth"])
    with pytest.raises(_lib.AmmcHipError):                                 # everything in order: no CPU fallback
        call()
    with pytest.raises(_lib.AmmcHipError):                                 # lists are accepted like CPU tensors
        call(pos_off=c["pos_off"].tolist(), neg_off=list(c["neg_off"]))
    for bad in (dict(chan=t["chan"].double()), dict(pos=t["pos"].long()), dict(neg=t["neg"][:-1]),
                dict(pos_off=t["pos_off"].float()), dict(pos_off=t["pos_off"][:-1]),                  # dtype; V + 1 entries
                dict(pos_off=t["pos_off"].reshape(2, 2)), dict(neg_off=t["neg_off"][:1]),
                dict(pos_off=t["pos_off"] + 1), dict(neg_off=torch.flip(t["neg_off"], [0])),         # first entry; decreasing
                dict(neg_off=torch.cat([t["neg_off"][:-1], t["neg_off"][-1:] - 1]))):                 # last entry != Q
        with pytest.raises(ValueError):
            call(**bad)
    # the limits, named
    n = ops.VIDEO_PAIRS_MAX_VIDEOS + 3
    idx = torch.arange(n, dtype=torch.int32)
    off = list(range(n - 1)) + [n - 2]
    with pytest.raises(ValueError, match=str(ops.VIDEO_PAIRS_MAX_VIDEOS)):
        ops.video_pairs(torch.zeros(1, n), idx[:n - 2], idx[n - 2:], off, [0] * (n - 2) + [2, 2], torch.ones(1, 1), torch.ones(1, 2))
    m = ops.VIDEO_PAIRS_MAX_SEGMENT + 1
    idx = torch.arange(2 * m + 2, dtype=torch.int32)
    with pytest.raises(ValueError, match=str(ops.VIDEO_PAIRS_MAX_SEGMENT)):
        ops.video_pairs(torch.zeros(1, 2 * m + 2), idx[:m + 2], idx[m + 2:], [0, m + 2, m + 2], [0, m, m], torch.ones(1, 1),
                        torch.ones(1, 2))

    pairs, mult = torch.zeros(4, 3, 3, dtype=torch.int64), torch.ones(5, 3, dtype=torch.int32)
    with pytest.raises(_lib.AmmcHipError):
        ops.bootstrap_pairs(pairs, mult)
    for bp, bm in ((pairs.int(), mult), (pairs, mult.long()), (pairs[:, :2], mult), (pairs, mult[:, :2]), (pairs[0], mult),
                   (pairs, mult[0]), (pairs.transpose(1, 2)[:, :, :], mult.t().contiguous().t())):
        with pytest.raises(ValueError):
            ops.bootstrap_pairs(bp, bm)


def test_video_offsets_on_a_hand_written_gt():
    D = Hn.DECIDABLE_IDX
    gt = [np.r_[np.ones(D), [0, 0, 1, 0]], np.ones(D), np.r_[np.zeros(D), [1]], np.zeros(D + 3), np.ones(2)]
    vo = Hn.video_offsets(gt, 0)
    assert vo["n_pos"].tolist() == [3, 0, 0, 3, 0] and vo["n_neg"].tolist() == [1, 0, 1, 0, 0]
    assert vo["pos_off"].tolist() == [0, 3, 3, 3, 6, 6] and vo["neg_off"].tolist() == [0, 1, 1, 2, 2, 2]
    sw = Hn.video_offsets(gt, 1)                                           # the other class as the positive one
    assert sw["n_pos"].tolist() == vo["n_neg"].tolist() and sw["neg_off"].tolist() == vo["pos_off"].tolist()
    pos_off, neg_off, n_pos, n_neg = VC.fixture_offsets()
    fo = Hn.video_offsets(FC.fixture()["gt"], 0)
    assert fo["pos_off"].tolist() == pos_off.tolist() and fo["neg_off"].tolist() == neg_off.tolist()
    assert len(n_pos) == 12 and (n_pos > 0).all() and (n_neg > 0).all() and n_neg[-1] == 1


def test_bootstrap_multiplicities():
    for V, B, seed in ((12, 1000, 0), (1, 3, 5), (107, 10, 2)):
        m = Hn.bootstrap_multiplicities(V, B, seed)
        assert m.dtype == np.int32 and m.shape == (B, V) and (m >= 0).all() and (m.sum(1) == V).all()
        assert np.array_equal(m, Hn.bootstrap_multiplicities(V, B, seed))
        want = np.random.Generator(np.random.PCG64(seed)).multinomial(V, np.full(V, 1 / V), size=B)
        assert np.array_equal(m, want)
    assert not np.array_equal(Hn.bootstrap_multiplicities(12, 1000, 0), Hn.bootstrap_multiplicities(12, 1000, 1))
    for seed in (0, 1, 2):                                                 # ped2: no replica without a class
        m = Hn.bootstrap_multiplicities(12, 1000, seed)
        assert m.max() <= 7


def _hand_made():
    """three videos: 0 and 2 hold both classes, 1 has positives only.  Two points; P_a, Q_a; blocks within 2 P_a Q_b."""
    n_pos, n_neg = np.array([2, 3, 1]), np.array([2, 0, 4])
    pairs = np.array([[[6, 0, 10], [9, 0, 20], [1, 0, 8]],
                      [[8, 0, 4], [3, 0, 24], [4, 0, 2]]], dtype=np.int64)
    assert (pairs <= 2 * n_pos[:, None] * n_neg[None, :]).all()
    return pairs, n_pos, n_neg


def test_replica_statistics_on_a_hand_made_block():
    pairs, n_pos, n_neg = _hand_made()
    diag = np.array([np.diag(p) for p in pairs])
    mult = np.array([[1, 1, 1], [3, 0, 0], [0, 3, 0], [0, 0, 3], [2, 1, 0], [1, 0, 2]])
    table = VC.bootstrap_brute(pairs, mult)
    assert table[0].tolist() == [pairs[0].sum(), pairs[1].sum()] and table[3].tolist() == [9 * 8, 9 * 2]
    st = Hn.replica_statistics(table, diag, mult, n_pos, n_neg, level=0.5, best=0)
    assert st["usable"].tolist() == [True, True, False, True, True, True] and st["replicas_dropped"] == 1
    pv = st["per_video_auc"]
    assert np.isnan(pv[:, 1]).all() and pv[0, 0] == 6 / 8 and pv[0, 2] == 1.0 and pv[1, 0] == 1.0 and pv[1, 2] == 0.25
    assert st["macro_auc"].tolist() == [(0.75 + 1.0) / 2, (1.0 + 0.25) / 2]
    auc_r = st["auc_r"]
    assert auc_r.shape == (5, 2)
    assert auc_r[0, 0] == pairs[0].sum() / (2.0 * 6 * 6) and auc_r[1].tolist() == [0.75, 1.0]      # video 0 alone, thrice
    assert auc_r[3, 0] == (4 * 6 + 2 * 9) / (2.0 * 7 * 4)                  # 2 x video 0 + video 1: its positives count too
    assert st["macro_auc_r"][3].tolist() == [0.75, 1.0]                    # the unscored video carries no weight
    assert st["macro_auc_r"][4].tolist() == [(0.75 + 2 * 1.0) / 3, (1.0 + 2 * 0.25) / 3]
    assert np.array_equal(st["auc_ci"], np.percentile(auc_r, [25.0, 75.0], axis=0).T)
    assert np.array_equal(st["macro_auc_ci"], np.percentile(st["macro_auc_r"], [25.0, 75.0], axis=0).T)
    want = np.mean(np.argmax(auc_r, axis=1) == 0)
    assert st["best_share"] == want and 0.0 < want < 1.0


def test_replica_statistics_refuses_more_than_half_dropped_and_resolves_ties_to_the_first_index():
    pairs, n_pos, n_neg = _hand_made()
    diag = np.array([np.diag(p) for p in pairs])
    mult = np.array([[0, 3, 0], [0, 3, 0], [1, 1, 1]])
    with pytest.raises(ValueError, match="2 of 3"):
        Hn.replica_statistics(VC.bootstrap_brute(pairs, mult), diag, mult, n_pos, n_neg)
    half = np.array([[0, 3, 0], [1, 1, 1]])                                # exactly half: not more than half
    assert Hn.replica_statistics(VC.bootstrap_brute(pairs, half), diag, half, n_pos, n_neg)["replicas_dropped"] == 1
    # no video holds both classes: a replica with both classes still has no macro figure, so every replica is dropped
    with pytest.raises(ValueError, match="2 of 2"):
        Hn.replica_statistics(np.zeros((2, 1), dtype=np.int64), np.zeros((1, 2), dtype=np.int64), [[2, 0], [1, 1]], [3, 0], [0, 2])
    # three points, the first and the third equal everywhere: each replica's argmax is the FIRST of the tied ones
    same = np.stack([pairs[0], pairs[1], pairs[0]])
    mult = np.array([[1, 1, 1], [3, 0, 0], [1, 0, 2], [0, 0, 3]])
    table = VC.bootstrap_brute(same, mult)
    diag3 = np.array([np.diag(p) for p in same])
    first = Hn.replica_statistics(table, diag3, mult, n_pos, n_neg, best=0)
    third = Hn.replica_statistics(table, diag3, mult, n_pos, n_neg, best=2)
    wins = np.mean(first["auc_r"][:, 0] >= first["auc_r"][:, 1])
    assert first["best_share"] == wins > 0 and third["best_share"] == 0.0
    # the grid may be a prefix of the points: the appended one never wins
    assert Hn.replica_statistics(table, diag3, mult, n_pos, n_neg, grid_points=2, best=0)["best_share"] == wins


def test_bootstrap_delta_reads_the_replica_table():
    rng = np.random.default_rng(0)
    rep = rng.random((50, 7))
    res = {"auc": np.zeros((2, 3)), "replica_auc": rep, "level": 0.9, "at_lam_map": {}}
    d = Hn.bootstrap_delta(res, (1, 2), 0)
    assert d["mean"] == float((rep[:, 5] - rep[:, 0]).mean())
    q = [100 * (1 - 0.9) / 2, 100 * (1 + 0.9) / 2]                         # the percentiles (1 - level) / 2 and (1 + level) / 2
    assert d["ci"] == [float(x) for x in np.percentile(rep[:, 5] - rep[:, 0], q)]
    assert Hn.bootstrap_delta(res, 3, "lam_map")["mean"] == float((rep[:, 3] - rep[:, 6]).mean())
    assert Hn.bootstrap_delta(res, 2, 2) == {"mean": 0.0, "ci": [0.0, 0.0]}


def test_pairs_brute_summed_over_blocks_is_the_golden_grid():
    fx = FC.fixture()
    pos_off, neg_off, _, _ = VC.fixture_offsets()
    grid = FC.fixture_grid()
    for g, s in ((0, 0), (1, 11), (1, 19), (17, 3), (33, 7), (50, 10), (64, 0), (80, 15), (99, 19), (99, 0)):
        key = FC.scores(fx["chan"], fx["weights"][g], *fx["smooth"][s])
        blocks = VC.pairs_brute(key, fx["pos"], fx["neg"], pos_off, neg_off)
        assert blocks.shape == (12, 12) and blocks.sum() == grid[g, s], (g, s)
        assert np.array_equal(blocks, VC.pairs_searchsorted(key, fx["pos"], fx["neg"], pos_off, neg_off))


def test_run_fusion_tells_the_bare_switch_from_the_number_of_synthetic_videos():
    from ammcnet_aaai2021_amd import run_fusion
    a, cv, vd = run_fusion.parse_args(["--synthetic", "--videos", "2", "--frames", "24"], videos=True)
    assert a.videos == 2 and not vd.videos and not cv.curves
    a, cv, vd = run_fusion.parse_args(["--records", "r.npz", "--videos", "--replicas", "200", "--curves"], videos=True)
    assert a.videos == 4 and vd.videos and vd.replicas == 200 and vd.seed == 0 and vd.level == 0.95 and cv.curves
    a, cv, vd = run_fusion.parse_args(["--synthetic", "--videos", "3", "--videos", "--seed", "7"], videos=True)
    assert a.videos == 3 and vd.videos and vd.seed == 7
    a, cv, vd = run_fusion.parse_args(["--synthetic", "--videos"], videos=True)
    assert a.videos == 4 and vd.videos
    a2, cv2 = run_fusion.parse_args(["--synthetic", "--videos", "2"])     # the two-part form is what it was
    assert a2.videos == 2 and not cv2.curves
