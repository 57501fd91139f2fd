"""Curve sweep, the part that needs no GPU: the numpy restatement (tests/curve_cases.py) against
the definitions pair by pair and against scikit-learn's recorded values (tests/golden/curve_metrics_ped2.npz), the host
restatement of sklearn's vertex rule (`harness.roc_eer`), the new C symbols and their argument errors, and the entry's
argument namespace."""
import numpy as np
import pytest

import curve_cases as CC
import fusion_cases as FC
from ammcnet_aaai2021_amd import _lib, harness as Hn, run_fusion


def _same(got, want):
    assert got["two_u"] == want["two_u"]
    assert np.array_equal(got["pts"], want["pts"]) and np.array_equal(got["thr"], want["thr"])
    assert np.abs(got["sums"] - want["sums"]).max() <= 1e-14 * max(1.0, want["sums"].max())


def test_restatement_against_the_definitions_pair_by_pair():
    cases = [(np.array([0.5, 0.5], dtype=np.float32), [0], [1]),                      # P = Q = 1, tied
             (np.array([0.7, 0.2], dtype=np.float32), [0], [1]),                      # P = Q = 1, separated
             (np.array([0.2, 0.7], dtype=np.float32), [0], [1]),                      # ... the wrong way round
             (np.full(9, 0.25, dtype=np.float32), [0, 3, 4, 8], [1, 2, 5, 6, 7]),     # every key equal
             (np.array([0.0, -0.0, 0.0, 1.0, -1.0], dtype=np.float32) + np.float32(0), [0, 1, 3], [2, 4])]
    rng = np.random.default_rng(27)
    for trial in range(300):
        n = int(rng.integers(2, 13))
        key = rng.normal(size=n).astype(np.float32)
        if trial % 3:
            key = np.round(key, trial % 3 - 1).astype(np.float32) + np.float32(0)     # ties
        idx = rng.permutation(n)
        m = int(rng.integers(1, n))
        cases.append((key, np.sort(idx[:m]), np.sort(idx[m:])))
    for key, pos, neg in cases:
        pos, neg = np.asarray(pos), np.asarray(neg)
        got = CC.curve_point(key, pos, neg)
        _same(got, CC.brute(key, pos, neg))
        P, Q = len(pos), len(neg)
        ga, gb = (P * got["pts"][1 + 2 * i] + Q * got["pts"][2 * i] - P * Q for i in (0, 1))
        assert ga <= 0 < gb
    one = CC.curve_point(cases[3][0], np.array(cases[3][1]), np.array(cases[3][2]))
    assert one["pts"].tolist() == [0, 0, 4, 5] and one["thr"][0] == np.inf and one["thr"][1] == np.float32(0.25)
    assert one["sums"].tolist() == [4 * (4 / 9), 0.5 * 4 * (1.0 + 4 / 9)]


RECORDED = ("eer_full", "eer_drop", "ap", "pr_auc")


def _golden_points():
    """(key, labels with 0 = positive, pos, neg, recorded values) of every recorded point"""
    gd, fx = CC.golden(), FC.fixture()
    S = len(fx["smooth"])
    for r, i in enumerate(gd["grid_index"]):
        key = FC.scores(fx["chan"], fx["weights"][i // S], *fx["smooth"][i % S])
        yield key, fx["labels"], fx["pos"], fx["neg"], {nm: gd["grid_" + nm][r] for nm in RECORDED}
    for r, row in enumerate(gd["syn_case"]):
        c, key = CC.synthetic_tied(row)
        labels = np.ones(len(key), dtype=np.int64)
        labels[c["pos"]] = 0
        yield key, labels, c["pos"], c["neg"], {nm: gd["syn_" + nm][r] for nm in RECORDED}


def test_restatement_and_roc_eer_against_scikit_learn():
    compared = left_out = differ = 0
    for key, labels, pos, neg, want in _golden_points():
        got = CC.curve_point(key, pos, neg)
        d = CC.derived(got["pts"], got["sums"], len(pos), len(neg))
        assert abs(d["ap"] - want["ap"]) <= 1e-14 and abs(d["pr_auc"] - want["pr_auc"]) <= 1e-14
        if d["tie"]:
            left_out += 1                             # |G_a| == |G_b|: the argmin of the float rates may take either vertex
        else:
            compared += 1
            assert d["eer_vertex"] == want["eer_full"]
        assert Hn.roc_eer(labels, key, pos_label=0) == want["eer_drop"]
        assert Hn.roc_eer(labels, key, pos_label=0, drop_intermediate=False) == want["eer_full"]
        differ += want["eer_drop"] != want["eer_full"]
        # the interpolated crossing lies between the two vertices' rates
        assert min(got["pts"][1], got["pts"][3]) / len(neg) <= d["eer"] <= max(got["pts"][1], got["pts"][3]) / len(neg)
    assert compared + left_out == 205 and left_out <= 0.05 * (compared + left_out)
    assert differ > 0                                  # sklearn's vertex dropping does move the reference's EER


def test_roc_area_from_the_vertices_is_the_fusion_sweeps():
    fx = FC.fixture()
    two_u = FC.fixture_grid()
    S = len(fx["smooth"])
    for i in range(0, two_u.size, 7):
        key = FC.scores(fx["chan"], fx["weights"][i // S], *fx["smooth"][i % S])
        tps, fps = CC.full_curve(key, fx["pos"], fx["neg"])
        assert int(((tps[1:] + tps[:-1]) * np.diff(fps)).sum()) == two_u[i // S, i % S]     # twice the trapezoids, in int64
        assert CC.curve_point(key, fx["pos"], fx["neg"])["two_u"] == two_u[i // S, i % S]


def test_negated_weights_negate_every_key_exactly():
    c = FC.synthetic(1025, 4, seed=8, decimals=2)
    for w in c["weights"]:
        for a, b in c["smooth"]:
            k1, k2 = FC.scores(c["chan"], w, a, b), FC.scores(c["chan"], -w, a, b)
            assert np.array_equal(k2, -k1 + np.float32(0)) and not np.signbit(k2[k2 == 0]).any()
            assert np.array_equal(Hn.fused_keys(c["chan"], w, (a, b)).view(np.uint32), k1.view(np.uint32))


def test_curve_metrics_is_the_header_derivation():
    c = FC.synthetic(300, 2, seed=4, decimals=1)
    want = CC.curve_grid(c["chan"], c["weights"], c["smooth"], c["pos"], c["neg"])
    P, Q = len(c["pos"]), len(c["neg"])
    got = Hn.curve_metrics(want["two_u"], want["pts"], want["thr"], want["sums"], P, Q)
    d = CC.derived(want["pts"], want["sums"], P, Q)
    for k in ("eer", "eer_vertex", "ap", "pr_auc"):
        assert got[k].shape == (5, 3) and np.array_equal(got[k], d[k]), k
    assert np.array_equal(got["auc"], want["two_u"] / (2.0 * P * Q))
    pts = want["pts"]
    first = np.abs(P * pts[..., 1] + Q * pts[..., 0] - P * Q) <= np.abs(P * pts[..., 3] + Q * pts[..., 2] - P * Q)
    assert first.any() and not first.all()
    assert np.array_equal(got["threshold_eer"][first], want["thr"][..., 0][first])
    assert np.array_equal(got["threshold_eer"][~first], want["thr"][..., 1][~first])


def test_symbols_are_exported_and_reject_argument_errors_without_a_gpu():
    lib = _lib.load()
    cap = lib.ammc_curve_sweep_max_class()
    assert cap == 32768
    q = lib.ammc_curve_sweep_workspace_bytes
    assert q(1, 1, 1) == 256 and q(3, 64, 2) == 3 * 256 and q(2, 65, 70) == 2 * 512 and q(2000, 1104, 858) == 2000 * 1152 * 4
    assert q(1, cap, 5000) == 4 * cap and q(0, 5, 5) == 0 and q(1, 0, 5) == 0 and q(1, cap + 1, 5) == 0 and q(1, 5, cap + 1) == 0
    # fake, aligned, never dereferenced addresses: every refusal below is decided before anything touches the device
    ok = dict(chan=0x100000, rs=50000, k=2, n=50000, w=0x200000, g=3, sm=0x300000, s=2, pos=0x400000, p=30000,
              neg=0x500000, q=20000, two_u=0x600000, pts=0x700000, thr=0x800000, sums=0x900000, ws=0xA00000,
              wsb=q(6, 30000, 20000))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ammc_curve_sweep_f32(a["chan"], a["rs"], a["k"], a["n"], a["w"], a["g"], a["sm"], a["s"], a["pos"], a["p"],
                                        a["neg"], a["q"], a["two_u"], a["pts"], a["thr"], a["sums"], a["ws"], a["wsb"], None)
    for name in ("chan", "w", "sm", "pos", "neg", "two_u", "pts", "thr", "sums", "ws"):
        assert call(**{name: None}) == -1, name                            # null pointers
    assert call(k=0) == -1 and call(k=9) == -1 and call(k=-1) == -1       # K < 1, K > 8
    assert call(n=1, p=1, q=0) == -1 and call(n=1, p=0, q=1) == -1 and call(n=0, p=0, q=0) == -1      # N < 2
    assert call(p=0, q=50000) == -1 and call(p=50000, q=0) == -1         # an empty class (and one over the capacity)
    assert call(p=30001) == -1                                            # P + Q != N
    assert call(g=0) == -1 and call(s=0) == -1 and call(g=-3) == -1       # G or S < 1
    assert call(rs=49999) == -1                                           # rows overlap
    for name, bad in (("chan", 0x100002), ("two_u", 0x600004), ("sums", 0x900004), ("pts", 0x700002), ("thr", 0x800001),
                      ("ws", 0xA00002)):
        assert call(**{name: bad}) == -1, name                            # alignment
    # over capacity: either class
    assert call(n=cap + 1 + 5, rs=cap + 6, p=cap + 1, q=5, wsb=1 << 40) == -1
    assert call(n=cap + 1 + 5, rs=cap + 6, p=5, q=cap + 1, wsb=1 << 40) == -1
    assert call(wsb=ok["wsb"] - 1) == -1 and call(wsb=0) == -1 and call(g=4) == -1      # a workspace below the query's answer
    assert call(g=1 << 16, s=1 << 15, wsb=1 << 62) == -2                  # the grid's x dimension
    with pytest.raises(_lib.AmmcHipError):
        _lib.check(call(k=9), "curve_sweep")


def test_ops_wrapper_refuses_cpu_tensors_and_names_the_limits():
    import torch
    from ammcnet_aaai2021_amd import ops
    assert ops.CURVE_MAX_CLASS == _lib.load().ammc_curve_sweep_max_class()
    c = FC.synthetic(65, 2)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items()}
    args = (t["chan"], t["pos"], t["neg"], t["weights"], t["smooth"])
    with pytest.raises(_lib.AmmcHipError):                                 # no CPU fallback
        ops.curve_sweep(*args)
    n = ops.CURVE_MAX_CLASS + 6
    idx = torch.arange(n, dtype=torch.int32)
    for cut in (5, n - 5):                                                 # either class over the capacity
        with pytest.raises(ValueError, match="32768"):
            ops.curve_sweep(torch.zeros(1, n), idx[:cut], idx[cut:], torch.ones(1, 1), torch.ones(1, 2))
    with pytest.raises(ValueError, match="max_workspace_bytes = 100 "):
        ops.curve_sweep(*args, max_workspace_bytes=100)
    with pytest.raises(ValueError):
        ops.curve_sweep(t["chan"], t["pos"], t["neg"][:-1], t["weights"], t["smooth"])           # P + Q != N
    with pytest.raises(ValueError):
        ops.curve_sweep(t["chan"], t["pos"].long(), t["neg"], t["weights"], t["smooth"])         # int32 lists
    with pytest.raises(ValueError):
        ops.curve_sweep(t["chan"].double(), t["pos"], t["neg"], t["weights"], t["smooth"])       # fp32 channels


def test_run_fusion_without_curves_parses_to_the_same_namespace():
    argv = ["--records", "rec.npz", "--channels", "rgb_img_pred,rgb_ssim", "--step", "0.25", "--out", "grid.npz"]
    before = run_fusion.build_parser().parse_args(argv)                    # the parser the entry had: its options are pinned
    a, c = run_fusion.parse_args(argv)                                     # by tests/test_eval_passes_host.py
    assert a == before and not hasattr(a, "curves") and not hasattr(a, "positive")
    assert c.curves is False and c.positive == "normal"
    a, c = run_fusion.parse_args(argv[:4] + ["--curves", "--positive", "anomalous"] + argv[4:])
    assert a == before and c.curves is True and c.positive == "anomalous"
    for bad in (["--positive", "both"], ["--curve"], ["--no_such_option"], ["stray"]):
        with pytest.raises(SystemExit):
            run_fusion.parse_args(argv + bad)
    assert "--curves" in run_fusion.build_parser().format_help()
