"""The curve sweep on the device (csrc/curve_sweep.hip, `ops.curve_sweep`, `harness.sweep_curves`, `run_fusion --curves`;
DESIGN.md section 5.27) against the numpy restatement of tests/curve_cases.py.  two_u, pts and thr are compared with ==;
the two sums, divided by P, within (P + 4) 2^-52: at most P terms of at most their multiplicity on each side, both sides
rounding (include/ammc_hip.h).

Shapes: the smallest at which the two sorts, the searches and the run detection can go wrong - N = 2 and 3, a class of
1, class sizes 255 / 256 / 257 (the thread count) and 4096 / 4097 (the step from 256 to 1024 threads, a padding edge),
each as the positive and as the negative class; every key equal; coarse channels; the capacity (32768 beside 5000)."""
import json

import numpy as np
import pytest
import torch

import curve_cases as CC
import fusion_cases as FC
from ammcnet_aaai2021_amd import harness as Hn, ops, run_fusion

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("two_u", "pts", "thr", "sums")


def _dev(c):
    return {k: torch.from_numpy(np.array(v, order="C")).to(DEV) for k, v in c.items()}       # (a copy: the fixture is read-only)


def _run(c, **kw):
    d = _dev(c)
    got = ops.curve_sweep(d["chan"], d["pos"], d["neg"], d["weights"], d["smooth"], **kw)
    two_u = ops.fusion_sweep(d["chan"], d["pos"], d["neg"], d["weights"], d["smooth"])
    assert tuple(got) == KEYS and torch.equal(got["two_u"], two_u)         # the fusion sweep's integers, on every case
    return {k: v.cpu().numpy() for k, v in got.items()}


def _want(c):
    return CC.curve_grid(c["chan"], c["weights"], c["smooth"], c["pos"], c["neg"])


def _check(got, want, P, tag=None):
    g, s = want["two_u"].shape
    assert got["two_u"].dtype == np.int64 and got["pts"].dtype == np.int32 and got["thr"].dtype == np.float32
    assert got["sums"].dtype == np.float64 and got["pts"].shape == (g, s, 4) and got["sums"].shape == (g, s, 2)
    assert np.array_equal(got["two_u"], want["two_u"]), tag
    assert np.array_equal(got["pts"], want["pts"]), tag
    assert np.array_equal(got["thr"], want["thr"]), tag
    err = np.abs(got["sums"] / P - want["sums"] / P).max()
    print(f"curve_sweep {tag}: P = {P}, worst |ap or pr_auc difference| = {err:.3e}, gate {CC.gate(P):.3e}")
    assert err <= CC.gate(P), (tag, err)


def _same(a, b):
    for k in KEYS:                                                         # the doubles included
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [2, 3, 65, 1025])
def test_sizes_and_channel_counts(n):
    for k in (1, 2, 8):
        for small in ("neg", "pos"):
            c = FC.synthetic(n, k, small=small)
            _check(_run(c), _want(c), len(c["pos"]), (n, k, small))


@pytest.mark.parametrize("small", ["neg", "pos"])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 4096, 4097])
def test_class_sizes_around_the_thread_count_and_the_padding_boundaries(m, small):
    # m as the smaller class beside a larger one just above it, and (m >= 255) as the larger class beside 100
    cases = [FC.synthetic(2 * m + m // 4 + 3, 2, m=m, small=small, g=2, s=2)]
    if m > 1:
        cases.append(FC.synthetic(m + 100, 2, m=100, small="pos" if small == "neg" else "neg", g=2, s=2))
        assert max(len(cases[1]["pos"]), len(cases[1]["neg"])) == m
    assert min(len(cases[0]["pos"]), len(cases[0]["neg"])) == m
    for c in cases:
        _check(_run(c), _want(c), len(c["pos"]), (m, small))


def test_every_key_equal_is_one_vertex():
    c = FC.synthetic(1025, 2, seed=5)
    c["chan"][1] = np.float32(0.3)
    c["weights"] = np.array([[0.0, 1.0]], dtype=np.float32)
    c["smooth"] = FC.pairs([0.0, 1.0, 0.5])                               # a * v + b * v == v exactly
    for case in (c, dict(c, pos=c["neg"], neg=c["pos"])):
        got = _run(case)
        P, Q = len(case["pos"]), len(case["neg"])
        assert (got["pts"] == np.array([0, 0, P, Q])).all() and np.isposinf(got["thr"][..., 0]).all()
        assert (got["thr"][..., 1] == np.float32(0.3)).all() and (got["two_u"] == P * Q).all()
        _check(got, _want(case), P, "constant")


def test_ties_from_coarse_channels_and_signed_zeros():
    for n, k in ((65, 2), (1025, 4), (5000, 2)):
        c = FC.synthetic(n, k, decimals=1, seed=3)
        c["weights"][1:] = np.round(c["weights"][1:], 1)
        key = FC.scores(c["chan"], c["weights"][0], *c["smooth"][1])
        assert len(np.unique(key)) < n // 2                                # ties are the rule here
        _check(_run(c), _want(c), len(c["pos"]), ("ties", n, k))
    rng = np.random.default_rng(11)
    n = 600
    chan = np.round(rng.normal(size=(1, n)), 1).astype(np.float32)         # signed, many exact zeros
    chan[0, rng.choice(n, size=200, replace=False)] = 0.0
    labels = rng.random(n) < 0.4
    c = {"chan": chan, "pos": np.flatnonzero(~labels).astype(np.int32), "neg": np.flatnonzero(labels).astype(np.int32),
         "weights": np.array([[-1.0], [1.0]], dtype=np.float32), "smooth": FC.pairs([1.0, 0.0, 0.5])}
    raw = FC.scores(chan, c["weights"][0], *c["smooth"][0], raw=True)
    assert np.signbit(raw[raw == 0]).any() and not np.signbit(raw[raw == 0]).all()      # both -0.0 and +0.0 are there
    got = _run(c)
    _check(got, _want(c), len(c["pos"]), "zeros")
    assert not np.signbit(got["thr"][got["thr"] == 0]).any()               # a threshold of zero is +0.0, the key's value


def test_fixture_full_reference_grid():
    fx = FC.fixture()
    c = {k: fx[k] for k in ("chan", "pos", "neg", "weights", "smooth")}
    got = _run(c)
    assert np.array_equal(got["two_u"], FC.fixture_grid())
    _check(got, CC.fixture_curves(), len(fx["pos"]), "ped2")


def test_placement_strides_chunks_out_repeats():
    c = FC.synthetic(5000, 4, seed=9)
    d = _dev(c)
    args = (d["pos"], d["neg"])
    base = ops.curve_sweep(d["chan"], *args, d["weights"], d["smooth"])
    _check({k: v.cpu().numpy() for k, v in base.items()}, _want(c), len(c["pos"]), "base")
    # a grid point alone = the same point inside the grid
    for g, s in ((0, 0), (3, 2), (4, 1)):
        one = ops.curve_sweep(d["chan"], *args, d["weights"][g:g + 1].contiguous(), d["smooth"][s:s + 1].contiguous())
        _same(one, {k: v[g:g + 1, s:s + 1] for k, v in base.items()})
    # a strided view of the channels (rows 5003 floats apart, an odd start)
    wide = torch.full((4, 5003), float("nan"), device=DEV)
    wide[:, 3:] = d["chan"]
    assert not wide[:, 3:].is_contiguous()
    _same(ops.curve_sweep(wide[:, 3:], *args, d["weights"], d["smooth"]), base)
    # one point per launch, two points per launch (parts of a weight row), two weight rows per launch
    row = ops._lib.load().ammc_curve_sweep_workspace_bytes(1, len(c["pos"]), len(c["neg"]))
    for points in (1, 2, 6):
        _same(ops.curve_sweep(d["chan"], *args, d["weights"], d["smooth"], max_workspace_bytes=points * row + 7), base)
    # out=: written in place and returned; a wrong or an unknown slot is refused
    out = {"sums": torch.zeros(5, 3, 2, dtype=torch.float64, device=DEV), "pts": torch.zeros(5, 3, 4, dtype=torch.int32, device=DEV)}
    ret = ops.curve_sweep(d["chan"], *args, d["weights"], d["smooth"], out=out)
    assert ret["sums"].data_ptr() == out["sums"].data_ptr() and ret["pts"].data_ptr() == out["pts"].data_ptr()
    _same(ret, base)
    with pytest.raises(ValueError):
        ops.curve_sweep(d["chan"], *args, d["weights"], d["smooth"], out={"sums": torch.zeros(5, 3, 2, device=DEV)})
    with pytest.raises(ValueError):
        ops.curve_sweep(d["chan"], *args, d["weights"], d["smooth"], out={"auc": torch.zeros(5, 3, device=DEV)})
    _same(ops.curve_sweep(d["chan"], *args, d["weights"], d["smooth"]), base)      # launches repeat


def test_capacity_exactly_and_one_beyond():
    cap = ops.CURVE_MAX_CLASS
    c = FC.synthetic(cap + 5000, 2, m=5000, small="neg", g=1, s=1)
    assert len(c["pos"]) == cap
    _check(_run(c), _want(c), cap, "capacity")
    c = FC.synthetic(cap + 5001, 2, m=5000, small="pos", g=1, s=1)
    d = _dev(c)
    out = {"two_u": torch.full((1, 1), -7, dtype=torch.int64, device=DEV)}
    with pytest.raises(ValueError, match=str(cap)):
        ops.curve_sweep(d["chan"], d["pos"], d["neg"], d["weights"], d["smooth"], out=out)
    torch.cuda.synchronize()
    assert int(out["two_u"].cpu()) == -7                                   # nothing was launched


def test_sweep_curves_on_the_fixture_and_its_golden_point():
    fx, gd = FC.fixture(), CC.golden()
    res = Hn.sweep_curves(fx["records"], fx["gt"], device=DEV)
    P, Q = len(fx["pos"]), len(fx["neg"])
    want = CC.fixture_curves()
    d = CC.derived(want["pts"], want["sums"], P, Q)
    assert np.array_equal(res["two_u"], FC.fixture_grid()) and np.array_equal(res["pts"], want["pts"])
    assert np.array_equal(res["auc"], FC.fixture_grid() / (2.0 * P * Q))
    assert np.array_equal(res["eer"], d["eer"]) and np.array_equal(res["eer_vertex"], d["eer_vertex"])       # from integers
    assert np.abs(res["ap"] - d["ap"]).max() <= CC.gate(P) and np.abs(res["pr_auc"] - d["pr_auc"]).max() <= CC.gate(P)
    # scikit-learn's recorded values at every 10th point
    flat = gd["grid_index"]
    assert np.abs(res["ap"].ravel()[flat] - gd["grid_ap"]).max() <= CC.gate(P) + 1e-14
    assert np.abs(res["pr_auc"].ravel()[flat] - gd["grid_pr_auc"]).max() <= CC.gate(P) + 1e-14
    sure = ~d["tie"].ravel()[flat]
    assert np.array_equal(res["eer_vertex"].ravel()[flat][sure], gd["grid_eer_full"][sure])
    # best: the first extremum in grid order, all values there, the reference's literal EER beside them
    for name, pick in (("auc", np.argmax), ("eer", np.argmin), ("ap", np.argmax)):
        b = res["best"][name]
        gi, si = np.unravel_index(pick(res[name]), res[name].shape)
        assert b["index"] == (gi, si) and b["weights"] == [float(x) for x in fx["weights"][gi]] and b["lam_smooth"] == fx["lam_smooth"][si]
        assert all(b[k] == res[k][gi, si] for k in Hn.CURVE_KEYS + ("threshold_eer",))
        key = FC.scores(fx["chan"], fx["weights"][gi], *fx["smooth"][si])
        assert b["eer_reference"] == Hn.roc_eer(fx["labels"], key, pos_label=0)
    # the published pair against scikit-learn's recorded values and against the restatement
    lam = Hn.LAM_MAP["ped2"]
    assert res["lam_map"] == lam == tuple(gd["lam_map"])
    key = FC.scores(fx["chan"], np.array([1 - lam[0], lam[0]], dtype=np.float32), *FC.pairs([lam[1]])[0])
    one = CC.curve_point(key, fx["pos"], fx["neg"])
    d1 = CC.derived(one["pts"], one["sums"], P, Q)
    at = res["at_lam_map"]
    assert not d1["tie"] and at["eer_vertex"] == float(d1["eer_vertex"]) == float(gd["lam_eer_full"])
    assert at["eer"] == float(d1["eer"]) and at["eer_reference"] == float(gd["lam_eer_drop"])
    assert abs(at["ap"] - gd["lam_ap"]) <= CC.gate(P) + 1e-14 and abs(at["pr_auc"] - gd["lam_pr_auc"]) <= CC.gate(P) + 1e-14
    assert abs(at["ap"] - d1["ap"]) <= CC.gate(P) and abs(at["pr_auc"] - d1["pr_auc"]) <= CC.gate(P)
    assert abs(at["auc"] - Hn.fuse_scores_auc(fx["records"], fx["gt"])["auc_raw"]) <= 1e-12
    assert at["eer_reference"] == Hn.roc_eer(fx["labels"], key, pos_label=0)
    assert at["threshold_eer"] in (float(one["thr"][0]), float(one["thr"][1])) and res["sweep_ms"] > 0


def test_sweep_curves_positive_anomalous_is_the_restatement_on_swapped_lists():
    fx = FC.fixture()
    w, lam_smooth = fx["weights"][::25], [0.0, 0.55, 1.0]
    res = Hn.sweep_curves(fx["records"], fx["gt"], weights=w, smooth=lam_smooth, positive="anomalous", device=DEV)
    want = CC.curve_grid(fx["chan"], -w, FC.pairs(lam_smooth), fx["neg"], fx["pos"])
    P, Q = len(fx["neg"]), len(fx["pos"])
    assert (res["n_pos"], res["n_neg"]) == (P, Q) and np.array_equal(res["weights"], w)
    d = CC.derived(want["pts"], want["sums"], P, Q)
    assert np.array_equal(res["pts"], want["pts"]) and np.array_equal(res["two_u"], want["two_u"])
    assert np.array_equal(res["eer"], d["eer"]) and np.abs(res["ap"] - d["ap"]).max() <= CC.gate(P)
    assert np.abs(res["pr_auc"] - d["pr_auc"]).max() <= CC.gate(P)
    normal = Hn.sweep_curves(fx["records"], fx["gt"], weights=w, smooth=lam_smooth, device=DEV)
    assert np.array_equal(normal["two_u"], res["two_u"])                   # the ROC area does not care which class is positive
    assert not np.array_equal(normal["ap"], res["ap"])                     # the average precision does
    with pytest.raises(ValueError):
        Hn.sweep_curves(fx["records"], fx["gt"], positive="both", device=DEV)


def test_two_streams():
    a, b = FC.synthetic(5000, 2, seed=1), FC.synthetic(1025, 8, seed=2)
    da, db = _dev(a), _dev(b)
    want_a, want_b = _want(a), _want(b)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    got_a, got_b = [], []
    for _ in range(3):
        with torch.cuda.stream(s1):
            got_a.append(ops.curve_sweep(da["chan"], da["pos"], da["neg"], da["weights"], da["smooth"]))
        with torch.cuda.stream(s2):
            got_b.append(ops.curve_sweep(db["chan"], db["pos"], db["neg"], db["weights"], db["smooth"]))
    torch.cuda.synchronize()
    for g in got_a:
        _check({k: v.cpu().numpy() for k, v in g.items()}, want_a, len(a["pos"]), "stream 1")
        _same(g, got_a[0])
    for g in got_b:
        _check({k: v.cpu().numpy() for k, v in g.items()}, want_b, len(b["pos"]), "stream 2")
        _same(g, got_b[0])


def test_run_fusion_curves_entry(tmp_path, capsys):
    rec_file, grid = tmp_path / "rec.npz", tmp_path / "grid.npz"
    fx = FC.fixture()
    np.savez(rec_file, **run_fusion.flatten_records(fx["records"], fx["gt"]))
    run_fusion.main(["--records", str(rec_file), "--dataset_name", "ped2"])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    run_fusion.main(["--records", str(rec_file), "--dataset_name", "ped2", "--curves", "--out", str(grid)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any("eer" in k or "pr_auc" in k or k.startswith("ap") for k in plain)
    assert all(line[k] == v for k, v in plain.items() if k != "sweep_ms")  # the flag only adds
    res = Hn.sweep_curves(fx["records"], fx["gt"], device=DEV)
    assert line["eer_best"] == res["eer"].min() and line["ap_best"] == res["ap"].max()
    assert line["pr_auc_best"] == res["best"]["ap"]["pr_auc"] and line["positive"] == "normal"
    for k in ("eer", "eer_vertex", "eer_reference", "pr_auc", "threshold_eer"):
        assert line[f"{k}_at_lam_map"] == res["at_lam_map"][k], k
    a = np.load(grid)
    assert {"auc", "two_u", "weights", "smooth", "eer", "eer_vertex", "ap", "pr_auc", "threshold_eer", "pts"} == set(a.files)
    assert np.array_equal(a["eer"], res["eer"]) and np.array_equal(a["pts"], res["pts"]) and a["ap"].shape == (100, 20)
    run_fusion.main(["--records", str(rec_file), "--dataset_name", "ped2", "--curves", "--positive", "anomalous"])
    other = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert other["positive"] == "anomalous" and other["auc_best"] == line["auc_best"] and other["ap_best"] != line["ap_best"]
