"""Score-fusion sweep, the part that needs no GPU: the new C symbols and their argument errors, the grids, the channel
table's orientation, and the numpy restatement (tests/fusion_cases.py) against the project's existing fusion and AUC."""
import ctypes as C

import numpy as np
import pytest

import fusion_cases as FC
from ammcnet_aaai2021_amd import _lib, harness as Hn


def test_symbols_are_exported_and_reject_argument_errors_without_a_gpu():
    lib = _lib.load()
    assert lib.ammc_fusion_sweep_max_sorted() == 32768
    cap = lib.ammc_fusion_sweep_max_sorted()
    # fake, aligned, never dereferenced addresses: every refusal below is decided before anything touches the device
    ok = dict(chan=0x100000, rs=100000, k=2, n=100000, w=0x200000, g=3, sm=0x300000, s=2, pos=0x400000, p=70000,
              neg=0x500000, q=30000, out=0x600000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ammc_fusion_sweep_f32(a["chan"], a["rs"], a["k"], a["n"], a["w"], a["g"], a["sm"], a["s"], a["pos"], a["p"],
                                         a["neg"], a["q"], a["out"], None)
    for name in ("chan", "w", "sm", "pos", "neg", "out"):
        assert call(**{name: None}) == -1, name                            # null pointers
    assert call(k=0) == -1 and call(k=9) == -1 and call(k=-1) == -1       # K < 1, K > 8
    assert call(n=1, p=1, q=0) == -1 and call(n=1, p=0, q=1) == -1 and call(n=0, p=0, q=0) == -1      # N < 2
    assert call(p=0, q=100000) == -1 and call(p=100000, q=0) == -1       # an empty class
    assert call(p=70001) == -1                                            # P + Q != N
    assert call(g=0) == -1 and call(s=0) == -1 and call(g=-3) == -1       # G or S < 1
    assert call(rs=99999) == -1                                           # rows overlap
    assert call(chan=0x100002) == -1 and call(out=0x600004) == -1         # alignment
    # over capacity: the smaller class, whichever it is
    assert call(n=2 * cap + 2, rs=2 * cap + 2, p=cap + 1, q=cap + 1) == -1
    assert call(n=100000 + cap + 1, rs=200000, p=100000, q=cap + 1) == -1
    assert call(n=100000 + cap + 1, rs=200000, p=cap + 1, q=100000) == -1
    assert call(g=1 << 16, s=1 << 15) == -2                               # the grid's x dimension
    with pytest.raises(_lib.AmmcHipError):
        _lib.check(call(k=9), "fusion_sweep")


def test_ops_wrapper_refuses_cpu_tensors_and_names_the_capacity():
    import torch
    from ammcnet_aaai2021_amd import ops
    assert ops.FUSION_MAX_SORTED == _lib.load().ammc_fusion_sweep_max_sorted()
    c = FC.synthetic(65, 2)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items()}
    with pytest.raises(_lib.AmmcHipError):                                 # no CPU fallback
        ops.fusion_sweep(t["chan"], t["pos"], t["neg"], t["weights"], t["smooth"])
    n = 2 * ops.FUSION_MAX_SORTED + 2
    idx = torch.arange(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="32768"):
        ops.fusion_sweep(torch.zeros(1, n), idx[: n // 2], idx[n // 2:], torch.ones(1, 1), torch.ones(1, 2))
    with pytest.raises(ValueError):
        ops.fusion_sweep(t["chan"], t["pos"], t["neg"][:-1], t["weights"], t["smooth"])          # P + Q != N
    with pytest.raises(ValueError):
        ops.fusion_sweep(t["chan"], t["pos"].long(), t["neg"], t["weights"], t["smooth"])        # int32 lists


def test_fusion_grid_two_channels_is_the_reference_grid():
    g = Hn.fusion_grid(2)
    assert g["lam_fea"] == [x * 0.01 for x in range(0, 100)]              # main/eval_metric.py:422
    assert g["lam_smooth"] == [x * 0.05 for x in range(0, 20)]            # main/eval_metric.py:423
    assert g["weights"].dtype == np.float32 and g["weights"].shape == (100, 2)
    assert g["smooth"].dtype == np.float32 and g["smooth"].shape == (20, 2)
    fx = FC.fixture()
    assert np.array_equal(g["weights"], fx["weights"]) and np.array_equal(g["smooth"], fx["smooth"])
    assert Hn.fusion_grid(2)["weights"][1].tolist() == [float(np.float32(0.99)), float(np.float32(0.01))]
    assert np.array_equal(Hn.fusion_grid(1, 0.5)["weights"], np.ones((1, 1), dtype=np.float32))


def test_fusion_grid_four_channels_step_tenth():
    w = Hn.fusion_grid(4)["weights"]
    assert w.shape == (286, 4) and w.dtype == np.float32
    assert np.array_equal(w, Hn.fusion_grid(4, 0.1)["weights"])
    assert len({tuple(v) for v in w.tolist()}) == 286
    m = np.rint(w.astype(np.float64) * 10).astype(int)
    assert (m >= 0).all() and (m.sum(1) == 10).all()
    assert np.array_equal(w, (m / 10).astype(np.float32))                 # each entry float32(m / M)
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 2.0 ** -23  # 1 ulp of fp32 at 1
    assert Hn.fusion_grid(4, 0.05)["weights"].shape[0] == 1771
    assert Hn.fusion_grid(2, 0.1)["weights"].shape == (11, 2)


def test_channel_table_orientation_reproduces_the_reference_fusion_bit_for_bit():
    fx = FC.fixture()
    for key in ("rgb_img_pred", "op_img_pred", "rgb_fea_comm", "op_fea_comm", "rgb_ssim", "op_ssim", "rgb_mse", "op_mse",
                "rgb_clip_comm", "op_clip_comm", "rgb_patch_psnr"):
        assert Hn.FUSION_CHANNELS[key][0] == key + "_records"
    kinds = {k: v[1] for k, v in Hn.FUSION_CHANNELS.items()}
    assert {k for k, v in kinds.items() if v == "comm"} == {"rgb_fea_comm", "op_fea_comm", "rgb_clip_comm", "op_clip_comm"}
    assert {k for k, v in kinds.items() if v == "mse"} == {"rgb_mse", "op_mse"}
    chan = Hn.fusion_channels(fx["records"], ("rgb_img_pred", "rgb_fea_comm"))
    assert chan.dtype == np.float32 and np.array_equal(chan, fx["chan"])
    # the restated scores are fuse_scores_auc's, in every bit, at every point of the reference's grid
    for g, l1 in enumerate(fx["lam_fea"]):
        for s, l2 in enumerate(fx["lam_smooth"]):
            want = Hn.fuse_scores_auc(fx["records"], fx["gt"], (l1, l2))["scores"]
            got = FC.scores(chan, fx["weights"][g], *fx["smooth"][s])
            assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32)), (l1, l2)
    # an error record is negated before the normalisation; a missing record is an error, not a silent skip
    rec = dict(fx["records"], rgb_mse_records=[-r for r in fx["records"]["rgb_img_pred_records"]])
    assert np.array_equal(Hn.fusion_channels(rec, ("rgb_mse",))[0], chan[0])
    with pytest.raises(ValueError):
        Hn.fusion_channels(fx["records"], ("rgb_ssim",))
    with pytest.raises(ValueError):
        Hn.fusion_channels(fx["records"], ("no_such_channel",))


def test_restatement_agrees_with_the_existing_auc_on_the_fixture_grid():
    fx = FC.fixture()
    two_u = FC.fixture_grid()
    denom = 2.0 * len(fx["pos"]) * len(fx["neg"])
    worst, tied = 0.0, 0
    for g in range(len(fx["weights"])):
        for s in range(len(fx["smooth"])):
            key = FC.scores(fx["chan"], fx["weights"][g], *fx["smooth"][s])
            worst = max(worst, abs(two_u[g, s] / denom - Hn.roc_auc(fx["labels"], key, pos_label=0)))
            tied += len(np.unique(key)) < len(key)
    assert worst <= 1e-12, worst
    assert tied > 0                                                        # the tie term is exercised by real data
    # the searchsorted form against the definition pair by pair, ties and signed zeros included
    c = FC.synthetic(65, 2, decimals=1)
    c["chan"][1, ::7] = 0.0
    for w in (c["weights"][1], np.array([-1.0, 0.0], dtype=np.float32), np.array([0.0, -1.0], dtype=np.float32)):
        for a, b in c["smooth"]:
            key = FC.scores(c["chan"], w, a, b)
            assert FC.two_u_point(key, c["pos"], c["neg"]) == FC.two_u_brute(key, c["pos"], c["neg"])


def test_restatement_rounds_to_the_golden_aucs():
    fx = FC.fixture()
    denom = 2.0 * len(fx["pos"]) * len(fx["neg"])
    for name, ((l1, l2), auc) in fx["golden"].items():
        key = FC.scores(fx["chan"], np.array([1 - l1, l1], dtype=np.float32), *FC.pairs([l2])[0])
        assert round(FC.two_u_point(key, fx["pos"], fx["neg"]) / denom, 3) == auc, name
