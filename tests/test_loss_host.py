"""CPU-side checks of the fused generator-loss feature: the library exports the loss entry points and answers bad
arguments with status codes before anything touches the device, the partial-row query is sane, `harness.FUSED_LOSS` is
off by default and changes nothing on CPU tensors."""
import os
import re
import subprocess
import sys

import torch

from ammcnet_aaai2021_amd import _lib, harness as Hn, synthetic as S
from conftest import ROOT

NEW = ("ammc_pred_loss_partial_rows", "ammc_pred_loss_fwd_f32", "ammc_pred_loss_bwd_f32", "ammc_l1_partials_f32")


def test_loss_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    n = 4 * 8 * 8                                           # the target's batch stride: room for the c = 4 probe
    fwd = [64, 128, n, 2, 3, 8, 8, 1, 256, None]            # fake (aligned, never dereferenced) addresses
    for pos, val, want in ((0, None, -1), (1, None, -1), (8, None, -1), (3, 0, -1), (5, 0, -1), (6, -1, -1), (0, 66, -1),
                           (2, 3 * 8 * 8 - 1, -1), (4, 4, -2), (4, 1, -2)):
        bad = list(fwd)
        bad[pos] = val
        assert lib.ammc_pred_loss_fwd_f32(*bad) == want, (pos, val)
    bwd = [64, 128, n, 192, 196, 2, 3, 8, 8, 256, None]
    for pos, val, want in ((0, None, -1), (1, None, -1), (9, None, -1), (5, 0, -1), (7, 0, -1), (8, 0, -1), (9, 258, -1),
                           (3, 193, -1), (6, 4, -2)):
        bad = list(bwd)
        bad[pos] = val
        assert lib.ammc_pred_loss_bwd_f32(*bad) == want, (pos, val)
    l1 = [64, 128, 100, 256, None]
    for pos, val in ((0, None), (1, None), (3, None), (2, 0), (2, -5), (0, 65)):
        bad = list(l1)
        bad[pos] = val
        assert lib.ammc_l1_partials_f32(*bad) == -1, (pos, val)


def test_partial_rows_query_and_header_constants():
    lib = _lib.load()
    assert lib.ammc_pred_loss_partial_rows(0, 8, 8) == 0 and lib.ammc_pred_loss_partial_rows(2, 0, 8) == 0
    assert lib.ammc_pred_loss_partial_rows(2, 8, -1) == 0
    last = 0
    for b, h in ((1, 1), (1, 3), (2, 8), (3, 27), (2, 64), (2, 256), (32, 256)):            # monotone in B * H
        rows = lib.ammc_pred_loss_partial_rows(b, h, 21)
        assert rows > 0 and rows >= last and rows == -(-b * h // _lib.AMMC_PRED_LOSS_ROWS), (b, h)
        last = rows
    text = open(os.path.join(ROOT, "include", "ammc_hip.h")).read()
    assert int(re.search(r"#define AMMC_PRED_LOSS_ROWS (\d+)", text).group(1)) == _lib.AMMC_PRED_LOSS_ROWS
    assert int(re.search(r"#define AMMC_L1_CHUNK (\d+)", text).group(1)) == _lib.AMMC_L1_CHUNK


def test_fused_loss_is_off_by_default():
    env = {k: v for k, v in os.environ.items() if k != "AMMC_FUSED_LOSS"}
    code = "from ammcnet_aaai2021_amd import harness; print(harness.FUSED_LOSS)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stderr[-2000:]
    from ammcnet_aaai2021_amd import run_train
    assert run_train.parse(["--rgb_root", "x", "--op_root", "y", "--out", "z", "--iterations", "1"]).fused_loss is False
    assert run_train.parse(["--stage", "op", "--op_root", "y", "--out", "z", "--iterations", "1", "--fused_loss"]).fused_loss is True


def test_flag_on_changes_nothing_on_cpu_tensors(monkeypatch):
    rgb_x, op_x, rgb_t, op_t = S.make_clips(2, 16, 16, tag="loss-host")
    rgb, op = S.hashed_uniform("lh-rgb", (2, 3, 16, 16)), S.hashed_uniform("lh-op", (2, 2, 16, 16))
    diffs = (torch.tensor([0.25]), torch.tensor([0.5]))
    d_gen, fp, fg = S.hashed_uniform("lh-d", (2, 1, 2, 2)), S.hashed_uniform("lh-fp", (2, 2, 16, 16)), S.hashed_uniform("lh-fg", (2, 2, 16, 16))

    def run():
        a, b = rgb.clone().requires_grad_(True), op.clone().requires_grad_(True)
        out = (a, b, diffs, None)
        v = [Hn.generator_loss(out, rgb_t, op_t), Hn.generator_loss_full(out, rgb_t, op_t, d_gen, fp, fg)]
        ls, ts = Hn.single_stream_loss("rgb", a, rgb_t, diffs[0], d_gen, fp, fg)
        lo, to = Hn.single_stream_loss("op", b, op_t, diffs[1])
        (v[0] + v[1] + ls + lo).backward()
        return v + [ls, lo] + list(ts.values()) + list(to.values()) + [a.grad, b.grad], list(ts) + list(to)
    monkeypatch.setattr(Hn, "FUSED_LOSS", False)
    off, keys_off = run()
    monkeypatch.setattr(Hn, "FUSED_LOSS", True)
    on, keys_on = run()
    assert keys_on == keys_off
    for x, y in zip(on, off):
        assert torch.equal(x, y)
