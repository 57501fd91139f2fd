"""What tests/test_gpu_s16_stream_kernels.py leans on, checked without a device: the facts of the S16 encoding
(tests/s16_codec.py), that the grid inputs make every reference exactly representable in fp32 (the licence for bit
equality), the new references against torch's own float64 operators, the host restatement of `pow2_to_1024`, and that
every `ammc_*` entry of csrc/train_kernels.hip is named by a GPU test of the stream kernels."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import synthetic as S

import s16_codec as Q
import s16_stream_cases as C
import stream_cases as K
import stream_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _codec_facts(t):
    """the three facts on an fp32 array with |t| <= 65504; returns the worst |decode - t| / (2^-22 |t| + 2^-36)"""
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    t = np.concatenate([t, np.zeros(-t.size % 8, dtype=np.float32)])
    hi_b, lo_b = Q.encode(t)
    hi, lo = hi_b.view(np.float16).astype(np.float64), lo_b.view(np.float16).astype(np.float64)
    t64 = t.astype(np.float64)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    diff32 = t - hi_b.view(np.float16).astype(np.float32)
    assert np.array_equal(diff32.astype(np.float64), t64 - hi), "t - hi rounds in fp32"
    dec = hi + lo / 2048.0
    assert np.array_equal(dec.astype(np.float32).astype(np.float64), dec), "hi + lo / 2048 does not fit fp32"
    assert np.array_equal(Q.decode(Q.pack(hi_b, lo_b)), dec)
    ratio = np.abs(dec - t64) / (2.0 ** -22 * np.abs(t64) + 2.0 ** -36)
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    return float(ratio.max())


def test_codec_facts_over_two_million_hashed_values():
    t = C.codec_values("codec", 2_000_000)
    assert float(np.abs(t).min()) < 1e-16 and float(np.abs(t).max()) > 60000.0
    worst = _codec_facts(t)
    assert worst > 0.9                                   # the bound is tight: nothing to give away
    # the edges: zeros of both signs, the largest half, the smallest normal and subnormal halves and their neighbours
    edge = np.array([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 * (1 - 2.0 ** -11),
                     1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)
    _codec_facts(edge)
    hi, lo = Q.encode(np.array([-0.0, 0.0], dtype=np.float32))
    assert hi.tolist() == [0x8000, 0] and lo.tolist() == [0, 0]


def test_pack_and_unpack_are_the_group_layout():
    t = C.codec_values("pk", 64).reshape(2, 2, 16)
    hi, lo = Q.encode(t)
    w = Q.pack(hi, lo)
    assert w.shape == t.shape and w.dtype == np.int32
    halves = w.view(np.uint16).reshape(2, 2, 32)
    assert np.array_equal(halves[..., 0:8], hi[..., 0:8]) and np.array_equal(halves[..., 8:16], lo[..., 0:8])
    assert np.array_equal(halves[..., 16:24], hi[..., 8:16]) and np.array_equal(halves[..., 24:32], lo[..., 8:16])
    h2, l2 = Q.unpack(w)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)


def test_grid_apply_has_no_lo_half():
    """on the 1/8 grid x scale + shift is a multiple of 1/64 of magnitude at most 2: hi is exact, lo == 0"""
    for shape in C.SHAPES:
        x, scale, shift, res = C.ssa_case("grid", shape)
        y = R.scale_shift_act(x, scale, shift, None, 0)
        assert R.fits_f32(y)
        hi, lo = Q.encode(y.float().numpy())
        assert not lo.any() or not (lo & 0x7FFF).any()
        assert np.array_equal(hi.view(np.float16).astype(np.float64), y.numpy())


@pytest.mark.parametrize("shape", C.SHAPES)
def test_codec_facts_on_the_cont_inputs(shape):
    x, scale, shift, res = C.ssa_case("cont", shape)
    for relu in (0, 1):
        _codec_facts(R.scale_shift_act(x, scale, shift, res, relu).float().numpy())
    x, dy, mean, invstd, scale, shift = K.bn_bwd_case("cont", shape, 1)
    sg, sgx = K.bn_apply_sums("cont", shape)
    dc = R.bn_bwd_apply(x, dy, mean, invstd, scale, shift, sg, sgx, 1).float().numpy()
    amax = float(np.abs(dc).max())
    _codec_facts(dc * np.float32(Q.pow2_to_1024(Q.f32_bits(amax))))


@pytest.mark.parametrize("shape", C.SHAPES + C.POOL_SHAPES)
def test_grid_references_fit_fp32(shape):
    b, h, w, c = shape
    x, scale, shift, res = C.ssa_case("grid", shape)
    for relu in (0, 1):
        assert R.fits_f32(R.scale_shift_act(x, scale, shift, res, relu))
        assert R.fits_f32(R.scale_shift_act(x, scale, shift, None, relu))
    if h % 2 == 0 and w % 2 == 0:
        xp, sp, hp = C.pool_case("grid", shape)
        assert R.fits_f32(R.scale_shift_act(xp, sp, hp, None, 1))
    if h >= 2 and w >= 2:
        add, dpo, idx = C.unpool_case("grid", shape)
        assert R.fits_f32(C.unpool_grad(add, dpo, idx))
    if K.is_pow2(b * h * w):
        for relu in (0, 1):
            xx, dy, mean, invstd, scale, shift = K.bn_bwd_case("grid", shape, relu)
            sg, sgx = K.bn_apply_sums("grid", shape)
            assert R.fits_f32(R.bn_bwd_apply(xx, dy, mean, invstd, scale, shift, sg, sgx, relu))
            if h >= 2 and w >= 2:
                assert R.fits_f32(R.bn_bwd_apply(xx, C.unpool_grad(add, dpo, idx), mean, invstd, scale, shift, sg, sgx, relu))


@pytest.mark.parametrize("shape", K.CHAN_SHAPES)
def test_grid_reduction_references_fit_fp32(shape):
    b, h, w, c = shape
    for relu in (0, 1):
        x, dy, mean, invstd, scale, shift = K.bn_bwd_case("grid", shape, relu)
        sg, sgx = R.bn_bwd_sums(x, dy, mean, invstd, scale, shift, relu)
        assert R.fits_f32(sg) and R.fits_f32(sgx)
        assert R.fits_f32((R.d(x) - R.d(mean)) * R.d(invstd))
        if c % 8 == 0 and h >= 2 and w >= 2:
            add, dpo, idx = C.unpool_case("grid", shape)
            g = C.unpool_grad(add, dpo, idx)
            sg, sgx = R.bn_bwd_sums(x, g, mean, invstd, scale, shift, relu)
            assert R.fits_f32(g) and R.fits_f32(sg) and R.fits_f32(sgx)
    assert R.fits_f32(R.chan_sums(K.values("grid", f"csa-grid-{shape}", shape))[0])


def test_unpool_gradient_against_autograd_of_batchnorm_relu_maxpool():
    """BatchNorm (training) + ReLU + max_pool2d in float64 through autograd, positions forced through a tie-free input: the
    gradient that reaches the convolution output = `R.bn_bwd_apply` on add + `R.unpool2x2`(dpo by those positions)"""
    b, h, w, c = 2, 7, 9, 8
    x = S.hashed_normal("hup-x", (b, h, w, c)).double() + 0.4            # distinct values: no ties
    gamma, beta = S.hashed_uniform("hup-g", (c,), 0.5, 1.5).double(), S.hashed_normal("hup-b", (c,), 0.3).double()
    add, dpo = S.hashed_normal("hup-a", (b, h, w, c)).double(), S.hashed_normal("hup-p", (b, h // 2, w // 2, c)).double()
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.relu(F.batch_norm(xt, None, None, gamma, beta, True, 0.1, 1e-5))
    pooled, where = F.max_pool2d(y, 2, return_indices=True)
    (pooled * dpo.permute(0, 3, 1, 2)).sum().backward(retain_graph=True)
    g_pool = xt.grad.clone()
    xt.grad = None
    (y * add.permute(0, 3, 1, 2)).sum().backward()
    want = (g_pool + xt.grad).permute(0, 2, 3, 1)
    s, ss = R.chan_sums(x)
    fin = R.bn_finalize(s, ss, b * h * w, gamma, beta, 1e-5, 0.1, torch.zeros(c), torch.ones(c))
    yy = y.detach().permute(0, 2, 3, 1)
    arg = R.maxpool2x2_arg(yy)
    # torch's flat index into the h x w plane -> the window position
    wy, wx = (where // w).permute(0, 2, 3, 1), (where % w).permute(0, 2, 3, 1)
    win = R._windows(yy)
    tied = (win == win.max(3, keepdim=True).values).sum(3) > 1          # (ReLU makes ties at 0: either position serves)
    assert bool(((wy % 2) * 2 + wx % 2 == arg)[~tied].all())
    assert 0 < int(tied.sum()) < tied.numel() // 2
    g = add + R.unpool2x2(dpo, arg, h, w)
    sg, sgx = R.bn_bwd_sums(x, g, fin["mean"], fin["invstd"], fin["scale"], fin["shift"], 1)
    got = R.bn_bwd_apply(x, g, fin["mean"], fin["invstd"], fin["scale"], fin["shift"], sg, sgx, 1)
    assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max())
    assert float(R.unpool2x2(dpo, arg, h, w)[:, -1].abs().max()) == 0.0 and float(R.unpool2x2(dpo, arg, h, w)[:, :, -1].abs().max()) == 0.0


@pytest.mark.parametrize("fh,fw", K.POOL_BWD_SIZES)
def test_positions_against_max_pool2d_indices(fh, fw):
    b, c = 2, 8
    x, dp, add = K.pool_bwd_case("cont", b, fh, fw, c)
    dec = torch.from_numpy(Q.decode(Q.words(x.numpy())))
    _, where = F.max_pool2d(dec.permute(0, 3, 1, 2), 2, return_indices=True)
    pos = ((where // fw) % 2 * 2 + (where % fw) % 2).permute(0, 2, 3, 1)
    assert torch.equal(pos, R.maxpool2x2_arg(dec))
    assert torch.equal(R.unpool2x2(dp, R.maxpool2x2_arg(dec), fh, fw), R.maxpool2x2_bwd(dec, dp))
    # the planted pairs of the grid case: the first of the two positions
    xg, _, _ = K.pool_bwd_case("grid", b, fh, fw, c)
    arg = R.maxpool2x2_arg(torch.from_numpy(Q.decode(Q.words(xg.numpy()))))[..., 0].reshape(-1)
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    assert arg.tolist() == [pairs[n % 6][0] for n in range(arg.numel())]


def test_pow2_to_1024_over_every_exponent_field():
    for field in range(0, 255):
        for mant in (0, 1, 0x7FFFFF):
            bits = (field << 23) | mant
            f = Q.pow2_to_1024(bits)
            if bits == 0:
                assert f == 1.0
                continue
            fe = 10 - (field - 127)
            assert f == 2.0 ** max(-60, min(60, fe))
            amax = float(np.array([bits], dtype=np.int32).view(np.float32)[0])
            if -60 <= fe <= 60 and field > 0:
                assert 1024.0 <= amax * f < 2048.0, (field, mant)
            elif fe > 60:
                assert amax * f < 1024.0                       # the clamp: small gradients stay small, never overflow
            assert float(np.float32(f)) == f and float(np.float32(1.0) / np.float32(f)) * f == 1.0
    assert Q.pow2_to_1024(Q.f32_bits(1.0)) == 1024.0
    assert Q.pow2_to_1024(Q.f32_bits(np.nextafter(np.float32(1), np.float32(0)))) == 2048.0
    assert Q.pow2_to_1024(Q.f32_bits(2.0 ** -140)) == 2.0 ** 60


NON_LAUNCHING = {"ammc_chan_reduce_blocks", "ammc_scale_shift_act_s16_pool_supported", "ammc_bn_bwd_unpool_supported",
                 "ammc_pack_filters_item_bytes"}
# the filter re-layouts of train_kernels.hip: no stream kernels - their isolated tests are the convolution tables they pack
# for (tests/conv_gemm_cases.py) and the pack + split test of tests/test_gpu_round4_kernels.py
TESTED_ELSEWHERE = {"ammc_pack_conv_dgrad_weight_f32": "conv_gemm_cases.py", "ammc_pack_filters_s16": "test_gpu_round4_kernels.py",
                    "ammc_pack_conv4_dgrad_weight_f32": "conv_gemm_cases.py", "ammc_transpose_pad_f32": "conv_gemm_cases.py"}


def test_every_entry_of_train_kernels_is_named_by_a_stream_test():
    src = open(os.path.join(HERE, "..", "ammcnet_aaai2021_amd", "csrc", "train_kernels.hip")).read()
    block = src[src.index('extern "C" {'):src.rindex('}  // extern "C"')]
    entries = set(re.findall(r"^int (ammc_\w+)\(", block, re.M))
    assert len(entries) >= 33 and "ammc_bn_bwd_apply_s16_unpool_f32" in entries
    tests = open(os.path.join(HERE, "test_gpu_stream_kernels.py")).read() + open(os.path.join(HERE, "test_gpu_s16_stream_kernels.py")).read()
    named = set(re.findall(r"lib\.(ammc_\w+)\(", tests))
    missing = sorted(e for e in entries if e not in named and e not in NON_LAUNCHING and e not in TESTED_ELSEWHERE)
    assert not missing, f"entry points of train_kernels.hip without an isolated stream test: {missing}"
    for e, f in TESTED_ELSEWHERE.items():
        assert e in entries and f"lib.{e}(" in open(os.path.join(HERE, f)).read(), (e, f)
    for e in NON_LAUNCHING:
        assert e in entries
    # the entry points of the other files that this table covers
    for e in ("ammc_absmax_bits_f32", "ammc_split_rows_scaled_f32", "ammc_split_rows_f32", "ammc_split_rows_guarded_f32",
              "ammc_nchw_to_s16_f32", "ammc_s16_to_nchw_f32", "ammc_maxpool2x2_s16", "ammc_maxpool2x2_s16_idx", "ammc_lrelu_s16",
              "ammc_zero_halo_f32"):
        assert e in named, e
