"""Host half of the input-pipeline and clip-bank kernel table (tests/pipeline_cases.py; the device half is
tests/test_gpu_pipeline_kernels.py).  No device: the reference the kernels are held to bit for bit
(oracle/pipeline_oracle.py) against an independent float64 witness on every geometry and pattern of the table, the answers
known by hand, the numpy gather reference against the oracle's loaders, the refusals the entries decide from their
arguments alone, and the ledger of entry points.

Measured on this table (CPU, oracle against witness - never a kernel): the 8-bit path is at most 0.783 grey levels from
the float64 value (`extremes`, 13x17 -> 19x23; the gate is < 1), the float path at most 0.20 of its bound."""
import os
import re

import numpy as np
import pytest

import pipeline_cases as K
from oracle import pipeline_oracle as PO

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ammcnet_aaai2021_amd", "csrc")
REQUIRED = [(1, 1, 4, 4), (1, 9, 4, 12), (7, 1, 8, 4), (5, 7, 1, 1), (8, 8, 8, 8), (16, 24, 8, 12), (32, 32, 8, 8), (8, 12, 16, 24),
            (4, 4, 16, 16), (13, 17, 19, 23), (97, 101, 31, 29), (2, 2, 256, 256), (9, 7, 2, 6), (6, 10, 7, 3), (256, 256, 64, 96),
            (1080, 1920, 64, 96), (1080, 1920, 256, 256),
            (240, 360, 256, 256), (360, 640, 256, 256), (256, 256, 256, 256), (158, 238, 256, 256), (480, 856, 64, 96), (3, 5, 8, 8)]
geoms = pytest.mark.parametrize("g", K.GEOMS, ids=K.geom_id)


def test_the_table_holds_the_geometries_sizes_and_patterns_it_promises():
    assert set(REQUIRED) <= set(K.GEOMS)
    assert all(K.nframes(g) == (1 if g[0] == 1080 else 3) for g in K.GEOMS)
    assert sum(len(K.alignments(g)) == 4 for g in K.GEOMS) >= 3
    assert set(K.FRAME_PATTERNS) == {"rand", "zero", "full", "checker", "extremes", "coords"}
    assert set(K.FLOW_PATTERNS) == {"rand", "ramp", "huge", "zeros"}
    assert [h * w for h, w in K.GATHER_SIZES] == [4, 60, 64, 1056, 4092, 16384, 16512, 17028, 65536]
    hw = {s: s[0] * s[1] for s in K.GATHER_SIZES}
    assert all(v % 4 == 0 for v in hw.values())
    assert hw[(128, 129)] % 16 == 0 and K.TIER_CHUNK < hw[(128, 129)] < 2 * K.TIER_CHUNK          # wide, a partial second chunk
    assert hw[(129, 132)] % 16 == 4 and hw[(129, 132)] - K.TIER_CHUNK < K.TIER_TRIP               # narrow, 4 trips + a partial one
    assert hw[(66, 62)] < K.TIER_TRIP and hw[(66, 62)] % 1024 != 0                                # ends between a lane's loads
    assert 256 * 4 < hw[(32, 33)] < 2 * 256 * 4                                                   # plain gathers: a partial second group
    # the tiered file's banks, rows and splits
    assert (K.N_RGB, K.N_OP, K.RGB_LEN, K.OP_LEN) == (11, 9, 5, 4) and K.SPLITS == [(0, 0), (3, 7), (11, 9), (6, 0)]
    assert list(K.RGB_FIRST) == [0, 1, 2, 3, 4, 5, 6, -1, 6] and list(K.OP_FIRST) == [0, 1, 2, 3, 4, 5, -1, 0, 5]


def test_the_patterns_are_what_the_table_says():
    g = (13, 17, 19, 23)
    m = K.mid(g)
    z, f = K.frames(g, "zero"), K.frames(g, "full")
    assert (z[m] == 0).all() and (np.delete(z, m, 0) == 0xA5).all() and K.source_guard("zero") == 0xA5
    assert (f[m] == 255).all() and (np.delete(f, m, 0) == 0).all() and K.source_guard("full") == 0
    c = K.frames(g, "coords")[0]
    assert c[5, 3].tolist() == [35, 15, 77] and c[12, 16].tolist() == [84, 80, 77]
    ck = K.frames(g, "checker")[0]
    assert ck[0, 0].tolist() == [0, 255, 0] and ck[0, 1].tolist() == [255, 0, 255] and ck[1, 0].tolist() == [255, 0, 255]
    assert set(np.unique(K.frames(g, "extremes"))) == {0, 255}
    r = K.flows(g, "ramp")[0]
    assert r[4, 6].tolist() == [0.0, 2.0]
    assert set(np.unique(K.flows(g, "huge"))) == {-K.HUGE, K.HUGE} and float(K.HUGE) == 1.666666752e9
    zs = K.flows(g, "zeros")[m]
    assert (zs == 0).all() and 0 < np.signbit(zs).sum() < zs.size                                 # both signs of zero
    tiny = np.finfo(np.float32).tiny
    for geo in K.GEOMS[:14]:
        for p in K.FLOW_PATTERNS:
            fl = K.flows(geo, p)
            assert fl.dtype == np.float32 and np.isfinite(fl).all() and not ((fl != 0) & (np.abs(fl) < tiny)).any(), (geo, p)


@geoms
def test_oracle_8bit_path_is_less_than_one_grey_level_from_the_float64_witness(g):
    """tests/test_pipeline_host.py's gate on the oracle, on every geometry and pattern of the table (its "equals the
    rounded exact value for most pixels" holds for random data only and is not applied to the planted patterns)"""
    worst = 0.0
    for p in K.FRAME_PATTERNS:
        for i, f in enumerate(K.frames(g, p)):
            err = float(np.abs(PO.resize_linear_u8(f, g[2], g[3]).astype(np.float64) - K.witness(f, g[2], g[3])).max())
            worst = max(worst, err)
            assert err < 1.0, (p, i, err)
    print(f"8-bit path, {K.geom_id(g)}: worst distance from the witness {worst:.3f} grey levels")


@geoms
def test_oracle_float_path_is_within_its_bound_of_the_float64_witness(g):
    worst = 0.0
    for p in K.FLOW_PATTERNS:
        for i, f in enumerate(K.flows(g, p)):
            err = float(np.abs(PO.resize_linear_f32(f, g[2], g[3]).astype(np.float64) - K.witness(f, g[2], g[3])).max())
            bound = K.float_bound(g) * float(np.abs(f).max())
            assert err <= bound, (p, i, err, bound)
            if bound:
                worst = max(worst, err / bound)
    print(f"float path, {K.geom_id(g)}: worst distance from the witness {worst:.3f} of the bound")


def test_the_witness_itself_on_answers_known_by_hand():
    img = np.arange(12, dtype=np.float64).reshape(3, 4, 1)
    assert np.array_equal(K.witness(img, 3, 4), img)
    assert np.array_equal(K.witness(img, 3, 2)[:, :, 0], img[:, 0::2, 0] + 0.5)                  # 2x down: the mean of two
    up = K.witness(img[:1, :2], 1, 4)[0, :, 0]                                                    # 0 1 -> clamp, 1/4, 3/4, clamp
    assert up.tolist() == [0.0, 0.25, 0.75, 1.0]
    assert np.array_equal(K.witness(img[:1, :1], 5, 3), np.zeros((5, 3, 1)))


def test_answers_known_by_hand_hold_for_the_oracle():
    rng = np.random.default_rng(3)
    for g in ((8, 8, 8, 8), (256, 256, 256, 256)):                                                # identity
        fr = K.frames(g, "rand")
        fl = K.flows(g, "rand")
        assert np.array_equal(K.want_frames_u8(fr, g), fr.transpose(0, 3, 1, 2))
        assert np.array_equal(K.want_frames_f32(fr, g), K.normalize(fr.transpose(0, 3, 1, 2)))
        assert np.array_equal(K.want_flows_f32(fl, g)[:, 0], fl[..., 0] / np.float32(g[2]))
    for g in K.GEOMS:                                                                             # constants stay constants
        for p, v, around in (("zero", 0, 0xA5), ("full", 255, 0)):
            got = K.want_frames_u8(K.frames(g, p), g)
            assert (got[K.mid(g)] == v).all() and (np.delete(got, K.mid(g), 0) == around).all(), (g, p)
    g = (1, 1, 4, 4)                                                                              # a 1 x 1 source
    fr = rng.integers(0, 256, (3, 1, 1, 3), dtype=np.uint8)
    assert np.array_equal(K.want_frames_u8(fr, g), np.broadcast_to(fr.transpose(0, 3, 1, 2), (3, 3, 4, 4)))
    fl = rng.normal(0, 3, (3, 1, 1, 2)).astype(np.float32)
    assert np.array_equal(K.want_flows_f32(fl, g)[:, 0], np.broadcast_to(fl[..., 0] / np.float32(4), (3, 4, 4)))
    for g in ((16, 24, 8, 12), (32, 32, 8, 8)):                                                   # the mean of the middle neighbours
        ramp = K.hramp(g[0], g[1])
        assert np.array_equal(PO.resize_linear_u8(ramp, g[2], g[3]), K.hramp_mean(g))
        assert ((ramp[0, 0::2].astype(int) + ramp[0, 1::2]) % 2 == 1).all()                       # every mean ends in .5
    g = (16, 24, 8, 12)                                                                           # the flows' ramp: exact in float32
    want = (np.arange(12, dtype=np.float32) + np.float32(0.25) - 3) / np.float32(8)
    assert np.array_equal(K.want_flows_f32(K.flows(g, "ramp"), g)[0, 0], np.tile(want, (8, 1)))


def test_hramp_mean_is_the_rounded_half_up_mean():
    assert K.hramp_mean((16, 24, 8, 12))[0, :3, 0].tolist() == [3, 13, 23]                        # (0 + 5 + 1) // 2, (10 + 15 + 1) // 2
    assert K.hramp_mean((32, 32, 8, 8))[0, :2, 1].tolist() == [9, 29]                             # columns 1, 2: (6 + 11 + 1) // 2


def test_the_numpy_gather_reference_equals_the_loaders_and_the_reference_clips():
    g = (12, 16, 8, 8)
    rng = np.random.default_rng(41)
    fr = rng.integers(0, 256, (K.N_RGB, 12, 16, 3), dtype=np.uint8)
    fl = rng.normal(0, 3, (K.N_OP, 12, 16, 2)).astype(np.float32)
    rgb_bank = K.want_frames_u8(fr, g)                                                            # what the rgb bank holds
    op_all = K.want_flows_f32(fl, g)
    op_bank = op_all[:, 0].copy()                                                                 # what the op bank holds
    want_rgb = PO.clips(K.want_frames_f32(fr, g), K.RGB_LEN)
    want_op = PO.clips(op_all, K.OP_LEN)
    got_rgb = K.gather_rgb_ref(rgb_bank, np.arange(len(want_rgb)), K.RGB_LEN)
    got_op = K.gather_op_ref(op_bank, np.arange(len(want_op)), K.OP_LEN)
    assert np.array_equal(got_rgb.view(np.int32), want_rgb.view(np.int32))
    assert np.array_equal(got_op.view(np.int32), want_op.view(np.int32))
    # NaN rows exactly where the clip leaves the bank: -1 and one past the last legal start
    first = np.array([-1, 0, K.N_RGB - K.RGB_LEN, K.N_RGB - K.RGB_LEN + 1], np.int32)
    got = K.gather_rgb_ref(rgb_bank, first, K.RGB_LEN)
    assert np.isnan(got[[0, 3]]).all() and np.isfinite(got[[1, 2]]).all()
    first = np.array([0, K.N_OP - K.OP_LEN, K.N_OP - K.OP_LEN + 1, -5], np.int32)
    got = K.gather_op_ref(op_bank, first, K.OP_LEN)
    assert np.isnan(got[[2, 3]]).all() and np.isfinite(got[[0, 1]]).all()


def test_the_clip_comparison_refuses_what_it_must():
    """`same_clips` is what the device file compares every gather with: one changed bit, one number in a refused row and
    one pixel of a refused row that still holds the pre-fill must each fail - the pre-fill is a NaN itself"""
    import torch
    _, op = K.gather_banks(6, 10)
    first = np.array([0, -1, 5, 6], np.int32)                                                     # 6: one past the last legal start
    want = torch.from_numpy(K.gather_op_ref(op, first, K.OP_LEN).view(np.int32).copy())
    refused = torch.tensor([False, True, False, True])
    assert np.isnan(np.array([K.SENT], np.int32).view(np.float32)[0])                             # the pre-fill is a NaN
    assert K.same_clips(want.clone(), want, refused)
    nan = torch.tensor(float("nan")).view(torch.int32)
    other = want.clone()
    other[1] = nan | 1                                                                            # any NaN but the pre-fill will do
    assert K.same_clips(other, want, refused)
    for b, v in ((0, int(want[0, 0, 0, 0, 0]) ^ 1), (2, K.SENT), (1, 0), (1, K.SENT), (3, K.SENT), (3, 0x3F800000)):
        bad = want.clone()
        bad[b, -1, -1, -1, -1] = v                                                                # the last pixel of the sample
        assert not K.same_clips(bad, want, refused), (b, hex(v))
    untouched = torch.full_like(want, K.SENT)                                                     # a kernel that wrote nothing
    untouched[~refused] = want[~refused]
    assert not K.same_clips(untouched, want, refused)
    assert not K.same_clips(want.view(torch.float32), want, refused)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """every refusal is decided from the arguments, before the runtime is asked: -1 (AMMC_EINVAL) on a machine without a
    device.  Among them the block-count guard of `ammc_frames_u8_to_f32` / `ammc_flows_to_f32` (their clip_bank.hip
    twins had it): n = 2^30, oh = ow = 2^15 over a pointer that is never dereferenced"""
    got = K.refusals()
    assert len(got) >= 60
    wrong = [(what, rc) for what, rc in got if rc != -1]
    assert not wrong, wrong


def _entries(name):
    src = open(os.path.join(CSRC, name)).read()
    return set(re.findall(r'^extern "C" \w+ (ammc_\w+)\(', src, re.M))


def test_every_entry_of_pipeline_and_clip_bank_is_called_by_the_kernel_file():
    entries = _entries("pipeline.hip") | _entries("clip_bank.hip")
    assert {"ammc_frames_u8_to_f32", "ammc_flows_to_f32", "ammc_frames_u8_resize_u8", "ammc_flows_resize_c0", "ammc_gather_clips",
            "ammc_gather_clips_one", "ammc_gather_clips_tiered"} <= entries
    # every `extern "C"` of the two files is one the pattern above sees
    for name in ("pipeline.hip", "clip_bank.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert src.count('extern "C"') == len(_entries(name)), name
    tests = open(os.path.join(HERE, "test_gpu_pipeline_kernels.py")).read()
    named = set(re.findall(r"lib\.(ammc_\w+)\(", tests))
    missing = sorted(entries - named)
    assert not missing, f"entry points of pipeline.hip / clip_bank.hip without a call in test_gpu_pipeline_kernels.py: {missing}"
