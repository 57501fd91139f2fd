"""The two-tier clip bank without a GPU: `pipeline.bank_tiers` (the split of a bank between device and pinned host
memory) and the argument checks of `ammc_gather_clips_tiered`, which are status codes decided before anything touches
a device."""
import pytest

from ammcnet_aaai2021_amd import _lib, pipeline as P

SIZE = (16, 8)                                  # (width, height): 128 pixels, an rgb frame 384 B, a flow 512 B
RGB_B, OP_B = 3 * 128, 4 * 128


def test_everything_fits_the_device():
    assert P.bank_tiers(40, 30, SIZE, 40 * RGB_B + 30 * OP_B, 0) == (40, 30)
    assert P.bank_tiers(40, 30, SIZE, 1e12, 0) == (40, 30)
    assert P.bank_tiers(40, 0, SIZE, 40 * RGB_B, 0) == (40, 0)                   # a one-kind bank


def test_nothing_fits_the_device():
    assert P.bank_tiers(40, 30, SIZE, 0, 1e9) == (0, 0)
    assert P.bank_tiers(40, 30, SIZE, RGB_B - 1, 1e9) == (0, 0)
    assert P.bank_tiers(0, 30, SIZE, OP_B - 1, 1e9) == (0, 0)


@pytest.mark.parametrize("n_rgb,n_op,device_bytes", [(40, 30, 15000), (40, 30, 15360), (1000, 999, 333333), (7, 90, 20001),
                                                      (90, 7, 20001), (40, 30, 30000)])
def test_partial_split_is_the_largest_that_fits_and_keeps_the_fractions(n_rgb, n_op, device_bytes):
    r, o = P.bank_tiers(n_rgb, n_op, SIZE, device_bytes, 1e9)
    assert 0 <= r < n_rgb and 0 <= o < n_op
    used = r * RGB_B + o * OP_B
    assert used <= device_bytes
    assert used + RGB_B > device_bytes and used + OP_B > device_bytes          # one more frame of either kind is too much
    # the same fraction of each kind: rounding the proportional share down loses less than one frame of each kind, so
    # less than 384 + 512 B are left for the top-up, at most two frames: no kind ends 3 frames from its share
    assert abs(r / n_rgb - o / n_op) < 3 / min(n_rgb, n_op)
    assert P.bank_tiers(n_rgb, n_op, SIZE, device_bytes, n_rgb * RGB_B + n_op * OP_B - used) == (r, o)   # host: exactly enough


def test_host_overflow_raises():
    total = 40 * RGB_B + 30 * OP_B
    r, o = P.bank_tiers(40, 30, SIZE, 15000, 1e9)
    rest = total - (r * RGB_B + o * OP_B)
    with pytest.raises(_lib.AmmcHipError, match="host budget"):
        P.bank_tiers(40, 30, SIZE, 15000, rest - 1)
    with pytest.raises(_lib.AmmcHipError, match="host budget"):
        P.bank_tiers(40, 30, SIZE, 0, 0)


def _call(**kw):
    """`ammc_gather_clips_tiered` on fake, aligned, never dereferenced addresses: every case below is refused by a check
    that needs no device"""
    a = dict(rgb_dev=0x100000, rgb_host=0x200000, n_rgb_dev=3, n_rgb=11, op_dev=0x300000, op_host=0x400000, n_op_dev=7,
             n_op=9, rgb_first=0x500000, op_first=0x600000, batch=2, rgb_len=5, op_len=4, h=8, w=8, rgb_out=0x700000,
             op_out=0x800000)
    a.update(kw)
    return _lib.load().ammc_gather_clips_tiered(a["rgb_dev"], a["rgb_host"], a["n_rgb_dev"], a["n_rgb"], a["op_dev"],
                                                a["op_host"], a["n_op_dev"], a["n_op"], a["rgb_first"], a["op_first"],
                                                a["batch"], a["rgb_len"], a["op_len"], a["h"], a["w"], a["rgb_out"],
                                                a["op_out"], None)


@pytest.mark.parametrize("bad", [
    dict(rgb_dev=None), dict(rgb_host=None), dict(op_dev=None), dict(op_host=None),      # NULL base of a non-empty tier
    dict(n_rgb_dev=12), dict(n_op_dev=10), dict(n_rgb_dev=-1),                            # n_dev outside [0, n]
    dict(h=3, w=5), dict(h=6, w=7),                                                       # h * w % 4 != 0
    dict(rgb_out=0x700004), dict(op_out=0x800008), dict(rgb_out=None),                    # outputs: 16-byte aligned
    dict(rgb_first=None, op_first=None),                                                  # nothing to gather
    dict(rgb_host=0x200004), dict(op_dev=0x300004), dict(rgb_dev=0x100001),               # bank alignment
    dict(batch=0), dict(batch=3450), dict(rgb_len=12), dict(op_len=0),                    # 3450 * 19 planes > 65535
])
def test_bad_arguments_are_status_codes_without_a_gpu(bad):
    assert _call(**bad) == -1                                                             # AMMC_EINVAL

