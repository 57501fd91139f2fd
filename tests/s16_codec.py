"""The S16 encoding restated in numpy (no device, no torch): an fp32 value t is kept as two halves, hi = float16(t) and
lo = float16((t - float32(hi)) * 2048), both rounded to nearest even by numpy's IEEE conversions.  A group of 8 channels
is 32 bytes: the 8 hi halves, then the 8 lo halves (csrc/ammc_common.h `ammc_s16_split8`, the scalar encoders of
csrc/train_kernels.hip).  tests/test_s16_stream_refs_host.py checks the facts the GPU tests lean on:
  * t - hi is exact in fp32 (so the encoders' subtraction cannot round);
  * hi + lo / 2048 is exact in fp32 (so a comparison of decoded values has one answer);
  * |decode - t| <= 2^-22 |t| + 2^-36 for |t| <= 65504."""
import numpy as np

LO = np.float32(2048.0)
HALF_MAX = 65504.0


def encode(t32):
    """(hi_bits, lo_bits), uint16 arrays of t's shape"""
    t = np.ascontiguousarray(np.asarray(t32, dtype=np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        hi = t.astype(np.float16)
        lo = ((t - hi.astype(np.float32)) * LO).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def pack(hi_bits, lo_bits):
    """uint16 [..., c] halves -> the int32 words [..., c] of the S16 buffer (per 8 channels: 4 words of hi, 4 of lo)"""
    hi, lo = np.asarray(hi_bits, dtype=np.uint16), np.asarray(lo_bits, dtype=np.uint16)
    sh = hi.shape
    assert sh[-1] % 8 == 0 and lo.shape == sh
    g = np.stack([hi.reshape(*sh[:-1], sh[-1] // 8, 8), lo.reshape(*sh[:-1], sh[-1] // 8, 8)], axis=-2)
    return np.ascontiguousarray(g).reshape(*sh[:-1], 2 * sh[-1]).view(np.int32)


def unpack(words):
    """the inverse of `pack`: int32 / float32 words [..., c] -> (hi_bits, lo_bits) uint16 [..., c]"""
    w = np.ascontiguousarray(words)
    sh = w.shape
    assert w.dtype.itemsize == 4 and sh[-1] % 8 == 0
    g = w.view(np.uint16).reshape(*sh[:-1], sh[-1] // 8, 2, 8)
    return (np.ascontiguousarray(g[..., 0, :]).reshape(sh), np.ascontiguousarray(g[..., 1, :]).reshape(sh))


def words(t32):
    """the int32 words of the S16 image of an fp32 array whose last dimension is a multiple of 8"""
    return pack(*encode(t32))


def decode(buf, c=None):
    """float64 values of the first c channels of an S16 buffer (4-byte words [..., ctot])"""
    hi, lo = unpack(np.asarray(buf))
    v = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64) / 2048.0
    return v if c is None else v[..., :c]


def pow2_to_1024(bits: int) -> float:
    """the power of two that brings a maximum with fp32 bit pattern `bits` (>= 0) into [1024, 2048): 2^(10 - e) with
    e the unbiased exponent FIELD (an fp32 subnormal has field 0: e = -127), 10 - e clamped to [-60, 60]; an all-zero
    tensor (bits == 0) keeps the factor 1 (`pow2_to_1024` of conv_gemm_s16.hip, `tk_pow2_to_1024` of train_kernels.hip)"""
    bits = int(bits)
    e = ((bits >> 23) & 255) - 127
    if bits == 0:
        e = 10
    fe = max(-60, min(60, 10 - e))
    return float(np.ldexp(1.0, fe))


def f32_bits(v) -> int:
    return int(np.asarray(v, dtype=np.float32).reshape(1).view(np.int32)[0])
