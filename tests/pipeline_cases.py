"""Cases of the input-pipeline and clip-bank kernels - csrc/pipeline.hip (`ammc_frames_u8_to_f32`, `ammc_flows_to_f32`),
csrc/clip_bank.hip (`ammc_frames_u8_resize_u8`, `ammc_flows_resize_c0`, `ammc_gather_clips`, `ammc_gather_clips_one`,
`ammc_gather_clips_tiered`) and the arithmetic they share (csrc/resize_common.h) - shared by
tests/test_pipeline_cases_host.py (the oracle against a float64 witness, answers known by hand, the gather reference,
refusals: no device) and tests/test_gpu_pipeline_kernels.py (the kernels against the oracle, bit for bit).  A helper
module like tests/wgrad_cases.py, not a test.

A resize case is a geometry (h, w, oh, ow) of GEOMS, a data pattern and an alignment variant.  The sources are n frames
(three; one at 1080p) inside a flat byte buffer with GUARD bytes of 0xA5 before and behind them; the destinations lie
inside buffers filled with the bit pattern SENT (floats) or 0xA5 (bytes).  The patterns make an error visible that random
data hides: on `zero` only the middle frame is zero and everything around it 0xA5, on `full` the middle frame is 255
inside zeros, `coords` changes under a transposed tap, a shifted coordinate or a channel swap, the flows' `zeros` carry
both signs of zero (a zero-weight tap of the other sign turns -0 into +0).

A gather case is a plane size of GATHER_SIZES over the banks, index rows and tier splits of
tests/test_gpu_clip_bank_tiered.py; the expected clips are restated here in numpy (`gather_rgb_ref`, `gather_op_ref`),
not taken from a kernel.

`witness` is the published half-pixel bilinear definition in float64, written out here; it does not call the oracle."""
import numpy as np

from oracle import pipeline_oracle as PO

SENT = 0x7FC07FC0          # as wgrad_cases.SENT: a NaN as a float
GUARD = 4096               # bytes of guard before and behind every source and every resize destination
GUARD_OUT = 16384          # bytes before and behind a gather output: more than a whole `base` trip of the tiered kernel
BYTE = 0xA5

# (h, w, oh, ow).  First the geometries nothing ran before, then the six of tests/test_gpu_pipeline.py
GEOMS = [
    (1, 1, 4, 4), (1, 9, 4, 12), (7, 1, 8, 4),             # a source of height / width 1: every pixel clamps
    (5, 7, 1, 1),                                          # a single output pixel
    (8, 8, 8, 8),                                          # identity
    (16, 24, 8, 12), (32, 32, 8, 8),                       # exact 2x / 4x down: fraction 0.5
    (8, 12, 16, 24), (4, 4, 16, 16),                       # exact 2x / 4x up: fractions 0.25, 0.75 / 0.125 ... 0.875
    (13, 17, 19, 23), (97, 101, 31, 29),                   # odd, coprime sizes, up and down
    (2, 2, 256, 256),                                      # extreme upscale: a quarter of the pixels clamp at each border
    (9, 7, 2, 6), (6, 10, 7, 3),                           # up along one axis, down along the other
    (256, 256, 64, 96),
    (1080, 1920, 64, 96), (1080, 1920, 256, 256),          # a source wider than 856; 6 MB a frame
    (240, 360, 256, 256), (360, 640, 256, 256), (256, 256, 256, 256), (158, 238, 256, 256), (480, 856, 64, 96), (3, 5, 8, 8),
]
assert len(set(GEOMS)) == len(GEOMS)
FRAME_PATTERNS = ("rand", "zero", "full", "checker", "extremes", "coords")
FLOW_PATTERNS = ("rand", "ramp", "huge", "zeros")
HUGE = np.float32(1.666666752e9)                           # Middlebury's "unknown flow"
# alignment variants: (is the source moved off its 16-byte boundary, is the destination).  Moved means: a uint8 buffer
# (a frame source, `ammc_frames_u8_resize_u8`'s destination) to an odd address, a float buffer 4 bytes off the boundary
ALIGNMENTS = {"aligned": (0, 0), "src-off": (1, 0), "dst-off": (0, 1), "both-off": (1, 1)}


def geom_id(g):
    return "%dx%d-to-%dx%d" % g


def nframes(g):
    return 1 if g[0] >= 1080 else 3


def mid(g):
    """the frame under test of the one-frame patterns (`zero`, `full`, the flows' `zeros`)"""
    return nframes(g) // 2


def alignments(g):
    """the variants a geometry runs: all of them, but the aligned one alone at 1080p (6 MB uploads)"""
    return list(ALIGNMENTS) if g[0] < 1080 else ["aligned"]


def _rng(g, pattern):
    return np.random.default_rng([g[0], g[1], g[2], g[3], sum(map(ord, pattern))])


def source_guard(pattern):
    """the byte around a source: 0xA5, zero around `full`"""
    return 0x00 if pattern == "full" else BYTE


def frames(g, pattern):
    """uint8 [n][h][w][3] (RGB)"""
    h, w = g[:2]
    n = nframes(g)
    rng = _rng(g, pattern)
    if pattern == "rand":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if pattern in ("zero", "full"):
        out = np.full((n, h, w, 3), source_guard(pattern), np.uint8)
        out[mid(g)] = 0 if pattern == "zero" else 255
        return out
    if pattern == "extremes":
        return (rng.integers(0, 2, (n, h, w, 3)) * 255).astype(np.uint8)
    k = np.arange(n)[:, None, None]
    row, col = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    out = np.empty((n, h, w, 3), np.uint8)
    if pattern == "checker":                               # one-pixel squares, green inverted
        on = ((row + col + k) & 1) * 255
        out[..., 0], out[..., 1], out[..., 2] = on, 255 - on, on
        return out
    assert pattern == "coords", pattern                    # frame 0: R = 7 row, G = 5 col, B = 77
    out[..., 0] = (7 * row + 11 * k) % 256
    out[..., 1] = (5 * col + 13 * k) % 256
    out[..., 2] = 77 + k
    return out


def flows(g, pattern):
    """float32 [n][h][w][2]: finite, no denormals"""
    h, w = g[:2]
    n = nframes(g)
    rng = _rng(g, pattern)
    rand = rng.normal(0, 3, (n, h, w, 2)).astype(np.float32)
    if pattern == "rand":
        return rand
    if pattern == "ramp":
        out = np.empty((n, h, w, 2), np.float32)
        out[..., 0] = 0.5 * np.arange(w)[None, None, :] - 3 + np.arange(n)[:, None, None]
        out[..., 1] = 0.25 * np.arange(h)[None, :, None] + 1
        return out
    sign = np.where(rng.integers(0, 2, (n, h, w, 2)) == 1, np.float32(-1), np.float32(1))
    if pattern == "huge":
        return (sign * HUGE).astype(np.float32)
    assert pattern == "zeros", pattern                     # the middle frame: +0 / -0 at random; its neighbours random
    rand[mid(g)] = sign[mid(g)] * np.float32(0)
    return rand


def hramp(h, w):
    """a horizontal ramp whose neighbours have an odd sum (their mean ends in .5): uint8 [h][w][3]"""
    assert 5 * (w - 1) + 2 < 256
    return np.tile((5 * np.arange(w)[None, :, None] + np.arange(3)[None, None, :]).astype(np.uint8), (h, 1, 1))


def hramp_mean(g):
    """what an exact 2x | 4x downscale of `hramp` must give: the mean of the two middle neighbours, .5 rounding up;
    uint8 [oh][ow][3]"""
    h, w, oh, ow = g
    k = w // ow
    assert w == k * ow and h == k * oh and k in (2, 4)
    src = hramp(h, w).astype(np.int32)
    left = src[0, k // 2 - 1::k]                             # columns k d + k / 2 - 1 and the next one
    right = src[0, k // 2::k]
    return np.tile(((left + right + 1) // 2).astype(np.uint8)[None], (oh, 1, 1))


# ---- references -----------------------------------------------------------------------------------------------------
def normalize(v_u8):
    """ToTensor + Normalize(0.5, 0.5) of 8-bit values, in float32"""
    return ((v_u8.astype(np.float32) / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)


def want_frames_u8(fr, g):
    """the oracle's 8-bit resize, planar: uint8 [n][3][oh][ow]"""
    return np.stack([PO.resize_linear_u8(f, g[2], g[3]).transpose(2, 0, 1) for f in fr])


def want_frames_f32(fr, g):
    return np.stack([PO.load_frame(f, (g[3], g[2])) for f in fr])


def want_flows_f32(fl, g):
    return np.stack([PO.load_op(f.copy(), (g[3], g[2])) for f in fl])


def witness(img, oh, ow):
    """bilinear resize by the published half-pixel definition, everything in float64: [h][w][c] -> [oh][ow][c].
    src = (d + 0.5) scale - 0.5, clamped at both borders, two taps per axis"""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]

    def taps(src, dst):
        x = (np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5
        s = np.floor(x)
        f = x - s
        lo, hi = s < 0, s >= src - 1
        s[lo], f[lo] = 0, 0.0
        s[hi], f[hi] = src - 1, 0.0
        s = s.astype(np.int64)
        return s, np.minimum(s + 1, src - 1), f
    y0, y1, fy = taps(h, oh)
    x0, x1, fx = taps(w, ow)
    rows = img[y0] * (1.0 - fy)[:, None, None] + img[y1] * fy[:, None, None]
    return rows[:, x0] * (1.0 - fx)[None, :, None] + rows[:, x1] * fx[None, :, None]


def float_bound(g):
    """of max|f|: tests/test_pipeline_host.py's bound on the float path (the oracle keeps the coordinate in float32)"""
    return max(2e-6, 8 * max(g[0], g[1]) * 2.0 ** -24)


# ---- gathers ----------------------------------------------------------------------------------------------------------
N_RGB, N_OP, RGB_LEN, OP_LEN = 11, 9, 5, 4                 # as tests/test_gpu_clip_bank_tiered.py
SPLITS = [(0, 0), (3, 7), (11, 9), (6, 0)]                 # (rgb, op) frames in the device tier
RGB_FIRST = np.array([0, 1, 2, 3, 4, 5, 6, -1, 6], np.int32)
OP_FIRST = np.array([0, 1, 2, 3, 4, 5, -1, 0, 5], np.int32)
PINNED_OFFSETS = (0, 64)                                   # bytes of the host tier into its pinned allocation
TIER_CHUNK, TIER_TRIP = 16384, 4096                        # pixels: clip_bank.hip's TIER_CHUNK, one trip of its `base` loops
GATHER_SIZES = [
    (2, 2),                                                # 4: the smallest legal plane
    (6, 10),                                               # 60: the narrow path
    (8, 8),                                                # 64: the wide path
    (32, 33),                                              # 1056: plain gathers - a second workgroup with 8 of 256 lanes in range
    (66, 62),                                              # 4092: one `base` trip that ends between a lane's loads
    (128, 128),                                            # 16384: exactly one tier chunk
    (128, 129),                                            # 16512, % 16 == 0: the wide host path on a partial second chunk
    (129, 132),                                            # 17028, % 16 == 4: narrow, four full trips and a partial chunk
    (256, 256),                                            # 65536: the production plane
]


def gather_banks(h, w):
    """rgb uint8 [N_RGB][3][h][w], op float32 [N_OP][h][w].  The last pixel of every op plane is +-HUGE, the first -0:
    the ends of a plane are where the tails of the kernels work"""
    rng = np.random.default_rng([h, w, 17])
    rgb = rng.integers(0, 256, (N_RGB, 3, h, w), dtype=np.uint8)
    op = rng.normal(0, 3, (N_OP, h, w)).astype(np.float32)
    op[:, 0, 0] = np.float32(-0.0)
    op[:, -1, -1] = HUGE * np.where(np.arange(N_OP) % 2 == 1, np.float32(-1), np.float32(1))
    return rgb, op


def _rows(first, length, n):
    first = np.asarray(first, np.int64)
    return first, (first >= 0) & (first + length <= n)


def gather_rgb_ref(bank, first, length):
    """float32 [B][length][3][h][w]: normalised frames first .. first + length - 1; NaN rows where the clip leaves the bank"""
    first, ok = _rows(first, length, bank.shape[0])
    out = np.full((len(first), length) + bank.shape[1:], np.nan, np.float32)
    for b in np.flatnonzero(ok):
        for t in range(length):
            out[b, t] = ((bank[first[b] + t].astype(np.float32) / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)
    return out


def gather_op_ref(bank, first, length):
    """float32 [B][length][2][h][w]: (c0, c0 / w) in float32; NaN rows where the clip leaves the bank"""
    first, ok = _rows(first, length, bank.shape[0])
    h, w = bank.shape[1:]
    out = np.full((len(first), length, 2, h, w), np.nan, np.float32)
    for b in np.flatnonzero(ok):
        c0 = bank[first[b]:first[b] + length]
        out[b, :, 0] = c0
        out[b, :, 1] = c0 / np.float32(w)
    return out


def same_clips(got, want, refused) -> bool:
    """The one comparison of gathered clips, of both test files.  `got`, `want`: int32 bit patterns, torch tensors on any
    device with the sample first; `refused`: bool per sample.  A sample the reference has is equal bit for bit; a refused
    one is NaN in every pixel AND none of its pixels still holds SENT - the outputs are pre-filled with SENT, which is a
    NaN itself, so NaN-ness alone would accept a row the kernel never wrote"""
    import torch
    if got.numel() != want.numel() or got.dtype != torch.int32 or want.dtype != torch.int32:
        return False
    got, want = got.reshape(len(refused), -1), want.reshape(len(refused), -1)
    rows = got[refused]
    return (bool(torch.equal(got[~refused], want[~refused])) and bool(torch.isnan(rows.view(torch.float32)).all())
            and not bool((rows == SENT).any()))


# ---- refusals: decided from the arguments alone, nothing launched, no device --------------------------------------------
A = 0x100000                                               # aligned, never dereferenced


def refusals():
    """[(what, status the entry returned)]: every one must be -1 (AMMC_EINVAL).  Only calls the argument checks refuse are
    made: one that passed them would launch a kernel on addresses that do not exist"""
    from ammcnet_aaai2021_amd import _lib
    lib = _lib.load()
    out = []
    big = (A, 1 << 30, 8, 8, A, 1 << 15, 1 << 15)            # 2^60 output pixels: more blocks than a grid has
    out.append(("frames_u8_to_f32: block count beyond 2^31", lib.ammc_frames_u8_to_f32(*big, 0, None)))
    out.append(("flows_to_f32: block count beyond 2^31", lib.ammc_flows_to_f32(*big, None)))
    out.append(("frames_u8_resize_u8: block count beyond 2^31", lib.ammc_frames_u8_resize_u8(*big, 0, None)))
    out.append(("flows_resize_c0: block count beyond 2^31", lib.ammc_flows_resize_c0(*big, None)))
    for what, args in (("null src", (None, 1, 8, 8, A, 4, 4)), ("null dst", (A, 1, 8, 8, None, 4, 4)), ("n 0", (A, 0, 8, 8, A, 4, 4)),
                       ("h 0", (A, 1, 0, 8, A, 4, 4)), ("w < 0", (A, 1, 8, -8, A, 4, 4)), ("oh 0", (A, 1, 8, 8, A, 0, 4)),
                       ("ow 0", (A, 1, 8, 8, A, 4, 0))):
        out.append((f"frames_u8_to_f32: {what}", lib.ammc_frames_u8_to_f32(*args, 0, None)))
        out.append((f"flows_to_f32: {what}", lib.ammc_flows_to_f32(*args, None)))

    # ammc_gather_clips_one(bank, n, kind, first, batch, len, h, w, out, stream)
    names = ["bank", "n", "kind", "first", "batch", "len", "h", "w", "out", "s"]
    ok = [A, 100, 0, A, 9, 5, 8, 8, A, None]
    for what, kw in (("kind 2", dict(kind=2)), ("kind -1", dict(kind=-1)), ("h w % 4", dict(h=3, w=5)), ("h w % 4, op", dict(kind=1, h=3, w=5)),
                     ("rgb bank off 4 bytes", dict(bank=A + 2)), ("op bank off 16 bytes", dict(kind=1, bank=A + 4)),
                     ("out off 16 bytes", dict(out=A + 8)), ("n < len", dict(n=4)), ("n < len, op", dict(kind=1, n=4)),
                     ("rgb: more than 65535 planes", dict(batch=5000)),          # 5000 x 15
                     ("op: more than 65535 planes", dict(kind=1, batch=20000)),  # 20000 x 5
                     ("null bank", dict(bank=None)), ("null first", dict(first=None)), ("null out", dict(out=None)),
                     ("batch 0", dict(batch=0)), ("len 0", dict(len=0)), ("w 0", dict(w=0))):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        out.append((f"gather_clips_one: {what}", lib.ammc_gather_clips_one(*a)))

    # ammc_gather_clips_tiered(rgb_dev, rgb_host, n_rgb_dev, n_rgb, op_dev, op_host, n_op_dev, n_op, rgb_first, op_first,
    #                          batch, rgb_len, op_len, h, w, rgb_out, op_out, stream)
    names = ["rgb_dev", "rgb_host", "n_rgb_dev", "n_rgb", "op_dev", "op_host", "n_op_dev", "n_op", "rf", "of", "batch", "rl", "ol",
             "h", "w", "ro", "oo", "s"]
    # The baseline is all-device (n_dev == n, host tiers NULL): it never asks the runtime about a host pointer, so a case
    # whose argument check were missing would come back with the runtime's launch error (a positive code), not with -1.
    # Only the cases that need a host tier leave that baseline, and they are refused for the NULL or the misalignment
    ok = [A, None, 11, 11, A, None, 9, 9, A, A, 9, 5, 4, 8, 8, A, A, None]
    for what, kw in (("both first NULL", dict(rf=None, of=None)),
                     ("n_rgb_dev > n_rgb", dict(n_rgb_dev=12)), ("n_op_dev > n_op", dict(n_op_dev=10)),
                     ("n_rgb_dev < 0", dict(n_rgb_dev=-1)), ("n_op_dev < 0", dict(n_op_dev=-1)),
                     ("rgb host tier needed but NULL", dict(n_rgb_dev=6)), ("op host tier needed but NULL", dict(n_op_dev=5)),
                     ("rgb device tier needed but NULL", dict(rgb_dev=None)), ("op device tier needed but NULL", dict(op_dev=None)),
                     ("rgb device tier off 4 bytes", dict(rgb_dev=A + 2)), ("op device tier off 16 bytes", dict(op_dev=A + 4)),
                     ("rgb host tier off 16 bytes", dict(n_rgb_dev=6, rgb_host=A + 4)),
                     ("op host tier off 16 bytes", dict(n_op_dev=5, op_host=A + 8)),
                     ("rgb_out off 16 bytes", dict(ro=A + 4)), ("op_out off 16 bytes", dict(oo=A + 8)),
                     ("rgb_out NULL", dict(ro=None)), ("op_out NULL", dict(oo=None)),
                     ("h w % 4", dict(h=3, w=5)), ("n_rgb < rgb_len", dict(n_rgb_dev=4, n_rgb=4)), ("n_op < op_len", dict(n_op_dev=3, n_op=3)),
                     ("rgb_len 0", dict(rl=0)), ("op_len 0", dict(ol=0)), ("batch 0", dict(batch=0)), ("h 0", dict(h=0)),
                     ("more than 65535 planes", dict(batch=4000)),              # 4000 x 19
                     # the single-kind forms: the other kind's arguments are not read, this kind's are
                     ("rgb only: n_rgb_dev > n_rgb", dict(of=None, n_rgb_dev=12)), ("op only: op_out off 16 bytes", dict(rf=None, oo=A + 4)),
                     ("rgb only: host tier needed but NULL", dict(of=None, n_rgb_dev=6)),
                     ("op only: host tier needed but NULL", dict(rf=None, n_op_dev=5))):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        out.append((f"gather_clips_tiered: {what}", lib.ammc_gather_clips_tiered(*a)))
    return out
