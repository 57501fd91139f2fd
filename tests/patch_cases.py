"""Cases of the four patch-resident S16 forward kernels - csrc/conv_tap_s16.hip (ten instances), conv_outc_s16.hip,
conv_first_s16.hip, conv_up_s16.hip - shared by tests/test_patch_cases_host.py (labels, references, sensitivity, the
refusals of the entry points: no device) and tests/test_gpu_patch_kernels.py (the kernels against fp64).  A helper module
like tests/conv_gemm_cases.py, not a test.

A case is one launch as a caller builds it: the shape, the entry point and its epilogue, which operands are channel
slices, the label `ammc_conv_gemm_s16_variant` must answer (conv_first / conv_up: the name of their own entry point) and
the per-call `s16_mf` / `outc_stream` of the descriptor - the only way an instance is selected here: no ammc_set_option,
no environment variable.  `host_ops` builds the operands (hashed-uniform, deterministic), `reference` evaluates the
reference model's operator sequence with torch in float64 on the operands as the kernel sees them (S16-rounded
activations, filters, residual), `run_case` packs with the library's own pack routines and launches.

Kinds
  tap    3x3 conv through ammc_conv_gemm_s16 on a conv_tap_s16 instance: y = act(scale conv(x, w) + shift) + res
  outc   the output layer (n = 32, n_store real filters, fp32 NCHW, tanh, fused squared error) on conv_outc_s16, or on the
         tap instance the dispatcher falls to
  first  ammc_conv_first_s16 / _bs: zero-padded conv of the NCHW fp32 clips + scale / shift + act
  up     ammc_conv_up_s16: ConvTranspose2d(k 2, s 2) + cat([skip, .]) + conv3x3 + BN(eval) + act

Guarded buffers: every output lives in the middle of a flat buffer filled with the bit pattern SENT (a NaN as a float and
as a pair of halfs).  After the launch every element of the interior must differ from SENT (written) and everything else
- the pads before and behind the tensor, the halo ring on all four sides, the other channel slice of a concat buffer -
must still be SENT, bit for bit.  No kernel here writes its output's halo, so the halo carries the sentinel too: that is
stricter than a pre-zeroed halo and needs no second form."""
import ctypes as C
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, AmmcConvDesc

GATE_S16 = 2e-6            # tap and outc frames, of max|ref| (the project's per-kernel gate)
GATE_SQ = 2e-5             # fused squared error (test_output_layer_vs_fp64)
GATE_UF = 3e-6             # conv_up, conv_first (tests/test_gpu_conv_up.py)
SENS_MIN = 10              # zeroing x's lo halves must move the fp64 truth by at least this many gates
DEV = "cuda:0"
SENT = 0x7FC07FC0
PAD = 1024                 # floats of sentinel before and behind every guarded tensor

_T = "conv_tap_s16<%s>"
KH64, T64_1, T64_0 = _T % "4, 1, 2, 2, 1, 0, 1", _T % "4, 1, 2, 2, 1, 1", _T % "4, 1, 2, 2, 1, 0"
W8_1, W8_0 = _T % "4, 2, 2, 2, 2, 1", _T % "4, 2, 2, 2, 2, 0"
T128_1, T128_0, KH128 = _T % "4, 1, 2, 4, 1, 1", _T % "4, 1, 2, 4, 1, 0", _T % "4, 1, 2, 4, 1, 0, 1"
O4, O8 = _T % "4, 1, 2, 1, 1, 1", _T % "8, 1, 1, 1, 1, 0"
OUTC, FIRST, FIRST_BS, UP = "conv_outc_s16", "ammc_conv_first_s16", "ammc_conv_first_s16_bs", "ammc_conv_up_s16"
TAP_INSTANCES = [KH64, T64_1, T64_0, W8_1, W8_0, T128_1, T128_0, KH128, O4, O8]
MF0, MF1 = 1, 2            # descriptor values of s16_mf: 1 = v_mfma_f32_32x32x16_f16 (MF 0), 2 = 16x16x32 (MF 1)
TAPK, STREAM = 1, 2        # descriptor values of outc_stream: 1 = halo-patch kernel, 2 = streaming kernel


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    B: int
    H: int                   # size of the OUTPUT (up: the skip tensor's)
    W: int
    cin: int                 # tap / outc: input channels; first: c; up: skip channels c (x2 has 2 c)
    n: int
    label: str
    mf: int = 0              # AmmcConvDesc.s16_mf
    outc: int = 0            # AmmcConvDesc.outc_stream
    act: int = ACT_NONE
    scale: str = "none"      # none (NULL) | bn (0.7 .. 1.3) | pow2 (per column 2^-3 .. 2^-5)
    shift: bool = False      # False = NULL
    res: str = "none"        # none | s16 | f32 (fp32 NHWC, needs y_f32)
    y_f32: int = 0
    n_store: int = 0         # > 0: fp32 NCHW, exactly B * n_store * H * W floats
    sq: bool = False         # fused squared error against a target
    sq0: float = 0.0         # what sq_acc holds on entry
    t_off: int = 0           # floats by which the target's base address is moved off its 16-byte alignment
    pool: bool = False       # second output: the 2x2 max-pool
    stats: bool = False      # per-patch channel sums of the stored values
    bnbwd: bool = False      # ... of the BatchNorm backward (needs stats)
    x_slice: bool = False    # x is the upper half of a buffer twice as wide
    y_slice: bool = False    # y likewise
    overflow: bool = False   # column 5 is shifted beyond the half range: the flag must rise
    win: int = -1            # first: x_bs = win * H * W planes (-1: the plain entry, c * H * W); 0 = every entry the same clip
    gen: tuple = ()          # (tag, B, n): operands are the leading part of those generated for this larger case


def _c(name, kind, B, H, W, cin, n, label, **kw):
    return Case(name, kind, B, H, W, cin, n, label, **kw)


BN = dict(scale="bn", shift=True, act=ACT_RELU)
LR = dict(shift=True, act=ACT_LRELU)
F32 = dict(scale="pow2", res="f32", y_f32=1)
ST = dict(y_f32=1, stats=True)
OC = dict(shift=True, act=ACT_TANH, y_f32=1)
S192, S1PI = (24, 16, 128), (192, 8, 32)          # 192 tiles: 8 per image / one per image (every patch touches all four borders)


def tiles(c: Case) -> int:
    return c.B * (c.H // 8) * (c.W // 32) * (1 if c.n <= 64 else c.n // 128)


def _tap_cases():
    out = []
    # ---- the 64-filter instances: floor 192 tiles -------------------------------------------------------------------------
    for tag, lab, mf in (("kh64", KH64, 0), ("t64mf1", T64_1, MF1), ("t64mf0", T64_0, MF0)):
        k = dict(mf=mf)
        out += [
            _c(tag + "-bn-pool-yslice", "tap", *S192, 32, 64, lab, **BN, pool=True, y_slice=True, **k),
            _c(tag + "-lrelu-xslice", "tap", *S1PI, 64, 64, lab, **LR, x_slice=True, **k),
            _c(tag + "-res-cin128", "tap", *S192, 128, 64, lab, **BN, res="s16", **k),
            _c(tag + "-f32-pow2-res", "tap", *S1PI, 32, 64, lab, **F32, **k),
        ]
        if lab != T64_1:
            out.append(_c(tag + "-stats", "tap", *S192, 32, 64, lab + "+stats", **ST, **k))
    out.append(_c("kh64-bnbwd", "tap", *S192, 64, 64, KH64 + "+bnbwd", y_f32=1, stats=True, bnbwd=True, scale="pow2"))
    # ---- the 8-wave instances: n % 128 == 0, fewer than 512 tiles -----------------------------------------------------------
    for tag, lab, mf in (("w8mf1", W8_1, 0), ("w8mf0", W8_0, MF0)):
        k = dict(mf=mf)
        out += [
            _c(tag + "-bn-pool-yslice", "tap", *S192, 32, 128, lab, **BN, pool=True, y_slice=True, **k),
            _c(tag + "-lrelu-xslice", "tap", *S1PI, 64, 128, lab, **LR, x_slice=True, **k),
            _c(tag + "-res-cin128", "tap", *S192, 128, 128, lab, **BN, res="s16", **k),
            _c(tag + "-f32-pow2-res", "tap", *S1PI, 32, 128, lab, **F32, **k),
            _c(tag + "-n256", "tap", 12, 16, 128, 32, 256, lab, **BN, **k),              # two N tiles, 192 tiles
        ]
    out.append(_c("w8mf0-stats", "tap", *S192, 32, 128, W8_0 + "+stats", **ST, mf=MF0))
    out.append(_c("w8mf1-forced", "tap", *S192, 32, 128, W8_1, **BN, mf=MF1))
    # one tile short of the 4-wave 128-filter forms: 511 (73 x 7 patches), forced and default; 1023 (93 x 11), default
    out.append(_c("w8mf1-511", "tap", 73, 56, 32, 32, 128, W8_1, **BN, mf=MF1))
    out.append(_c("w8mf0-511", "tap", 73, 56, 32, 32, 128, W8_0, **BN, mf=MF0))
    out.append(_c("w8mf1-1023-default", "tap", 93, 88, 32, 32, 128, W8_1, **BN))
    # ---- the 4-wave 128-filter instances: at least 512 tiles, s16_mf forced --------------------------------------------------
    S512, S512B = (64, 16, 128), (512, 8, 32)
    for tag, lab, mf in (("t128mf1", T128_1, MF1), ("t128mf0", T128_0, MF0)):
        k = dict(mf=mf)
        out += [
            _c(tag + "-bn-pool-yslice", "tap", *S512, 32, 128, lab, **BN, pool=True, y_slice=True, **k),
            _c(tag + "-lrelu-xslice", "tap", *S512B, 32, 128, lab, **LR, x_slice=True, **k),
            _c(tag + "-res-cin64", "tap", *S512, 64, 128, lab, **BN, res="s16", **k),
            _c(tag + "-f32-pow2-res", "tap", *S512B, 32, 128, lab, **F32, **k),
            _c(tag + "-n256", "tap", 32, 16, 128, 32, 256, lab, **BN, **k),              # two N tiles, 512 tiles
        ]
    out.append(_c("t128mf0-stats", "tap", *S512, 32, 128, T128_0 + "+stats", **ST, mf=MF0))
    # ---- the k-half-major 128-filter instance: at least 1024 tiles, default dispatch -----------------------------------------
    S1024 = (128, 16, 128)
    out += [
        _c("kh128-bn-pool-yslice", "tap", *S1024, 32, 128, KH128, **BN, pool=True, y_slice=True),
        _c("kh128-lrelu-xslice", "tap", 1024, 8, 32, 32, 128, KH128, **LR, x_slice=True),
        _c("kh128-res-cin64", "tap", *S1024, 64, 128, KH128, **BN, res="s16"),
        _c("kh128-f32-pow2-res", "tap", *S1024, 32, 128, KH128, **F32),
        _c("kh128-stats", "tap", *S1024, 32, 128, KH128 + "+stats", **ST),
        _c("kh128-bnbwd", "tap", *S1024, 32, 128, KH128 + "+bnbwd", y_f32=1, stats=True, bnbwd=True, scale="pow2"),
    ]
    # ---- the 32-filter instances (outc_stream off): n_store NCHW + tanh + squared error, fp32 NHWC, statistics ----------------
    for tag, lab, mf in (("o4", O4, 0), ("o8", O8, MF0)):
        k = dict(mf=mf, outc=TAPK)
        out += [
            _c(tag + "-ns3-sq", "tap", *S192, 64, 32, lab, **OC, n_store=3, sq=True, **k),
            _c(tag + "-ns2-1pi", "tap", *S1PI, 32, 32, lab, **OC, n_store=2, sq=True, sq0=3.0, **k),
            _c(tag + "-ns4-sq", "tap", *S192, 32, 32, lab, **OC, n_store=4, sq=True, **k),
            # all 32 columns stored: the 16x16x32 instance holds one 16-filter tile and stores four filters of it, so the
            # dispatcher sends anything wider to the 32x32x16 form (before: 16 of 32 channels of every pixel unwritten)
            _c(tag + "-f32-nhwc", "tap", *S192, 32, 32, O8, **F32, **k),
        ]
    out.append(_c("o8-stats", "tap", *S192, 32, 32, O8 + "+stats", **ST, mf=MF0, outc=TAPK))
    # ---- the overflow flag: one case per S16 store form (the 16x16x32 and the 32x32x16 epilogue) ------------------------------
    out.append(_c("overflow-mf1", "tap", *S192, 32, 128, W8_1, scale="bn", shift=True, overflow=True))
    out.append(_c("overflow-mf0", "tap", *S192, 32, 64, KH64, scale="bn", shift=True, overflow=True))
    return out


def _outc_cases():
    out = []
    oc = dict(outc=STREAM, **OC)
    # tile totals: 192 (fewer than the 256 workgroups), 256 (the last all-single-tile total), 257 (one workgroup takes a
    # second tile), 784 (workgroups with three and with four tiles: the three-stage ring wraps).  cin 32 = one unit per
    # tile (fewer units than stages at 192 / 256), cin 64 = two
    for tot, shp in ((192, S192), (256, (32, 16, 128)), (257, (257, 8, 32)), (784, (49, 32, 128))):
        for cin in (32, 64):
            ns = {192: 3, 256: 2, 257: 1, 784: 3}[tot] if cin == 64 else {192: 1, 256: 4, 257: 3, 784: 2}[tot]
            out.append(_c(f"outc-{tot}-cin{cin}-ns{ns}-sq", "outc", *shp, cin, 32, OUTC, **oc, n_store=ns, sq=True,
                          sq0=(2.5 if tot in (192, 784) else 0.0)))
    out += [
        _c("outc-ns4-sq-wrap", "outc", 49, 32, 128, 64, 32, OUTC, **oc, n_store=4, sq=True),
        _c("outc-ns4-nosq", "outc", *S192, 64, 32, OUTC, **oc, n_store=4, sq0=7.0),
        _c("outc-ns3-nosq-257", "outc", 257, 8, 32, 32, 32, OUTC, **oc, n_store=3, sq0=7.0),
        _c("outc-ns2-nosq-784", "outc", 49, 32, 128, 64, 32, OUTC, **oc, n_store=2, sq0=7.0),
        _c("outc-target-unaligned", "outc", 257, 8, 32, 64, 32, OUTC, **oc, n_store=3, sq=True, sq0=1.0, t_off=1),
        _c("outc-target-unaligned-cin32", "outc", *S192, 32, 32, OUTC, **oc, n_store=2, sq=True, t_off=3),
        _c("outc-ns5-falls-to-tap", "outc", *S192, 64, 32, O8, **oc, n_store=5, sq=True, sq0=2.5),
        _c("outc-ns5-falls-to-tap-nosq", "outc", *S192, 32, 32, O8, **oc, n_store=5, sq0=7.0),
    ]
    return out


def _first_cases():
    out = []
    f = lambda name, B, H, W, c, **kw: _c(name, "first", B, H, W, c, 64, FIRST_BS if kw.get("win", -1) >= 0 else FIRST, **kw)
    sizes = ((8, 32), (16, 64), (24, 96))     # one tile (all borders); the four corner classes; an interior tile
    for i, cc in enumerate((1, 3, 6, 12, 13, 16)):
        H, W = sizes[i % 3]
        out.append(f(f"first-c{cc}-{H}x{W}-relu", 2, H, W, cc, **BN))
        H, W = sizes[(i + 1) % 3]
        out.append(f(f"first-c{cc}-{H}x{W}-none", 3, H, W, cc, scale="bn", shift=True))
    out += [
        f("first-c12-24x96-relu", 2, 24, 96, 12, **BN),
        f("first-c3-null-scale", 2, 16, 64, 3, shift=True, act=ACT_RELU),
        f("first-c6-null-shift", 2, 16, 64, 6, scale="bn"),
        f("first-c12-null-both", 2, 8, 32, 12),
        f("first-c12-512-tiles", 32, 16, 256, 12, **BN),               # exactly the persistent grid
        f("first-c12-513-tiles", 19, 72, 96, 12, **BN),                # one workgroup takes a second tile
        f("first-c3-513-tiles", 19, 72, 96, 3, **BN),                  # ... of the generic channel-count instance
        f("first-c12-yslice", 2, 16, 64, 12, **BN, y_slice=True),
        f("first-c12-overflow", 2, 16, 64, 12, scale="bn", shift=True, overflow=True),
        # through _bs
        f("first-bs-contiguous-c12", 3, 16, 64, 12, **BN, win=12),       # bit-equal to the plain entry (asserted by the test)
        f("first-bs-windows-c12-k3", 5, 16, 64, 12, **BN, win=3),        # evaluate_stream: clip b = frames b .. b + 3 of RGB planes
        f("first-bs-windows-c6-k2", 4, 24, 96, 6, **BN, win=2),
        f("first-bs-windows-c13-k1", 3, 8, 32, 13, **BN, win=1),
        f("first-bs-same-clip", 3, 16, 64, 12, **BN, win=0),
    ]
    return out


def _up_cases():
    out = []
    u = lambda name, B, H, W, c, n, **kw: _c(name, "up", B, H, W, c, n, UP, scale="bn", shift=True, **kw)
    for (H, W) in ((8, 32), (16, 32), (8, 64)):
        for n in (64, 128):
            for B in (1, 3):
                act = ACT_RELU if (B + n // 64) % 2 else ACT_NONE
                out.append(u(f"up-{H}x{W}-n{n}-b{B}", B, H, W, 64, n, act=act))
    out += [
        u("up-n256", 2, 8, 32, 64, 256, act=ACT_RELU),
        u("up-c32-one-skip-block", 3, 8, 32, 32, 64, act=ACT_RELU),
        u("up-c32-n128-16x64", 2, 16, 64, 32, 128),
        u("up-yslice", 3, 8, 32, 64, 64, act=ACT_RELU, y_slice=True),
        u("up-yslice-n128", 1, 16, 32, 32, 128, y_slice=True),
        u("up-overflow", 2, 8, 32, 32, 64, overflow=True),
        u("up-overflow-n128", 1, 8, 64, 32, 128, act=ACT_RELU, overflow=True),
    ]
    return out


CASES = _tap_cases() + _outc_cases() + _first_cases() + _up_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BIG = [c for c in CASES if c.kind in ("tap", "outc") and tiles(c) >= 1024]      # reference by torch's fp64 conv on the device

# cross-instance agreement: the same activations and the same bank of 128 filters (n = 64 / 32: its first filters; the
# 8-wave instances, which exist below 512 tiles only: the first 24 images)
_SH = ("shared", 128, 128)
SHARED = [
    _c("shared-kh128", "tap", 128, 16, 128, 32, 128, KH128, **BN, gen=_SH),
    _c("shared-t128mf1", "tap", 128, 16, 128, 32, 128, T128_1, **BN, mf=MF1, gen=_SH),
    _c("shared-t128mf0", "tap", 128, 16, 128, 32, 128, T128_0, **BN, mf=MF0, gen=_SH),
    _c("shared-w8mf1", "tap", 24, 16, 128, 32, 128, W8_1, **BN, gen=_SH),
    _c("shared-w8mf0", "tap", 24, 16, 128, 32, 128, W8_0, **BN, mf=MF0, gen=_SH),
    _c("shared-kh64", "tap", 128, 16, 128, 32, 64, KH64, **BN, gen=_SH),
    _c("shared-t64mf1", "tap", 128, 16, 128, 32, 64, T64_1, **BN, mf=MF1, gen=_SH),
    _c("shared-t64mf0", "tap", 128, 16, 128, 32, 64, T64_0, **BN, mf=MF0, gen=_SH),
    _c("shared-o4", "tap", 128, 16, 128, 32, 32, O4, **BN, y_f32=1, n_store=4, outc=TAPK, gen=_SH),      # (it stores <= 4 filters)
    _c("shared-o8", "tap", 128, 16, 128, 32, 32, O8, **BN, y_f32=1, outc=TAPK, mf=MF0, gen=_SH),
]


def gate(c: Case) -> float:
    return GATE_S16 if c.kind in ("tap", "outc") else GATE_UF


def out_channels(c: Case) -> int:
    return c.n_store or c.n


# ---- operands and references ------------------------------------------------------------------------------------------------
class Ops:
    pass


def s16_round(t: torch.Tensor) -> torch.Tensor:
    """what an fp32 tensor decodes to after the S16 split (ammc_common.h ammc_s16_split8): hi = half(v), lo = half((v - hi) 2^11)"""
    t = t.float()
    hi = t.half().float()
    lo = ((t - hi) * 2048.0).half().float()
    return hi.double() + lo.double() / 2048.0


def hi_only(t: torch.Tensor) -> torch.Tensor:
    return t.float().half().double()


def first_planes(c: Case) -> int:
    """planes of the frame tensor a `first` case reads its clips from"""
    return c.B * c.cin if c.win < 0 else (c.B - 1) * c.win + c.cin


def host_ops(c: Case) -> Ops:
    o = Ops()
    t, gB, gn = c.gen or ("pc-" + c.name, c.B, out_channels(c) if c.kind != "up" else c.n)
    nt = out_channels(c)
    o.scale = o.shift = o.res = o.target = o.bn = None
    if c.kind in ("tap", "outc"):
        o.x = S.hashed_uniform(t + "x", (gB, c.cin, c.H, c.W))[:c.B]
        o.w = (S.hashed_uniform(t + "w", (gn, c.cin, 3, 3)) * (2.0 / (9 * c.cin)) ** 0.5)[:nt]
    elif c.kind == "first":
        o.x = S.hashed_uniform(t + "x", (first_planes(c), c.H, c.W)) * 1.7          # the frame planes; clips: first_clips
        o.w = S.hashed_uniform(t + "w", (64, c.cin, 3, 3)) * (2.0 / (9 * c.cin)) ** 0.5
    else:
        o.x = S.hashed_uniform(t + "sk", (c.B, c.cin, c.H, c.W))                   # the skip tensor
        o.x2 = S.hashed_uniform(t + "x2", (c.B, 2 * c.cin, c.H // 2, c.W // 2))
        o.w = S.hashed_uniform(t + "w3", (c.n, 2 * c.cin, 3, 3)) * (2.0 / (18 * c.cin)) ** 0.5
        o.wt = S.hashed_uniform(t + "wt", (2 * c.cin, c.cin, 2, 2)) * (1.0 / (2 * c.cin)) ** 0.5
        o.bt = S.hashed_uniform(t + "bt", (c.cin,)) * 0.3
    if c.scale == "bn":
        o.scale = S.hashed_uniform(t + "s", (max(gn, c.n),), 0.7, 1.3)[:c.n].clone()
    elif c.scale == "pow2":
        o.scale = torch.tensor([2.0 ** -(3 + i % 3) for i in range(c.n)])
        o.x = o.x * 16.0
    if c.shift:
        o.shift = S.hashed_uniform(t + "b", (max(gn, c.n),), -0.2, 0.2)[:c.n].clone()
        o.shift[nt:] = 0
    if c.overflow:
        o.shift[5] = 1.0e5
    if c.res != "none":
        o.res = S.hashed_uniform(t + "r", (c.B, c.n, c.H, c.W))
    if c.sq:
        o.target = S.hashed_uniform(t + "t", (c.B, nt, c.H, c.W))
    if c.bnbwd:
        # the saved conv output in steps of 1/64, scale a power of two, shift an odd multiple of 1/256: `pre` is exact in
        # fp32 (with or without an fma) and never zero, so the ReLU mask has no rounding cases
        o.bn = dict(c=torch.round(S.hashed_uniform(t + "bc", (c.B, c.n, c.H, c.W)) * 64) / 64,
                    mean=S.hashed_uniform(t + "bm", (c.n,), -0.1, 0.1), invstd=S.hashed_uniform(t + "bi", (c.n,), 0.8, 1.6),
                    scale=torch.tensor([1.0, 0.5][:] * (c.n // 2)),
                    shift=(torch.round(S.hashed_uniform(t + "bb", (c.n,)) * 32) * 2 + 1) / 256)
    return o


def first_clips(c: Case, planes: torch.Tensor) -> torch.Tensor:
    """[B][c][H][W]: the clips a `first` case's launch reads from its frame planes, by explicit slicing"""
    step = c.cin if c.win < 0 else c.win
    return torch.stack([planes[b * step:b * step + c.cin] for b in range(c.B)])


def _act(y, act):
    if act == ACT_RELU:
        return y.clamp_min(0)
    if act == ACT_LRELU:
        return torch.where(y > 0, y, 0.1 * y)
    if act == ACT_TANH:
        return torch.tanh(y)
    return y


def reference(c: Case, o: Ops, x=None, w=None, res=None, x2=None):
    """the case's operation in float64 on the given operands (defaults: the S16-rounded host operands), on their device:
    [B, n_store or n, H, W]"""
    x = s16_round(o.x) if x is None else x.double()
    dev = x.device
    w = (s16_round(o.w) if w is None else w.double()).to(dev)
    v = lambda t: t.double().to(dev).view(1, -1, 1, 1)
    nt = out_channels(c)
    if c.kind == "first":
        xc = first_clips(c, x) if x.dim() == 3 else x
        y = F.conv2d(xc, w, padding=1)                                                # the zero-padded conv
    elif c.kind == "up":
        x2 = (s16_round(o.x2) if x2 is None else x2.double()).to(dev)
        upx = F.conv_transpose2d(x2, o.wt.double().to(dev), o.bt.double().to(dev), stride=2)
        y = F.conv2d(torch.cat([x, upx], 1), o.w.double().to(dev), padding=1)        # fp32 filters: the kernel composes them in double
    else:
        y = F.conv2d(x, w, padding=1)
    if o.scale is not None:
        y = y * v(o.scale[:nt])
    if o.shift is not None:
        y = y + v(o.shift[:nt])
    y = _act(y, c.act)
    if c.res != "none":
        r = (s16_round(o.res) if c.res == "s16" else o.res.double()) if res is None else res.double()
        y = y + r.to(dev)
    return y


def compare_mask(c: Case, want: torch.Tensor) -> torch.Tensor:
    m = torch.ones_like(want, dtype=torch.bool)
    if c.overflow:
        m[:, 5] = False
    return m


def rel_err(got, want, mask=None) -> float:
    got, want = got.double(), want.double().to(got.device)
    if mask is not None:
        got, want = got[mask], want[mask]
    return float((got - want).abs().max() / want.abs().max())


def sensitivity(c: Case, o: Ops, dev="cpu") -> float:
    """how far the fp64 truth moves, in gates, when x (up: both activations) loses its lo halves"""
    want = reference(c, o, x=s16_round(o.x).to(dev))
    kw = dict(x2=hi_only(o.x2).to(dev)) if c.kind == "up" else {}
    want_hi = reference(c, o, x=hi_only(o.x).to(dev), **kw)
    return rel_err(want_hi, want, compare_mask(c, want)) / gate(c)


def want_sq(c: Case, o: Ops, want: torch.Tensor) -> torch.Tensor:
    """sq_acc after the launch: it ACCUMULATES (include/ammc_hip.h: 'adds ... to sq_acc[sample]')"""
    return ((o.target.double().to(want.device) - want) * 0.5).pow(2).sum(dim=(1, 2, 3)).cpu() + c.sq0


# ---- descriptors --------------------------------------------------------------------------------------------------------------
def conv_desc(c: Case, x=0x10000000, w=0x20000000, y=0x30000000) -> AmmcConvDesc:
    """the descriptor of a tap / outc / up case over buffers at the given addresses of pixel-(0, 0) halo corners (fake ones
    for the label); the launcher fills in the optional operands"""
    d = AmmcConvDesc()
    xct, xoff = (2 * c.cin, c.cin) if c.x_slice else (c.cin, 0)
    if c.kind == "up":
        xct, xoff = 2 * c.cin, 0                            # the skip tensor is the first half of the concat buffer
    d.x, d.w = x + 4 * xoff, w
    d.batch, d.height, d.width, d.cin, d.ntaps, d.n, d.up, d.cgroup, d.act = c.B, c.H, c.W, c.cin, 9, c.n, 1, c.n, c.act
    d.x_bs, d.x_rs, d.x_ps = (c.H + 2) * (c.W + 2) * xct, (c.W + 2) * xct, xct
    d.y_f32, d.s16_mf, d.outc_stream = c.y_f32, c.mf, c.outc
    if c.n_store:
        d.y = y
        d.n_store, d.y_cs = c.n_store, c.H * c.W
        d.y_bs, d.y_rs, d.y_ps = c.n_store * c.H * c.W, c.W, 1
    else:
        yct, yoff = (2 * c.n, c.n) if c.y_slice else (c.n, 0)
        d.y_bs, d.y_rs, d.y_ps = (c.H + 2) * (c.W + 2) * yct, (c.W + 2) * yct, yct
        d.y = y + 4 * (d.y_rs + d.y_ps + yoff)
    d.scale, d.shift = (0x60000000 if c.scale != "none" else None), (0x61000000 if c.shift else None)
    if c.res != "none":
        d.res = 0x40000000
        d.r_bs, d.r_rs, d.r_ps = c.H * c.W * c.n, c.W * c.n, c.n
    if c.sq:
        d.sq_target, d.sq_acc = 0x70000000, 0x71000000
    if c.pool:
        d.pool_y = 0x72000000
        d.pool_bs, d.pool_rs, d.pool_ps = (c.H // 2 + 2) * (c.W // 2 + 2) * c.n, (c.W // 2 + 2) * c.n, c.n
    if c.stats:
        d.stats = 0x73000000
    if c.bnbwd:
        d.bn_c, d.bn_mean, d.bn_invstd, d.bn_scale, d.bn_shift, d.bn_relu = 0x74000000, 0x75000000, 0x75100000, 0x75200000, 0x75300000, 1
        d.bn_bs, d.bn_rs, d.bn_ps = c.H * c.W * c.n, c.W * c.n, c.n
    return d


def label_of(c: Case) -> str:
    """what the library's own dispatch answers for the case (no device needed); conv_first / conv_up: their entry point"""
    if c.kind in ("first", "up"):
        return FIRST_BS if (c.kind == "first" and c.win >= 0) else (FIRST if c.kind == "first" else UP)
    from ammcnet_aaai2021_amd.engine import s16_variant
    return s16_variant(conv_desc(c))


# ---- the refusals of the entry points (they return before anything is launched: no device needed) ----------------------------
def first_refusals():
    """[(what, status the entry returns, expected status)] of ammc_conv_first_s16 / _bs"""
    lib = _lib.load()
    X, WI, Y = 0x10000000, 0x20000000, 0x30000000

    def call(c=12, h=16, w=64, y=Y, st=(18 * 66 * 64, 66 * 64, 64), act=ACT_RELU, x=X, wi=WI, bs=None):
        if bs is None:
            return lib.ammc_conv_first_s16(x, 2, c, h, w, wi, None, None, act, y, *st, None, None)
        return lib.ammc_conv_first_s16_bs(x, bs, 2, c, h, w, wi, None, None, act, y, *st, None, None)
    return [
        ("c = 17", call(c=17), -2), ("w % 32", call(w=48), -2), ("h % 8", call(h=12), -2),
        ("y not 32-byte aligned", call(y=Y + 16), -1), ("stride not a multiple of 8", call(st=(18 * 66 * 64 + 4, 66 * 64, 64)), -1),
        ("pixel stride not a multiple of 8", call(st=(18 * 66 * 68, 66 * 68, 68)), -1),
        ("tanh", call(act=ACT_TANH), -2), ("null x", call(x=None), -1), ("null filter image", call(wi=None), -1),
        ("negative x_bs", call(bs=-1), -1), ("c = 17 through _bs", call(c=17, bs=0), -2),
    ]


def up_refusals():
    """[(what, status the entry returns, expected status)] of ammc_conv_up_s16"""
    lib = _lib.load()
    base = BY_NAME["up-8x32-n64-b1"]

    def call(up_cin=None, up_x=0x50000000, up_st=(6 * 18 * 128, 18 * 128, 128), up_w=0x51000000, s9=0x52000000, **kw):
        d = conv_desc(base)
        for k, val in kw.items():
            setattr(d, k, val)
        return lib.ammc_conv_up_s16(C.byref(d), up_x, *up_st, 2 * d.cin if up_cin is None else up_cin, up_w, s9, None)
    d0 = conv_desc(base)
    return [
        ("up_cin != 2 cin", call(up_cin=64), -2), ("y_f32", call(y_f32=1), -2), ("res", call(res=0x40000000), -2),
        ("pool_y", call(pool_y=0x72000000), -2), ("n_store", call(n_store=3), -2), ("y_cs", call(y_cs=256), -2),
        ("w % 32", call(width=48), -2), ("h % 8", call(height=12), -2), ("n = 96", call(n=96), -2), ("cin = 48", call(cin=48, up_cin=96), -2),
        ("x not 16-byte aligned", call(x=d0.x + 4), -1), ("y not 32-byte aligned", call(y=d0.y + 16), -1),
        ("up_x not 16-byte aligned", call(up_x=0x50000004), -1), ("up_w not 16-byte aligned", call(up_w=0x51000008), -1),
        ("shift9 not 16-byte aligned", call(s9=0x52000004), -1), ("y stride", call(y_rs=d0.y_rs + 4), -1),
        ("x stride", call(x_ps=d0.x_ps + 4), -1), ("up stride", call(up_st=(6 * 18 * 128, 18 * 128 + 4, 128)), -1),
        ("null up_x", call(up_x=None), -1), ("null shift9", call(s9=None), -1),
    ]


# ---- the device half ------------------------------------------------------------------------------------------------------------
def _ptr(t: torch.Tensor, off: int = 0) -> int:
    return t.data_ptr() + 4 * off


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guard:
    """a tensor of `shape` in the middle of a flat buffer, everything filled with SENT; `interior` = the index (a tuple of
    slices into the tensor) the kernel must fill"""

    def __init__(self, shape, interior=None):
        n = 1
        for s in shape:
            n *= s
        self.flat = torch.full((PAD + n + PAD,), SENT, dtype=torch.int32, device=DEV)
        self.bits = self.flat[PAD:PAD + n].view(shape)
        self.t = self.bits.view(torch.float32)
        self.interior = interior if interior is not None else tuple(slice(None) for _ in shape)

    def check(self, what):
        """every interior element written, everything else still the sentinel (halo ring on all four sides, the other
        channel slice, the pads before and behind the tensor)"""
        untouched = self.flat == SENT
        assert bool(untouched[:PAD].all()), f"{what}: written BEFORE the tensor"
        assert bool(untouched[-PAD:].all()), f"{what}: written BEHIND the tensor"
        inside = torch.zeros(self.bits.shape, dtype=torch.bool, device=DEV)
        inside[self.interior] = True
        body = untouched[PAD:-PAD].view(self.bits.shape)
        assert bool(body[~inside].all()), f"{what}: written outside the interior (halo ring / other channel slice)"
        assert not bool(body[inside].any()), f"{what}: an interior element was never written"


def _s16_act(x, ctot, coff, junk_tag=None):
    """NCHW fp32 (host) -> halo-1 S16 activation in channels [coff, coff + C) of a zeroed buffer `ctot` wide; returns
    (buffer, the values as the kernel sees them [NCHW, device, fp32])"""
    lib, s = _lib.load(), _stream()
    B, Cc, H, W = x.shape
    buf = torch.zeros(B, H + 2, W + 2, ctot, device=DEV)
    st = ((H + 2) * (W + 2) * ctot, (W + 2) * ctot, ctot)
    pix0 = st[1] + st[2]
    if junk_tag and ctot > Cc:                  # the other slice holds large values: a read of it shows
        other = 0 if coff else Cc
        junk = (S.hashed_uniform(junk_tag, (B, ctot - Cc, H, W)) * 100).to(DEV)
        _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(junk), B, ctot - Cc, H, W, _ptr(buf, pix0 + other), *st, ctot - Cc, s), "junk")
    xd = x.to(DEV).contiguous()
    _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(xd), B, Cc, H, W, _ptr(buf, pix0 + coff), *st, Cc, s), "nchw_to_s16")
    back = torch.empty(B, Cc, H, W, device=DEV)
    _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(buf, pix0 + coff), *st, B, Cc, H, W, _ptr(back), s), "s16_to_nchw")
    return buf, back


def _s16_filter(w, n):
    """OIHW (host) -> the S16 GEMM filter [n][9 cin] (zero rows up to n)"""
    lib, s = _lib.load(), _stream()
    nt, cin = w.shape[0], w.shape[1]
    wn = torch.zeros(n, cin, 3, 3, device=DEV)
    wn[:nt] = w.to(DEV)
    wp = torch.full((n, 9 * cin), float("nan"), device=DEV)
    _lib.check(lib.ammc_pack_conv_weight_f32(_ptr(wn), n, cin, 3, cin, _ptr(wp), s), "pack_conv")
    assert bool(torch.isfinite(wp).all())
    ws = torch.empty_like(wp)
    _lib.check(lib.ammc_split_rows_f32(_ptr(wp), wp.numel(), _ptr(ws), s), "split")
    return ws


def _nhwc_guard(c: Case, n):
    yct, yoff = (2 * n, n) if c.y_slice else (n, 0)
    g = Guard((c.B, c.H + 2, c.W + 2, yct), (slice(None), slice(1, c.H + 1), slice(1, c.W + 1), slice(yoff, yoff + n)))
    st = ((c.H + 2) * (c.W + 2) * yct, (c.W + 2) * yct, yct)
    return g, st, st[1] + st[2] + yoff


def _read_s16(g: Guard, st, pix0, B, n, H, W):
    lib, s = _lib.load(), _stream()
    got = torch.empty(B, n, H, W, device=DEV)
    _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(g.t, pix0), *st, B, n, H, W, _ptr(got), s), "y back")
    return got


def _run_conv(c: Case, o: Ops, r: dict):
    lib, s = _lib.load(), _stream()
    nt = out_channels(c)
    xct, xoff = (2 * c.cin, c.cin) if c.x_slice else (c.cin, 0)
    xbuf, r["x"] = _s16_act(o.x, xct, xoff, "junk" + c.name)
    ws = _s16_filter(o.w, c.n)
    keep = [xbuf, ws]
    d = conv_desc(c, x=_ptr(xbuf), w=_ptr(ws), y=0)
    dv = lambda t: t.to(DEV).contiguous() if t is not None else None
    scale, shift = dv(o.scale), dv(o.shift)
    d.scale, d.shift = (_ptr(scale) if scale is not None else None), (_ptr(shift) if shift is not None else None)
    if c.res == "s16":
        rbuf = torch.zeros(c.B, c.H, c.W, c.n, device=DEV)
        rd = dv(o.res)
        _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(rd), c.B, c.n, c.H, c.W, _ptr(rbuf), d.r_bs, d.r_rs, d.r_ps, c.n, s), "res")
        rr = torch.empty_like(rd)
        _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(rbuf), d.r_bs, d.r_rs, d.r_ps, c.B, c.n, c.H, c.W, _ptr(rr), s), "res back")
        d.res, r["res"] = _ptr(rbuf), rr
        keep.append(rbuf)
    elif c.res == "f32":
        rbuf = dv(o.res).permute(0, 2, 3, 1).contiguous()
        d.res, r["res"] = _ptr(rbuf), o.res
        keep.append(rbuf)
    if c.n_store:
        g, st, pix0 = Guard((c.B, c.n_store, c.H, c.W)), None, 0
    else:
        g, st, pix0 = _nhwc_guard(c, c.n)
    d.y = _ptr(g.t, pix0)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    d.overflow_flag = flag.data_ptr()
    sq = torch.full((c.B,), c.sq0, device=DEV) if c.n_store else None
    if sq is not None:
        d.sq_acc = _ptr(sq)                                  # also without a target: it must then stay as it is
    d.sq_target = None
    if c.sq:
        tflat = torch.zeros(o.target.numel() + 8, device=DEV)
        tflat[c.t_off:c.t_off + o.target.numel()] = dv(o.target).reshape(-1)
        d.sq_target = _ptr(tflat, c.t_off)
        keep.append(tflat)
    gp = None
    if c.pool:
        gp = Guard((c.B, c.H // 2 + 2, c.W // 2 + 2, c.n), (slice(None), slice(1, c.H // 2 + 1), slice(1, c.W // 2 + 1), slice(None)))
        d.pool_y = _ptr(gp.t, d.pool_rs + d.pool_ps)
    gs = None
    if c.stats:
        if c.bnbwd:
            bn = {k: dv(v) for k, v in o.bn.items()}
            bn["c"] = bn["c"].permute(0, 2, 3, 1).contiguous()
            d.bn_c, d.bn_mean, d.bn_invstd, d.bn_scale, d.bn_shift = (_ptr(bn[k]) for k in ("c", "mean", "invstd", "scale", "shift"))
            keep.append(bn)
        rows = lib.ammc_conv_gemm_s16_stats_rows(C.byref(d))
        assert rows == c.B * (c.H // 8) * (c.W // 32), rows
        gs = Guard((rows, 4 if c.bnbwd else 2, c.n))
        d.stats = _ptr(gs.t)
    from ammcnet_aaai2021_amd.engine import s16_variant
    r["label"] = s16_variant(d)
    rc = lib.ammc_conv_gemm_s16(C.byref(d), s)
    r["status"] = rc
    if rc != 0:
        return
    torch.cuda.synchronize()
    g.check(c.name + " y")
    s16_out = not c.y_f32
    read = lambda gg: (_read_s16(gg, st, pix0, c.B, c.n, c.H, c.W) if s16_out else
                       (gg.t.clone() if c.n_store else gg.t[gg.interior].permute(0, 3, 1, 2).contiguous()))
    r["got"] = read(g)
    r["flag"] = int(flag.item())
    r["sq"] = sq.cpu() if sq is not None else None
    if gp is not None:
        gp.check(c.name + " pool")
        pst = (d.pool_bs, d.pool_rs, d.pool_ps)
        r["pool"] = _read_s16(gp, pst, d.pool_rs + d.pool_ps, c.B, c.n, c.H // 2, c.W // 2)
    if gs is not None:
        gs.check(c.name + " stats")
        r["stats"] = gs.t.clone()
    # determinism: a second launch into a fresh guarded buffer gives the same bits (the squared error goes through atomics
    # and is left out; the frames beside it are not)
    g2 = Guard(tuple(g.bits.shape), g.interior)
    d.y = _ptr(g2.t, pix0)
    if gp is not None:
        gp2 = Guard(tuple(gp.bits.shape), gp.interior)
        d.pool_y = _ptr(gp2.t, d.pool_rs + d.pool_ps)
    if gs is not None:
        gs2 = Guard(tuple(gs.bits.shape))
        d.stats = _ptr(gs2.t)
    _lib.check(lib.ammc_conv_gemm_s16(C.byref(d), s), "second launch")
    torch.cuda.synchronize()
    r["same"] = torch.equal(g.bits, g2.bits) and (gp is None or torch.equal(gp.bits, gp2.bits)) and (gs is None or torch.equal(gs.bits, gs2.bits))
    del keep


def _run_first(c: Case, o: Ops, r: dict):
    lib, s = _lib.load(), _stream()
    x = o.x.to(DEV).contiguous()
    w = o.w.to(DEV).contiguous()
    img = torch.empty(lib.ammc_first_conv_image_floats(), device=DEV)
    _lib.check(lib.ammc_pack_first_conv_f32(_ptr(w), 64, c.cin, _ptr(img), s), "pack_first")
    dv = lambda t: t.to(DEV).contiguous() if t is not None else None
    scale, shift = dv(o.scale), dv(o.shift)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    r["x"], r["label"] = s16_round(o.x), label_of(c)
    outs = []
    tail = (_ptr(scale) if scale is not None else None, _ptr(shift) if shift is not None else None)
    # the case's own entry, the plain entry where x_bs = c h w must give the same bits, and the case's own entry again
    for entry in [r["label"]] + ([FIRST] if c.win == c.cin else []) + [r["label"]]:
        g, st, pix0 = _nhwc_guard(c, 64)
        args = (_ptr(img), *tail, c.act, _ptr(g.t, pix0), *st, flag.data_ptr(), s)
        if entry == FIRST_BS:
            rc = lib.ammc_conv_first_s16_bs(_ptr(x), c.win * c.H * c.W, c.B, c.cin, c.H, c.W, *args)
        else:
            rc = lib.ammc_conv_first_s16(_ptr(x), c.B, c.cin, c.H, c.W, *args)
        r["status"] = rc
        if rc != 0:
            return
        torch.cuda.synchronize()
        g.check(f"{c.name} y ({entry})")
        outs.append(g)
    r["got"] = _read_s16(outs[0], st, pix0, c.B, 64, c.H, c.W)
    r["flag"] = int(flag.item())
    r["same"] = all(torch.equal(outs[0].bits, g.bits) for g in outs[1:])       # the repeat, and the plain entry when x_bs = c h w


def _run_up(c: Case, o: Ops, r: dict):
    lib, s = _lib.load(), _stream()
    cc, n = c.cin, c.n
    skbuf, r["x"] = _s16_act(o.x, 2 * cc, 0, "junk" + c.name)           # the skip tensor is the first half of the concat buffer
    x2buf, r["x2"] = _s16_act(o.x2, 2 * cc, 0)
    ws = _s16_filter(o.w, n)
    dv = lambda t: t.to(DEV).contiguous()
    w3, wt, bt, scale, shift = dv(o.w), dv(o.wt), dv(o.bt), dv(o.scale), dv(o.shift)
    w2 = torch.full((n, 16 * 2 * cc), float("nan"), device=DEV)
    shift9 = torch.full((9, n), float("nan"), device=DEV)
    _lib.check(lib.ammc_pack_up_conv_f32(_ptr(w3), _ptr(wt), _ptr(bt), _ptr(scale), _ptr(shift), n, cc, _ptr(w2), _ptr(shift9), s), "pack_up")
    assert bool(torch.isfinite(w2).all()) and bool(torch.isfinite(shift9).all())
    w2s = torch.empty_like(w2)
    _lib.check(lib.ammc_split_rows_f32(_ptr(w2), w2.numel(), _ptr(w2s), s), "split")
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = conv_desc(c, x=_ptr(skbuf), w=_ptr(ws), y=0)
    d.scale, d.shift, d.overflow_flag = _ptr(scale), None, flag.data_ptr()
    h2, w2_ = c.H // 2, c.W // 2
    ust = ((h2 + 2) * (w2_ + 2) * 2 * cc, (w2_ + 2) * 2 * cc, 2 * cc)
    r["label"] = UP
    outs = []
    for _ in range(2):
        g, st, pix0 = _nhwc_guard(c, n)
        d.y = _ptr(g.t, pix0)
        rc = lib.ammc_conv_up_s16(C.byref(d), _ptr(x2buf), *ust, 2 * cc, _ptr(w2s), _ptr(shift9), s)
        r["status"] = rc
        if rc != 0:
            return
        torch.cuda.synchronize()
        g.check(c.name + " y")
        outs.append(g)
    r["got"] = _read_s16(outs[0], st, pix0, c.B, n, c.H, c.W)
    r["flag"] = int(flag.item())
    r["same"] = torch.equal(outs[0].bits, outs[1].bits)


def run_case(c: Case, o: Ops) -> dict:
    """pack, launch twice, read back.  Returns got [B, n_store or n, H, W] (device), the activations as the kernel saw
    them (x, x2, res), label, status, flag, sq, pool, stats, same (the second launch gave the same bits); the guards are
    asserted here"""
    r = dict(status=0, res=None, x2=None)
    {"tap": _run_conv, "outc": _run_conv, "first": _run_first, "up": _run_up}[c.kind](c, o, r)
    return r


def device_want(c: Case, o: Ops, r: dict, dev="cpu"):
    """fp64 truth on the operands as the kernel saw them, evaluated on `dev`"""
    mv = lambda t: t.to(dev) if t is not None else None
    return reference(c, o, x=mv(r["x"]), res=mv(r["res"]), x2=mv(r["x2"]))
