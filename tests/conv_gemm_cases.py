"""Descriptor cases of the implicit-GEMM convolutions (csrc/conv_gemm_s16.hip, csrc/conv_gemm_f32.hip), shared by
tests/test_conv_gemm_cases_host.py (dispatch labels, the CPU half of every case) and tests/test_gpu_conv_gemm.py (the
kernels against fp64).  A helper module like tests/truth.py, not a test.

A case is one layer as a caller builds it: the shape, the epilogue, the gather mode, and the
`ammc_conv_gemm_s16_variant` label it must reach.  `host_ops` builds its operands (hashed-uniform, deterministic) on
the CPU, `reference` evaluates the operation with torch in any dtype (fp64 = the truth, fp32 = the witness of the
fp32 gate), `run_case` packs the operands with the library's own pack routines and launches the kernel.

Kinds
  conv    y = act(scale * conv(x, w, stride = x_step) + shift) + res; 3x3 pad 1 (ntaps 9), 4x4 pad 2 (16), 1x1 (1)
  up      ConvTranspose2d(k 2, s 2) + bias: ntaps 1, up = 2, scattered into a channel slice of a concat buffer
  dgrad3  input gradient of a 3x3 conv: x = dY, filter from ammc_pack_conv_dgrad_weight_f32
  dgrad1  input gradient of a 1x1 conv: filter from ammc_transpose_pad_f32
  dgradT  input gradient of the ConvTranspose: ntaps 4, x_step 2, filter = transpose of the packed ConvTranspose filter
  dgrad4  input gradient of a 4x4 conv (ammc_pack_conv4_dgrad_weight_f32): stride 1 = one 16-tap conv; stride 2 = four
          2x2-tap parity convs (ntaps 4, x_step 1) through doubled output strides, pad 2 (PixelDiscriminator) or pad 1
          (= the forward of FlowNet2-SD's ConvTranspose2d(k 4, s 2, p 1))
The reference of every dgrad kind is torch's own gradient (torch.nn.grad.conv2d_input / autograd), so the pack
routine's flip is part of what is checked."""
import ctypes as C
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, AmmcConvDesc

GATE_S16 = 2e-6          # the project's per-kernel gate (test_gpu_conv_tap.py, test_gpu_conv_up.py)
GATE_SQ = 2e-5           # fused squared error (test_output_layer_vs_fp64)
SENS_MIN = 10 * GATE_S16  # dropping x's lo halves must move the result by at least this: the gate can see a lost cross term
WITNESS_FACTOR = 3.0     # fp32 gate: e_hip <= 3 e_witness (1.5 of DESIGN 5.4 for a sequential chain over K <= 4608, x 2)
DEV = "cuda:0"

L128, L256, L64, L32 = "conv_gemm_s16<128x128>", "conv_gemm_s16<256x128>", "conv_gemm_s16<128x64>", "conv_gemm_s16<128x32>"


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    B: int
    H: int                 # pixel space of m (dgrad4 stride 2: the size of the whole input gradient; the phases derive theirs)
    W: int
    cin: int               # GEMM channels per tap (padded)
    n: int                 # GEMM N
    ntaps: int
    label: str             # what ammc_conv_gemm_s16_variant must answer (dgrad4 stride 2: for every phase)
    c_true: int = 0        # logical channels of x (0 = cin): the rest of cin is zero padding
    n_true: int = 0        # logical output channels (0 = n)
    x_step: int = 1
    act: int = ACT_NONE
    scale: str = "none"    # none | bn (0.7 .. 1.3) | pow2 (per-column 2^-3 .. 2^-5, what undoes a gradient's rescaling)
    shift: bool = False
    res: str = "none"      # none | s16 | f32 (S16 runs; the fp32 kernel always takes an fp32 NHWC residual)
    y_f32: int = 0
    nchw: bool = False     # n_store = n_true, y_cs = H * W, exactly B * n_true * H * W floats
    sq: bool = False       # fused squared error against a target
    x_slice: bool = False  # x is the upper half of a buffer twice as wide
    y_slice: bool = False  # y likewise (up: always)
    splitk: int = 0        # floats of split-K workspace attached (0 = none)
    overflow: bool = False  # column 5 is shifted beyond the half range: the flag must rise
    stride: int = 1        # dgrad4: stride of the convolution whose gradient this is
    pad: int = 2           # dgrad4: its padding
    skip_hw: Optional[Tuple[int, int]] = None     # up: size of the concat buffer when it is not (2H, 2W) (the odd crop)
    status: int = 0        # status code the entry must return (0 = it runs)


def _c(name, kind, B, H, W, cin, n, ntaps, label, **kw):
    return Case(name, kind, B, H, W, cin, n, ntaps, label, **kw)


BN = dict(scale="bn", shift=True, act=ACT_RELU)
CASES = [
    # ---- every instance of conv_gemm_s16's dispatcher (conv_gemm_s16.hip, conv_gemm_s16_dispatch) ----------------------
    _c("t128-3x3-25x25", "conv", 3, 25, 25, 64, 128, 9, L128, **BN, res="s16"),          # M = 1875: tail, tiles span images
    _c("t128-3x3-9x13", "conv", 1, 9, 13, 32, 256, 9, L128, **BN),                         # M = 117 < one tile, two N tiles
    # split-K: nchunks 18, ksplit = nchunks / 4 = 4, 18 % 4 != 0 (slices of 5, 5, 5, 3 chunks)
    _c("splitk4-9x13", "conv", 1, 9, 13, 64, 128, 9, L128 + "+splitk4", **BN, res="s16", splitk=1 << 20),
    # K = 4608 (cin 512), 15 tiles: ksplit = ceil(512 / 15) = 35, 144 % 35 != 0 (29 slices of 5 chunks, 6 empty ones)
    _c("splitk35-k4608", "conv", 3, 25, 25, 512, 128, 9, L128 + "+splitk35", **BN, splitk=35 * 1875 * 128),
    # the same layer with room for 7 slices only: ksplit capped by splitk_ws_floats, 144 % 7 != 0
    _c("splitk7-capped", "conv", 3, 25, 25, 512, 128, 9, L128 + "+splitk7", **BN, splitk=7 * 1875 * 128 + 100),
    _c("splitk-lrelu-4x4", "conv", 2, 9, 9, 64, 128, 16, L128 + "+splitk8", shift=True, act=ACT_LRELU, splitk=1 << 21),
    # 256-row tiles: M >= 131072 * 128 / n and nchunks > 16, W % 32 != 0 so the halo-patch kernel refuses
    _c("t256-48x48", "conv", 16, 48, 48, 64, 512, 9, L256, **BN),                          # M = 36864 = 144 * 256
    _c("t256-tail-47x49", "conv", 15, 47, 49, 64, 512, 9, L256, **BN, res="s16"),          # M = 34545: not a multiple of 256
    _c("t64-3x3-25x25", "conv", 3, 25, 25, 32, 64, 9, L64, **BN),
    _c("t64-1x1-f32out", "conv", 2, 9, 13, 512, 64, 1, L64, shift=True, y_f32=1),          # vq `enc` at a tail size
    _c("t64-n192", "conv", 2, 9, 13, 32, 192, 9, L64, **BN),                               # three N tiles of the 128x64 instance
    # outc at W = 100: the streaming and halo-patch kernels refuse; 3 of 32 columns stored, NCHW, tanh, squared error
    _c("t32-outc-100x100", "conv", 2, 100, 100, 64, 32, 9, L32, n_true=3, shift=True, act=ACT_TANH, y_f32=1, nchw=True, sq=True),
    _c("t32-outc-36x52", "conv", 3, 36, 52, 64, 32, 9, L32, n_true=2, shift=True, act=ACT_TANH, y_f32=1, nchw=True, sq=True),
    # ---- M tails and thin images ------------------------------------------------------------------------------------------
    _c("tail-w1", "conv", 5, 37, 1, 32, 64, 9, L64, **BN),
    _c("tail-h1", "conv", 3, 1, 45, 32, 128, 9, L128, **BN),
    _c("tail-27x21-b7", "conv", 7, 27, 21, 32, 128, 9, L128, **BN, x_slice=True, y_slice=True),   # both ends channel slices
    # ---- channel padding ----------------------------------------------------------------------------------------------------
    _c("cin8-of-3", "conv", 2, 25, 25, 8, 64, 9, L64, c_true=3, **BN),                     # K = 72 -> Kpad 96
    _c("cin16-of-12", "conv", 2, 36, 52, 16, 64, 9, L64, c_true=12, **BN),                 # inc.0 of the network
    _c("cin512-k4608", "conv", 1, 16, 16, 512, 512, 9, L128, **BN, res="s16"),             # the 16x16 level at batch 1, no workspace
    # ---- gather modes -------------------------------------------------------------------------------------------------------
    _c("3x3-stride2", "conv", 2, 13, 9, 64, 128, 9, L128, x_step=2, shift=True, act=ACT_LRELU),      # FlowNet2-SD conv1 .. conv6
    _c("4x4-stride1", "conv", 2, 14, 10, 64, 128, 16, L128, shift=True, act=ACT_LRELU),             # PixelDiscriminator, halo 2
    _c("4x4-stride2", "conv", 2, 14, 10, 8, 64, 16, L64, c_true=3, x_step=2, shift=True, act=ACT_LRELU),
    _c("4x4-head-nchw", "conv", 2, 11, 7, 64, 32, 16, L32, n_true=1, shift=True, y_f32=1, nchw=True),  # the discriminator's head
    _c("1x1-dec-res", "conv", 2, 9, 13, 128, 512, 1, L128, shift=True, res="s16"),          # vq `dec` + `out += x`
    # ---- up = 2 -------------------------------------------------------------------------------------------------------------
    _c("up-slice-s16", "up", 2, 13, 9, 128, 256, 1, L128, shift=True),                       # into the upper slice, S16 out
    _c("up-slice-f32out", "up", 2, 13, 9, 128, 256, 1, L128, shift=True, y_f32=1),           # training: fp32 output
    _c("up-odd-crop", "up", 2, 12, 12, 64, 128, 1, L128, shift=True, skip_hw=(25, 25)),      # 24x24 into 25x25
    # ---- input gradients (y_f32, per-column power-of-two scale, fp32 residual) ------------------------------------------
    _c("dgrad3-64to12", "dgrad3", 2, 25, 25, 64, 64, 9, L64, n_true=12, scale="pow2", res="f32", y_f32=1),
    _c("dgrad3-128to64", "dgrad3", 3, 9, 13, 128, 64, 9, L64, scale="pow2", res="f32", y_f32=1),
    _c("dgrad1-enc", "dgrad1", 2, 9, 13, 64, 512, 1, L128, scale="pow2", res="f32", y_f32=1),
    _c("dgradT-convt", "dgradT", 2, 13, 9, 64, 128, 4, L128, x_step=2, scale="pow2", res="f32", y_f32=1),
    _c("dgrad4-stride1", "dgrad4", 2, 13, 9, 64, 64, 16, L64, n_true=32, scale="pow2", y_f32=1, stride=1),
    _c("dgrad4-stride2", "dgrad4", 2, 13, 10, 64, 64, 4, L64, n_true=32, scale="pow2", y_f32=1, stride=2),
    _c("dgrad4-stride2-nchw", "dgrad4", 2, 12, 9, 64, 32, 4, L32, n_true=3, scale="pow2", y_f32=1, stride=2, nchw=True),
    _c("deconv4-parity", "dgrad4", 2, 14, 10, 64, 64, 4, L64, n_true=64, shift=True, y_f32=0, stride=2, pad=1),   # FlowNet2-SD deconv
    # ---- the overflow flag --------------------------------------------------------------------------------------------------
    _c("overflow-flag", "conv", 1, 9, 13, 32, 64, 9, L64, scale="bn", shift=True, overflow=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def _ksize(c):
    return {9: 3, 16: 4, 1: 1, 4: 2}[c.ntaps]


def x_geom(c: Case):
    """(channels, height, width, halo) of the logical x tensor"""
    ct = c.c_true or c.cin
    if c.kind == "conv":
        k, s = _ksize(c), c.x_step
        pad = {3: 1, 4: 2, 1: 0}[k]
        if s == 1:
            return ct, c.H + k - 1 - 2 * pad, c.W + k - 1 - 2 * pad, pad
        return (ct, 2 * c.H, 2 * c.W, 1) if k == 3 else (ct, 2 * c.H - 2, 2 * c.W - 2, 2)
    if c.kind in ("up", "dgrad1"):
        return ct, c.H, c.W, 0
    if c.kind == "dgrad3":
        return ct, c.H, c.W, 1
    if c.kind == "dgradT":
        return ct, 2 * c.H, 2 * c.W, 0
    if c.stride == 1:                                   # dgrad4: x = the gradient of the 4x4 conv's output
        return ct, c.H + 1, c.W + 1, 1
    return (ct, c.H // 2 + 1, c.W // 2 + 1, 1) if c.pad == 2 else (ct, c.H // 2, c.W // 2, 1)


def out_geom(c: Case):
    """(channels per pixel, height, width) of the output tensor and the (height, width) the kernel fills"""
    nt = c.n_true or c.n
    if c.kind == "up":
        co = c.n // 4
        hw = c.skip_hw or (2 * c.H, 2 * c.W)
        return co, hw[0], hw[1], 2 * c.H, 2 * c.W
    ch = nt if c.nchw else c.n
    return ch, c.H, c.W, c.H, c.W


def w_shape(c: Case):
    ct, nt = c.c_true or c.cin, c.n_true or c.n
    if c.kind == "conv":
        return (nt, ct, _ksize(c), _ksize(c))
    if c.kind == "up":
        return (ct, c.n // 4, 2, 2)                     # ConvTranspose2d IOHW
    if c.kind == "dgrad3":
        return (ct, nt, 3, 3)                           # the conv whose gradient this is: OIHW, O = channels of dY
    if c.kind == "dgrad1":
        return (ct, nt, 1, 1)
    if c.kind == "dgradT":
        return (nt, ct, 2, 2)                           # ConvTranspose IOHW: I = layer input = what the gradient goes to
    return (ct, nt, 4, 4)


def phases(c: Case):
    """launches of the case: (phase index, py, px, height, width, x offset in pixels (dy, dx) from the window corner)"""
    if c.kind != "dgrad4" or c.stride == 1:
        return [(0, 0, 0, c.H, c.W, 0, 0)]
    out = []
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        hh, ww = (c.H - py + 1) // 2, (c.W - px + 1) // 2
        # output q = 2 i + p reads g[(q + pad - r) / 2] for r = r0, r0 + 2 (r0 = (p + pad) % 2): window origin i + off
        oy = (py + c.pad - (py + c.pad) % 2 - 2) // 2
        ox = (px + c.pad - (px + c.pad) % 2 - 2) // 2
        out.append((ph, py, px, hh, ww, oy, ox))
    return out


# ---- operands and references ------------------------------------------------------------------------------------------------
class Ops:
    pass


def host_ops(c: Case) -> Ops:
    o = Ops()
    ct, hx, wx, _ = x_geom(c)
    t = "cg-" + c.name
    o.x = S.hashed_uniform(t + "x", (c.B, ct, hx, wx))
    ws = w_shape(c)
    fan = ws[1] * ws[2] * ws[3] if c.kind in ("conv",) else ws[0] * ws[2] * ws[3]
    o.w = S.hashed_uniform(t + "w", ws) * (2.0 / fan) ** 0.5
    o.scale = o.shift = o.res = o.target = None
    if c.scale == "bn":
        o.scale = S.hashed_uniform(t + "s", (c.n,), 0.7, 1.3)
    elif c.scale == "pow2":
        o.scale = torch.tensor([2.0 ** -(3 + i % 3) for i in range(c.n)])
        o.x = o.x * 16.0                                # a gradient rescaled by a power of two, undone per column
    if c.shift:
        o.shift = S.hashed_uniform(t + "b", (c.n,), -0.2, 0.2)
        if c.kind == "up":                              # the same bias for each of the four (dy, dx) groups
            o.shift = o.shift[:c.n // 4].repeat(4).contiguous()
        if c.n_true:
            o.shift[c.n_true:] = 0
    if c.overflow:
        o.shift[5] = 1.0e5
    if c.res != "none":
        o.res = S.hashed_uniform(t + "r", (c.B, c.n, c.H, c.W))
    if c.sq:
        o.target = S.hashed_uniform(t + "t", (c.B, c.n_true, c.H, c.W))
    return o


def s16_round(t: torch.Tensor) -> torch.Tensor:
    """what an fp32 tensor decodes to after the S16 split (ammc_common.h ammc_s16_split2): hi = half(v), lo = half((v - hi) 2^11)"""
    t = t.float()
    hi = t.half().float()
    lo = ((t - hi) * 2048.0).half().float()
    return hi + lo / 2048.0


def hi_only(t: torch.Tensor) -> torch.Tensor:
    return t.float().half().float()


def reference(c: Case, o: Ops, dtype, x=None, w=None, res=None):
    """the case's operation on the given operands in `dtype`: [B, channels, H, W] of the output tensor (out_geom)"""
    x = (o.x if x is None else x).to(dtype)
    w = (o.w if w is None else w).to(dtype)
    res = o.res if res is None else res
    ct, nt = c.c_true or c.cin, c.n_true or c.n
    if c.kind == "conv":
        y = F.conv2d(x, w, stride=c.x_step, padding={3: 1, 4: 2, 1: 0}[_ksize(c)])
    elif c.kind == "up":
        y = F.conv_transpose2d(x, w, stride=2)
    elif c.kind == "dgrad3":
        y = torch.nn.grad.conv2d_input((c.B, nt, c.H, c.W), w, x, padding=1)
    elif c.kind == "dgrad1":
        y = torch.nn.grad.conv2d_input((c.B, nt, c.H, c.W), w, x)
    elif c.kind == "dgradT":
        inp = torch.zeros(c.B, nt, c.H, c.W, dtype=dtype, requires_grad=True)
        (F.conv_transpose2d(inp, w, stride=2) * x).sum().backward()
        y = inp.grad
    else:
        y = torch.nn.grad.conv2d_input((c.B, nt, c.H, c.W), w, x, stride=c.stride, padding=c.pad)
    assert tuple(y.shape[2:]) == ((2 * c.H, 2 * c.W) if c.kind == "up" else (c.H, c.W)), (c.name, y.shape)
    if c.kind == "up":
        co = c.n // 4
        if o.shift is not None:
            y = y + o.shift[:co].to(dtype).view(1, -1, 1, 1)
        ch, ho, wo, _, _ = out_geom(c)
        full = torch.zeros(c.B, co, ho, wo, dtype=dtype)            # the pad row / column of an odd crop stays zero
        full[:, :, :2 * c.H, :2 * c.W] = y
        return full
    if y.shape[1] < c.n:                                            # zero filter rows up to n
        y = torch.cat([y, torch.zeros(c.B, c.n - y.shape[1], c.H, c.W, dtype=dtype)], 1)
    if o.scale is not None:
        y = y * o.scale.to(dtype).view(1, -1, 1, 1)
    if o.shift is not None:
        y = y + o.shift.to(dtype).view(1, -1, 1, 1)
    if c.act == ACT_RELU:
        y = y.clamp_min(0)
    elif c.act == ACT_LRELU:
        y = torch.where(y > 0, y, 0.1 * y)
    elif c.act == ACT_TANH:
        y = torch.tanh(y)
    if res is not None:
        y = y + res.to(dtype)
    return y[:, :nt] if c.nchw else y


def compare_mask(c: Case, want: torch.Tensor) -> torch.Tensor:
    """elements that take part in the comparison: everything, except the column the overflow case pushes out of range"""
    m = torch.ones_like(want, dtype=torch.bool)
    if c.overflow:
        m[:, 5] = False
    return m


def rel_err(got: torch.Tensor, want: torch.Tensor, mask=None) -> float:
    got, want = got.double(), want.double()
    if mask is not None:
        got, want = got[mask], want[mask]
    return float((got - want).abs().max() / want.abs().max())


def host_half(c: Case) -> dict:
    """everything of a case that needs no device: operands, the fp64 truth of the S16-rounded and of the fp32 operands,
    the witness error of torch's own fp32 evaluation, and the sensitivity of the S16 truth to x's lo halves"""
    o = host_ops(c)
    xr, wr = s16_round(o.x), s16_round(o.w)
    rr = s16_round(o.res) if (o.res is not None and c.res == "s16") else o.res
    want = reference(c, o, torch.float64, xr, wr, rr)
    want_hi = reference(c, o, torch.float64, hi_only(o.x), wr, rr)
    m = compare_mask(c, want)
    sens = rel_err(want_hi, want, m)
    want32 = reference(c, o, torch.float64)
    wit = reference(c, o, torch.float32)
    return dict(ops=o, want_s16=want, sens=sens, want_f32=want32, e_witness=rel_err(wit, want32, m))


# ---- descriptors --------------------------------------------------------------------------------------------------------------
class Bufs:
    pass


def _strides(hbuf, wbuf, ctot):
    return hbuf * wbuf * ctot, wbuf * ctot, ctot


def build_desc(c: Case, ph, s16: bool, xb=0x10000000, wb=0x20000000, yb=0x30000000, rb=0x40000000, ws=0x50000000):
    """the descriptor of one launch of the case over buffers at the given base addresses (fake ones: the label only);
    returns (desc, layout) with the layout of the buffers the addresses assume"""
    _, py, px, hh, ww, oy, ox = ph
    ct, hx, wx, halo = x_geom(c)
    ch, ho, wo, _, _ = out_geom(c)
    lay = Bufs()
    lay.x_ctot, lay.x_off = (2 * c.cin, c.cin) if c.x_slice else (c.cin, 0)
    lay.x_shape = (c.B, hx + 2 * halo, wx + 2 * halo, lay.x_ctot)
    lay.x_halo = halo
    xbs, xrs, xps = _strides(hx + 2 * halo, wx + 2 * halo, lay.x_ctot)
    lay.x_strides = (xbs, xrs, xps)
    d = AmmcConvDesc()
    # window corner of pixel (0, 0): the buffer corner when the halo is the padding; dgrad4 moves it by its phase offset
    corner = 0
    if c.kind == "dgrad4":
        corner = (halo + oy) * xrs + (halo + ox) * xps if c.stride == 2 else 0
    d.x = xb + 4 * (corner + lay.x_off)
    d.w = wb + 4 * ph[0] * c.n * kpad(c)
    d.batch, d.height, d.width = c.B, hh, ww
    d.cin, d.ntaps, d.n, d.x_step, d.act = c.cin, c.ntaps, c.n, c.x_step, c.act
    d.up, d.cgroup = (2, c.n // 4) if c.kind == "up" else (1, c.n)
    d.x_bs, d.x_rs, d.x_ps = xbs, xrs, xps
    d.y_f32 = c.y_f32 if s16 else 0
    lay.nchw = c.nchw
    if c.nchw:
        d.n_store, d.y_cs = ch, ho * wo
        ybs, yrs, yps = ch * ho * wo, wo, 1
        lay.y_off = 0
        d.y = yb + 4 * (py * yrs + px * yps)
    else:
        sliced = c.y_slice or c.kind == "up"
        lay.y_ctot, lay.y_off = (2 * ch, ch) if sliced else (ch, 0)
        lay.y_shape = (c.B, ho + 2, wo + 2, lay.y_ctot)
        ybs, yrs, yps = _strides(ho + 2, wo + 2, lay.y_ctot)
        d.y = yb + 4 * ((1 + py) * yrs + (1 + px) * yps + lay.y_off)
    lay.y_strides = (ybs, yrs, yps)
    m2 = 2 if (c.kind == "dgrad4" and c.stride == 2) else 1
    d.y_bs, d.y_rs, d.y_ps = ybs, m2 * yrs, m2 * yps
    if c.res != "none":
        d.res = rb
        d.r_bs, d.r_rs, d.r_ps = _strides(c.H, c.W, c.n)
    d.scale, d.shift = (0x60000000 if c.scale != "none" else None), (0x61000000 if c.shift else None)
    if s16 and c.splitk:
        d.splitk_ws, d.splitk_ws_floats = ws, c.splitk
    return d, lay


def kpad(c: Case) -> int:
    return (c.ntaps * c.cin + 31) // 32 * 32


def s16_label(c: Case, ph=None) -> str:
    from ammcnet_aaai2021_amd.engine import s16_variant
    d, _ = build_desc(c, ph or phases(c)[0], True)
    if c.sq:
        d.sq_target, d.sq_acc = 0x70000000, 0x71000000
    return s16_variant(d)


# ---- the device half ------------------------------------------------------------------------------------------------------------
def _ptr(t: torch.Tensor, off: int = 0) -> int:
    return t.data_ptr() + 4 * off


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _s16_roundtrip(t: torch.Tensor) -> torch.Tensor:
    """fp32 tensor (device) -> its S16 image -> fp32 again, element by element, through the library's own kernels"""
    lib, s = _lib.load(), _stream()
    flat = torch.zeros((t.numel() + 7) // 8 * 8, device=DEV)
    flat[:t.numel()] = t.reshape(-1)
    img = torch.empty_like(flat)
    _lib.check(lib.ammc_split_rows_f32(_ptr(flat), flat.numel(), _ptr(img), s), "split")
    g = flat.numel() // 8
    back = torch.empty(8, g, device=DEV)                         # NCHW [1][8][1][g] of an NHWC [1][1][g][8] image
    _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(img), flat.numel(), flat.numel(), 8, 1, 8, 1, g, _ptr(back), s), "s16_to_nchw")
    return back.t().reshape(-1)[:t.numel()].reshape(t.shape)


def pack_weights(c: Case, w: torch.Tensor) -> torch.Tensor:
    """the fp32 GEMM filter(s) of the case, [phases][n][kpad], by the library's pack routines"""
    lib, s = _lib.load(), _stream()
    ct, nt = c.c_true or c.cin, c.n_true or c.n
    kp = kpad(c)
    w = w.to(DEV).contiguous()
    if c.kind == "conv":
        wn = torch.zeros((c.n,) + tuple(w.shape[1:]), device=DEV)
        wn[:nt] = w
        out = torch.full((c.n, kp), float("nan"), device=DEV)
        _lib.check(lib.ammc_pack_conv_weight_f32(_ptr(wn), c.n, ct, _ksize(c), c.cin, _ptr(out), s), "pack_conv")
    elif c.kind == "up":
        out = torch.full((c.n, kp), float("nan"), device=DEV)
        _lib.check(lib.ammc_pack_convt_weight_f32(_ptr(w), ct, c.n // 4, _ptr(out), s), "pack_convt")
    elif c.kind == "dgrad3":
        out = torch.full((c.n, kp), float("nan"), device=DEV)
        _lib.check(lib.ammc_pack_conv_dgrad_weight_f32(_ptr(w), ct, nt, c.cin, c.n, _ptr(out), s), "pack_dgrad")
    elif c.kind == "dgrad1":
        wp = torch.empty(ct, nt, device=DEV)
        _lib.check(lib.ammc_pack_conv_weight_f32(_ptr(w), ct, nt, 1, nt, _ptr(wp), s), "pack_conv1")
        out = torch.full((c.n, kp), float("nan"), device=DEV)
        _lib.check(lib.ammc_transpose_pad_f32(_ptr(wp), ct, nt, kp, _ptr(out), s), "transpose_pad")
    elif c.kind == "dgradT":
        wp = torch.empty(4 * ct, nt, device=DEV)                  # the ConvTranspose's forward filter [4 co][cin]
        _lib.check(lib.ammc_pack_convt_weight_f32(_ptr(w), nt, ct, _ptr(wp), s), "pack_convt")
        out = torch.full((c.n, kp), float("nan"), device=DEV)
        _lib.check(lib.ammc_transpose_pad_f32(_ptr(wp), 4 * ct, nt, 4 * ct, _ptr(out), s), "transpose_pad")
    else:
        nph = 4 if c.stride == 2 else 1
        out = torch.full((nph, c.n, kp), float("nan"), device=DEV)
        _lib.check(lib.ammc_pack_conv4_dgrad_weight_f32(_ptr(w), ct, nt, c.cin, c.n, c.stride, c.pad, _ptr(out), s), "pack_conv4_dgrad")
    assert bool(torch.isfinite(out).all()), "the pack routine left part of the filter unwritten"
    return out


CANARY = 1234.5


def run_case(c: Case, o: Ops, s16: bool, splitk: bool = True):
    """pack, launch, read back.  Returns a dict: got (like reference()), the operands as the kernel saw them (x, w, res),
    sq, flag, status and the findings of the out-of-bounds checks (asserted here)."""
    lib, s = _lib.load(), _stream()
    ct, hx, wx, halo = x_geom(c)
    ch, ho, wo, fh, fw = out_geom(c)
    _, lay = build_desc(c, phases(c)[0], s16)
    r = dict(status=0)
    # ---- x ----
    xbuf = torch.zeros(lay.x_shape, device=DEV)
    xd = o.x.to(DEV).contiguous()
    pix0 = halo * (lay.x_strides[1] + lay.x_strides[2])
    if s16:
        if c.x_slice:                                             # the other slice holds large values: a read of it shows
            junk = (S.hashed_uniform("junk" + c.name, (c.B, c.cin, hx, wx)) * 100).to(DEV)
            _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(junk), c.B, c.cin, hx, wx, _ptr(xbuf, pix0), *lay.x_strides, c.cin, s), "junk")
        _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(xd), c.B, ct, hx, wx, _ptr(xbuf, pix0 + lay.x_off), *lay.x_strides, c.cin, s), "x")
        xr = torch.empty(c.B, c.cin, hx, wx, device=DEV)
        _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(xbuf, pix0 + lay.x_off), *lay.x_strides, c.B, c.cin, hx, wx, _ptr(xr), s), "x back")
        assert float(xr[:, ct:].abs().max()) == 0.0 if ct < c.cin else True
        r["x"] = xr[:, :ct].cpu()
    else:
        if c.x_slice:
            xbuf[:, halo:halo + hx, halo:halo + wx, :c.cin] = 100.0
        xbuf[:, halo:halo + hx, halo:halo + wx, lay.x_off:lay.x_off + ct] = xd.permute(0, 2, 3, 1)
        r["x"] = o.x
    # ---- w ----
    wp = pack_weights(c, o.w)
    if s16:
        w16 = torch.empty_like(wp)
        _lib.check(lib.ammc_split_rows_f32(_ptr(wp), wp.numel(), _ptr(w16), s), "split w")
        r["w"] = _s16_roundtrip(o.w.to(DEV)).cpu()               # the split is element-wise: the same values as in the image
        wdev = w16
    else:
        r["w"], wdev = o.w, wp
    # ---- epilogue operands ----
    scale = o.scale.to(DEV) if o.scale is not None else None
    shift = o.shift.to(DEV) if o.shift is not None else None
    rbuf = None
    if o.res is not None:
        rd = o.res.to(DEV).contiguous()
        rbuf = torch.zeros(c.B, c.H, c.W, c.n, device=DEV)
        if s16 and c.res == "s16":
            _lib.check(lib.ammc_nchw_to_s16_f32(_ptr(rd), c.B, c.n, c.H, c.W, _ptr(rbuf), *_strides(c.H, c.W, c.n), c.n, s), "res")
            rr = torch.empty_like(rd)
            _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(rbuf), *_strides(c.H, c.W, c.n), c.B, c.n, c.H, c.W, _ptr(rr), s), "res back")
            r["res"] = rr.cpu()
        else:
            rbuf.copy_(rd.permute(0, 2, 3, 1))
            r["res"] = o.res
    else:
        r["res"] = None
    s16_out = s16 and not c.y_f32
    if s16 and c.res == "f32":
        assert c.y_f32, "an fp32 residual needs an fp32 output"
    # ---- y ----
    tail = 256
    if c.nchw:
        ybuf = torch.full((c.B * ch * ho * wo + tail,), float("nan"), device=DEV)   # exactly the tensor + a canary tail
        ybuf[-tail:] = CANARY
    else:
        ybuf = torch.zeros(lay.y_shape, device=DEV)
        ybuf[:, 1:1 + fh, 1:1 + fw, lay.y_off:lay.y_off + ch] = float("nan")        # every element must be written
        if lay.y_off:
            other = S.hashed_uniform("other" + c.name, (c.B, ho + 2, wo + 2, ch)).to(DEV)
            ybuf[..., :lay.y_off] = other
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    sq = torch.zeros(c.B, device=DEV)
    target = o.target.to(DEV).contiguous() if o.target is not None else None
    wsb = torch.zeros(c.splitk, device=DEV) if (s16 and c.splitk and splitk) else None
    r["labels"] = []
    for ph in phases(c):
        if ph[3] <= 0 or ph[4] <= 0:
            continue
        d, _ = build_desc(c, ph, s16, xb=_ptr(xbuf), wb=_ptr(wdev), yb=_ptr(ybuf), rb=_ptr(rbuf) if rbuf is not None else 0,
                          ws=_ptr(wsb) if wsb is not None else 0)
        d.scale = _ptr(scale) if scale is not None else None
        d.shift = _ptr(shift) if shift is not None else None
        if wsb is None:
            d.splitk_ws, d.splitk_ws_floats = None, 0
        if target is not None:
            d.sq_target, d.sq_acc = _ptr(target), _ptr(sq)
        if s16:
            d.overflow_flag = flag.data_ptr()
            from ammcnet_aaai2021_amd.engine import s16_variant
            r["labels"].append(s16_variant(d))
            rc = lib.ammc_conv_gemm_s16(C.byref(d), s)
        else:
            rc = lib.ammc_conv_gemm_f32(C.byref(d), s)
        if rc != 0:
            r["status"] = rc
            return r
    torch.cuda.synchronize()
    # ---- read back + nothing outside the output was written ----
    if c.nchw:
        assert bool((ybuf[-tail:] == CANARY).all()), "written past the end of the NCHW output"
        got = ybuf[:-tail].view(c.B, ch, ho, wo).clone()
    else:
        ys = lay.y_strides
        if s16_out:
            got = torch.empty(c.B, ch, ho, wo, device=DEV)
            _lib.check(lib.ammc_s16_to_nchw_f32(_ptr(ybuf, ys[1] + ys[2] + lay.y_off), *ys, c.B, ch, ho, wo, _ptr(got), s), "y back")
        else:
            got = ybuf[:, 1:1 + ho, 1:1 + wo, lay.y_off:lay.y_off + ch].permute(0, 3, 1, 2).contiguous()
        halo_sum = ybuf[:, 0].abs().sum() + ybuf[:, -1].abs().sum() + ybuf[:, :, 0].abs().sum() + ybuf[:, :, -1].abs().sum()
        if lay.y_off:
            assert torch.equal(ybuf[..., :lay.y_off], other), "the other channel slice of the concat buffer changed"
            halo_sum = (ybuf[:, 0, :, lay.y_off:].abs().sum() + ybuf[:, -1, :, lay.y_off:].abs().sum() +
                        ybuf[:, :, 0, lay.y_off:].abs().sum() + ybuf[:, :, -1, lay.y_off:].abs().sum())
        assert float(halo_sum) == 0.0, "the output's halo was written"
        if (fh, fw) != (ho, wo):                                   # the pad row / column of the odd crop
            assert float(got[:, :, fh:].abs().sum()) == 0.0 and float(got[:, :, :, fw:].abs().sum()) == 0.0, "pad row / column written"
    r["got"] = got.cpu()
    r["sq"], r["flag"] = sq.cpu(), int(flag.item())
    return r


def device_want(c: Case, o: Ops, r: dict):
    """fp64 truth on the operands as the kernel saw them"""
    return reference(c, o, torch.float64, r["x"], r["w"], r["res"])


if __name__ == "__main__":
    # child process of the 256-row-tile test: run one S16 case under the caller's environment, save output and labels
    name, out_path = sys.argv[1], sys.argv[2]
    case = BY_NAME[name]
    res = run_case(case, host_ops(case), True)
    torch.save(dict(got=res["got"], labels=res["labels"], status=res["status"]), out_path)
