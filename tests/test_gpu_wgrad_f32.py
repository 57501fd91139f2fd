"""`ammc_conv_wgrad_f32` (csrc/wgrad_f32.hip) alone against fp64: the weight gradient of every layer form it serves -
3x3 (first layer with zero-padded channels, 64 and 512 channels, `outc`'s 32-row tile), 1x1 at the vq shapes, the
ConvTranspose form (ntaps 4, a_step 2, with the odd crop), the 4x4 window at stride 1 and 2 (PixelDiscriminator) - at
pixel counts with tails.  Reference: autograd of the fp64 operation; the packed result goes through
`ammc_unpack_conv_wgrad_f32` / `ammc_unpack_convt_wgrad_f32`.

Gate: as the fp32 convolution's (test_gpu_conv_gemm.py): torch's fp32 autograd on the CPU is the witness, e_hip <= 3
e_witness.  Measured figures: DESIGN.md section 7.  The entry accumulates with fp32 atomics into a caller-zeroed buffer:
a second launch gives twice the gradient, and padded channels / rows of the packed buffer stay exactly zero."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd._lib import AmmcWgradDesc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 3.0

# name, kind, B, H, W (pixel space of g), rows n (true), cin_p (true), a_step, skip size (convt odd crop)
CASES = [
    ("3x3-first-cin8of3", "conv3", 3, 25, 25, (64, 64), (8, 3), 1, None),
    ("3x3-cin64-n128", "conv3", 3, 25, 25, (128, 128), (64, 64), 1, None),
    ("3x3-cin512-n128", "conv3", 1, 9, 13, (128, 128), (512, 512), 1, None),
    ("3x3-outc-n32of3", "conv3", 2, 9, 13, (32, 3), (64, 64), 1, None),
    ("1x1-dec-n512-cin128", "conv1", 2, 9, 13, (512, 512), (128, 128), 1, None),
    ("1x1-enc-n32of24-cin512", "conv1", 3, 25, 25, (32, 24), (512, 512), 1, None),
    ("convt-n128-co64", "convt", 2, 13, 9, (128, 128), (64, 64), 2, None),
    ("convt-odd-crop", "convt", 2, 12, 12, (64, 64), (32, 32), 2, (25, 25)),
    ("4x4-stride1", "conv4", 2, 14, 10, (64, 64), (32, 32), 1, None),
    ("4x4-stride2-cin8of3", "conv4", 2, 14, 10, (64, 64), (8, 3), 2, None),
]


def _ptr(t, off=0):
    return t.data_ptr() + 4 * off


def _nhwc(t, cp, halo, hw=None):
    """NCHW (cpu) -> device NHWC buffer with `halo` zero pixels and channels zero-padded to cp; hw: a larger buffer"""
    B, Cc, H, W = t.shape
    bh, bw = hw or (H, W)
    buf = torch.zeros(B, bh + 2 * halo, bw + 2 * halo, cp, device=DEV)
    buf[:, halo:halo + H, halo:halo + W, :Cc] = t.to(DEV).permute(0, 2, 3, 1)
    return buf


def _strides(buf):
    return buf.shape[1] * buf.shape[2] * buf.shape[3], buf.shape[2] * buf.shape[3], buf.shape[3]


def _truth(kind, g, a, wshape, a_step, dtype):
    """dL/dw for L = sum(op(a, w) * g) in `dtype` by autograd"""
    w = torch.zeros(wshape, dtype=dtype, requires_grad=True)
    g, a = g.to(dtype), a.to(dtype)
    if kind == "conv3":
        y = F.conv2d(a, w, padding=1)
    elif kind == "conv1":
        y = F.conv2d(a, w)
    elif kind == "conv4":
        y = F.conv2d(a, w, padding=2, stride=a_step)
    else:                                    # ConvTranspose: "g" is the layer input, "a" the output gradient
        y, g, a = F.conv_transpose2d(g, w, stride=2), a, None
    (y * g).sum().backward()
    return w.grad.detach()


@pytest.mark.parametrize("name,kind,B,H,W,nn,cc,a_step,skip", CASES, ids=[c[0] for c in CASES])
def test_conv_wgrad_f32_vs_fp64(name, kind, B, H, W, nn, cc, a_step, skip):
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    (n, n_true), (cin, c_true) = nn, cc
    tag = "wg-" + name
    g = S.hashed_uniform(tag + "g", (B, n_true, H, W))
    ntaps = {"conv3": 9, "conv1": 1, "conv4": 16, "convt": 4}[kind]
    if kind == "conv3":
        a = S.hashed_uniform(tag + "a", (B, c_true, H, W))
        abuf, a_corner, wshape = _nhwc(a, cin, 1), 0, (n_true, c_true, 3, 3)
    elif kind == "conv1":
        a = S.hashed_uniform(tag + "a", (B, c_true, H, W))
        abuf, a_corner, wshape = _nhwc(a, cin, 0), 0, (n_true, c_true, 1, 1)
    elif kind == "conv4":                    # g is the OUTPUT of Conv2d(k 4, padding 2, stride a_step): a is larger / smaller
        ah, aw = (H - 1, W - 1) if a_step == 1 else (2 * H - 2, 2 * W - 2)
        a = S.hashed_uniform(tag + "a", (B, c_true, ah, aw))
        abuf, a_corner, wshape = _nhwc(a, cin, 2), 0, (n_true, c_true, 4, 4)
    else:                                    # a = the output gradient at twice the resolution, inside the skip-sized buffer
        a = S.hashed_uniform(tag + "a", (B, c_true, 2 * H, 2 * W))
        abuf = _nhwc(a, cin, 1, skip)
        a_corner = _strides(abuf)[1] + _strides(abuf)[2]
        wshape = (n_true, c_true, 2, 2)      # ConvTranspose2d IOHW
    gbuf = _nhwc(g, n, 1)
    kpad = (ntaps * cin + 31) // 32 * 32
    dw = torch.zeros(n, kpad, device=DEV)
    zeros = torch.zeros(1024, device=DEV)
    d = AmmcWgradDesc()
    d.g, d.a, d.dw, d.zeros = _ptr(gbuf, _strides(gbuf)[1] + _strides(gbuf)[2]), _ptr(abuf, a_corner), _ptr(dw), _ptr(zeros)
    d.batch, d.height, d.width, d.n, d.cin, d.ntaps, d.a_step = B, H, W, n, cin, ntaps, a_step
    d.g_bs, d.g_rs, d.g_ps = _strides(gbuf)
    d.a_bs, d.a_rs, d.a_ps = _strides(abuf)

    def unpack(packed):
        if kind == "convt":
            out = torch.empty(wshape, device=DEV)
            _lib.check(lib.ammc_unpack_convt_wgrad_f32(_ptr(packed), n_true, c_true, _ptr(out), s), "unpack_convt")
        else:
            out = torch.empty(wshape, device=DEV)
            _lib.check(lib.ammc_unpack_conv_wgrad_f32(_ptr(packed), n_true, c_true, wshape[2], cin, _ptr(out), s), "unpack")
        return out.cpu()

    _lib.check(lib.ammc_conv_wgrad_f32(C.byref(d), s), "wgrad")
    once_packed = dw.clone()
    once = unpack(dw)
    _lib.check(lib.ammc_conv_wgrad_f32(C.byref(d), s), "wgrad again")
    twice = unpack(dw)
    want = _truth(kind, g, a, wshape, a_step, torch.float64)
    wit = _truth(kind, g, a, wshape, a_step, torch.float32)
    scale = float(want.abs().max())
    e_hip = float((once.double() - want).abs().max()) / scale
    e_wit = float((wit.double() - want).abs().max()) / scale
    e_twice = float((twice.double() - 2 * want).abs().max()) / (2 * scale)
    print(f"wgrad_f32 {name}: e_hip {e_hip:.3e} e_witness {e_wit:.3e} ratio {e_hip / e_wit:.2f}; second launch {e_twice:.3e}")
    assert e_hip <= FACTOR * e_wit, (e_hip, e_wit)
    assert e_twice <= FACTOR * e_wit, (e_twice, e_wit)             # accumulation: twice the gradient within the gate
    # padded rows (n_true .. n) and padded channels (c_true .. cin of every tap) of the packed buffer: exactly zero
    taps = once_packed[:, :ntaps * cin].view(n, ntaps, cin)
    if kind == "convt":
        assert n == n_true and cin == c_true
    assert float(once_packed[n_true:].abs().max() if n_true < n else 0.0) == 0.0
    assert float(taps[:, :, c_true:].abs().max() if c_true < cin else 0.0) == 0.0
    assert bool(torch.isfinite(once_packed).all())
