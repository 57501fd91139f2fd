"""Inputs of the render tests (`ops.render_panels` / `ops.flow_to_rgb`, csrc/render.hip),
generated on the CPU and shared by tests/test_render_host.py, tests/test_gpu_render.py and
tests/golden/make_render_golden.py, with `harness.render_reference` of each case computed once.

The seven flow cases of the fixture tests/golden/flow_colour.npz (32 x 48 each; the fixture stores the inputs as well,
`golden_flows` only says how they were made):
  gauss     Gaussian, sigma 3                       ramp      a linear ramp, u -4 .. 5 along x, v -3 .. 3 along y
  small     Gaussian x 1e-3                         lattice   the integer lattice (x - 24, y - 16): angles on the wheel's
  unknown   Gaussian with three unknown pixels                boundaries and the +/- pi seam
            (1e9, -2e7, both)                       zeros     all zeros: must come out white
  uniform   uniform on [-1, 1) x 1 / 256
"""
import functools

import numpy as np
import torch

from ammcnet_aaai2021_amd import harness as Hn

GOLDEN_CASES = ("gauss", "ramp", "small", "lattice", "unknown", "zeros", "uniform")
GOLDEN_HW = (32, 48)
UNKNOWN_AT = ((3, 5), (17, 40), (30, 2))           # (y, x) of the `unknown` case's three pixels
# the pixels of a case that are compared with the reference's output: those whose radius lies clearly below the
# largest one (the reference dims the one or two that attain it at the whim of a float64 rounding)
COMPARE_BELOW = 1.0 - 2.0 ** -20
MAX_EXCLUDED = 2

# (B, H, W): one quad, the tail path with odd sizes, a ragged last quad on two workgroups, a batch that is a multiple of
# nothing, the evaluation batch
DEVICE_SHAPES = ((1, 8, 8), (3, 21, 27), (2, 36, 50), (17, 16, 16), (16, 64, 64))


def golden_flows() -> dict:
    """name -> fp32 [32, 48, 2] (HWC, as the reference's `flow_to_image` takes a flow)"""
    h, w = GOLDEN_HW
    g = torch.Generator().manual_seed(2021)
    gauss = (3.0 * torch.randn(h, w, 2, generator=g)).numpy()
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ramp = np.stack([-4.0 + 9.0 * xx / (w - 1), -3.0 + 6.0 * yy / (h - 1)], axis=2)
    lattice = np.stack([xx - 24.0, yy - 16.0], axis=2)
    unknown = (3.0 * torch.randn(h, w, 2, generator=g)).numpy()
    unknown[UNKNOWN_AT[0]][0] = 1e9
    unknown[UNKNOWN_AT[1]][1] = -2e7
    unknown[UNKNOWN_AT[2]] = (1e9, -2e7)
    uniform = ((torch.rand(h, w, 2, generator=g) * 2 - 1) / 256.0).numpy()
    out = {"gauss": gauss, "ramp": ramp, "small": gauss * 1e-3, "lattice": lattice, "unknown": unknown,
           "zeros": np.zeros((h, w, 2)), "uniform": uniform}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def compared(raw: np.ndarray, max_rad: float) -> np.ndarray:
    """the mask of the pixels whose colour is compared with the fixture: raw < max_rad * (1 - 2^-20), in float64 - and
    the pixels without a radius (raw == 0: white on either side of any rounding; all of the `zeros` case)"""
    raw = raw.astype(np.float64)
    return (raw < float(max_rad) * COMPARE_BELOW) | (raw == 0.0)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(rgb_pred, rgb_target, op_pred, op_target) fp32 on the CPU for (B, H, W) (shared, read-only): frames on [-1, 1]
    with a few values beyond it, flows of a few pixels with a NaN and unknown values planted in both, a zero-flow sample
    (the last one's target flow) and a `pred == target` sample (sample 0: heat_max = 0)"""
    b, h, w = shape
    g = torch.Generator().manual_seed(1000 + b * 131 + h * 17 + w)
    rgb_t = torch.rand(b, 3, h, w, generator=g) * 2.2 - 1.1
    rgb_p = (rgb_t + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(-1, 1)
    op_t = 2.0 * torch.randn(b, 2, h, w, generator=g) / 256.0
    op_p = op_t + 0.3 * torch.randn(b, 2, h, w, generator=g) / 256.0
    op_t[b - 1] = 0.0                                        # a zero flow: white
    rgb_p[0], op_p[0] = rgb_t[0], op_t[0]                    # nothing to show: heat_max = 0
    s = b // 2                                               # (sample 0 where b == 1: its flows then differ in the planted pixels only)
    op_t[s, 0, h // 2, w // 3] = float("nan")
    op_t[s, 1, 0, w - 1] = 1e9
    op_p[s, 0, h - 1, 0] = -3e8
    op_p[s, 1, h // 3, w // 2] = float("nan")
    return rgb_p, rgb_t, op_p, op_t


FLOW_SCALE = (1.0, 1.0)


@functools.lru_cache(maxsize=None)
def reference(shape, flow_norm="target"):
    """`harness.render_reference` of `inputs(shape)` with the default tiles (CPU; shared, read-only)"""
    return Hn.render_reference(*inputs(shape), flow_scale=FLOW_SCALE, flow_norm=flow_norm)
