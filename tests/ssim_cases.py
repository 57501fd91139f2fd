"""Inputs of the SSIM tests (`ops.ssim`, csrc/ssim.hip), generated on the CPU and shared by
tests/test_ssim_host.py, tests/test_gpu_ssim.py and tests/golden/make_ssim_golden.py, with the float64 reference and the
two fp32 witnesses of each case computed once.

Four seeded recipes.  Flat mid-grey regions are avoided on purpose: there both means are near 0 and the variance is 0, the
denominator falls toward C1 * C2 = 9e-8 and fp32 SSIM is rounding noise for the reference as well.
  random   pred = tanh of normals, target uniform on [-1, 1]: SSIM near 0, the map goes negative
  close    target = a 9 x 9 box-blurred uniform field times 3, clamped to [-1, 1]; pred = target + 0.02 sigma of noise,
           clamped: SSIM about 0.97, the regime of a trained model
  smooth   the same target with 0.05 sigma of noise: SSIM about 0.87
  planted  `random` with pred == target inside a PLANT x PLANT block of sample 0 (frames of at least PLANT x PLANT)
"""
import functools

import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import harness as Hn, ops

RECIPES = ("random", "close", "smooth", "planted")
PLANT = 24
NOISE = {"close": 0.02, "smooth": 0.05}
# what the fixture tests/golden/ssim_reference.npz was recorded on: one small shape per recipe
FIXTURE_CASES = (("random", 11, (2, 3, 27, 21)), ("close", 12, (2, 3, 40, 36)), ("smooth", 13, (2, 2, 33, 40)),
                 ("planted", 14, (2, 3, 40, 44)))


def plant_origin(h: int, w: int):
    return (h - PLANT) // 2, (w - PLANT) // 2


@functools.lru_cache(maxsize=None)
def inputs(recipe: str, seed: int, shape):
    """(pred, target) fp32 on the CPU (shared, read-only)"""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    if recipe in ("random", "planted"):
        pred = torch.tanh(torch.randn(b, c, h, w, generator=g))
        target = torch.rand(b, c, h, w, generator=g) * 2 - 1
        if recipe == "planted":
            assert h >= PLANT and w >= PLANT
            y, x = plant_origin(h, w)
            pred[0, :, y:y + PLANT, x:x + PLANT] = target[0, :, y:y + PLANT, x:x + PLANT]
        return pred, target
    field = torch.rand(b, c, h, w, generator=g) * 2 - 1
    target = (3.0 * F.avg_pool2d(field, 9, stride=1, padding=4)).clamp(-1, 1)
    pred = (target + NOISE[recipe] * torch.randn(b, c, h, w, generator=g)).clamp(-1, 1)
    return pred, target


@functools.lru_cache(maxsize=None)
def reference(recipe: str, seed: int, shape):
    """`harness.ssim_reference` in float64: the truth (CPU; shared, read-only)"""
    return Hn.ssim_reference(*inputs(recipe, seed, shape))


def separable_fp32(pred: torch.Tensor, target: torch.Tensor):
    """the definition of include/ammc_hip.h restated in fp32 with plain torch: zero padding, the row pass over the 11
    taps and then the column pass, each a running sum in tap order (rounded products and adds; the kernel's chains are
    fused) -> {"map_c", "map", "ssim_c", "ssim"}"""
    win = ops.ssim_window()
    b, c, h, w = pred.shape

    def G(f):
        p = F.pad(f, (5, 5, 5, 5))
        rows = torch.zeros(b, c, h + 10, w)
        for k in range(11):
            rows = rows + win[k] * p[..., k:k + w]
        out = torch.zeros(b, c, h, w)
        for k in range(11):
            out = out + win[k] * rows[..., k:k + h, :]
        return out
    mu1, mu2 = G(pred), G(target)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = G(pred * pred) - m11, G(target * target) - m22, G(pred * target) - m12
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    map_c = ((2 * m12 + c1) * (2 * s12 + c2)) / ((m11 + m22 + c1) * (s1 + s2 + c2))
    ssim_c = map_c.mean(dim=(2, 3))
    return {"map_c": map_c, "map": map_c.mean(1), "ssim_c": ssim_c, "ssim": ssim_c.mean(1)}


@functools.lru_cache(maxsize=None)
def witnesses(recipe: str, seed: int, shape):
    """the two fp32 witnesses on the same tensors: the reference's own arithmetic (`ssim_reference(dtype=float32)`) and
    the separable restatement"""
    pred, target = inputs(recipe, seed, shape)
    return Hn.ssim_reference(pred, target, dtype=torch.float32), separable_fp32(pred, target)
