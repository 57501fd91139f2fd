"""The definitions of the fused localisation maps (include/ammc_hip.h) restated as plain loops over
pixels and windows in float64, the case list of the kernel tests and the error bounds derived from a case.  Nothing here
shares code with `harness.fuse_maps_reference`, `harness.fuse_coefficients` or the kernel."""
import numpy as np

FRAME_SIZES = ((8, 8), (17, 23), (40, 72), (64, 64))     # below a tile; odd, a clamped 2 x 2 coarse grid; two tiles across, two down;
BATCH = 3                                                #   whole patches
CELLS = (1, 1, 8, 8)
RADII = (0, 1, 4)                                        # radius 4 at 8 x 8 clips the window on both sides
PATCHES = (8, 16, 32)
U = 2.0 ** -24                                           # the unit roundoff of fp32


def grid_shape(h, w, cell):
    """the coarse grid of a channel: floor(h / cell) x floor(w / cell), at least 1 x 1 (17 x 23 in cells of 8: 2 x 2, whose
    last row and column also serve the pixels beyond 16 by clamping)"""
    return max(1, h // cell), max(1, w // cell)


def kernel_cases():
    """(h, w, n_ch): every frame size with 1..4 channels; each runs every radius and patch"""
    return [(h, w, n_ch) for h, w in FRAME_SIZES for n_ch in (1, 2, 3, 4)]


def make_sources(h, w, n_ch, batch=BATCH, tag="fuse"):
    """non-negative fp32 sources [batch, gh_c, gw_c] from `synthetic.hashed_uniform` and coefficients in [0.25, 1.25)"""
    from ammcnet_aaai2021_amd import synthetic
    src = [synthetic.hashed_uniform(f"{tag}:{h}x{w}:src{c}", (batch,) + grid_shape(h, w, CELLS[c]), 0, 1).numpy().astype(np.float32)
           for c in range(n_ch)]
    coef = (0.25 + synthetic.hashed_uniform(f"{tag}:{h}x{w}:coef", (n_ch,), 0, 1).numpy()).astype(np.float32)
    return src, coef


def expand(src, cell, h, w):
    """[B, gh, gw] -> [B, h, w]: pixel (y, x) reads cell (min(y // cell, gh - 1), min(x // cell, gw - 1))"""
    b, gh, gw = src.shape
    out = np.empty((b, h, w), dtype=np.float64)
    for y in range(h):
        for x in range(w):
            out[:, y, x] = src[:, min(y // cell, gh - 1), min(x // cell, gw - 1)]
    return out


def fuse_loops(sources, cells, coef, radius, patch, h, w):
    """raw, pixel, patch_mean and frame_max in float64, by loops over pixels, windows and patches"""
    b = sources[0].shape[0]
    raw = np.zeros((b, h, w), dtype=np.float64)
    for c, (s, cell) in enumerate(zip(sources, cells)):
        raw += float(coef[c]) * expand(np.asarray(s, dtype=np.float64), cell, h, w)
    pixel = np.empty_like(raw)
    for y in range(h):
        for x in range(w):
            total, n = np.zeros(b), 0
            for yy in range(y - radius, y + radius + 1):
                for xx in range(x - radius, x + radius + 1):
                    if 0 <= yy < h and 0 <= xx < w:
                        total += raw[:, yy, xx]
                        n += 1
            pixel[:, y, x] = total / n
    return {"raw": raw, "pixel": pixel, "patch_mean": patch_means(pixel, patch), "frame_max": pixel.reshape(b, -1).max(axis=1)}


def patch_means(pixel, patch):
    """float64 means of `pixel` [B, h, w] over the patch grid anchored at (0, 0), the last row / column ragged"""
    b, h, w = pixel.shape
    ph, pw = -(-h // patch), -(-w // patch)
    out = np.empty((b, ph, pw), dtype=np.float64)
    for i in range(ph):
        for j in range(pw):
            out[:, i, j] = np.asarray(pixel[:, i * patch:(i + 1) * patch, j * patch:(j + 1) * patch], dtype=np.float64).mean(axis=(1, 2))
    return out


def patch_counts(h, w, patch):
    ph, pw = -(-h // patch), -(-w // patch)
    rows = np.minimum(patch, h - patch * np.arange(ph))
    cols = np.minimum(patch, w - patch * np.arange(pw))
    return rows[:, None] * cols[None, :]


def pixel_bound(n_ch, radius):
    """relative, per element: one rounding per product (n_ch), per add of raw and of the window (< n_ch + (2 r + 1)^2) and
    one for the division; every term is non-negative, so the bound is relative"""
    return 1.01 * (2 * n_ch + (2 * radius + 1) ** 2) * U


def patch_bound(h, w, patch):
    """relative, per patch: rows * cols - 1 adds and the division, + 1"""
    return 1.01 * (patch_counts(h, w, patch) + 1) * U


def coefficients(weights, maxima, normalise, scales=None):
    """`harness.fuse_coefficients` in numpy fp32: "video" w / max (one fp32 division), 0 where max == 0; "none" w * scale"""
    w = np.asarray(weights, dtype=np.float32)
    if normalise == "video":
        mx = np.asarray(maxima, dtype=np.float32)
        out = np.zeros_like(w)
        for c in range(w.size):
            if mx[c] != 0:
                out[c] = np.float32(w[c]) / np.float32(mx[c])
        return out
    sc = np.ones_like(w) if scales is None else np.asarray(scales, dtype=np.float32)
    return (w * sc).astype(np.float32)


def torch_sources(src, device):
    import torch
    return [torch.tensor(s, device=device) for s in src]
