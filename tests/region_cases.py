"""The region-based criterion restated in numpy and plain Python (definitions in
include/ammc_hip.h), and the cases tests/test_region_scores_host.py and tests/test_gpu_region_scores.py share.

  flood_label      connected components by breadth-first flood fill, numbered in raster order of their first pixel
  label_regions    what `ammc_label_regions_u8` returns for one mask: (labels uint8, count)
  matches          the match rule in Python integers
  scores           what `ammc_region_scores_f32` returns for one sample: a loop over components and regions
  curve_area       the area of `harness.region_curve_area` in exact rationals
  tracks           the track ids of `harness.region_tracks` by brute force
  pictures, smooth_maps, rectangles   the cases
"""
from collections import deque
from fractions import Fraction

import numpy as np

MAX_REGIONS = 32


def flood_label(fg: np.ndarray, connectivity: int = 8):
    """fg bool [h, w] -> (comp int32 [h, w]: 0 background, 1.. in raster order of each component's first pixel, sizes)"""
    h, w = fg.shape
    comp = np.zeros((h, w), dtype=np.int32)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    sizes = []
    fgl = fg.tolist()
    for y0 in range(h):
        for x0 in range(w):
            if not fgl[y0][x0] or comp[y0, x0]:
                continue
            cid = len(sizes) + 1
            comp[y0, x0] = cid
            queue, size = deque([(y0, x0)]), 0
            while queue:
                y, x = queue.popleft()
                size += 1
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and fgl[yy][xx] and not comp[yy, xx]:
                        comp[yy, xx] = cid
                        queue.append((yy, xx))
            sizes.append(size)
    return comp, sizes


def label_regions(mask: np.ndarray, min_area: int = 1, connectivity: int = 8):
    """mask [h, w] -> (labels uint8 [h, w] with the kept components 1..32 in raster order, beyond 32 as 0; the true count)"""
    comp, sizes = flood_label(mask != 0, connectivity)
    rank, count = [0], 0
    for s in sizes:
        if s >= min_area:
            count += 1
            rank.append(count if count <= MAX_REGIONS else 0)
        else:
            rank.append(0)
    return np.asarray(rank, dtype=np.uint8)[comp], count


def matches(c: int, g: int, inter: int, num: int, den: int) -> bool:
    return int(inter) * int(den) >= int(num) * (int(c) + int(g) - int(inter))


def scores(amap: np.ndarray, labels: np.ndarray, thresholds, num: int = 1, den: int = 10, min_area: int = 1, connectivity: int = 8):
    """one sample -> {n_px, n_comp, n_fp, hit}: int32 [T]"""
    thresholds = np.asarray(thresholds, dtype=np.float32)
    out = {k: np.zeros(len(thresholds), dtype=np.int32) for k in ("n_px", "n_comp", "n_fp", "hit")}
    lab = np.where(labels > MAX_REGIONS, 0, labels).astype(np.int64).ravel()
    gsize = np.bincount(lab, minlength=MAX_REGIONS + 1).tolist()
    for j, t in enumerate(thresholds):
        with np.errstate(invalid="ignore"):
            fg = amap >= t
        comp, sizes = flood_label(fg, connectivity)
        flat = comp.ravel()
        n_comp = n_fp = hit = 0
        for c, size in enumerate(sizes, start=1):
            if size < min_area:
                continue
            n_comp += 1
            inter = np.bincount(lab[flat == c], minlength=MAX_REGIONS + 1).tolist()
            matched = False
            for r in range(1, MAX_REGIONS + 1):
                if gsize[r] and inter[r] and matches(size, gsize[r], inter[r], num, den):
                    matched = True
                    hit |= 1 << (r - 1)
            n_fp += not matched
        out["n_px"][j], out["n_comp"][j], out["n_fp"][j] = int(fg.sum()), n_comp, n_fp
        out["hit"][j] = np.array(hit, dtype=np.uint32).view(np.int32)
    return out


def batch_scores(maps, labels, thresholds, **kw):
    rows = [scores(a, k, thresholds, **kw) for a, k in zip(maps, labels)]
    return {key: np.stack([r[key] for r in rows]) for key in rows[0]}


def curve_area(fpr, rate) -> Fraction:
    """the area as the definitions give it, in exact rationals of the floats"""
    pts = {}
    for x, y in zip(fpr, rate):
        x, y = Fraction(float(x)), Fraction(float(y))
        pts[x] = max(pts.get(x, y), y)
    pts.setdefault(Fraction(0), Fraction(0))
    xs = sorted(pts)
    line = [(x, pts[x]) for x in xs]
    if xs[-1] < 1:
        line.append((Fraction(1), line[-1][1]))
    area = Fraction(0)
    for (x0, y0), (x1, y1) in zip(line, line[1:]):
        if x0 >= 1:
            break
        if x1 > 1:
            y1 = y0 + (y1 - y0) * (1 - x0) / (x1 - x0)
            x1 = Fraction(1)
        area += (x1 - x0) * (y0 + y1) / 2
    return area


def tracks(labels_per_frame):
    """-> (ids per frame [count_f], n): regions as graph nodes, an edge where regions of consecutive frames share a pixel,
    components by repeated relabelling to the smallest node; ids in order of first appearance"""
    frames = [np.asarray(f) for f in labels_per_frame]
    nodes = [(f, r) for f, img in enumerate(frames) for r in range(1, int(img.max()) + 1 if img.size else 1)]
    comp = {nd: i for i, nd in enumerate(nodes)}
    edges = []
    for f in range(len(frames) - 1):
        for ra in range(1, int(frames[f].max()) + 1):
            for rb in range(1, int(frames[f + 1].max()) + 1):
                if ((frames[f] == ra) & (frames[f + 1] == rb)).any():
                    edges.append(((f, ra), (f + 1, rb)))
    changed = True
    while changed:
        changed = False
        for a, b in edges:
            lo = min(comp[a], comp[b])
            if comp[a] != lo or comp[b] != lo:
                comp[a] = comp[b] = lo
                changed = True
    ids, out = {}, [[] for _ in frames]
    for nd in nodes:
        out[nd[0]].append(ids.setdefault(comp[nd], len(ids)))
    return [np.asarray(o, dtype=np.int64) for o in out], len(ids)


# ---- cases --------------------------------------------------------------------------------------------------------------

def _spiral(n: int) -> np.ndarray:
    """a one-pixel-wide spiral with one-pixel gaps on an n x n grid: one component, the longest chain of equivalences"""
    img = np.zeros((n, n), dtype=bool)
    y0, y1, x0, x1 = 0, n - 1, 0, n - 1
    y = x = 0
    img[0, 0] = True
    while True:
        moved = False
        for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            while y0 <= y + dy <= y1 and x0 <= x + dx <= x1 and not img[y + dy, x + dx]:
                # stop one short of touching an earlier arm
                ny, nx = y + 2 * dy, x + 2 * dx
                if 0 <= ny < n and 0 <= nx < n and img[ny, nx]:
                    break
                y, x = y + dy, x + dx
                img[y, x] = True
                moved = True
        if not moved:
            return img


def pictures() -> dict:
    """name -> bool [h, w]: the shapes at which labelling can go wrong"""
    rng = np.random.default_rng(24)
    out = {}
    for h, w in ((1, 1), (1, 7), (7, 1), (5, 3), (17, 23), (33, 31)):
        out[f"random_{h}x{w}"] = rng.random((h, w)) < 0.55
    out["one_1x1"] = np.ones((1, 1), dtype=bool)
    yy, xx = np.mgrid[0:8, 0:8]
    out["checkerboard"] = (yy + xx) % 2 == 0                    # 32 components under 4-connectivity, 1 under 8
    out["spiral"] = _spiral(16)
    r, c = np.mgrid[0:16, 0:16]
    out["serpentine"] = (r % 2 == 0) | (c == np.where(r % 4 == 1, 15, 0))
    out["u"] = ((c == 2) | (c == 13) | (r == 15)) & (c >= 2) & (c <= 13)
    out["comb"] = (c % 2 == 0) | (r == 15)                      # teeth that merge only in the last row
    out["diagonal_blobs"] = ((r < 8) & (c < 8)) | ((r >= 8) & (c >= 8))
    out["empty"] = np.zeros((16, 16), dtype=bool)
    out["full"] = np.ones((16, 16), dtype=bool)
    out["ring"] = (r == 0) | (c == 0) | (r == 15) | (c == 15)
    cells = [(y, x) for y in range(0, 33, 2) for x in range(0, 31, 2)]
    for k in (32, 33):                                          # 32 and 33 single pixels: the last region and one too many
        img = np.zeros((33, 31), dtype=bool)
        for y, x in cells[:k]:
            img[y, x] = True
        out[f"dots_{k}"] = img
    return out


def smooth_maps(b: int, h: int, w: int, cell: int, seed: int = 0) -> np.ndarray:
    """fp32 [b, h, w] in [0, 1): random values on a grid of `cell`-pixel cells, bilinearly interpolated - about
    (h / cell) * (w / cell) / 8 components at a mid threshold"""
    rng = np.random.default_rng(seed)
    gh, gw = h // cell + 2, w // cell + 2
    g = rng.random((b, gh, gw))
    ys, xs = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
    a = g[:, y0][:, :, x0] * (1 - fy) * (1 - fx) + g[:, y0 + 1][:, :, x0] * fy * (1 - fx) + \
        g[:, y0][:, :, x0 + 1] * (1 - fy) * fx + g[:, y0 + 1][:, :, x0 + 1] * fy * fx
    return np.ascontiguousarray(a, dtype=np.float32)


def rectangles(b: int, h: int, w: int, k: int = 3, seed: int = 1) -> np.ndarray:
    """uint8 [b, h, w]: k rectangles of ones per sample"""
    rng = np.random.default_rng(seed)
    out = np.zeros((b, h, w), dtype=np.uint8)
    for i in range(b):
        for _ in range(k):
            rh, rw = rng.integers(1, max(2, h // 3)), rng.integers(1, max(2, w // 3))
            y0, x0 = rng.integers(0, h - rh + 1), rng.integers(0, w - rw + 1)
            out[i, y0:y0 + rh, x0:x0 + rw] = 1
    return out
