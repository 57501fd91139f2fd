// Fused localisation maps: up to four score maps of different resolution become one smoothed fp32 map, its patch means
// and its largest value (the definitions are in include/ammc_hip.h).
//
//   raw(b, y, x)   = ((coef[0] * m_0 + coef[1] * m_1) + coef[2] * m_2) + coef[3] * m_3          (n_ch terms)
//   m_c            = src_c[b, min(y / cell_c, gh_c - 1), min(x / cell_c, gw_c - 1)]              (blocky expansion)
//   pixel[b, y, x] = (sum of raw over the in-frame pixels of the (2 radius + 1)^2 window) / their number
//
// One 256-thread workgroup owns a 32 x 64 tile of a sample (whole patches of 8, 16 and 32 pixels), in five phases
// that meet in LDS, each a strided loop over a task list - so the routine also runs as ONE thread on the host
// (FmHost, under AMMC_FUSE_HOST: tools/fuse_maps_host_check.cpp runs it under the host sanitizers):
//
//   1 stage   raw of the tile and its halo, (32 + 2 r) x (64 + 2 r) values, 0 outside the frame          -> raw
//   2 rows    per staged row and tile column: raw[x - r'] + ... + raw[x + r''], the in-frame columns,
//             left to right, starting FROM the first term                                              -> hs
//   3 columns a task owns a quad (4 consecutive pixels of a row): per pixel hs of the in-frame rows top to bottom,
//             then ONE division by (rows * columns in frame); 16-byte store where the layout allows; the quad's
//             sum (p0 + p1) + (p2 + p3) with 0 for pixels outside the frame                             -> qs
//             and its largest in-frame value                                                            -> tm
//   4 patch rows  per tile row and patch column: the patch / 4 quad sums, left to right                 -> rs
//   5 patches     per patch: its `patch` row sums top to bottom, / (rows * cols in frame); the tile's maximum
//
// Sums only add (no sliding-window subtraction): with non-negative inputs a pixel carries at most 2 n_ch - 1 roundings
// of raw, 4 r of the window and one of the division.  The order of every sum is a function of the pixel's (the
// patch's) position in the frame alone; nothing is atomic; tile maxima go to a workspace and a tail launch takes the
// sample's.  The maximum propagates NaN (as the sums do).  Contraction into FMAs is off.  Plain C++, vector stores.
#ifndef AMMC_FUSE_HOST
#include "ammc_common.h"
#define FM_FN __device__ __forceinline__
#else
#include <math.h>
#include <stdint.h>
#define FM_FN static inline
#endif

namespace ammc_impl {

constexpr int FM_TH = 32, FM_TW = 64;                  // the tile: multiples of the largest patch
constexpr int FM_THREADS = 256;
constexpr int FM_MAX_CH = 4, FM_MAX_RADIUS = 8;
constexpr int FM_QW = FM_TW / 4;                       // quads across a tile
constexpr int FM_QUADS = FM_TH * FM_QW;
constexpr int FM_RAW_FLOATS = (FM_TH + 2 * FM_MAX_RADIUS) * (FM_TW + 2 * FM_MAX_RADIUS);
constexpr int FM_HS_FLOATS = (FM_TH + 2 * FM_MAX_RADIUS) * FM_TW;
constexpr int FM_RS_FLOATS = FM_TH * (FM_TW / 8);
constexpr int FM_TAIL_THREADS = 64;

struct FmSrc {
  const float* p;                                      // [batch][gh][gw], samples bs floats apart
  int64_t bs;
  int gh, gw, cell, shift;                             // shift: log2(cell) where cell is a power of two, else -1
};

struct FmArgs {
  FmSrc src[FM_MAX_CH];
  const float* coef;
  int n_ch, h, w, radius, patch, ph, pw, tiles_x, tiles_y;
  float* pixel;
  int64_t px_bs;
  int px_vec;                                          // 16-byte stores: base, batch stride and w allow them
  float* patch_mean;
  int64_t pm_bs;
  float* tile_max;                                     // [batch][tiles_y * tiles_x]
};

FM_FN int fm_cell(int v, const FmSrc& s, int last) {
  const int g = s.shift >= 0 ? v >> s.shift : v / s.cell;
  return g < last ? g : last;
}

FM_FN float fm_max(float m, float v) { return (v > m || v != v) ? v : m; }     // a NaN stays

// one tile (ty, tx) of sample b; raw, hs, qs, tm, rs: the workgroup's scratch of (32 + 2 r)(64 + 2 r), (32 + 2 r) 64,
// FM_QUADS, FM_QUADS and 32 * (64 / patch) floats
template <class X>
FM_FN void fm_tile(const X& x, const FmArgs& a, int b, int ty, int tx, float* raw, float* hs, float* qs, float* tm, float* rs) {
#pragma clang fp contract(off)
  const int tid = x.tid(), nt = x.nt();
  const int r = a.radius, sw = FM_TW + 2 * r, sh = FM_TH + 2 * r;
  const int y0 = ty * FM_TH, x0 = tx * FM_TW;
  float cf[FM_MAX_CH];
#pragma unroll
  for (int c = 0; c < FM_MAX_CH; ++c) cf[c] = c < a.n_ch ? a.coef[c] : 0.f;

  // 1: task = staged row * 128 + staged column (columns >= sw idle: the decode stays a shift)
  for (int t = tid; t < sh * 128; t += nt) {
    const int sy = t >> 7, sx = t & 127;
    if (sx >= sw) continue;
    const int gy = y0 - r + sy, gx = x0 - r + sx;
    float v = 0.f;
    if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
#pragma unroll
      for (int c = 0; c < FM_MAX_CH; ++c) {
        if (c >= a.n_ch) break;
        const FmSrc& s = a.src[c];
        const float m = s.p[b * s.bs + (int64_t)fm_cell(gy, s, s.gh - 1) * s.gw + fm_cell(gx, s, s.gw - 1)];
        const float term = cf[c] * m;
        v = c == 0 ? term : v + term;
      }
    }
    raw[sy * sw + sx] = v;
  }
  x.sync();

  // 2: task = staged row * 64 + tile column
  for (int t = tid; t < sh * FM_TW; t += nt) {
    const int sy = t >> 6, lx = t & (FM_TW - 1);
    const int gx = x0 + lx;
    float acc = 0.f;
    if (gx < a.w) {
      const int lo = gx - r < 0 ? 0 : gx - r, hi = gx + r > a.w - 1 ? a.w - 1 : gx + r;
      const float* row = raw + sy * sw + (lo - (x0 - r));
      acc = row[0];
      for (int k = 1; k <= hi - lo; ++k) acc = acc + row[k];
    }
    hs[sy * FM_TW + lx] = acc;
  }
  x.sync();

  // 3: task = tile row * 16 + quad column
  for (int t = tid; t < FM_QUADS; t += nt) {
    const int ly = t >> 4, qc = t & (FM_QW - 1);
    const int gy = y0 + ly, gx = x0 + 4 * qc;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    float best = -INFINITY;
    const int n = gy < a.h ? (a.w - gx < 4 ? a.w - gx : 4) : 0;          // pixels of the quad in the frame (<= 0: none)
    if (n > 0) {
      const int lo = gy - r < 0 ? 0 : gy - r, hi = gy + r > a.h - 1 ? a.h - 1 : gy + r;
      const float* col = hs + (lo - (y0 - r)) * FM_TW + 4 * qc;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= n) break;
        const int xl = gx + k - r < 0 ? 0 : gx + k - r, xh = gx + k + r > a.w - 1 ? a.w - 1 : gx + k + r;
        float acc = col[k];
        for (int j = 1; j <= hi - lo; ++j) acc = acc + col[j * FM_TW + k];
        p[k] = acc / (float)((hi - lo + 1) * (xh - xl + 1));
        best = fm_max(best, p[k]);
      }
      float* o = a.pixel + b * a.px_bs + (int64_t)gy * a.w + gx;
      if (a.px_vec && n == 4) {
        x.st4(o, p);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) o[k] = p[k];
      }
    }
    qs[t] = (p[0] + p[1]) + (p[2] + p[3]);
    tm[t] = best;
  }
  x.sync();

  // 4: task = tile row * (patches across the tile) + patch column
  const int P = a.patch, npx = FM_TW / P, npy = FM_TH / P, qp = P / 4;
  for (int t = tid; t < FM_TH * npx; t += nt) {
    const int ly = t / npx, j = t - ly * npx;
    const float* q = qs + ly * FM_QW + j * qp;
    float acc = q[0];
    for (int k = 1; k < qp; ++k) acc = acc + q[k];
    rs[t] = acc;
  }
  // (the tile's maximum, first step: FM_TAIL_THREADS strided partial maxima, in place)
  for (int t = tid; t < FM_TAIL_THREADS; t += nt) {
    float m = tm[t];
    for (int k = t + FM_TAIL_THREADS; k < FM_QUADS; k += FM_TAIL_THREADS) m = fm_max(m, tm[k]);
    tm[t] = m;
  }
  x.sync();

  // 5: task = patch of the tile; the last task takes the tile's maximum
  for (int t = tid; t < npy * npx + 1; t += nt) {
    if (t == npy * npx) {
      float m = tm[0];
      for (int k = 1; k < FM_TAIL_THREADS; ++k) m = fm_max(m, tm[k]);
      a.tile_max[(int64_t)b * a.tiles_y * a.tiles_x + ty * a.tiles_x + tx] = m;
      continue;
    }
    const int pi = t / npx, j = t - pi * npx;
    const int gi = ty * npy + pi, gj = tx * npx + j;
    if (gi >= a.ph || gj >= a.pw) continue;
    const float* q = rs + pi * P * npx + j;
    float acc = q[0];
    for (int k = 1; k < P; ++k) acc = acc + q[k * npx];
    const int rows = a.h - gi * P < P ? a.h - gi * P : P, cols = a.w - gj * P < P ? a.w - gj * P : P;
    a.patch_mean[b * a.pm_bs + (int64_t)gi * a.pw + gj] = acc / (float)(rows * cols);
  }
}

#ifdef AMMC_FUSE_HOST

struct FmHost {                                        // one thread is the whole workgroup
  int tid() const { return 0; }
  int nt() const { return 1; }
  void sync() const {}
  void st4(float* o, const float (&p)[4]) const { for (int k = 0; k < 4; ++k) o[k] = p[k]; }
};

#else

struct FmDev {
  FM_FN int tid() const { return (int)threadIdx.x; }
  FM_FN int nt() const { return FM_THREADS; }
  FM_FN void sync() const { __syncthreads(); }
  FM_FN void st4(float* o, const float (&p)[4]) const {
    const f32x4 v = {p[0], p[1], p[2], p[3]};
    *reinterpret_cast<f32x4*>(o) = v;
  }
};

__global__ __launch_bounds__(FM_THREADS) void fuse_maps_kernel(FmArgs a) {
  __shared__ __attribute__((aligned(16))) float raw[FM_RAW_FLOATS];
  __shared__ __attribute__((aligned(16))) float hs[FM_HS_FLOATS];
  __shared__ float qs[FM_QUADS], tm[FM_QUADS], rs[FM_RS_FLOATS];
  const int per = a.tiles_y * a.tiles_x;
  const int b = (int)blockIdx.x / per, t = (int)blockIdx.x - b * per;
  fm_tile(FmDev(), a, b, t / a.tiles_x, t % a.tiles_x, raw, hs, qs, tm, rs);
}

// per sample: the largest of its tiles' maxima (a NaN stays)
__global__ __launch_bounds__(FM_TAIL_THREADS) void fuse_maps_tail_kernel(const float* __restrict__ tile_max, int per,
                                                                        float* __restrict__ frame_max) {
  __shared__ float part[FM_TAIL_THREADS];
  const float* __restrict__ tmx = tile_max + (int64_t)blockIdx.x * per;
  float m = -INFINITY;
  for (int k = (int)threadIdx.x; k < per; k += FM_TAIL_THREADS) m = fm_max(m, tmx[k]);
  part[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < FM_TAIL_THREADS; ++k) m = fm_max(m, part[k]);
    frame_max[blockIdx.x] = m;
  }
}

#endif  // AMMC_FUSE_HOST

}  // namespace ammc_impl

#ifndef AMMC_FUSE_HOST
using namespace ammc_impl;

extern "C" {

int ammc_fuse_maps_f32(const float* const* src, const int64_t* src_bs, const int32_t* gh, const int32_t* gw, const int32_t* cell,
                       int32_t n_ch, const float* coef, int32_t batch, int32_t h, int32_t w, int32_t radius, int32_t patch,
                       float* pixel, int64_t px_bs, float* patch_mean, int64_t pm_bs, float* frame_max, float* workspace,
                       void* stream) {
  if (!src || !src_bs || !gh || !gw || !cell || !coef || !pixel || !patch_mean || !frame_max || !workspace) return AMMC_EINVAL;
  if (n_ch < 1 || n_ch > FM_MAX_CH || batch < 1 || h < 1 || w < 1) return AMMC_EINVAL;
  if (radius < 0 || radius > FM_MAX_RADIUS) return AMMC_EINVAL;
  if (patch != 8 && patch != 16 && patch != 32) return AMMC_EINVAL;
  if (((uintptr_t)coef | (uintptr_t)pixel | (uintptr_t)patch_mean | (uintptr_t)frame_max | (uintptr_t)workspace) & 3)
    return AMMC_EINVAL;
  if ((int64_t)h * w > (1LL << 28)) return AMMC_EUNSUP;
  FmArgs a = {};
  for (int c = 0; c < n_ch; ++c) {
    if (!src[c] || ((uintptr_t)src[c] & 3) || cell[c] < 1) return AMMC_EINVAL;
    const int fh = h / cell[c], ch = (h + cell[c] - 1) / cell[c], fw = w / cell[c], cw = (w + cell[c] - 1) / cell[c];
    if (gh[c] < 1 || gw[c] < 1 || (gh[c] != fh && gh[c] != ch) || (gw[c] != fw && gw[c] != cw)) return AMMC_EINVAL;
    if (batch > 1 && src_bs[c] < (int64_t)gh[c] * gw[c]) return AMMC_EINVAL;
    int shift = -1;
    for (int s = 0; s < 31; ++s)
      if (cell[c] == (1 << s)) shift = s;
    a.src[c] = {src[c], batch > 1 ? src_bs[c] : 0, gh[c], gw[c], cell[c], shift};
  }
  const int ph = (h + patch - 1) / patch, pw = (w + patch - 1) / patch;
  if (batch > 1 && (px_bs < (int64_t)h * w || pm_bs < (int64_t)ph * pw)) return AMMC_EINVAL;
  const int tiles_y = (h + FM_TH - 1) / FM_TH, tiles_x = (w + FM_TW - 1) / FM_TW;
  const int64_t per = (int64_t)tiles_y * tiles_x;
  if (per * batch >= (1LL << 31)) return AMMC_EUNSUP;
  a.coef = coef;
  a.n_ch = n_ch, a.h = h, a.w = w, a.radius = radius, a.patch = patch, a.ph = ph, a.pw = pw;
  a.tiles_x = tiles_x, a.tiles_y = tiles_y;
  a.pixel = pixel, a.px_bs = batch > 1 ? px_bs : 0;
  a.px_vec = ((uintptr_t)pixel & 15) == 0 && ((a.px_bs | (int64_t)w) & 3) == 0;
  a.patch_mean = patch_mean, a.pm_bs = batch > 1 ? pm_bs : 0;
  a.tile_max = workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fuse_maps_kernel, dim3((unsigned)(per * batch)), dim3(FM_THREADS), 0, s, a);
  const int rc = ammc_launch_status();
  if (rc != AMMC_OK) return rc;
  hipLaunchKernelGGL(fuse_maps_tail_kernel, dim3((unsigned)batch), dim3(FM_TAIL_THREADS), 0, s, workspace, (int)per, frame_max);
  return ammc_launch_status();
}

}  // extern "C"
#endif
