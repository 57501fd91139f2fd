// SSIM and squared-error frame scores: a stand-alone scoring pass over a predicted frame and its target (NCHW fp32,
// pixel stride 1, any batch / channel / row strides).  The reference's `ssim_error` (utils/pytorch_ssim.py: an 11 x 11
// Gaussian window of sigma 1.5, zero padding, C1 = 0.01^2 and C2 = 0.03^2 applied to the values AS THEY ARE, i.e. to
// frames on [-1, 1]) and the squared error its `mse_error` / `psnr_error` are functions of.
//
//   G(f)(y, x) = sum_i win[i] * ( sum_j win[j] * f(y + i - 5, x + j - 5) )      f = 0 outside the frame
//                the row pass (j) and then the column pass (i) are each ONE fmaf chain from 0 in tap order
//   mu1 = G(pred), mu2 = G(target), s1 = G(pred^2) - mu1^2, s2 = G(target^2) - mu2^2, s12 = G(pred target) - mu1 mu2
//   ssim_px = ((2 mu1 mu2 + C1) (2 s12 + C2)) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2))
//
// Two plain launches, no atomics, no arrival counter: every output and every workspace slot has one writer.
//
// Launch 1: a workgroup (256 threads) owns one SS_T x SS_T output tile of one sample and goes through the channels one
// after the other:
//   * stage: rows y0 - 5 .. y0 + SS_T + 4 and columns x0 - 8 .. x0 + SS_T + 7 of both tensors go to LDS as quads of 4
//     pixels that start at a multiple of 4 (x0 is a multiple of SS_T): one 16-byte load where the bases and strides
//     allow (VEC) and the quad lies inside the frame, four guarded scalar loads otherwise - the same values land in the
//     same LDS words, and everything behind the staging is the same code.  Pixels outside the frame are staged as 0,
//     so a tap on the padding adds an exact + 0;
//   * row pass: thread t owns column t % SS_T and the staged rows t / SS_T, t / SS_T + 8, ...; it forms the five moment
//     rows (p, t, p p, t t, p t; the products are rounded products) by five fmaf chains over the 11 taps;
//   * column pass: thread t owns column t % SS_T and the 4 output rows 4 (t / SS_T) ..+3: per moment image 14 LDS reads
//     feed four fmaf chains over the 11 taps; then ssim_px, the map (channels added in order, divided by c) and
//     d^2 = (target - pred)^2 from the staged centre.  Pixels of the tile past the frame's edge enter every sum as 0.
//   * sums of the tile, per channel for ssim_px and once for d^2:
//       thread:   (v0 + v1) + (v2 + v3) over its 4 rows;  d^2 additionally over the channels in order
//       wave:     a fixed xor tree over the 64 lanes (offsets 1, 2, .. 32)
//       tile:     the 4 waves in order
//     one partial per channel and one for d^2, written to workspace[(b * tiles + tile) * (c + 1) + k].
// Launch 2: one workgroup per sample; thread k <= c adds the partials k of the sample's tiles sequentially in double,
// in tile order (row-major), and rounds once to fp32.
//
// The order in which a tile's terms are added is a function of (c, rows, cols) of that tile alone - not of the sample's
// place in the batch, the batch size, a stride or an alignment.  The longest chain of dependent fp32 adds behind a
// d^2 term: 2 (rows) + (c - 1) (channels) + 6 (lanes) + 3 (waves) = c + 10 <= 14; the double sum over the tiles adds
// nothing visible in fp32 and the final rounding one more.
//
// LDS: the staged images are [42][48] floats each (quads are written at 16 * item bytes: contiguous ds_write_b128);
// the five moment images are [42][SS_T] floats.  Every read and write of both passes has the 32 lanes of a half-wave
// on 32 CONSECUTIVE words of one row (the lane is the column; the other half-wave is on another row), so the 32 banks
// of ds_read_b32 / ds_write_b32 are hit once each whatever the row stride: the column pass walks its 14 rows at a fixed
// column without bank conflicts.  43.1 KB per workgroup: three workgroups per CU.
// Contraction into FMAs is off: the only fused operations are the explicit fmaf chains of the two passes.
#include "ammc_common.h"

namespace ammc_impl {

constexpr int SS_T = 32;                               // tile edge (output pixels)
constexpr int SS_R = 5;                                // window radius
constexpr int SS_TAPS = 2 * SS_R + 1;
constexpr int SS_THREADS = 256;
constexpr int SS_ROWS = SS_T + 2 * SS_R;               // staged rows
constexpr int SS_LEFT = 8;                             // staged columns start at x0 - 8 (a multiple of 4)
constexpr int SS_SW = SS_T + 2 * SS_LEFT;              // staged columns
constexpr int SS_SLOTS = SS_THREADS / SS_T;            // row slots of the row pass
constexpr int SS_PER = SS_T / SS_SLOTS;                // output rows of a thread in the column pass
constexpr int SS_WAVES = SS_THREADS / AMMC_WAVE;
constexpr int SS_TAIL_THREADS = 64;
constexpr int SS_MAX_C = 4;

struct SsTensor {
  const float* p;
  int64_t bs, cs, rs;
};

struct SsWindow {
  float w[SS_TAPS];
};

// one channel plane's rows y0 - 5 .. and columns x0 - 8 .. into dst[SS_ROWS][SS_SW]; outside the frame: 0
template <bool VEC>
__device__ __forceinline__ void ss_stage(float* __restrict__ dst, const float* __restrict__ plane, int64_t rs, int y0,
                                         int x0, int H, int W) {
  constexpr int QW = SS_SW / 4;
  for (int i = threadIdx.x; i < SS_ROWS * QW; i += SS_THREADS) {
    const int r = i / QW, q = i - r * QW;
    const int py = y0 - SS_R + r, px = x0 - SS_LEFT + 4 * q;       // px is a multiple of 4: a quad is inside or outside on the left
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const float* __restrict__ p = plane + (int64_t)py * rs + px;
      if (VEC && px + 4 <= W) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (px + k < W) v[k] = p[k];
      }
    }
    *reinterpret_cast<f32x4*>(dst + 4 * i) = v;
  }
}

template <int C, bool VEC>
__global__ __launch_bounds__(SS_THREADS) void ssim_kernel(SsTensor pred, SsTensor target, SsWindow win, int H, int W, int tw,
                                                          int tiles, float* __restrict__ map, int64_t map_bs,
                                                          float* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float st[2][SS_ROWS * SS_SW];
  __shared__ float mom[5][SS_ROWS][SS_T];
  __shared__ float red[SS_WAVES][C + 1];
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tw, tx = tile - ty * tw;
  const int y0 = ty * SS_T, x0 = tx * SS_T;
  const int x = threadIdx.x % SS_T, g = threadIdx.x / SS_T;
  const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
  const float* __restrict__ pp = pred.p + (int64_t)b * pred.bs;
  const float* __restrict__ tp = target.p + (int64_t)b * target.bs;
  bool valid[SS_PER];
#pragma unroll
  for (int j = 0; j < SS_PER; ++j) valid[j] = x0 + x < W && y0 + SS_PER * g + j < H;

  float part[C + 1];                                   // this thread's ssim_px sums per channel, then its d^2 sum
  float macc[SS_PER];                                  // ssim_px of its pixels, channels added in order
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    if (ch) __syncthreads();                           // the column pass of the channel before has read st and mom
    ss_stage<VEC>(st[0], pp + ch * pred.cs, pred.rs, y0, x0, H, W);
    ss_stage<VEC>(st[1], tp + ch * target.cs, target.rs, y0, x0, H, W);
    __syncthreads();
    // row pass: output column x reads the staged columns x + 3 .. x + 13 (pixel x0 + x - 5 + k)
    for (int r = g; r < SS_ROWS; r += SS_SLOTS) {
      const float* __restrict__ a = &st[0][r * SS_SW + x + SS_LEFT - SS_R];
      const float* __restrict__ t = &st[1][r * SS_SW + x + SS_LEFT - SS_R];
      float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
      for (int k = 0; k < SS_TAPS; ++k) {
        const float p = a[k], q = t[k], w = win.w[k];
        m1 = __builtin_fmaf(w, p, m1);
        m2 = __builtin_fmaf(w, q, m2);
        e11 = __builtin_fmaf(w, p * p, e11);
        e22 = __builtin_fmaf(w, q * q, e22);
        e12 = __builtin_fmaf(w, p * q, e12);
      }
      mom[0][r][x] = m1, mom[1][r][x] = m2, mom[2][r][x] = e11, mom[3][r][x] = e22, mom[4][r][x] = e12;
    }
    __syncthreads();
    // column pass: output rows 4 g .. 4 g + 3 read the moment rows 4 g .. 4 g + 13
    float G[5][SS_PER];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      float col[SS_PER + SS_TAPS - 1];
#pragma unroll
      for (int i = 0; i < SS_PER + SS_TAPS - 1; ++i) col[i] = mom[m][SS_PER * g + i][x];
#pragma unroll
      for (int j = 0; j < SS_PER; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) acc = __builtin_fmaf(win.w[k], col[j + k], acc);
        G[m][j] = acc;
      }
    }
    float v[SS_PER], d2[SS_PER];
#pragma unroll
    for (int j = 0; j < SS_PER; ++j) {
      const float mu1 = G[0][j], mu2 = G[1][j];
      const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
      const float s1 = G[2][j] - m11, s2 = G[3][j] - m22, s12 = G[4][j] - m12;
      const float num = (2.f * m12 + C1) * (2.f * s12 + C2);
      const float den = ((m11 + m22) + C1) * ((s1 + s2) + C2);
      v[j] = valid[j] ? num / den : 0.f;
      const int c0 = (SS_PER * g + j + SS_R) * SS_SW + x + SS_LEFT;
      const float d = st[1][c0] - st[0][c0];            // (both 0 outside the frame)
      d2[j] = d * d;
      macc[j] = ch ? macc[j] + v[j] : v[j];
    }
    part[ch] = (v[0] + v[1]) + (v[2] + v[3]);
    const float dq = (d2[0] + d2[1]) + (d2[2] + d2[3]);
    part[C] = ch ? part[C] + dq : dq;
  }
  if (map) {
    float* __restrict__ o = map + (int64_t)b * map_bs + (int64_t)(y0 + SS_PER * g) * W + x0 + x;
#pragma unroll
    for (int j = 0; j < SS_PER; ++j)
      if (valid[j]) o[(int64_t)j * W] = macc[j] / (float)C;
  }
  // a + b == b + a: every lane of a wave ends with the same bits
#pragma unroll
  for (int k = 0; k <= C; ++k) {
    float s = part[k];
#pragma unroll
    for (int o = 1; o < AMMC_WAVE; o <<= 1) s = s + __shfl_xor(s, o, AMMC_WAVE);
    part[k] = s;
  }
  if (threadIdx.x % AMMC_WAVE == 0) {
#pragma unroll
    for (int k = 0; k <= C; ++k) red[threadIdx.x / AMMC_WAVE][k] = part[k];
  }
  __syncthreads();
  if (threadIdx.x <= C) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < SS_WAVES; ++k) s = s + red[k][threadIdx.x];
    ws[(int64_t)blockIdx.x * (C + 1) + threadIdx.x] = s;
  }
}

// per sample: thread k < c owns channel k, thread c the squared error; each adds its partial of every tile in tile
// order in double and rounds once; thread 0 then forms the frame's value from the STORED per-channel means
__global__ __launch_bounds__(SS_TAIL_THREADS) void ssim_tail_kernel(const float* __restrict__ ws, int tiles, int c, int h,
                                                                    int w, float* __restrict__ ssim,
                                                                    float* __restrict__ ssim_c, float* __restrict__ sq) {
  __shared__ float mean_c[SS_MAX_C];
  const int b = blockIdx.x, k = threadIdx.x;
  if (k <= c) {
    const float* __restrict__ p = ws + (int64_t)b * tiles * (c + 1) + k;
    double total = 0.0;
    for (int t = 0; t < tiles; ++t) total += (double)p[(int64_t)t * (c + 1)];
    if (k < c) {
      const float m = (float)(total / ((double)h * (double)w));
      mean_c[k] = m;
      ssim_c[(int64_t)b * c + k] = m;
    } else {
      sq[b] = (float)total;
    }
  }
  __syncthreads();
  if (k == 0) {
    double s = (double)mean_c[0];
    for (int i = 1; i < c; ++i) s += (double)mean_c[i];
    ssim[b] = (float)(s / (double)c);
  }
}

// a [batch][c][h][w] view: row stride >= w, each outer stride >= the extent below it
inline bool ss_strides_ok(int64_t bs, int64_t cs, int64_t rs, int c, int h, int w) {
  if (rs < w) return false;
  const int64_t plane = (int64_t)(h - 1) * rs + w;
  if (cs < plane) return false;
  return bs >= (int64_t)(c - 1) * cs + plane;
}

inline int64_t ss_tiles(int h, int w) { return (int64_t)((h + SS_T - 1) / SS_T) * ((w + SS_T - 1) / SS_T); }

template <int C>
inline void ss_launch(bool vec, unsigned grid, hipStream_t stream, const SsTensor& pred, const SsTensor& target,
                      const SsWindow& win, int h, int w, int tw, int tiles, float* map, int64_t map_bs, float* ws) {
  if (vec)
    hipLaunchKernelGGL((ssim_kernel<C, true>), dim3(grid), dim3(SS_THREADS), 0, stream, pred, target, win, h, w, tw, tiles,
                       map, map_bs, ws);
  else
    hipLaunchKernelGGL((ssim_kernel<C, false>), dim3(grid), dim3(SS_THREADS), 0, stream, pred, target, win, h, w, tw, tiles,
                       map, map_bs, ws);
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_ssim_tile(void) { return SS_T; }

int64_t ammc_ssim_workspace_floats(int32_t batch, int32_t c, int32_t h, int32_t w) {
  if (batch <= 0 || c <= 0 || h <= 0 || w <= 0) return 0;
  return (int64_t)batch * ss_tiles(h, w) * ((int64_t)c + 1);
}

int ammc_ssim_f32(const float* pred, int64_t p_bs, int64_t p_cs, int64_t p_rs, const float* target, int64_t t_bs,
                  int64_t t_cs, int64_t t_rs, int32_t batch, int32_t c, int32_t h, int32_t w, const float* win, float* ssim,
                  float* ssim_c, float* sq, float* map, int64_t map_bs, float* workspace, int64_t workspace_floats,
                  void* stream) {
  if (!pred || !target || !win || !ssim || !ssim_c || !sq || !workspace) return AMMC_EINVAL;
  if (batch <= 0 || c <= 0 || h <= 0 || w <= 0) return AMMC_EINVAL;
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)win | (uintptr_t)ssim | (uintptr_t)ssim_c | (uintptr_t)sq |
       (uintptr_t)map | (uintptr_t)workspace) & 3)
    return AMMC_EINVAL;
  if (!ss_strides_ok(p_bs, p_cs, p_rs, c, h, w) || !ss_strides_ok(t_bs, t_cs, t_rs, c, h, w)) return AMMC_EINVAL;
  if (map && map_bs < (int64_t)h * w) return AMMC_EINVAL;
  if (workspace_floats < ammc_ssim_workspace_floats(batch, c, h, w)) return AMMC_EINVAL;
  if (c > SS_MAX_C) return AMMC_EUNSUP;
  const int64_t tiles = ss_tiles(h, w);
  // the 1-D grid and the 32-bit tile index; element offsets are 64-bit
  if ((int64_t)batch * tiles >= (1LL << 31)) return AMMC_EUNSUP;

  SsWindow wv;
  for (int k = 0; k < SS_TAPS; ++k) wv.w[k] = win[k];
  const SsTensor tp = {pred, p_bs, p_cs, p_rs}, tt = {target, t_bs, t_cs, t_rs};
  // 16-byte loads: every quad of both tensors starts on a 16-byte boundary (quads start at multiples of 4 pixels)
  const bool vec = (((uintptr_t)pred | (uintptr_t)target) & 15) == 0 && ((p_bs | p_cs | p_rs | t_bs | t_cs | t_rs) & 3) == 0;
  const int tw = (w + SS_T - 1) / SS_T;
  const unsigned grid = (unsigned)(batch * tiles);
  hipStream_t s = (hipStream_t)stream;
  switch (c) {
    case 1: ss_launch<1>(vec, grid, s, tp, tt, wv, h, w, tw, (int)tiles, map, map_bs, workspace); break;
    case 2: ss_launch<2>(vec, grid, s, tp, tt, wv, h, w, tw, (int)tiles, map, map_bs, workspace); break;
    case 3: ss_launch<3>(vec, grid, s, tp, tt, wv, h, w, tw, (int)tiles, map, map_bs, workspace); break;
    case 4: ss_launch<4>(vec, grid, s, tp, tt, wv, h, w, tw, (int)tiles, map, map_bs, workspace); break;
  }
  int rc = ammc_launch_status();
  if (rc != AMMC_OK) return rc;
  hipLaunchKernelGGL(ssim_tail_kernel, dim3((unsigned)batch), dim3(SS_TAIL_THREADS), 0, s, workspace, (int)tiles, c, h, w,
                     ssim, ssim_c, sq);
  return ammc_launch_status();
}

}  // extern "C"
