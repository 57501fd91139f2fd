// The per-pixel terms of the generator's objective at the module boundary (NCHW fp32 predictions and clip targets) and
// their gradient: one forward launch and one backward launch per (prediction, target) pair instead of the chain of
// elementwise and reduction launches autograd runs for them.
//
// Reference semantics (Code/models/losses/losses_utils.py):
//   * `L2` (:124-129): mean over pixels of the channel norm,  int = mean_p sqrt(sum_c (pred - target)^2);
//   * `Gradient_Loss` (:30-61) with alpha = 1: the [-1, 1] filters on the channel SUM s, zero padding on the left / top,
//       gx[x] = s[x] - s[x-1] (gx[0] = s[0]), gy likewise down the rows,  gdl = mean_p |tx - gx| + |ty - gy|;
//   * `Flow_Loss` (:10-15): mean |a - b|.
// Their backward is torch's: norm backward is 0 where the norm is 0, abs backward uses sign(0) = 0.
//
// Geometry (a function of the shape alone: the same partial sums on every launch, no atomics): a wave owns one image
// row (b, y) - its b, y and row offsets are computed once, the lanes walk the row in 16-byte pieces (4-byte pieces when
// W % 4 != 0 or a tensor starts off a 16-byte boundary: rows are then not 16-byte aligned) - and a workgroup of PL_WAVES waves owns PL_WAVES consecutive rows, so
// the row above / below a wave needs for the y filter is the row its neighbour wave streams (L1 / L2 hits, not HBM).
// Forward: lane sums, a fixed shuffle tree per wave, the waves of the workgroup in order -> partial[workgroup][2]
// (int, gdl); a partial accumulates PL_WAVES * W pixels.  ammc_reduce_partials_f32(partial, rows, 2, 1 / (B H W), out)
// combines them in double, in fixed order.
#include "ammc_common.h"

namespace ammc_impl {

constexpr int PL_WAVES = AMMC_PRED_LOSS_ROWS;         // image rows per workgroup
constexpr int PL_THREADS = PL_WAVES * AMMC_WAVE;
constexpr int L1_U = 4;                               // 16-byte loads of each operand per thread
static_assert(AMMC_L1_CHUNK == 256 * 4 * L1_U, "a workgroup of ammc_l1_partials_f32 sums AMMC_L1_CHUNK elements");

template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = t[i];
  } else {
    v[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    p[0] = v[0];
  }
}

// channel sum of V pixels, in torch's order ((c0 + c1) + c2)
template <int C, int V>
__device__ __forceinline__ void chan_sum(const float* __restrict__ p, int64_t plane, float (&s)[V]) {
  float a[V];
  ldv<V>(p, s);
#pragma unroll
  for (int c = 1; c < C; ++c) {
    ldv<V>(p + c * plane, a);
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] += a[i];
  }
}

template <int C>
__device__ __forceinline__ float chan_sum1(const float* __restrict__ p, int64_t plane) {
  float s = p[0];
#pragma unroll
  for (int c = 1; c < C; ++c) s += p[c * plane];
  return s;
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// sum over the lanes of a wave, fixed tree; the total is valid in lane 0
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = AMMC_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, AMMC_WAVE);
  return v;
}

template <int C, int V, bool GDL>
__global__ __launch_bounds__(PL_THREADS) void pred_loss_fwd_kernel(const float* __restrict__ pred,
                                                                   const float* __restrict__ target, int64_t t_bs, int rows,
                                                                   int H, int W, float* __restrict__ partial) {
  __shared__ float red[2][PL_WAVES];
  const int wave = threadIdx.x / AMMC_WAVE, lane = threadIdx.x % AMMC_WAVE;
  const int r = blockIdx.x * PL_WAVES + wave;
  float s_int = 0.f, s_gdl = 0.f;
  if (r < rows) {
    const int b = r / H, y = r - b * H;                       // once per wave
    const int64_t plane = (int64_t)H * W;
    const int64_t base = ((int64_t)b * C * H + y) * W;        // channel 0 of row (b, y)
    const float* __restrict__ p0 = pred + base;
    const float* __restrict__ t0 = target + (int64_t)b * t_bs + (int64_t)y * W;
    const bool up = y > 0;
    for (int x = lane * V; x < W; x += AMMC_WAVE * V) {
      float p[C][V], t[C][V];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        ldv<V>(p0 + c * plane + x, p[c]);
        ldv<V>(t0 + c * plane + x, t[c]);
      }
      float spu[V], stu[V], spl = 0.f, stl = 0.f;
      if (GDL) {                                              // every load of the trip before its first sum
#pragma unroll
        for (int i = 0; i < V; ++i) spu[i] = stu[i] = 0.f;
        if (up) {
          chan_sum<C, V>(p0 - W + x, plane, spu);
          chan_sum<C, V>(t0 - W + x, plane, stu);
        }
        const int xl = x > 0 ? x - 1 : 0;
        spl = chan_sum1<C>(p0 + xl, plane);
        stl = chan_sum1<C>(t0 + xl, plane);
        if (x == 0) spl = stl = 0.f;
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float n2 = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float d = p[c][i] - t[c][i];
          n2 += d * d;
        }
        s_int += sqrtf(n2);
      }
      if (GDL) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          float sp = p[0][i], st = t[0][i];
#pragma unroll
          for (int c = 1; c < C; ++c) { sp += p[c][i]; st += t[c][i]; }
          const float ex = fabsf((st - stl) - (sp - spl));    // |tx - gx|
          const float ey = fabsf((st - stu[i]) - (sp - spu[i]));
          s_gdl += ex + ey;
          spl = sp;
          stl = st;
        }
      }
    }
  }
  s_int = wave_sum(s_int);
  if (GDL) s_gdl = wave_sum(s_gdl);
  if (lane == 0) {
    red[0][wave] = s_int;
    red[1][wave] = s_gdl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = red[0][0], g = red[1][0];
#pragma unroll
    for (int j = 1; j < PL_WAVES; ++j) { a += red[0][j]; g += red[1][j]; }
    partial[2 * (int64_t)blockIdx.x] = a;
    partial[2 * (int64_t)blockIdx.x + 1] = g;
  }
}

// d_pred[b][c][y][x] = (p_c - t_c) * (g_int * inv / norm)                                   (0 where norm == 0)
//                    + (-sgn(dx[x]) + sgn(dx[x+1]) - sgn(dy[y]) + sgn(dy[y+1])) * (g_gdl * inv)
// with dx = tx - gx, dy = ty - gy of the forward; the [x+1] / [y+1] terms are absent in the last column / row.
template <int C, int V, bool GDL>
__global__ __launch_bounds__(PL_THREADS) void pred_loss_bwd_kernel(const float* __restrict__ pred,
                                                                   const float* __restrict__ target, int64_t t_bs,
                                                                   const float* __restrict__ g_int,
                                                                   const float* __restrict__ g_gdl, float inv, int rows, int H,
                                                                   int W, float* __restrict__ d_pred) {
  const int wave = threadIdx.x / AMMC_WAVE, lane = threadIdx.x % AMMC_WAVE;
  const int r = blockIdx.x * PL_WAVES + wave;
  if (r >= rows) return;
  const float ci = (g_int ? g_int[0] : 0.f) * inv;
  const float cg = (GDL ? g_gdl[0] : 0.f) * inv;
  const int b = r / H, y = r - b * H;
  const int64_t plane = (int64_t)H * W;
  const int64_t base = ((int64_t)b * C * H + y) * W;
  const float* __restrict__ p0 = pred + base;
  const float* __restrict__ t0 = target + (int64_t)b * t_bs + (int64_t)y * W;
  float* __restrict__ o0 = d_pred + base;
  const bool up = y > 0, down = y + 1 < H;
  for (int x = lane * V; x < W; x += AMMC_WAVE * V) {
    float p[C][V], t[C][V];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      ldv<V>(p0 + c * plane + x, p[c]);
      ldv<V>(t0 + c * plane + x, t[c]);
    }
    float k[V];
#pragma unroll
    for (int i = 0; i < V; ++i) k[i] = 0.f;
    if (GDL) {
      float spu[V], stu[V], spd[V], std_[V];
#pragma unroll
      for (int i = 0; i < V; ++i) spu[i] = stu[i] = spd[i] = std_[i] = 0.f;
      if (up) {
        chan_sum<C, V>(p0 - W + x, plane, spu);
        chan_sum<C, V>(t0 - W + x, plane, stu);
      }
      if (down) {
        chan_sum<C, V>(p0 + W + x, plane, spd);
        chan_sum<C, V>(t0 + W + x, plane, std_);
      }
      const int xl = x > 0 ? x - 1 : 0;
      const bool right = x + V < W;
      const int xr = right ? x + V : x;
      float spl = chan_sum1<C>(p0 + xl, plane), stl = chan_sum1<C>(t0 + xl, plane);
      const float spr = chan_sum1<C>(p0 + xr, plane), str_ = chan_sum1<C>(t0 + xr, plane);
      if (x == 0) spl = stl = 0.f;
      float sp[V], st[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        sp[i] = p[0][i];
        st[i] = t[0][i];
#pragma unroll
        for (int c = 1; c < C; ++c) { sp[i] += p[c][i]; st[i] += t[c][i]; }
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float pl = i ? sp[i - 1] : spl, tl = i ? st[i - 1] : stl;
        const float dxc = (st[i] - tl) - (sp[i] - pl);
        const float dyc = (st[i] - stu[i]) - (sp[i] - spu[i]);
        float kk = -sgn(dxc) - sgn(dyc);
        const bool inner = i + 1 < V;                        // the right neighbour is in this piece
        const float pr = inner ? sp[(i + 1) % V] : spr, tr = inner ? st[(i + 1) % V] : str_;
        if (inner || right) kk += sgn((tr - st[i]) - (pr - sp[i]));
        if (down) kk += sgn((std_[i] - st[i]) - (spd[i] - sp[i]));
        k[i] = kk * cg;
      }
    }
    float q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float n2 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float d = p[c][i] - t[c][i];
        n2 += d * d;
      }
      const float nrm = sqrtf(n2);
      q[i] = nrm > 0.f ? ci / nrm : 0.f;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float o[V];
#pragma unroll
      for (int i = 0; i < V; ++i) o[i] = (p[c][i] - t[c][i]) * q[i] + k[i];
      stv<V>(o0 + c * plane + x, o);
    }
  }
}

// partial[workgroup] = sum |a - b| over its AMMC_L1_CHUNK elements (the last one short)
template <bool VEC>
__global__ __launch_bounds__(256) void l1_partials_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t count,
                                                          float* __restrict__ partial) {
  __shared__ float red[256 / AMMC_WAVE];
  const int64_t i0 = (int64_t)blockIdx.x * AMMC_L1_CHUNK + threadIdx.x * 4;
  float va[L1_U][4], vb[L1_U][4];
#pragma unroll
  for (int u = 0; u < L1_U; ++u) {
    const int64_t i = i0 + u * 1024;
    if (VEC && i + 3 < count) {
      ldv<4>(a + i, va[u]);
      ldv<4>(b + i, vb[u]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = i + j < count;
        va[u][j] = ok ? a[i + j] : 0.f;
        vb[u][j] = ok ? b[i + j] : 0.f;
      }
    }
  }
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < L1_U; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += fabsf(va[u][j] - vb[u][j]);
  s = wave_sum(s);
  if (threadIdx.x % AMMC_WAVE == 0) red[threadIdx.x / AMMC_WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

inline int pred_loss_check(const void* pred, const void* target, int64_t t_bs, int32_t batch, int32_t c, int32_t h, int32_t w) {
  if (!pred || !target || batch <= 0 || c <= 0 || h <= 0 || w <= 0) return AMMC_EINVAL;
  if (t_bs < (int64_t)c * h * w) return AMMC_EINVAL;
  if (((uintptr_t)pred | (uintptr_t)target) & 3) return AMMC_EINVAL;
  if (c != 2 && c != 3) return AMMC_EUNSUP;
  if ((int64_t)batch * h >= (1LL << 31) - PL_WAVES) return AMMC_EUNSUP;      // (row indices are 32-bit)
  return AMMC_OK;
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_pred_loss_partial_rows(int32_t batch, int32_t h, int32_t w) {
  if (batch <= 0 || h <= 0 || w <= 0 || (int64_t)batch * h >= (1LL << 31) - PL_WAVES) return 0;
  return (int)(((int64_t)batch * h + PL_WAVES - 1) / PL_WAVES);
}

int ammc_pred_loss_fwd_f32(const float* pred, const float* target, int64_t target_bs, int32_t batch, int32_t c, int32_t h,
                           int32_t w, int32_t want_gdl, float* partial, void* stream) {
  const int rc = pred_loss_check(pred, target, target_bs, batch, c, h, w);
  if (rc != AMMC_OK) return rc;
  if (!partial || ((uintptr_t)partial & 3)) return AMMC_EINVAL;
  const int rows = batch * h;
  const dim3 grid((unsigned)ammc_pred_loss_partial_rows(batch, h, w));
  const bool vec = ((w | target_bs) & 3) == 0 && (((uintptr_t)pred | (uintptr_t)target) & 15) == 0;   // rows 16-byte aligned
#define AMMC_PL_FWD(CC, VV, GG)                                                                                          \
  hipLaunchKernelGGL((pred_loss_fwd_kernel<CC, VV, GG>), grid, dim3(PL_THREADS), 0, (hipStream_t)stream, pred, target,      \
                     target_bs, rows, h, w, partial)
  if (c == 3) {
    if (vec) { if (want_gdl) AMMC_PL_FWD(3, 4, true); else AMMC_PL_FWD(3, 4, false); }
    else { if (want_gdl) AMMC_PL_FWD(3, 1, true); else AMMC_PL_FWD(3, 1, false); }
  } else {
    if (vec) { if (want_gdl) AMMC_PL_FWD(2, 4, true); else AMMC_PL_FWD(2, 4, false); }
    else { if (want_gdl) AMMC_PL_FWD(2, 1, true); else AMMC_PL_FWD(2, 1, false); }
  }
#undef AMMC_PL_FWD
  return ammc_launch_status();
}

int ammc_pred_loss_bwd_f32(const float* pred, const float* target, int64_t target_bs, const float* g_int, const float* g_gdl,
                           int32_t batch, int32_t c, int32_t h, int32_t w, float* d_pred, void* stream) {
  const int rc = pred_loss_check(pred, target, target_bs, batch, c, h, w);
  if (rc != AMMC_OK) return rc;
  if (!d_pred || (((uintptr_t)d_pred | (uintptr_t)g_int | (uintptr_t)g_gdl) & 3)) return AMMC_EINVAL;
  const int rows = batch * h;
  const float inv = (float)(1.0 / ((double)batch * h * w));
  const dim3 grid((unsigned)ammc_pred_loss_partial_rows(batch, h, w));
  const bool vec = ((w | target_bs) & 3) == 0 && (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)d_pred) & 15) == 0;
  const bool gdl = g_gdl != nullptr;
#define AMMC_PL_BWD(CC, VV, GG)                                                                                          \
  hipLaunchKernelGGL((pred_loss_bwd_kernel<CC, VV, GG>), grid, dim3(PL_THREADS), 0, (hipStream_t)stream, pred, target,      \
                     target_bs, g_int, g_gdl, inv, rows, h, w, d_pred)
  if (c == 3) {
    if (vec) { if (gdl) AMMC_PL_BWD(3, 4, true); else AMMC_PL_BWD(3, 4, false); }
    else { if (gdl) AMMC_PL_BWD(3, 1, true); else AMMC_PL_BWD(3, 1, false); }
  } else {
    if (vec) { if (gdl) AMMC_PL_BWD(2, 4, true); else AMMC_PL_BWD(2, 4, false); }
    else { if (gdl) AMMC_PL_BWD(2, 1, true); else AMMC_PL_BWD(2, 1, false); }
  }
#undef AMMC_PL_BWD
  return ammc_launch_status();
}

int ammc_l1_partials_f32(const float* a, const float* b, int64_t count, float* partial, void* stream) {
  if (!a || !b || !partial || count <= 0) return AMMC_EINVAL;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)partial) & 3) return AMMC_EINVAL;
  const int64_t nblk = (count + AMMC_L1_CHUNK - 1) / AMMC_L1_CHUNK;
  if (nblk >= (1LL << 31)) return AMMC_EUNSUP;
  if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0)
    hipLaunchKernelGGL(l1_partials_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, a, b, count, partial);
  else                                                          // (a slice that starts off a 16-byte boundary: 4-byte loads)
    hipLaunchKernelGGL(l1_partials_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, a, b, count, partial);
  return ammc_launch_status();
}

}  // extern "C"
