// Anomaly localisation: where in the frame the prediction error sits.  A stand-alone scoring pass over a predicted frame
// and its target (NCHW fp32, pixel stride 1, any batch / channel / row strides): per-patch squared-error sums and means,
// an optional per-pixel map, and per sample the frame's squared error, its worst patch and that patch's index.
//
//   e(b, ch, y, x) = 0.5f * (target - pred)          the reference's `psnr_error` on the [0, 1] range (utils/utils.py:143-147)
//   pixel[b, y, x]      = (e_0^2 + e_1^2 + ...) / c                            (channels added in order)
//   patch_sum[b, i, j]  = sum of e^2 over the channels and the pixels of patch (i, j)
//   patch_mean[b, i, j] = patch_sum / (c * rows * cols)                        (the patch's true pixel count)
//   frame_sq[b]         = fp32( sum_i ( sum_j (double)patch_sum[b, i, j] ) )   (both sums sequential, in index order)
//   worst[b], worst_idx[b] = the largest patch_mean and the lowest i * pw + j that attains it
//
// Two plain launches, no atomics, no arrival counter: every output is written once by one thread, so two runs give
// the same bits.  The order in which a patch's terms are added is a function of (c, rows, cols, patch) of that patch
// ALONE - not of the sample index, the batch size, a stride or an alignment:
//
//   * a lane owns a "quad", 4 consecutive pixels of one image row starting at a multiple of 4 (a patch is 8, 16 or 32
//     wide, so a quad never straddles two patches).  It loads them as one 16-byte access where the base addresses and
//     strides allow (EM_VEC) and as four scalars where they do not - the values land in the same registers and the
//     arithmetic behind the load is the same code.  Pixels past the frame's edge enter as e = 0 (x + 0 is exact);
//   * per pixel: the channels in order; per quad: (p0 + p1) + (p2 + p3);
//   * a workgroup (256 threads) owns one patch row and a chunk of CQ quad columns: thread t owns quad column t % CQ and
//     the image rows t / CQ, t / CQ + RS, ... of the patch row (RS = 256 / CQ row slots), added in that order; rows
//     past the frame's edge are skipped;
//   * the patch / 4 lanes of one patch and one row slot are neighbours in a wave: a fixed xor tree over them;
//   * the RS row slots of a patch meet in LDS and are added in slot order.
//
// The longest chain of dependent adds: (c - 1) + 2 + patch / RS + log2(patch / 4) + RS <= 3 + 2 + 4 + 3 + 8 = 20.
// CQ is a function of the patch size alone (64 quads for patch 8, 32 for 16 and 32), chosen so that batch 16 at
// 256 x 256 gives 512 / 512 / 256 workgroups.  Contraction into FMAs is off in the arithmetic: a square is a rounded
// product, as the fp64 reference of the tests assumes.
#include "ammc_common.h"

namespace ammc_impl {

constexpr int EM_THREADS = 256;
constexpr int EM_TAIL_THREADS = 256;

template <int P>
struct EmGeom {
  static constexpr int QP = P / 4;                     // quads (lanes) across one patch
  static constexpr int CQ = P == 8 ? 64 : 32;          // quad columns of a workgroup
  static constexpr int RS = EM_THREADS / CQ;           // row slots of a workgroup
  static constexpr int NP = CQ / QP;                   // patches across a workgroup
};

struct EmTensor {
  const float* p;
  int64_t bs, cs, rs;
};

// the quad (4 pixels) at `p` of C channel planes `cs` apart; `n` pixels exist (1..4), the rest read as 0
template <int C, bool VEC>
__device__ __forceinline__ void em_load(const float* __restrict__ p, int64_t cs, int n, float (&v)[C][4]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ q = p + c * cs;
    if (VEC && n == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = t[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = i < n ? q[i] : 0.f;
    }
  }
}

// per-pixel channel sums of e^2 of one quad (the one place the squares are formed: both load forms end here)
template <int C>
__device__ __forceinline__ void em_quad(const float (&a)[C][4], const float (&t)[C][4], float (&s)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float e0 = 0.5f * (t[0][i] - a[0][i]);
    float acc = e0 * e0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
      const float e = 0.5f * (t[c][i] - a[c][i]);
      acc = acc + e * e;
    }
    s[i] = acc;
  }
}

template <int P, int C, bool VEC>
__global__ __launch_bounds__(EM_THREADS) void error_maps_kernel(EmTensor pred, EmTensor target, int H, int W, int ph, int pw,
                                                                float* __restrict__ patch_sum,
                                                                float* __restrict__ patch_mean, int64_t ps_bs,
                                                                float* __restrict__ pixel, int64_t px_bs, int px_vec) {
#pragma clang fp contract(off)
  using G = EmGeom<P>;
  __shared__ float red[G::RS][G::NP];
  const int b = blockIdx.x / ph, i = blockIdx.x - b * ph;       // sample, patch row
  const int qc = threadIdx.x % G::CQ, slot = threadIdx.x / G::CQ;
  const int x = (blockIdx.y * G::CQ + qc) * 4;                  // first pixel of this thread's quad
  const int y0 = i * P;
  const int rows = min(P, H - y0);                              // image rows of this patch row (ragged at the bottom)
  const int n = min(4, W - x);                                  // pixels of the quad that exist (<= 0: none)
  float acc = 0.f;
  if (n > 0) {
    const float* __restrict__ pp = pred.p + (int64_t)b * pred.bs + x;
    const float* __restrict__ tp = target.p + (int64_t)b * target.bs + x;
    float* __restrict__ px = pixel ? pixel + (int64_t)b * px_bs + x : nullptr;
    for (int r = slot; r < rows; r += G::RS) {
      const int y = y0 + r;
      float a[C][4], t[C][4], s[4];
      em_load<C, VEC>(pp + (int64_t)y * pred.rs, pred.cs, n, a);
      em_load<C, VEC>(tp + (int64_t)y * target.rs, target.cs, n, t);
      em_quad<C>(a, t, s);
      if (px) {
        float* __restrict__ o = px + (int64_t)y * W;
        if (px_vec && n == 4) {
          const f32x4 v = {s[0] / (float)C, s[1] / (float)C, s[2] / (float)C, s[3] / (float)C};
          *reinterpret_cast<f32x4*>(o) = v;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < n) o[k] = s[k] / (float)C;
        }
      }
      acc = acc + ((s[0] + s[1]) + (s[2] + s[3]));
    }
  }
  // the QP neighbouring lanes of one patch (same row slot): fixed xor tree; a + b == b + a, so every lane of the group
  // ends with the same bits and lanes past the frame's edge add an exact 0
#pragma unroll
  for (int o = 1; o < G::QP; o <<= 1) acc = acc + __shfl_xor(acc, o, AMMC_WAVE);
  if (qc % G::QP == 0) red[slot][qc / G::QP] = acc;
  __syncthreads();
  if (threadIdx.x < G::NP) {
    const int j = blockIdx.y * G::NP + threadIdx.x;
    if (j < pw) {
      float s = red[0][threadIdx.x];
#pragma unroll
      for (int k = 1; k < G::RS; ++k) s = s + red[k][threadIdx.x];
      const int cols = min(P, W - j * P);
      const int64_t o = (int64_t)b * ps_bs + (int64_t)i * pw + j;
      patch_sum[o] = s;
      patch_mean[o] = s / (float)(C * rows * cols);
    }
  }
}

// per sample: thread r owns patch row r (its sequential double sum, its largest mean and where), thread 0 then adds
// the rows in order; frames of more than EM_TAIL_THREADS patch rows go through in chunks, still in index order
__global__ __launch_bounds__(EM_TAIL_THREADS) void error_maps_tail_kernel(const float* __restrict__ patch_sum,
                                                                          const float* __restrict__ patch_mean,
                                                                          int64_t ps_bs, int ph, int pw,
                                                                          float* __restrict__ frame_sq,
                                                                          float* __restrict__ worst,
                                                                          int* __restrict__ worst_idx) {
  __shared__ double row_sum[EM_TAIL_THREADS];
  __shared__ float row_best[EM_TAIL_THREADS];
  __shared__ int row_at[EM_TAIL_THREADS];
  const int b = blockIdx.x;
  const float* __restrict__ ps = patch_sum + (int64_t)b * ps_bs;
  const float* __restrict__ pm = patch_mean + (int64_t)b * ps_bs;
  double total = 0.0;
  float best = 0.f;
  int at = 0;
  for (int base = 0; base < ph; base += EM_TAIL_THREADS) {
    const int r = base + (int)threadIdx.x;
    if (r < ph) {
      const int64_t o = (int64_t)r * pw;
      double s = 0.0;
      float m = pm[o];
      int mi = 0;
      for (int j = 0; j < pw; ++j) {
        s += (double)ps[o + j];
        const float v = pm[o + j];
        if (v > m) m = v, mi = j;                      // strict: the lowest index among equal values stays
      }
      row_sum[threadIdx.x] = s;
      row_best[threadIdx.x] = m;
      row_at[threadIdx.x] = r * pw + mi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = min(EM_TAIL_THREADS, ph - base);
      for (int k = 0; k < cnt; ++k) {
        total += row_sum[k];
        if ((base == 0 && k == 0) || row_best[k] > best) best = row_best[k], at = row_at[k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    frame_sq[b] = (float)total;
    worst[b] = best;
    worst_idx[b] = at;
  }
}

// a [batch][c][h][w] view: row stride >= w, each outer stride >= the extent below it
inline bool em_strides_ok(int64_t bs, int64_t cs, int64_t rs, int c, int h, int w) {
  if (rs < w) return false;
  const int64_t plane = (int64_t)(h - 1) * rs + w;
  if (cs < plane) return false;
  return bs >= (int64_t)(c - 1) * cs + plane;
}

template <int P, int C>
inline void em_launch(bool vec, dim3 grid, hipStream_t stream, const EmTensor& pred, const EmTensor& target, int h, int w,
                      int ph, int pw, float* patch_sum, float* patch_mean, int64_t ps_bs, float* pixel, int64_t px_bs,
                      int px_vec) {
  if (vec)
    hipLaunchKernelGGL((error_maps_kernel<P, C, true>), grid, dim3(EM_THREADS), 0, stream, pred, target, h, w, ph, pw,
                       patch_sum, patch_mean, ps_bs, pixel, px_bs, px_vec);
  else
    hipLaunchKernelGGL((error_maps_kernel<P, C, false>), grid, dim3(EM_THREADS), 0, stream, pred, target, h, w, ph, pw,
                       patch_sum, patch_mean, ps_bs, pixel, px_bs, px_vec);
}

template <int P>
inline void em_launch_c(int c, bool vec, dim3 grid, hipStream_t stream, const EmTensor& pred, const EmTensor& target, int h,
                        int w, int ph, int pw, float* patch_sum, float* patch_mean, int64_t ps_bs, float* pixel,
                        int64_t px_bs, int px_vec) {
#define AMMC_EM_C(CC)                                                                                                  \
  case CC:                                                                                                             \
    em_launch<P, CC>(vec, grid, stream, pred, target, h, w, ph, pw, patch_sum, patch_mean, ps_bs, pixel, px_bs, px_vec); \
    break
  switch (c) {
    AMMC_EM_C(1);
    AMMC_EM_C(2);
    AMMC_EM_C(3);
    AMMC_EM_C(4);
  }
#undef AMMC_EM_C
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_error_maps_patch_count(int32_t h, int32_t w, int32_t patch) {
  if (h <= 0 || w <= 0 || (patch != 8 && patch != 16 && patch != 32)) return 0;
  const int64_t n = (int64_t)((h + patch - 1) / patch) * ((w + patch - 1) / patch);
  return n < (1LL << 31) ? (int)n : 0;
}

int ammc_error_maps_f32(const float* pred, int64_t p_bs, int64_t p_cs, int64_t p_rs, const float* target, int64_t t_bs,
                        int64_t t_cs, int64_t t_rs, int32_t batch, int32_t c, int32_t h, int32_t w, int32_t patch,
                        float* patch_sum, int64_t ps_bs, float* patch_mean, float* pixel, int64_t px_bs, float* frame_sq,
                        float* worst, int32_t* worst_idx, void* stream) {
  if (!pred || !target || !patch_sum || !patch_mean || !frame_sq || !worst || !worst_idx) return AMMC_EINVAL;
  if (batch <= 0 || c <= 0 || h <= 0 || w <= 0) return AMMC_EINVAL;
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)patch_sum | (uintptr_t)patch_mean | (uintptr_t)pixel |
       (uintptr_t)frame_sq | (uintptr_t)worst | (uintptr_t)worst_idx) & 3)
    return AMMC_EINVAL;
  if (!em_strides_ok(p_bs, p_cs, p_rs, c, h, w) || !em_strides_ok(t_bs, t_cs, t_rs, c, h, w)) return AMMC_EINVAL;
  if (pixel && px_bs < (int64_t)h * w) return AMMC_EINVAL;
  if (patch != 8 && patch != 16 && patch != 32) return AMMC_EUNSUP;      // (the maps' extent needs the patch size)
  const int ph = (h + patch - 1) / patch, pw = (w + patch - 1) / patch;
  if (ps_bs < (int64_t)ph * pw) return AMMC_EINVAL;
  if (c > 4) return AMMC_EUNSUP;
  const int cq = patch == 8 ? 64 : 32;
  const int64_t chunks = ((int64_t)(w + 3) / 4 + cq - 1) / cq;
  // grid limits and the 32-bit patch indices (worst_idx, r * pw + j); element offsets are 64-bit
  if ((int64_t)batch * ph >= (1LL << 31) || chunks > 65535 || (int64_t)ph * pw >= (1LL << 31)) return AMMC_EUNSUP;

  const EmTensor tp = {pred, p_bs, p_cs, p_rs}, tt = {target, t_bs, t_cs, t_rs};
  // 16-byte loads: every quad of both tensors starts on a 16-byte boundary (quads start at multiples of 4 pixels)
  const bool vec = (((uintptr_t)pred | (uintptr_t)target) & 15) == 0 && ((p_bs | p_cs | p_rs | t_bs | t_cs | t_rs) & 3) == 0;
  const int px_vec = pixel && ((uintptr_t)pixel & 15) == 0 && ((px_bs | (int64_t)w) & 3) == 0;
  const dim3 grid((unsigned)(batch * ph), (unsigned)chunks);
  hipStream_t s = (hipStream_t)stream;
  if (patch == 8)
    em_launch_c<8>(c, vec, grid, s, tp, tt, h, w, ph, pw, patch_sum, patch_mean, ps_bs, pixel, px_bs, px_vec);
  else if (patch == 16)
    em_launch_c<16>(c, vec, grid, s, tp, tt, h, w, ph, pw, patch_sum, patch_mean, ps_bs, pixel, px_bs, px_vec);
  else
    em_launch_c<32>(c, vec, grid, s, tp, tt, h, w, ph, pw, patch_sum, patch_mean, ps_bs, pixel, px_bs, px_vec);
  int rc = ammc_launch_status();
  if (rc != AMMC_OK) return rc;
  hipLaunchKernelGGL(error_maps_tail_kernel, dim3((unsigned)batch), dim3(EM_TAIL_THREADS), 0, s, patch_sum, patch_mean, ps_bs,
                     ph, pw, frame_sq, worst, worst_idx);
  return ammc_launch_status();
}

}  // extern "C"
