// Qualitative evaluation: finished uint8 panels of the predicted / target frames, the Middlebury colour code of the
// predicted / target flows and heat maps of the per-pixel errors, from a pass of its own behind the evaluation forward
// (the definitions are in include/ammc_hip.h).  Inputs fp32 NCHW, a sample contiguous, each with a batch stride of its
// own; output HWC uint8, one panel of rows x cols tiles of h x w x 3 bytes per sample, batch stride in bytes.
//
// Two kernels, both pure streaming:
//
//   render_stats_kernel   per sample the four maxima the tiles are normalised by (flow radius of the target and of the
//                         predicted flow, per-pixel error of the frame pair and of the flow pair).  A workgroup takes
//                         its maxima through a shuffle tree and LDS and publishes them with one integer atomicMax per
//                         value on the bits of the float: the values are non-negative and never NaN, so the order of
//                         their bits is the order of their values and the result is THE maximum - the same bits on
//                         every launch and for every grid.  The four words per sample are zeroed by a memset node on the
//                         same stream in front of the kernel, so nothing depends on what they held.
//   render_panels_kernel  a thread owns a "quad", 4 consecutive pixels of one image row starting at a multiple of 4, reads
//                         it ONCE from every input plane a chosen tile needs (one 16-byte load per plane) and writes its
//                         12 bytes of every chosen tile (three dwords).  Where w is not a multiple of 4, or a base or a
//                         batch stride is not aligned, the same code runs on scalar loads and byte stores (the last
//                         quad of a row is ragged); both forms hand the same registers to the same arithmetic.
//
// Arithmetic: fp32, nothing contracted into an FMA except where an fmaf is written out.  hipcc's division and square
// root are correctly rounded (the default -fhip-fp32-correctly-rounded-divide-sqrt), so the maxima equal an fp32
// restatement in any IEEE library bit for bit; atan2f is the one library call (a few ulp from others).
#include "ammc_common.h"

namespace ammc_impl {

constexpr int RD_THREADS = 256;
constexpr int RD_WAVES = RD_THREADS / AMMC_WAVE;
constexpr int RD_STAT_CHUNKS = 64;                     // workgroups per sample of the stats kernel, at most
constexpr int RD_NTILE = 6;
constexpr int RD_NCOL = 55;                            // entries of the colour wheel
enum { RD_RGB_PRED = 0, RD_RGB_TARGET = 1, RD_OP_PRED = 2, RD_OP_TARGET = 3 };                      // inputs
enum { RD_T_RGB_TARGET = 0, RD_T_RGB_PRED, RD_T_RGB_HEAT, RD_T_OP_TARGET, RD_T_OP_PRED, RD_T_OP_HEAT };   // tiles (the C ABI's ids)

// the Middlebury wheel from its published segment lengths (red-yellow 15, yellow-green 6, green-cyan 4, cyan-blue 11,
// blue-magenta 13, magenta-red 6): one channel ramps floor(255 i / n) up or down along a segment; stored as value / 255
struct RdWheel {
  float c[RD_NCOL][3];
  constexpr RdWheel() : c{} {
    const int seg[6] = {15, 6, 4, 11, 13, 6};
    const int full[6] = {0, 1, 1, 2, 2, 0};            // the channel at 255 along the segment
    const int ramp[6] = {1, 0, 2, 1, 0, 2};            // the channel that ramps: up in even segments, down in odd ones
    int k = 0;
    for (int s = 0; s < 6; ++s)
      for (int i = 0; i < seg[s]; ++i, ++k) {
        const int r = 255 * i / seg[s];
        int v[3] = {0, 0, 0};
        v[full[s]] = 255;
        v[ramp[s]] = s % 2 == 0 ? r : 255 - r;
        for (int ch = 0; ch < 3; ++ch) c[k][ch] = (float)v[ch] / 255.0f;
      }
  }
};
__constant__ RdWheel rd_wheel = RdWheel();

struct RdArgs {
  const float* src[4];                                 // rgb_pred, rgb_target, op_pred, op_target (NULL: not read)
  int64_t bs[4];
  int h, w;
  float su, sv, alpha;
  int cols;                                            // tiles per panel row
  int cell[RD_NTILE];                                  // per tile id: its place in the panel (row-major), -1 = not drawn
  const float* stats;                                  // [batch][4] of render_stats_kernel (NULL where every value is supplied)
  const float* max_rad;                                // [batch] or NULL: supplied flow normalisation (both flow tiles)
  const float* heat_rgb;                               // [batch] or NULL: supplied heat_max of the frame pair
  const float* heat_op;                                // [batch] or NULL: of the flow pair
  int each;                                            // the predicted flow by its own maximum, not the target's
  uint8_t* out;
  int64_t out_bs;
};

// 4 consecutive pixels at `p` of C planes `plane` floats apart; `cnt` of them exist (1..4), the rest read as 0
template <int C, bool VEC>
__device__ __forceinline__ void rd_load(const float* __restrict__ p, int64_t plane, int cnt, float (&v)[C][4]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ q = p + c * plane;
    if (VEC && cnt == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = t[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = i < cnt ? q[i] : 0.f;
    }
  }
}

template <int C>
__device__ __forceinline__ void rd_zero(float (&v)[C][4]) {
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
}

struct RdFlow {
  float u, v, raw;                                     // scaled components (0 where unknown) and their radius
  bool known;
};

__device__ __forceinline__ RdFlow rd_flow(float f0, float f1, float su, float sv) {
#pragma clang fp contract(off)
  RdFlow r;
  const float u = su * f0, v = sv * f1;
  r.known = fabsf(u) <= 1e7f && fabsf(v) <= 1e7f;      // false for a NaN as well
  r.u = r.known ? u : 0.f;
  r.v = r.known ? v : 0.f;
  r.raw = sqrtf(r.u * r.u + r.v * r.v);
  return r;
}

// mean over the channels of ((target - pred) / 2)^2, channels added in order: ops.error_maps' `pixel`
template <int C>
__device__ __forceinline__ float rd_err(const float (&p)[C][4], const float (&t)[C][4], int i) {
#pragma clang fp contract(off)
  const float e0 = 0.5f * (t[0][i] - p[0][i]);
  float acc = e0 * e0;
#pragma unroll
  for (int c = 1; c < C; ++c) {
    const float e = 0.5f * (t[c][i] - p[c][i]);
    acc = acc + e * e;
  }
  const float e = acc / (float)C;
  return e == e ? e : 0.f;                             // a NaN error counts as none
}

// floor(clamp((x + 1) * 127.5, 0, 255) + 0.5) of the REAL value: x is clamped to [-1, 1] first (NaN -> -1), the affine
// map is one fmaf (one rounding), and where that rounding reached the next integer from below the sign of a second
// fmaf - exact value minus that integer, whose sign no rounding changes - takes the step back
__device__ __forceinline__ unsigned rd_frame_u8(float x) {
  const float xc = fminf(fmaxf(x, -1.f), 1.f);
  float n = floorf(fmaf(xc, 127.5f, 128.f));
  if (fmaf(xc, 127.5f, 128.f - n) < 0.f) n -= 1.f;
  return (unsigned)n;
}

__device__ __forceinline__ unsigned rd_pack(float r, float g, float b) {
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// the colour code of one flow vector; maxrad / inv: the sample's normalisation
__device__ __forceinline__ unsigned rd_flow_rgb(const RdFlow& fl, float maxrad, float inv) {
#pragma clang fp contract(off)
  if (!fl.known) return 0u;
  const bool inside = fl.raw <= maxrad;
  const float rad = fminf(fl.raw * inv, 1.f);
  const float a = atan2f(-fl.v, -fl.u) / 3.14159265358979323846f;
  const float fk = (a + 1.f) / 2.f * (float)(RD_NCOL - 1) + 1.f;
  const float k0f = fminf(fmaxf(floorf(fk), 1.f), (float)RD_NCOL);
  const int k0 = (int)k0f;
  const int k1 = k0 == RD_NCOL ? 1 : k0 + 1;
  const float f = fk - k0f;
  float o[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float col = (1.f - f) * rd_wheel.c[k0 - 1][ch] + f * rd_wheel.c[k1 - 1][ch];
    col = inside ? 1.f - rad * (1.f - col) : col * 0.75f;
    o[ch] = fminf(fmaxf(floorf(255.f * col), 0.f), 255.f);
  }
  return rd_pack(o[0], o[1], o[2]);
}

// the heat colour of error e over the grey value `grey` (0..255)
__device__ __forceinline__ unsigned rd_heat_rgb(float e, float hmax, float grey, float alpha) {
#pragma clang fp contract(off)
  const float t = hmax > 0.f ? fminf(e / hmax, 1.f) : 0.f;
  const float base = (1.f - alpha) * grey, gain = alpha * 255.f;
  float o[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float c = fminf(fmaxf(1.5f - fabsf(4.f * t - (float)(3 - ch)), 0.f), 1.f);
    o[ch] = fminf(fmaxf(floorf(base + gain * c + 0.5f), 0.f), 255.f);
  }
  return rd_pack(o[0], o[1], o[2]);
}

struct RdBytes12 {
  unsigned a, b, c;
};

// 4 pixels (0x00BBGGRR each) as 12 consecutive bytes r g b r g b ...
template <bool VEC>
__device__ __forceinline__ void rd_store(uint8_t* __restrict__ o, const unsigned (&px)[4], int cnt) {
  if (VEC) {
    RdBytes12 v;
    v.a = px[0] | (px[1] << 24);
    v.b = (px[1] >> 8) | (px[2] << 16);
    v.c = (px[2] >> 16) | (px[3] << 8);
    *reinterpret_cast<RdBytes12*>(o) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < cnt) {
        o[3 * i] = (uint8_t)(px[i] & 0xffu);
        o[3 * i + 1] = (uint8_t)((px[i] >> 8) & 0xffu);
        o[3 * i + 2] = (uint8_t)((px[i] >> 16) & 0xffu);
      }
  }
}

// VEC: every quad of every given plane starts on a 16-byte boundary (h * w % 4 == 0, bases and batch strides aligned)
template <bool VEC>
__global__ __launch_bounds__(RD_THREADS) void render_stats_kernel(RdArgs a, float* __restrict__ stats) {
  __shared__ float red[RD_WAVES][4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = (int64_t)a.h * a.w, nq = (n + 3) / 4;
  const bool rgb = a.src[RD_RGB_PRED] && a.src[RD_RGB_TARGET];
  const bool fp_on = a.src[RD_OP_PRED] != nullptr, ft_on = a.src[RD_OP_TARGET] != nullptr;
  float m[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t q = (int64_t)blockIdx.x * RD_THREADS + tid; q < nq; q += (int64_t)gridDim.x * RD_THREADS) {
    const int64_t pix = q * 4;
    const int cnt = (int)(n - pix < 4 ? n - pix : 4);
    float rp[3][4], rt[3][4], fp[2][4], ft[2][4];
    if (rgb) {
      rd_load<3, VEC>(a.src[RD_RGB_PRED] + b * a.bs[RD_RGB_PRED] + pix, n, cnt, rp);
      rd_load<3, VEC>(a.src[RD_RGB_TARGET] + b * a.bs[RD_RGB_TARGET] + pix, n, cnt, rt);
    } else {
      rd_zero<3>(rp), rd_zero<3>(rt);
    }
    if (fp_on) rd_load<2, VEC>(a.src[RD_OP_PRED] + b * a.bs[RD_OP_PRED] + pix, n, cnt, fp);
    else rd_zero<2>(fp);
    if (ft_on) rd_load<2, VEC>(a.src[RD_OP_TARGET] + b * a.bs[RD_OP_TARGET] + pix, n, cnt, ft);
    else rd_zero<2>(ft);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= cnt) continue;
      const RdFlow t = rd_flow(ft[0][i], ft[1][i], a.su, a.sv), p = rd_flow(fp[0][i], fp[1][i], a.su, a.sv);
      m[0] = t.raw > m[0] ? t.raw : m[0];
      m[1] = p.raw > m[1] ? p.raw : m[1];
      if (rgb) {
        const float e = rd_err<3>(rp, rt, i);
        m[2] = e > m[2] ? e : m[2];
      }
      if (fp_on && ft_on) {
        const float e = t.known && p.known ? rd_err<2>(fp, ft, i) : 0.f;
        m[3] = e > m[3] ? e : m[3];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 1; o < AMMC_WAVE; o <<= 1) m[k] = fmaxf(m[k], __shfl_xor(m[k], o, AMMC_WAVE));
  }
  if (tid % AMMC_WAVE == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[tid / AMMC_WAVE][k] = m[k];
  }
  __syncthreads();
  if (tid < 4) {
    float v = red[0][tid];
#pragma unroll
    for (int wv = 1; wv < RD_WAVES; ++wv) v = fmaxf(v, red[wv][tid]);
    // non-negative, never NaN: the unsigned order of the bits is the order of the values
    atomicMax(reinterpret_cast<unsigned*>(stats) + 4 * (int64_t)b + tid, __float_as_uint(v));
  }
}

// VEC: w % 4 == 0, every base 16-byte and the output 4-byte aligned, batch strides whole quads / dwords
template <bool VEC>
__global__ __launch_bounds__(RD_THREADS) void render_panels_kernel(RdArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int qw = (a.w + 3) >> 2;
  const int64_t q = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x;
  if (q >= (int64_t)a.h * qw) return;
  const int y = (int)(q / qw), x0 = (int)(q - (int64_t)y * qw) * 4;
  const int cnt = min(4, a.w - x0);
  const int64_t plane = (int64_t)a.h * a.w, pix = (int64_t)y * a.w + x0;

  const bool d_rt = a.cell[RD_T_RGB_TARGET] >= 0, d_rp = a.cell[RD_T_RGB_PRED] >= 0, d_rh = a.cell[RD_T_RGB_HEAT] >= 0;
  const bool d_ft = a.cell[RD_T_OP_TARGET] >= 0, d_fp = a.cell[RD_T_OP_PRED] >= 0, d_fh = a.cell[RD_T_OP_HEAT] >= 0;
  float rp[3][4], rt[3][4], fp[2][4], ft[2][4];
  if (d_rp || d_rh) rd_load<3, VEC>(a.src[RD_RGB_PRED] + b * a.bs[RD_RGB_PRED] + pix, plane, cnt, rp);
  else rd_zero<3>(rp);
  if (d_rt || d_rh) rd_load<3, VEC>(a.src[RD_RGB_TARGET] + b * a.bs[RD_RGB_TARGET] + pix, plane, cnt, rt);
  else rd_zero<3>(rt);
  if (d_fp || d_fh) rd_load<2, VEC>(a.src[RD_OP_PRED] + b * a.bs[RD_OP_PRED] + pix, plane, cnt, fp);
  else rd_zero<2>(fp);
  if (d_ft || d_fh) rd_load<2, VEC>(a.src[RD_OP_TARGET] + b * a.bs[RD_OP_TARGET] + pix, plane, cnt, ft);
  else rd_zero<2>(ft);

  // the sample's normalisations (uniform over the workgroup)
  float mr_t = 0.f, mr_p = 0.f, hm_rgb = 0.f, hm_op = 0.f;
  if (d_ft || d_fp) {
    mr_t = a.max_rad ? a.max_rad[b] : a.stats[4 * (int64_t)b];
    mr_p = a.max_rad ? mr_t : (a.each ? a.stats[4 * (int64_t)b + 1] : mr_t);
  }
  if (d_rh) hm_rgb = a.heat_rgb ? a.heat_rgb[b] : a.stats[4 * (int64_t)b + 2];
  if (d_fh) hm_op = a.heat_op ? a.heat_op[b] : a.stats[4 * (int64_t)b + 3];
  const float inv_t = 1.f / (mr_t + 0x1p-52f), inv_p = 1.f / (mr_p + 0x1p-52f);

  unsigned c_rt[4], c_rp[4], c_rh[4], c_ft[4], c_fp[4], c_fh[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c_rt[i] = c_rp[i] = c_rh[i] = c_ft[i] = c_fp[i] = c_fh[i] = 0u;
    if (d_rt || d_rh) {
      const unsigned r = rd_frame_u8(rt[0][i]), g = rd_frame_u8(rt[1][i]), bl = rd_frame_u8(rt[2][i]);
      c_rt[i] = r | (g << 8) | (bl << 16);
      if (d_rh) c_rh[i] = rd_heat_rgb(rd_err<3>(rp, rt, i), hm_rgb, (float)(r + g + bl) / 3.f, a.alpha);
    }
    if (d_rp) c_rp[i] = rd_frame_u8(rp[0][i]) | (rd_frame_u8(rp[1][i]) << 8) | (rd_frame_u8(rp[2][i]) << 16);
    if (d_ft || d_fp || d_fh) {
      const RdFlow t = rd_flow(ft[0][i], ft[1][i], a.su, a.sv), p = rd_flow(fp[0][i], fp[1][i], a.su, a.sv);
      if (d_ft) c_ft[i] = rd_flow_rgb(t, mr_t, inv_t);
      if (d_fp) c_fp[i] = rd_flow_rgb(p, mr_p, inv_p);
      if (d_fh) c_fh[i] = rd_heat_rgb(t.known && p.known ? rd_err<2>(fp, ft, i) : 0.f, hm_op, 128.f, a.alpha);
    }
  }

  uint8_t* __restrict__ ob = a.out + b * a.out_bs;
  const int64_t row_bytes = (int64_t)a.cols * a.w * 3;
#define RD_EMIT(ID, PX)                                                                                    \
  if (a.cell[ID] >= 0) {                                                                                   \
    const int tr = a.cell[ID] / a.cols, tc = a.cell[ID] - tr * a.cols;                                     \
    rd_store<VEC>(ob + ((int64_t)tr * a.h + y) * row_bytes + ((int64_t)tc * a.w + x0) * 3, PX, cnt);       \
  }
  RD_EMIT(RD_T_RGB_TARGET, c_rt)
  RD_EMIT(RD_T_RGB_PRED, c_rp)
  RD_EMIT(RD_T_RGB_HEAT, c_rh)
  RD_EMIT(RD_T_OP_TARGET, c_ft)
  RD_EMIT(RD_T_OP_PRED, c_fp)
  RD_EMIT(RD_T_OP_HEAT, c_fh)
#undef RD_EMIT
}

static bool rd_aligned(const RdArgs& a, int batch, int64_t unit) {
  // every given input: base 16-byte aligned, batch stride whole quads; `unit` (w or h * w) a multiple of 4
  if (unit & 3) return false;
  for (int k = 0; k < 4; ++k)
    if (a.src[k] && (((uintptr_t)a.src[k] & 15) || (batch > 1 && (a.bs[k] & 3)))) return false;
  return true;
}

// shapes and inputs, common to the entries: 0 or a status code
static int rd_check_inputs(const RdArgs& a, int batch) {
  if (batch < 1 || a.h < 1 || a.w < 1) return AMMC_EINVAL;
  if (!(fabsf(a.su) <= 3.0e38f) || !(fabsf(a.sv) <= 3.0e38f)) return AMMC_EINVAL;      // finite scales
  const int64_t n = (int64_t)a.h * a.w;
  const int chans[4] = {3, 3, 2, 2};
  for (int k = 0; k < 4; ++k) {
    if (!a.src[k]) continue;
    if ((uintptr_t)a.src[k] & 3) return AMMC_EINVAL;
    if (batch > 1 && a.bs[k] < chans[k] * n) return AMMC_EINVAL;
  }
  if (batch > 65535 || n > (1LL << 28)) return AMMC_EUNSUP;      // the grid's y dimension; quads on its x dimension
  return AMMC_OK;
}

static int rd_stats(const RdArgs& a, int batch, float* stats, hipStream_t s) {
  const int64_t n = (int64_t)a.h * a.w, nq = (n + 3) / 4;
  int64_t chunks = (nq + RD_THREADS * 4 - 1) / (RD_THREADS * 4);
  chunks = chunks > RD_STAT_CHUNKS ? RD_STAT_CHUNKS : chunks;
  const dim3 grid((unsigned)chunks, (unsigned)batch), block(RD_THREADS);
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(float) * 4 * (size_t)batch, s);
  if (e != hipSuccess) return (int)e;
  if (rd_aligned(a, batch, n)) hipLaunchKernelGGL(render_stats_kernel<true>, grid, block, 0, s, a, stats);
  else hipLaunchKernelGGL(render_stats_kernel<false>, grid, block, 0, s, a, stats);
  return ammc_launch_status();
}

static int rd_panels(const RdArgs& a, int batch, hipStream_t s) {
  const int64_t quads = (int64_t)a.h * ((a.w + 3) / 4);
  const dim3 grid((unsigned)((quads + RD_THREADS - 1) / RD_THREADS), (unsigned)batch), block(RD_THREADS);
  const bool vec = rd_aligned(a, batch, a.w) && ((uintptr_t)a.out & 3) == 0 && (batch == 1 || (a.out_bs & 3) == 0);
  if (vec) hipLaunchKernelGGL(render_panels_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(render_panels_kernel<false>, grid, block, 0, s, a);
  return ammc_launch_status();
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_render_stats_f32(const float* rgb_pred, int64_t rp_bs, const float* rgb_target, int64_t rt_bs, const float* op_pred,
                          int64_t fp_bs, const float* op_target, int64_t ft_bs, int32_t batch, int32_t h, int32_t w, float su,
                          float sv, float* stats, void* stream) {
  if (!stats || ((uintptr_t)stats & 3)) return AMMC_EINVAL;
  if (!rgb_pred != !rgb_target) return AMMC_EINVAL;                // the frame pair: both or neither
  if (!rgb_pred && !op_pred && !op_target) return AMMC_EINVAL;
  RdArgs a = {};
  a.src[RD_RGB_PRED] = rgb_pred, a.src[RD_RGB_TARGET] = rgb_target, a.src[RD_OP_PRED] = op_pred, a.src[RD_OP_TARGET] = op_target;
  a.bs[RD_RGB_PRED] = rp_bs, a.bs[RD_RGB_TARGET] = rt_bs, a.bs[RD_OP_PRED] = fp_bs, a.bs[RD_OP_TARGET] = ft_bs;
  a.h = h, a.w = w, a.su = su, a.sv = sv;
  const int rc = rd_check_inputs(a, batch);
  if (rc != AMMC_OK) return rc;
  return rd_stats(a, batch, stats, (hipStream_t)stream);
}

int ammc_render_panels_u8(const float* rgb_pred, int64_t rp_bs, const float* rgb_target, int64_t rt_bs, const float* op_pred,
                          int64_t fp_bs, const float* op_target, int64_t ft_bs, int32_t batch, int32_t h, int32_t w, float su,
                          float sv, const int32_t* tiles, int32_t rows, int32_t cols, const float* stats, int32_t flow_each,
                          const float* max_rad, const float* heat_rgb, const float* heat_op, float alpha, uint8_t* out,
                          int64_t out_bs, void* stream) {
  if (!tiles || !out) return AMMC_EINVAL;
  if (rows < 1 || cols < 1 || (int64_t)rows * cols > RD_NTILE) return AMMC_EINVAL;
  if (!(alpha >= 0.f && alpha <= 1.f) || (flow_each != 0 && flow_each != 1)) return AMMC_EINVAL;
  RdArgs a = {};
  a.src[RD_RGB_PRED] = rgb_pred, a.src[RD_RGB_TARGET] = rgb_target, a.src[RD_OP_PRED] = op_pred, a.src[RD_OP_TARGET] = op_target;
  a.bs[RD_RGB_PRED] = rp_bs, a.bs[RD_RGB_TARGET] = rt_bs, a.bs[RD_OP_PRED] = fp_bs, a.bs[RD_OP_TARGET] = ft_bs;
  a.h = h, a.w = w, a.su = su, a.sv = sv, a.alpha = alpha, a.cols = cols;
  a.stats = stats, a.max_rad = max_rad, a.heat_rgb = heat_rgb, a.heat_op = heat_op, a.each = flow_each;
  a.out = out, a.out_bs = out_bs;
  for (int t = 0; t < RD_NTILE; ++t) a.cell[t] = -1;
  for (int c = 0; c < rows * cols; ++c) {
    const int t = tiles[c];
    if (t < 0 || t >= RD_NTILE || a.cell[t] >= 0) return AMMC_EINVAL;      // an ordered subset: every tile at most once
    a.cell[t] = c;
  }
  const bool d_rt = a.cell[RD_T_RGB_TARGET] >= 0, d_rp = a.cell[RD_T_RGB_PRED] >= 0, d_rh = a.cell[RD_T_RGB_HEAT] >= 0;
  const bool d_ft = a.cell[RD_T_OP_TARGET] >= 0, d_fp = a.cell[RD_T_OP_PRED] >= 0, d_fh = a.cell[RD_T_OP_HEAT] >= 0;
  if (((d_rp || d_rh) && !rgb_pred) || ((d_rt || d_rh) && !rgb_target) || ((d_fp || d_fh) && !op_pred) ||
      ((d_ft || d_fh) && !op_target))
    return AMMC_EINVAL;                                            // a chosen tile reads an input that is not given
  const bool need_stats = ((d_ft || d_fp) && !max_rad) || (d_rh && !heat_rgb) || (d_fh && !heat_op);
  if (need_stats && !stats) return AMMC_EINVAL;
  if (((uintptr_t)stats | (uintptr_t)max_rad | (uintptr_t)heat_rgb | (uintptr_t)heat_op) & 3) return AMMC_EINVAL;
  const int rc = rd_check_inputs(a, batch);
  if (rc != AMMC_OK) return rc;
  if (batch > 1 && out_bs < (int64_t)rows * cols * h * w * 3) return AMMC_EINVAL;
  return rd_panels(a, batch, (hipStream_t)stream);
}

int ammc_flow_colour_u8(const float* flow, int64_t flow_bs, int32_t batch, int32_t h, int32_t w, float su, float sv,
                        const float* max_rad, float* workspace, uint8_t* out, int64_t out_bs, void* stream) {
  if (!flow || !out) return AMMC_EINVAL;
  if (!max_rad && (!workspace || ((uintptr_t)workspace & 3))) return AMMC_EINVAL;
  if ((uintptr_t)max_rad & 3) return AMMC_EINVAL;
  RdArgs a = {};
  a.src[RD_OP_TARGET] = flow, a.bs[RD_OP_TARGET] = flow_bs;
  a.h = h, a.w = w, a.su = su, a.sv = sv, a.cols = 1;
  a.stats = workspace, a.max_rad = max_rad, a.out = out, a.out_bs = out_bs;
  for (int t = 0; t < RD_NTILE; ++t) a.cell[t] = -1;
  a.cell[RD_T_OP_TARGET] = 0;
  int rc = rd_check_inputs(a, batch);
  if (rc != AMMC_OK) return rc;
  if (batch > 1 && out_bs < (int64_t)h * w * 3) return AMMC_EINVAL;
  if (!max_rad) {
    rc = rd_stats(a, batch, workspace, (hipStream_t)stream);
    if (rc != AMMC_OK) return rc;
  }
  return rd_panels(a, batch, (hipStream_t)stream);
}

}  // extern "C"
