// Device-resident clip bank of the training loop (pipeline.ClipBank, run_train.py): every frame of the training set is
// decoded once per run, resized once into the bank, and each iteration's clips are gathered from it by one launch.
//
// The bank holds exactly what the reference's per-clip arithmetic (two_stream_dataset.py:307-333) depends on, so a
// gathered clip is bit-identical to `frames_u8_kernel` / `flows_kernel` (pipeline.hip) on the same frame:
//   rgb bank: uint8 [N][3][H][W], the 8-bit fixed-point resize result `v` (planar, RGB order); the float a clip
//             holds is a function of `v` alone (`normalize_u8`), a quarter of the fp32 bytes.
//   op bank : float32 [N][H][W], channel 0 of `_load_op` (`c0 = u / H`); channel 1 is `c0 / W` (:329-330), derived at
//             gather time as `flows_kernel` derives it.
#include "resize_common.h"

namespace ammc_impl {

__global__ __launch_bounds__(256) void frames_resize_u8_kernel(const uint8_t* __restrict__ src, int n, int h, int w,
                                                               uint8_t* __restrict__ dst, int oh, int ow, int bgr,
                                                               double sx, double sy) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n * oh * ow) return;
  const int dx = (int)(gid % ow);
  const int dy = (int)((gid / ow) % oh);
  const int f = (int)(gid / ((int64_t)ow * oh));
  const uint8_t* img = src + (int64_t)f * h * w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int co = bgr ? 2 - c : c;
    dst[(((int64_t)f * 3 + co) * oh + dy) * ow + dx] = (uint8_t)resize_u8_px(img, h, w, dx, dy, sx, sy, c);
  }
}

__global__ __launch_bounds__(256) void flows_resize_c0_kernel(const float* __restrict__ src, int n, int h, int w,
                                                              float* __restrict__ dst, int oh, int ow, double sx,
                                                              double sy) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n * oh * ow) return;
  const int dx = (int)(gid % ow);
  const int dy = (int)((gid / ow) % oh);
  const int f = (int)(gid / ((int64_t)ow * oh));
  dst[((int64_t)f * oh + dy) * ow + dx] = resize_flow_c0(src + (int64_t)f * h * w * 2, h, w, dx, dy, sx, sy, oh);
}

// One launch per iteration.  blockIdx.y = (sample b, source plane r): r < rgb_len * 3 is (frame, channel) of the rgb
// clip, the rest one op frame (its c0 plane becomes the clip's two channels).  Each thread moves 4 pixels: a uchar4 /
// float4 load, 16-byte stores.  A first index outside [0, n - len] (the host validates them all, this is the last line)
// reads nothing and writes NaN, so a bad index can never reach outside the banks.
__global__ __launch_bounds__(256) void gather_clips_kernel(const uint8_t* __restrict__ rgb_bank, int64_t n_rgb,
                                                           const float* __restrict__ op_bank, int64_t n_op,
                                                           const int32_t* __restrict__ rgb_first,
                                                           const int32_t* __restrict__ op_first, int rgb_len,
                                                           int op_len, int h, int w, float* __restrict__ rgb_out,
                                                           float* __restrict__ op_out) {
  const int64_t hw = (int64_t)h * w;
  const int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (q >= hw) return;
  const int planes = rgb_len * 3 + op_len;
  const int b = (int)blockIdx.y / planes, r = (int)blockIdx.y % planes;
  const float nan = __builtin_nanf("");
  if (r < rgb_len * 3) {
    const int t = r / 3, c = r % 3;
    const int64_t first = rgb_first[b];
    float4 o = make_float4(nan, nan, nan, nan);
    if (first >= 0 && first + rgb_len <= n_rgb) {
      const uchar4 v = *reinterpret_cast<const uchar4*>(rgb_bank + ((first + t) * 3 + c) * hw + q);
      o = make_float4(normalize_u8(v.x), normalize_u8(v.y), normalize_u8(v.z), normalize_u8(v.w));
    }
    *reinterpret_cast<float4*>(rgb_out + (((int64_t)b * rgb_len + t) * 3 + c) * hw + q) = o;
  } else {
    const int t = r - rgb_len * 3;
    const int64_t first = op_first[b];
    float4 c0 = make_float4(nan, nan, nan, nan), c1 = c0;
    if (first >= 0 && first + op_len <= n_op) {
      c0 = *reinterpret_cast<const float4*>(op_bank + (first + t) * hw + q);
      c1 = make_float4(flow_c1(c0.x, w), flow_c1(c0.y, w), flow_c1(c0.z, w), flow_c1(c0.w, w));
    }
    float* dst = op_out + (((int64_t)b * op_len + t) * 2) * hw + q;
    *reinterpret_cast<float4*>(dst) = c0;
    *reinterpret_cast<float4*>(dst + hw) = c1;
  }
}

// The clips of ONE bank (a single-stream training stage: rgb or op only), the same scheme as `gather_clips_kernel`:
// blockIdx.y = (sample b, source plane r) of that bank alone, so every clip is written by the same arithmetic as the
// matching half of `gather_clips_kernel` - bit-identical for the same indices.  `op` selects the bank: 0 = rgb (uint8
// [N][3][H][W] -> normalised float, 3 planes per frame), 1 = op (c0 float [N][H][W] -> (c0, c0 / w), 1 plane per frame).
__global__ __launch_bounds__(256) void gather_clips_one_kernel(const void* __restrict__ bank, int64_t n, int op,
                                                               const int32_t* __restrict__ first_idx, int len, int h,
                                                               int w, float* __restrict__ out) {
  const int64_t hw = (int64_t)h * w;
  const int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (q >= hw) return;
  const int planes = op ? len : len * 3;
  const int b = (int)blockIdx.y / planes, r = (int)blockIdx.y % planes;
  const int64_t first = first_idx[b];
  const bool ok = first >= 0 && first + len <= n;
  const float nan = __builtin_nanf("");
  if (!op) {
    const int t = r / 3, c = r % 3;
    float4 o = make_float4(nan, nan, nan, nan);
    if (ok) {
      const uchar4 v = *reinterpret_cast<const uchar4*>((const uint8_t*)bank + ((first + t) * 3 + c) * hw + q);
      o = make_float4(normalize_u8(v.x), normalize_u8(v.y), normalize_u8(v.z), normalize_u8(v.w));
    }
    *reinterpret_cast<float4*>(out + (((int64_t)b * len + t) * 3 + c) * hw + q) = o;
  } else {
    const int t = r;
    float4 c0 = make_float4(nan, nan, nan, nan), c1 = c0;
    if (ok) {
      c0 = *reinterpret_cast<const float4*>((const float*)bank + (first + t) * hw + q);
      c1 = make_float4(flow_c1(c0.x, w), flow_c1(c0.y, w), flow_c1(c0.z, w), flow_c1(c0.w, w));
    }
    float* dst = out + (((int64_t)b * len + t) * 2) * hw + q;
    *reinterpret_cast<float4*>(dst) = c0;
    *reinterpret_cast<float4*>(dst + hw) = c1;
  }
}

// ---- two tiers: frames [0, n_dev) of a kind in device memory, frames [n_dev, n) in pinned, device-mapped host memory ----
//
// One launch for a batch whose clips lie anywhere in a bank split between the tiers (pipeline.ClipBank with a host
// budget).  blockIdx.y = (sample b, source plane r) as in `gather_clips_kernel`; a kind whose `first` is NULL has no
// planes, so the same kernel serves the joint stage and both single stages.  blockIdx.x = a chunk of TIER_CHUNK pixels
// of the plane.  The frame, and with it the tier, is a function of (b, r) alone: `first` goes through readfirstlane,
// the choice of tier is a scalar branch and a clip may straddle the split.  Every path writes what
// `gather_clips_kernel` writes for the pixel (`normalize_u8`, `flow_c1`, NaN for a first index outside [0, n - len],
// nothing read), so the output is bit-identical wherever the split lies.
//
// The host tier is read over the host link, where the latency of a load is microseconds and nothing is cached between
// launches: its loads are 16 bytes per lane (1 KiB contiguous per wave instruction) and each lane issues TIER_LOADS
// independent ones before the first use, so a wave has 4 KiB and a workgroup 16 KiB of contiguous reads in flight.
//   rgb, h * w % 16 == 0: a uint4 = 16 pixels in, four float4 stores out;  op: one float4 in, two out;
//   rgb otherwise (h * w % 4 == 0): uchar4 loads, TIER_LOADS in flight as well.
// A lane past the end of the plane loads the plane's last 16 bytes again (an address select, no branch: a branch around
// a load makes the compiler wait for the loads before it) and stores nothing.
constexpr int TIER_LOADS = 4;                          // independent 16-byte loads per lane before the first use
constexpr int64_t TIER_CHUNK = 256 * 16 * TIER_LOADS;  // pixels of one plane per workgroup: 16 KiB of wide rgb reads

__device__ __forceinline__ float4 normalize_u8x4(uint32_t p) {
  return make_float4(normalize_u8((uint8_t)(p & 0xff)), normalize_u8((uint8_t)((p >> 8) & 0xff)),
                     normalize_u8((uint8_t)((p >> 16) & 0xff)), normalize_u8((uint8_t)(p >> 24)));
}

// 4 pixels per load (the device tier, and a host tier whose planes are no multiple of 16 pixels)
__device__ __forceinline__ void tier_rgb_narrow(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t q0,
                                                int64_t hw) {
  for (int64_t base = q0; base < q0 + TIER_CHUNK && base < hw; base += 256 * 4 * TIER_LOADS) {
    uint32_t v[TIER_LOADS];
#pragma unroll
    for (int i = 0; i < TIER_LOADS; ++i) {
      const int64_t q = base + ((int64_t)i * 256 + threadIdx.x) * 4;
      v[i] = *reinterpret_cast<const uint32_t*>(src + (q < hw ? q : hw - 4));
    }
#pragma unroll
    for (int i = 0; i < TIER_LOADS; ++i) {
      const int64_t q = base + ((int64_t)i * 256 + threadIdx.x) * 4;
      if (q < hw) *reinterpret_cast<float4*>(dst + q) = normalize_u8x4(v[i]);
    }
  }
}

// 16 pixels per load: the whole chunk is TIER_LOADS loads per lane, all issued before the first conversion
__device__ __forceinline__ void tier_rgb_wide(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t q0,
                                              int64_t hw) {
  uint4 v[TIER_LOADS];
#pragma unroll
  for (int i = 0; i < TIER_LOADS; ++i) {
    const int64_t q = q0 + ((int64_t)i * 256 + threadIdx.x) * 16;
    v[i] = *reinterpret_cast<const uint4*>(src + (q < hw ? q : hw - 16));
  }
#pragma unroll
  for (int i = 0; i < TIER_LOADS; ++i) {
    const int64_t q = q0 + ((int64_t)i * 256 + threadIdx.x) * 16;
    if (q < hw) {
      float4* o = reinterpret_cast<float4*>(dst + q);
      o[0] = normalize_u8x4(v[i].x);
      o[1] = normalize_u8x4(v[i].y);
      o[2] = normalize_u8x4(v[i].z);
      o[3] = normalize_u8x4(v[i].w);
    }
  }
}

__device__ __forceinline__ void tier_op(const float* __restrict__ src, float* __restrict__ dst, int64_t q0, int64_t hw,
                                        int w) {
  for (int64_t base = q0; base < q0 + TIER_CHUNK && base < hw; base += 256 * 4 * TIER_LOADS) {
    float4 v[TIER_LOADS];
#pragma unroll
    for (int i = 0; i < TIER_LOADS; ++i) {
      const int64_t q = base + ((int64_t)i * 256 + threadIdx.x) * 4;
      v[i] = *reinterpret_cast<const float4*>(src + (q < hw ? q : hw - 4));
    }
#pragma unroll
    for (int i = 0; i < TIER_LOADS; ++i) {
      const int64_t q = base + ((int64_t)i * 256 + threadIdx.x) * 4;
      if (q < hw) {
        const float4 c0 = v[i];
        *reinterpret_cast<float4*>(dst + q) = c0;
        *reinterpret_cast<float4*>(dst + hw + q) =
            make_float4(flow_c1(c0.x, w), flow_c1(c0.y, w), flow_c1(c0.z, w), flow_c1(c0.w, w));
      }
    }
  }
}

// NaN over the chunk of `count` consecutive output planes (1: an rgb plane; 2: both channels of an op frame)
__device__ __forceinline__ void tier_nan(float* __restrict__ dst, int64_t q0, int64_t hw, int count) {
  const float nan = __builtin_nanf("");
  const float4 o = make_float4(nan, nan, nan, nan);
  for (int64_t q = q0 + (int64_t)threadIdx.x * 4; q < q0 + TIER_CHUNK && q < hw; q += 256 * 4)
    for (int p = 0; p < count; ++p) *reinterpret_cast<float4*>(dst + p * hw + q) = o;
}

struct TierBank {
  const void* dev;        // frames [0, n_dev)
  const void* host;       // frames [n_dev, n), device-mapped host memory
  int64_t n_dev, n;
};

__global__ __launch_bounds__(256) void gather_clips_tiered_kernel(TierBank rgb, TierBank op,
                                                                  const int32_t* __restrict__ rgb_first,
                                                                  const int32_t* __restrict__ op_first, int rgb_len,
                                                                  int op_len, int h, int w, float* __restrict__ rgb_out,
                                                                  float* __restrict__ op_out) {
  const int64_t hw = (int64_t)h * w;
  const int64_t q0 = (int64_t)blockIdx.x * TIER_CHUNK;
  const int rgb_planes = rgb_first ? rgb_len * 3 : 0;
  const int planes = rgb_planes + (op_first ? op_len : 0);
  const int b = (int)blockIdx.y / planes, r = (int)blockIdx.y % planes;
  if (r < rgb_planes) {
    const int t = r / 3, c = r % 3;
    const int64_t first = __builtin_amdgcn_readfirstlane(rgb_first[b]);
    float* dst = rgb_out + (((int64_t)b * rgb_len + t) * 3 + c) * hw;
    if (first < 0 || first + rgb_len > rgb.n) {
      tier_nan(dst, q0, hw, 1);
      return;
    }
    const int64_t f = first + t;
    if (f < rgb.n_dev) {
      tier_rgb_narrow((const uint8_t*)rgb.dev + (f * 3 + c) * hw, dst, q0, hw);
    } else {
      const uint8_t* src = (const uint8_t*)rgb.host + ((f - rgb.n_dev) * 3 + c) * hw;
      if (hw % 16 == 0)
        tier_rgb_wide(src, dst, q0, hw);
      else
        tier_rgb_narrow(src, dst, q0, hw);
    }
  } else {
    const int t = r - rgb_planes;
    const int64_t first = __builtin_amdgcn_readfirstlane(op_first[b]);
    float* dst = op_out + (((int64_t)b * op_len + t) * 2) * hw;
    if (first < 0 || first + op_len > op.n) {
      tier_nan(dst, q0, hw, 2);
      return;
    }
    const int64_t f = first + t;
    const float* src = f < op.n_dev ? (const float*)op.dev + f * hw : (const float*)op.host + (f - op.n_dev) * hw;
    tier_op(src, dst, q0, hw, w);
  }
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" int ammc_frames_u8_resize_u8(const uint8_t* src, int32_t n, int32_t h, int32_t w, uint8_t* dst, int32_t oh,
                                        int32_t ow, int32_t bgr, void* stream) {
  if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return AMMC_EINVAL;
  const int64_t total = (int64_t)n * oh * ow;
  if ((total + 255) / 256 > 0x7fffffff) return AMMC_EINVAL;
  hipLaunchKernelGGL(frames_resize_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src, n, h, w, dst, oh, ow, bgr ? 1 : 0, (double)w / (double)ow, (double)h / (double)oh);
  return ammc_launch_status();
}

extern "C" int ammc_flows_resize_c0(const float* src, int32_t n, int32_t h, int32_t w, float* dst, int32_t oh,
                                    int32_t ow, void* stream) {
  if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return AMMC_EINVAL;
  const int64_t total = (int64_t)n * oh * ow;
  if ((total + 255) / 256 > 0x7fffffff) return AMMC_EINVAL;
  hipLaunchKernelGGL(flows_resize_c0_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src, n, h, w, dst, oh, ow, (double)w / (double)ow, (double)h / (double)oh);
  return ammc_launch_status();
}

extern "C" int ammc_gather_clips(const uint8_t* rgb_bank, int64_t n_rgb, const float* op_bank, int64_t n_op,
                                 const int32_t* rgb_first, const int32_t* op_first, int32_t batch, int32_t rgb_len,
                                 int32_t op_len, int32_t h, int32_t w, float* rgb_out, float* op_out, void* stream) {
  if (!rgb_bank || !op_bank || !rgb_first || !op_first || !rgb_out || !op_out) return AMMC_EINVAL;
  if (batch <= 0 || rgb_len <= 0 || op_len <= 0 || h <= 0 || w <= 0 || n_rgb < rgb_len || n_op < op_len)
    return AMMC_EINVAL;
  const int64_t hw = (int64_t)h * w;
  if (hw % 4 != 0) return AMMC_EINVAL;                                  // 4 pixels per thread, 16-byte aligned planes
  if (((uintptr_t)rgb_bank & 3) || ((uintptr_t)op_bank & 15) || ((uintptr_t)rgb_out & 15) || ((uintptr_t)op_out & 15))
    return AMMC_EINVAL;
  const int64_t grid_y = (int64_t)batch * ((int64_t)rgb_len * 3 + op_len);
  const int64_t grid_x = (hw / 4 + 255) / 256;
  if (grid_y > 65535 || grid_x > 0x7fffffff) return AMMC_EINVAL;
  hipLaunchKernelGGL(gather_clips_kernel, dim3((unsigned)grid_x, (unsigned)grid_y), dim3(256), 0, (hipStream_t)stream,
                     rgb_bank, n_rgb, op_bank, n_op, rgb_first, op_first, (int)rgb_len, (int)op_len, (int)h, (int)w,
                     rgb_out, op_out);
  return ammc_launch_status();
}

extern "C" int ammc_gather_clips_one(const void* bank, int64_t n, int32_t kind, const int32_t* first, int32_t batch,
                                     int32_t len, int32_t h, int32_t w, float* out, void* stream) {
  if (!bank || !first || !out || (kind != 0 && kind != 1)) return AMMC_EINVAL;
  if (batch <= 0 || len <= 0 || h <= 0 || w <= 0 || n < len) return AMMC_EINVAL;
  const int64_t hw = (int64_t)h * w;
  if (hw % 4 != 0) return AMMC_EINVAL;                                  // 4 pixels per thread, 16-byte aligned planes
  if (((uintptr_t)bank & (kind ? 15 : 3)) || ((uintptr_t)out & 15)) return AMMC_EINVAL;
  const int64_t grid_y = (int64_t)batch * (kind ? len : (int64_t)len * 3);
  const int64_t grid_x = (hw / 4 + 255) / 256;
  if (grid_y > 65535 || grid_x > 0x7fffffff) return AMMC_EINVAL;
  hipLaunchKernelGGL(gather_clips_one_kernel, dim3((unsigned)grid_x, (unsigned)grid_y), dim3(256), 0,
                     (hipStream_t)stream, bank, n, (int)kind, first, (int)len, (int)h, (int)w, out);
  return ammc_launch_status();
}

// A host tier reaches the kernel only as memory the device can address: pinned (hipHostMalloc) or registered
// (hipHostRegister).  `*mapped` is the address the device uses for it.  A pageable pointer - which the runtime reports
// as an error or as unregistered memory, depending on its version - is refused.
static bool tier_host_mapped(const void* host, const void** mapped) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, host) != hipSuccess) {
    (void)hipGetLastError();                                            // not this launch's error: clear it
    return false;
  }
  if (at.type != hipMemoryTypeHost || !at.devicePointer) return false;
  *mapped = at.devicePointer;
  return true;
}

extern "C" int ammc_gather_clips_tiered(const uint8_t* rgb_dev, const uint8_t* rgb_host, int64_t n_rgb_dev,
                                        int64_t n_rgb, const float* op_dev, const float* op_host, int64_t n_op_dev,
                                        int64_t n_op, const int32_t* rgb_first, const int32_t* op_first, int32_t batch,
                                        int32_t rgb_len, int32_t op_len, int32_t h, int32_t w, float* rgb_out,
                                        float* op_out, void* stream) {
  if (!rgb_first && !op_first) return AMMC_EINVAL;
  if (batch <= 0 || h <= 0 || w <= 0) return AMMC_EINVAL;
  const int64_t hw = (int64_t)h * w;
  if (hw % 4 != 0) return AMMC_EINVAL;                                  // 4 pixels per thread, 16-byte aligned planes
  if (rgb_first) {
    if (!rgb_out || ((uintptr_t)rgb_out & 15) || rgb_len <= 0 || n_rgb_dev < 0 || n_rgb_dev > n_rgb || n_rgb < rgb_len)
      return AMMC_EINVAL;
    if (n_rgb_dev > 0 && (!rgb_dev || ((uintptr_t)rgb_dev & 3))) return AMMC_EINVAL;
    if (n_rgb > n_rgb_dev && (!rgb_host || ((uintptr_t)rgb_host & 15))) return AMMC_EINVAL;
  }
  if (op_first) {
    if (!op_out || ((uintptr_t)op_out & 15) || op_len <= 0 || n_op_dev < 0 || n_op_dev > n_op || n_op < op_len)
      return AMMC_EINVAL;
    if (n_op_dev > 0 && (!op_dev || ((uintptr_t)op_dev & 15))) return AMMC_EINVAL;
    if (n_op > n_op_dev && (!op_host || ((uintptr_t)op_host & 15))) return AMMC_EINVAL;
  }
  const int64_t grid_y = (int64_t)batch * ((rgb_first ? (int64_t)rgb_len * 3 : 0) + (op_first ? op_len : 0));
  const int64_t grid_x = (hw + TIER_CHUNK - 1) / TIER_CHUNK;
  if (grid_y > 65535 || grid_x > 0x7fffffff) return AMMC_EINVAL;
  // the one check that asks the runtime comes last: everything above is decided without a device
  TierBank rgb = {rgb_dev, nullptr, n_rgb_dev, n_rgb}, op = {op_dev, nullptr, n_op_dev, n_op};
  if (rgb_first && n_rgb > n_rgb_dev && !tier_host_mapped(rgb_host, &rgb.host)) return AMMC_EINVAL;
  if (op_first && n_op > n_op_dev && !tier_host_mapped(op_host, &op.host)) return AMMC_EINVAL;
  if (((uintptr_t)rgb.host & 15) || ((uintptr_t)op.host & 15)) return AMMC_EINVAL;
  hipLaunchKernelGGL(gather_clips_tiered_kernel, dim3((unsigned)grid_x, (unsigned)grid_y), dim3(256), 0,
                     (hipStream_t)stream, rgb, op, rgb_first, op_first, (int)rgb_len, (int)op_len, (int)h, (int)w,
                     rgb_out, op_out);
  return ammc_launch_status();
}
