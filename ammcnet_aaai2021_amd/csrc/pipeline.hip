// Device half of the input pipeline: what the reference's loaders do per frame on the CPU
// (Code/dataset/two_stream_dataset.py:72-99, 503-506) done once per frame on the GPU, from the raw decoded bytes.
//
//   frames: uint8 RGB (or BGR) [n][h][w][3] -> cv2.resize INTER_LINEAR (8-bit fixed-point form) -> ToTensor (/255)
//           -> Normalize(0.5, 0.5) -> float32 [n][3][oh][ow]
//   flows : float32 [n][h][w][2] (.flo payload) -> cv2.resize INTER_LINEAR (float form) -> channel 0 / oh,
//           channel 1 = (scaled channel 0) / ow (the reference's `_load_op`, :94-95) -> float32 [n][2][oh][ow]
//
// One thread per output pixel; HBM-bound streaming (uploading 1 byte per sample instead of 4, and each frame once
// instead of once per clip that contains it, is the point).  The arithmetic follows oracle/pipeline_oracle.py
// operation by operation (no FMA contraction: see `rounded`), so the results are bit-identical.
#include "resize_common.h"

namespace ammc_impl {

__global__ __launch_bounds__(256) void frames_u8_kernel(const uint8_t* __restrict__ src, int n, int h, int w,
                                                        float* __restrict__ dst, int oh, int ow, int bgr,
                                                        double sx, double sy) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n * oh * ow) return;
  const int dx = (int)(gid % ow);
  const int dy = (int)((gid / ow) % oh);
  const int f = (int)(gid / ((int64_t)ow * oh));
  const uint8_t* img = src + (int64_t)f * h * w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float o = normalize_u8(resize_u8_px(img, h, w, dx, dy, sx, sy, c));
    const int co = bgr ? 2 - c : c;
    dst[(((int64_t)f * 3 + co) * oh + dy) * ow + dx] = o;
  }
}

__global__ __launch_bounds__(256) void flows_kernel(const float* __restrict__ src, int n, int h, int w,
                                                    float* __restrict__ dst, int oh, int ow, double sx, double sy) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n * oh * ow) return;
  const int dx = (int)(gid % ow);
  const int dy = (int)((gid / ow) % oh);
  const int f = (int)(gid / ((int64_t)ow * oh));
  const float c0 = resize_flow_c0(src + (int64_t)f * h * w * 2, h, w, dx, dy, sx, sy, oh);
  const float c1 = flow_c1(c0, ow);
  dst[(((int64_t)f * 2 + 0) * oh + dy) * ow + dx] = c0;
  dst[(((int64_t)f * 2 + 1) * oh + dy) * ow + dx] = c1;
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" int ammc_frames_u8_to_f32(const uint8_t* src, int32_t n, int32_t h, int32_t w, float* dst, int32_t oh,
                                     int32_t ow, int32_t bgr, void* stream) {
  if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return AMMC_EINVAL;
  const int64_t total = (int64_t)n * oh * ow;
  if ((total + 255) / 256 > 0x7fffffff) return AMMC_EINVAL;
  hipLaunchKernelGGL(frames_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n,
                     h, w, dst, oh, ow, bgr ? 1 : 0, (double)w / (double)ow, (double)h / (double)oh);
  return ammc_launch_status();
}

extern "C" int ammc_flows_to_f32(const float* src, int32_t n, int32_t h, int32_t w, float* dst, int32_t oh, int32_t ow,
                                 void* stream) {
  if (!src || !dst || n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return AMMC_EINVAL;
  const int64_t total = (int64_t)n * oh * ow;
  if ((total + 255) / 256 > 0x7fffffff) return AMMC_EINVAL;
  hipLaunchKernelGGL(flows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n, h,
                     w, dst, oh, ow, (double)w / (double)ow, (double)h / (double)oh);
  return ammc_launch_status();
}
