// Shared arithmetic of the input pipeline's resize (pipeline.hip, clip_bank.hip): the cv2.resize INTER_LINEAR source
// coordinate and the FMA barrier, so every kernel that resizes a frame rounds exactly as oracle/pipeline_oracle.py does.
#pragma once
#include "ammc_common.h"

// hipcc contracts a * b + c into an FMA by default (its __fmul_rn / __fadd_rn are plain operators and a file-scope
// `#pragma clang fp contract(off)` did not stop it): every product that feeds a sum goes through `rounded()`, an
// empty asm the optimiser cannot look through, so products and sums are rounded separately, as the CPU loaders
// (and the oracle) compute them
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

namespace ammc_impl {

struct Coord { int s; float f; };

__device__ __forceinline__ Coord src_coord(int d, double scale, int src) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f = __fsub_rn(f, (float)s);
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  Coord c; c.s = s; c.f = f;
  return c;
}

// the 8-bit fixed-point resize of channel c of one output pixel of an interleaved uint8 [h][w][3] image: the value `v`
// that ToTensor / Normalize then see (`frames_u8_kernel`, `frames_resize_u8_kernel`)
__device__ __forceinline__ int resize_u8_px(const uint8_t* img, int h, int w, int dx, int dy, double sx, double sy,
                                            int c) {
  const Coord cx = src_coord(dx, sx, w), cy = src_coord(dy, sy, h);
  const int ax1 = (int)rintf(__fmul_rn(cx.f, 2048.f)), ax0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, cx.f), 2048.f));
  const int by1 = (int)rintf(__fmul_rn(cy.f, 2048.f)), by0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, cy.f), 2048.f));
  const int x1 = min(cx.s + 1, w - 1), y1 = min(cy.s + 1, h - 1);
  const uint8_t* r0 = img + (int64_t)cy.s * w * 3;
  const uint8_t* r1 = img + (int64_t)y1 * w * 3;
  const int s0 = (int)r0[cx.s * 3 + c] * ax0 + (int)r0[x1 * 3 + c] * ax1;
  const int s1 = (int)r1[cx.s * 3 + c] * ax0 + (int)r1[x1 * 3 + c] * ax1;
  const int v = (((by0 * (s0 >> 4)) >> 16) + ((by1 * (s1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ToTensor (/255) + Normalize(0.5, 0.5) of a resized 8-bit value
__device__ __forceinline__ float normalize_u8(int v) {
  const float t = __fdiv_rn((float)v, 255.f);
  return __fdiv_rn(__fsub_rn(t, 0.5f), 0.5f);
}

// the float resize of channel 0 of one output pixel of a [h][w][2] flow, divided by the output height: `c0` of `_load_op`
__device__ __forceinline__ float resize_flow_c0(const float* img, int h, int w, int dx, int dy, double sx, double sy,
                                                int oh) {
  const Coord cx = src_coord(dx, sx, w), cy = src_coord(dy, sy, h);
  const float a1 = cx.f, a0 = __fsub_rn(1.f, cx.f), b1 = cy.f, b0 = __fsub_rn(1.f, cy.f);
  const int x1 = min(cx.s + 1, w - 1), y1 = min(cy.s + 1, h - 1);
  const float* r0 = img + (int64_t)cy.s * w * 2;
  const float* r1 = img + (int64_t)y1 * w * 2;
  // only channel 0 reaches the output: channel 1 is re-derived from it (two_stream_dataset.py:94-95)
  const float s0 = rounded(r0[cx.s * 2] * a0) + rounded(r0[x1 * 2] * a1);
  const float s1 = rounded(r1[cx.s * 2] * a0) + rounded(r1[x1 * 2] * a1);
  const float u = rounded(rounded(s0) * b0) + rounded(rounded(s1) * b1);
  return rounded(u) / (float)oh;                      // `img * 1.0 / image_height` (the * 1.0 is exact)
}

// channel 1 of `_load_op`: the already scaled channel 0 over the output width
__device__ __forceinline__ float flow_c1(float c0, int ow) { return rounded(c0) / (float)ow; }

}  // namespace ammc_impl
