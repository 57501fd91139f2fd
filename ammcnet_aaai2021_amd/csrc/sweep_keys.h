// What the score-fusion sweep (fusion_sweep.hip) and the curve sweep (curve_sweep.hip) share: the order-preserving key of
// a frame at one grid point and the bitonic network that sorts such keys in LDS.  Contraction into FMAs is off from
// here to the end of the including file: every product and sum of a key is a rounded fp32 operation.
#pragma once
#include "ammc_common.h"

#pragma clang fp contract(off)

namespace ammc_impl {

constexpr int FS_MAX_K = 8;
constexpr unsigned FS_SENTINEL = 0xFFFFFFFFu;          // above every finite key and both infinities: pads a sorted array

// the order-preserving key of frame i at one grid point: a set sign bit flips the word, a clear one sets it
__device__ __forceinline__ unsigned fs_key(const float* __restrict__ chan, int64_t rs, int k, int n, const float (&w)[FS_MAX_K],
                                           float a, float b, int i) {
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);
  const int h = i > 0 ? i - 1 : 0;
  float f = w[0] * chan[i], fh = w[0] * chan[h];
#pragma unroll
  for (int c = 1; c < FS_MAX_K; ++c) {
    if (c < k) {
      const float* __restrict__ row = chan + (int64_t)c * rs;
      f = f + w[c] * row[i];
      fh = fh + w[c] * row[h];
    }
  }
  const float t = i > 0 ? a * fh + b * f : f;
  const unsigned u = __float_as_uint(t + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the fp32 value a key stands for
__device__ __forceinline__ float fs_key_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// ascending bitonic network over mpad (a power of two) words of LDS, by the whole workgroup; a barrier behind each stage
__device__ __forceinline__ void fs_bitonic_sort(unsigned* __restrict__ keys, int mpad, int tid, int nt) {
  const int half = mpad >> 1;
  for (int k2 = 2; k2 <= mpad; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < half; t += nt) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const unsigned x = keys[lo], y = keys[hi];
        const bool up = (lo & k2) == 0;
        if ((x > y) == up) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace ammc_impl
