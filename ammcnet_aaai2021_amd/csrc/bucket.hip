// Gradient buckets of data-parallel training (parallel.BucketedGradReducer): the gather of a bucket's member tensors
// into its flat all-reduce buffer, and the way back with the 1 / world average folded in - one launch each instead of
// torch's multi-tensor copy, multiply and copy.
//
// The member table (base pointers and end offsets in the flat buffer) travels BY VALUE in the kernel arguments (2 KB for
// AMMC_BUCKET_MAX members): nothing is uploaded, nothing on the device outlives the launch, so `.grad` tensors that are
// re-made every step cost nothing.  A workgroup owns BUCKET_CHUNK consecutive floats of the flat buffer, finds the first
// member that reaches into its chunk by a binary search of the end offsets (wave-uniform: scalar loads of the kernel
// arguments) and walks on through every member the chunk straddles.  A (chunk, member) run whose two sides are congruent
// modulo 16 bytes moves as float4 between a scalar head and tail; any other run moves float by float.
#include "ammc_common.h"

namespace ammc_impl {

constexpr int BUCKET_CHUNK = 4096;     // floats per workgroup: 4 float4 per lane

__device__ __forceinline__ int64_t bucket_start(const AmmcBucketTable& tab, int m, int pad) {
  if (m == 0) return 0;
  const int64_t e = tab.end[m - 1];
  return pad == 4 ? (e + 3) & ~(int64_t)3 : e;
}

template <bool UNPACK>
__global__ __launch_bounds__(256) void bucket_kernel(const AmmcBucketTable tab, const int n, const int pad,
                                                     float* __restrict__ flat, const float scale) {
  const int64_t c0 = (int64_t)blockIdx.x * BUCKET_CHUNK;
  const int64_t total = tab.end[n - 1];
  const int64_t c1 = c0 + BUCKET_CHUNK < total ? c0 + BUCKET_CHUNK : total;
  int lo = 0, hi = n - 1;                                   // first member with end > c0 (c0 < total: there is one)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab.end[mid] > c0) hi = mid; else lo = mid + 1;
  }
  const int t = (int)threadIdx.x;
  for (int m = lo; m < n; ++m) {
    const int64_t start = bucket_start(tab, m, pad);
    if (start >= c1) break;
    const int64_t end = tab.end[m];
    const int64_t a = start > c0 ? start : c0, b = end < c1 ? end : c1;
    if (a >= b) continue;                                   // (the chunk ends in the padding before this member)
    float* __restrict__ mem = (float*)tab.ptr[m] - start;   // indexed by the flat offset: mem[i] pairs with flat[i]
    const int64_t len = b - a;
    const bool vec = ((((uintptr_t)(flat + a)) ^ ((uintptr_t)(mem + a))) & 15) == 0;
    if (vec) {
      int64_t head = (int64_t)((16 - (((uintptr_t)(flat + a)) & 15)) & 15) >> 2;
      if (head > len) head = len;
      const int64_t nvec = (len - head) >> 2;
      const int64_t body = a + head, tail = body + 4 * nvec;
      for (int64_t i = t; i < nvec; i += 256) {
        if (UNPACK) {
          f32x4 v = *reinterpret_cast<const f32x4*>(flat + body + 4 * i);
          v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
          *reinterpret_cast<f32x4*>(mem + body + 4 * i) = v;
        } else {
          *reinterpret_cast<f32x4*>(flat + body + 4 * i) = *reinterpret_cast<const f32x4*>(mem + body + 4 * i);
        }
      }
      // at most 3 floats before and 3 after the vector body
      if (t < head) {
        if (UNPACK) mem[a + t] = flat[a + t] * scale; else flat[a + t] = mem[a + t];
      }
      if (t >= 64 && tail + (t - 64) < b) {
        const int64_t i = tail + (t - 64);
        if (UNPACK) mem[i] = flat[i] * scale; else flat[i] = mem[i];
      }
    } else {
      for (int64_t i = a + t; i < b; i += 256) {
        if (UNPACK) mem[i] = flat[i] * scale; else flat[i] = mem[i];
      }
    }
  }
}

static int bucket_check(const AmmcBucketTable* table, int32_t n, int32_t pad, const void* flat, int64_t* grid) {
  if (!table || !flat || n <= 0 || n > AMMC_BUCKET_MAX || (pad != 1 && pad != 4)) return AMMC_EINVAL;
  if ((uintptr_t)flat & (pad == 4 ? 15 : 3)) return AMMC_EINVAL;
  int64_t prev = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t start = pad == 4 ? (prev + 3) & ~(int64_t)3 : prev;
    if (!table->ptr[i] || ((uintptr_t)table->ptr[i] & 3) || table->end[i] <= start) return AMMC_EINVAL;
    prev = table->end[i];
  }
  *grid = (prev + BUCKET_CHUNK - 1) / BUCKET_CHUNK;
  return *grid > 0x7fffffff ? AMMC_EINVAL : AMMC_OK;
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" int ammc_bucket_pack_f32(const AmmcBucketTable* table, int32_t n, int32_t pad, float* flat, void* stream) {
  int64_t grid = 0;
  const int rc = bucket_check(table, n, pad, flat, &grid);
  if (rc != AMMC_OK) return rc;
  hipLaunchKernelGGL(bucket_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, *table, (int)n,
                     (int)pad, flat, 1.0f);
  return ammc_launch_status();
}

extern "C" int ammc_bucket_unpack_scale_f32(const AmmcBucketTable* table, int32_t n, int32_t pad, const float* flat,
                                            float scale, void* stream) {
  int64_t grid = 0;
  const int rc = bucket_check(table, n, pad, flat, &grid);
  if (rc != AMMC_OK) return rc;
  hipLaunchKernelGGL(bucket_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, *table, (int)n,
                     (int)pad, const_cast<float*>(flat), scale);
  return ammc_launch_status();
}
