// Score-fusion sweep: the exact AUC numerator of a weighted, one-tap-smoothed fusion of K score channels at every point
// of a (weight vector, smoothing pair) grid - a stand-alone pass over [K][N] normalised frame scores and a partition of
// the N frames into the positive (normal) and the negative class.  The definition is in include/ammc_hip.h:
//
//   f[i]   = ((w[g][0] * chan[0][i] + w[g][1] * chan[1][i]) + w[g][2] * chan[2][i]) + ...      rounded fp32, left to right
//   t[0]   = f[0];  t[i] = a * f[i - 1] + b * f[i]     (a, b) = sm[s]; from the UNSMOOTHED neighbour, no restart
//   key    = t + 0.0f                                   (-0.0 and +0.0 tie)
//   two_u[g][s] = sum over positive p, negative q of (2 [t_p > t_q] + [t_p == t_q])           int64, exact
//
// One launch, one workgroup per grid point, nothing passes between workgroups, no atomics, no arrival counter: the only
// reduction is an integer sum, so the result does not depend on an order.
//   1. the keys of the SMALLER class (m of them) are computed straight from chan (index i and i - 1 from global memory:
//      the channels stay in L2) and mapped to order-preserving uint32: a set sign bit flips the word, a clear one sets
//      it - every finite key and both infinities lie below the sentinel 0xFFFFFFFF that pads the array to mpad, the
//      next power of two;
//   2. a bitonic network sorts the mpad words in LDS: log2(mpad) (log2(mpad) + 1) / 2 stages of mpad / 2
//      compare-exchanges, a barrier behind each.  A thread's pair is (i, i | j) with the bit j inserted into its item
//      number: for j >= 32 the 32 lanes of a half-wave are on 32 consecutive words twice (no bank conflict); for j < 32
//      the lanes' words are 2 j-periodic with a hole of j, so the 32 lanes fall on 16 banks twice over (a 2-way conflict
//      on both the low and the high word) - 5 log2(mpad) - 10 of the stages, 65 of the 120 at mpad = 32768;
//   3. every thread takes its share of the OTHER class, computes the key and finds lb = #{sorted < key} and
//      ub = #{sorted <= key} by binary search over the m real words (ub starts at lb);
//        negatives sorted: a positive adds lb + ub            (2 lb below it + (ub - lb) ties)
//        positives sorted: a negative adds 2 m - lb - ub      (2 (m - ub) above it + (ub - lb) ties)
//   4. the counts are added in int64: a xor tree over the 64 lanes, the waves through LDS (the key array is dead by
//      then), one plain vector store of the total.
// LDS: 4 mpad bytes, dynamic (at least 128 for the wave totals): several workgroups per CU for a small class, 128 KiB
// of the CU's 160 at mpad = 32768 = ammc_fusion_sweep_max_sorted().  256 threads up to mpad = 4096, 1024 above.
// Frame indices are clamped to [0, n): a list that is not a partition of 0..n-1 gives a meaningless count, never an
// access outside chan.  Contraction into FMAs is off for the whole file: every product and sum above is rounded.
#include "sweep_keys.h"                                // fs_key, fs_bitonic_sort; contraction off for the whole file

namespace ammc_impl {

constexpr int FS_MAX_SORTED = 32768;
constexpr int FS_THREADS_SMALL = 256;
constexpr int FS_THREADS_LARGE = 1024;
constexpr int FS_SMALL_PAD = 4096;                     // mpad up to which a workgroup has FS_THREADS_SMALL threads
constexpr int FS_MAX_WAVES = FS_THREADS_LARGE / AMMC_WAVE;

struct FsArgs {
  const float* chan;
  int64_t rs;
  const float* w;
  const float* sm;
  const int32_t* sorted_idx;                           // the smaller class: m frame indices
  const int32_t* other_idx;                            // the other class: r frame indices
  long long* two_u;
  int k, n, s, m, mpad, r;
  int sorted_is_neg;
};

extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];

__global__ __launch_bounds__(FS_THREADS_LARGE) void fusion_sweep_kernel(FsArgs p) {
  unsigned* __restrict__ keys = reinterpret_cast<unsigned*>(fs_smem);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int g = blockIdx.x / p.s, s = blockIdx.x - g * p.s;
  float w[FS_MAX_K];
#pragma unroll
  for (int c = 0; c < FS_MAX_K; ++c) w[c] = c < p.k ? p.w[(int64_t)g * p.k + c] : 0.f;
  const float a = p.sm[2 * s], b = p.sm[2 * s + 1];

  for (int j = tid; j < p.mpad; j += nt)
    keys[j] = j < p.m ? fs_key(p.chan, p.rs, p.k, p.n, w, a, b, p.sorted_idx[j]) : FS_SENTINEL;
  __syncthreads();

  fs_bitonic_sort(keys, p.mpad, tid, nt);

  long long acc = 0;
  for (int e = tid; e < p.r; e += nt) {
    const unsigned key = fs_key(p.chan, p.rs, p.k, p.n, w, a, b, p.other_idx[e]);
    int lo = 0, hi = p.m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int lb = lo;
    hi = p.m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    const int ub = lo;
    acc += p.sorted_is_neg ? (long long)lb + ub : 2LL * p.m - lb - ub;
  }
#pragma unroll
  for (int o = 1; o < AMMC_WAVE; o <<= 1) acc += __shfl_xor(acc, o, AMMC_WAVE);
  __syncthreads();                                     // every search has read the keys: the array is free
  long long* __restrict__ red = reinterpret_cast<long long*>(fs_smem);
  if (tid % AMMC_WAVE == 0) red[tid / AMMC_WAVE] = acc;
  __syncthreads();
  if (tid == 0) {
    long long total = red[0];
    for (int v = 1; v < nt / AMMC_WAVE; ++v) total += red[v];
    p.two_u[blockIdx.x] = total;
  }
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_fusion_sweep_max_sorted(void) { return FS_MAX_SORTED; }

int ammc_fusion_sweep_f32(const float* chan, int64_t chan_rs, int32_t k, int32_t n, const float* w, int32_t g, const float* sm,
                          int32_t s, const int32_t* pos_idx, int32_t n_pos, const int32_t* neg_idx, int32_t n_neg,
                          int64_t* two_u, void* stream) {
  if (!chan || !w || !sm || !pos_idx || !neg_idx || !two_u) return AMMC_EINVAL;
  if (k < 1 || k > FS_MAX_K || n < 2 || g < 1 || s < 1 || n_pos < 1 || n_neg < 1) return AMMC_EINVAL;
  if ((int64_t)n_pos + (int64_t)n_neg != (int64_t)n || chan_rs < (int64_t)n) return AMMC_EINVAL;
  if (((uintptr_t)chan | (uintptr_t)w | (uintptr_t)sm | (uintptr_t)pos_idx | (uintptr_t)neg_idx) & 3) return AMMC_EINVAL;
  if ((uintptr_t)two_u & 7) return AMMC_EINVAL;
  const bool sort_neg = n_neg <= n_pos;
  const int m = sort_neg ? n_neg : n_pos;
  if (m > FS_MAX_SORTED) return AMMC_EINVAL;
  if ((int64_t)g * s >= (1LL << 31)) return AMMC_EUNSUP;     // the grid's x dimension

  int mpad = 1;
  while (mpad < m) mpad <<= 1;
  FsArgs a;
  a.chan = chan, a.rs = chan_rs, a.w = w, a.sm = sm;
  a.sorted_idx = sort_neg ? neg_idx : pos_idx;
  a.other_idx = sort_neg ? pos_idx : neg_idx;
  a.two_u = reinterpret_cast<long long*>(two_u);
  a.k = k, a.n = n, a.s = s, a.m = m, a.mpad = mpad, a.r = n - m;
  a.sorted_is_neg = sort_neg ? 1 : 0;
  const size_t wave_bytes = FS_MAX_WAVES * sizeof(long long);
  const size_t lds = (size_t)mpad * 4 > wave_bytes ? (size_t)mpad * 4 : wave_bytes;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fusion_sweep_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int threads = mpad <= FS_SMALL_PAD ? FS_THREADS_SMALL : FS_THREADS_LARGE;
  hipLaunchKernelGGL(fusion_sweep_kernel, dim3((unsigned)(g * s)), dim3(threads), lds, (hipStream_t)stream, a);
  return ammc_launch_status();
}

}  // extern "C"
