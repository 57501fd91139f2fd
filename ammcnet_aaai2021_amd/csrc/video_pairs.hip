// Per-video pair counts of the score-fusion sweep, and the bilinear form that turns them into bootstrap replicas
// (the definitions are in include/ammc_hip.h).
//
//   C[g][s][a][b] = sum over the positive frames p of video a and the negative frames q of video b of
//                   (2 [key_p > key_q] + [key_p == key_q])                                    int64, exact
//
// with key = fs_key of the WHOLE sequence (sweep_keys.h): the smoothing takes its neighbour across video boundaries, so
// the sum of a block is ammc_fusion_sweep_f32's two_u of the same grid point, and C[a][a] / (2 P_a Q_a) video a's own AUC.
//
// video_pairs_kernel: one workgroup per (grid point, video b of the overall SMALLER class), nothing between workgroups.
//   1. the offsets of the other class's videos go to LDS (V + 1 words) and the V int64 totals are cleared;
//   2. the m_b keys of video b's frames of the smaller class are computed into LDS, padded with FS_SENTINEL to the next
//      power of two of m_b and sorted by fs_bitonic_sort (an empty video skips 2 and 3);
//   3. the other class is walked in one flat pass, 64 consecutive frames per wave and round: a lane computes its frame's
//      key, finds lb and ub by fusion_sweep's two binary searches, and its video a = the last one whose offset is <= its
//      position (a binary search over the V + 1 words in LDS; empty videos share an offset and are passed over).  The
//      lanes of a round that share a video - nearly always all 64 - add their counts by an xor tree, and lane 0 adds
//      the sum to the video's total with ONE 64-bit integer LDS add.  Integer sums: no order to fix;
//   4. after a barrier the V totals leave by plain vector stores: C[a][b] for a = 0 .. V - 1 when the negatives are the
//      sorted class, C[b][a] when the positives are.  The V workgroups of a grid point write its V x V block exactly once.
// LDS (dynamic): [V] int64 totals | [V + 1] int32 offsets, rounded up to 8 bytes | [mpad] uint32 keys, mpad the next power
// of two of the caller's bound on the longest segment.  At the limits (V = 1024, a segment of 32768): 8 KiB + 4 KiB + 128
// KiB = 140 KiB of the CU's 160.  256 threads up to mpad = 4096, 1024 above, as fusion_sweep.  The binary-search probes
// of a wave are data-dependent (up to 64 distinct words a probe); the sort's banking is fs_bitonic_sort's (5.20).
// Every offset read from the device is clamped into its list and every segment to the LDS it was given: malformed
// offsets give meaningless counts, never an access outside an array.
//
// bootstrap_pairs_kernel: out[r][g] = sum_ab mult[r][a] * mult[r][b] * pairs[g][a][b] in int64.  One workgroup per (128
// replicas, block g), a thread per replica.  Columns go in tiles of 64: the tile's multiplicities are put in LDS
// transposed ([64][128] words: a lane reads its own bank), then for every row a the thread forms sum_b m_b C[a][b] over
// the tile - C[a][b] is one address for the whole workgroup, the block is read once per 128 replicas - and adds m_a
// times it.  One plain store per replica.
#include "sweep_keys.h"                                // fs_key, fs_bitonic_sort; contraction off for the whole file

namespace ammc_impl {

constexpr int VP_MAX_SEGMENT = 32768;
constexpr int VP_MAX_VIDEOS = 1024;
constexpr int VP_THREADS_SMALL = 256;
constexpr int VP_THREADS_LARGE = 1024;
constexpr int VP_SMALL_PAD = 4096;                     // mpad up to which a workgroup has VP_THREADS_SMALL threads
constexpr int BP_REPLICAS = 128;                       // replicas (threads) per workgroup
constexpr int BP_TILE = 64;                            // columns per LDS tile

struct VpArgs {
  const float* chan;
  int64_t rs;
  const float* w;
  const float* sm;
  const int32_t* sorted_idx;                           // the smaller class: m frame indices in video order
  const int32_t* other_idx;                            // the other class: r frame indices in video order
  const int32_t* sorted_off;                           // [v + 1] offsets into sorted_idx
  const int32_t* other_off;                            // [v + 1] offsets into other_idx
  long long* pairs;
  int k, n, s, m, r, v, mpad;
  int sorted_is_neg;
};

extern __shared__ __attribute__((aligned(16))) unsigned char vp_smem[];

__device__ __forceinline__ int vp_clamp(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

__global__ __launch_bounds__(VP_THREADS_LARGE) void video_pairs_kernel(VpArgs p) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid % AMMC_WAVE;
  const int point = blockIdx.x / p.v, b = blockIdx.x - point * p.v;
  const int g = point / p.s, s = point - g * p.s;
  unsigned long long* __restrict__ tot = reinterpret_cast<unsigned long long*>(vp_smem);
  int* __restrict__ off = reinterpret_cast<int*>(vp_smem + (size_t)p.v * 8);
  unsigned* __restrict__ keys = reinterpret_cast<unsigned*>(vp_smem + (size_t)p.v * 8 + (((size_t)p.v + 2) & ~(size_t)1) * 4);

  for (int a = tid; a < p.v; a += nt) tot[a] = 0ull;
  for (int a = tid; a <= p.v; a += nt) off[a] = vp_clamp(p.other_off[a], p.r);
  const int sb = vp_clamp(p.sorted_off[b], p.m);
  int mb = vp_clamp(p.sorted_off[b + 1], p.m) - sb;
  mb = mb < 0 ? 0 : (mb > p.mpad ? p.mpad : mb);

  if (mb > 0) {                                        // (uniform over the workgroup)
    float w[FS_MAX_K];
#pragma unroll
    for (int c = 0; c < FS_MAX_K; ++c) w[c] = c < p.k ? p.w[(int64_t)g * p.k + c] : 0.f;
    const float fa = p.sm[2 * s], fb = p.sm[2 * s + 1];
    int mpad = 1;
    while (mpad < mb) mpad <<= 1;
    for (int j = tid; j < mpad; j += nt)
      keys[j] = j < mb ? fs_key(p.chan, p.rs, p.k, p.n, w, fa, fb, p.sorted_idx[sb + j]) : FS_SENTINEL;
    __syncthreads();                                   // the keys, the offsets and the cleared totals
    fs_bitonic_sort(keys, mpad, tid, nt);

    for (int base = tid - lane; base < p.r; base += nt) {
      const int e = base + lane;
      const bool live = e < p.r;
      long long c = 0;
      int a = -1;
      if (live) {
        const unsigned key = fs_key(p.chan, p.rs, p.k, p.n, w, fa, fb, p.other_idx[e]);
        int lo = 0, hi = mb;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        const int lb = lo;
        hi = mb;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (keys[mid] <= key) lo = mid + 1; else hi = mid;
        }
        const int ub = lo;
        c = p.sorted_is_neg ? (long long)lb + ub : 2LL * mb - lb - ub;
        lo = 0, hi = p.v - 1;                          // the last video whose offset is <= e
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (off[mid] <= e) lo = mid; else hi = mid - 1;
        }
        a = lo;
      }
      unsigned long long todo = __ballot(live);
      while (todo) {                                   // (uniform over the wave) one round per video among the 64 frames
        const int a0 = __shfl(a, __ffsll(todo) - 1, AMMC_WAVE);
        const bool mine = a == a0;
        long long part = mine ? c : 0;
#pragma unroll
        for (int o = 1; o < AMMC_WAVE; o <<= 1) part += __shfl_xor(part, o, AMMC_WAVE);
        if (lane == 0) atomicAdd(&tot[a0], (unsigned long long)part);
        todo &= ~__ballot(mine);
      }
    }
  }
  __syncthreads();                                     // every wave's adds (with mb == 0: the cleared totals)
  long long* __restrict__ blk = p.pairs + (int64_t)point * p.v * p.v;
  for (int a = tid; a < p.v; a += nt)
    blk[p.sorted_is_neg ? (int64_t)a * p.v + b : (int64_t)b * p.v + a] = (long long)tot[a];
}

__global__ __launch_bounds__(BP_REPLICAS) void bootstrap_pairs_kernel(const long long* __restrict__ pairs,
                                                                      const int32_t* __restrict__ mult, long long* __restrict__ out,
                                                                      int m, int v, int nb) {
  __shared__ int tile[BP_TILE][BP_REPLICAS];
  const int tid = threadIdx.x;
  const int g = blockIdx.x, r0 = blockIdx.y * BP_REPLICAS;
  const int r = r0 + tid < nb ? r0 + tid : nb - 1;     // (a thread past the last replica repeats it and stores nothing)
  const long long* __restrict__ blk = pairs + (int64_t)g * v * v;
  const int32_t* __restrict__ row = mult + (int64_t)r * v;
  long long acc = 0;
  for (int b0 = 0; b0 < v; b0 += BP_TILE) {
    const int nbt = v - b0 < BP_TILE ? v - b0 : BP_TILE;
    __syncthreads();                                   // the previous tile has been read
    for (int j = 0; j < nbt; ++j) tile[j][tid] = row[b0 + j];
    __syncthreads();
    for (int a = 0; a < v; ++a) {
      const long long* __restrict__ ca = blk + (int64_t)a * v + b0;
      long long inner = 0;
      for (int j = 0; j < nbt; ++j) inner += (long long)tile[j][tid] * ca[j];
      acc += (long long)row[a] * inner;
    }
  }
  if (r0 + tid < nb) out[(int64_t)r * m + g] = acc;
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_video_pairs_max_segment(void) { return VP_MAX_SEGMENT; }
int ammc_video_pairs_max_videos(void) { return VP_MAX_VIDEOS; }

int ammc_video_pairs_f32(const float* chan, int64_t chan_rs, int32_t k, int32_t n, const float* w, int32_t g, const float* sm,
                         int32_t s, const int32_t* pos_idx, int32_t n_pos, const int32_t* neg_idx, int32_t n_neg,
                         const int32_t* pos_off, const int32_t* neg_off, int32_t v, int32_t max_segment, int64_t* pairs,
                         void* stream) {
  if (!chan || !w || !sm || !pos_idx || !neg_idx || !pos_off || !neg_off || !pairs) return AMMC_EINVAL;
  if (k < 1 || k > FS_MAX_K || n < 2 || g < 1 || s < 1 || n_pos < 1 || n_neg < 1) return AMMC_EINVAL;
  if ((int64_t)n_pos + (int64_t)n_neg != (int64_t)n || chan_rs < (int64_t)n) return AMMC_EINVAL;
  if (v < 1 || v > VP_MAX_VIDEOS || max_segment < 1 || max_segment > VP_MAX_SEGMENT) return AMMC_EINVAL;
  if (((uintptr_t)chan | (uintptr_t)w | (uintptr_t)sm | (uintptr_t)pos_idx | (uintptr_t)neg_idx | (uintptr_t)pos_off |
       (uintptr_t)neg_off) & 3) return AMMC_EINVAL;
  if ((uintptr_t)pairs & 7) return AMMC_EINVAL;
  if ((int64_t)g * s * v >= (1LL << 31)) return AMMC_EUNSUP;  // the grid's x dimension

  const bool sort_neg = n_neg <= n_pos;
  const int m = sort_neg ? n_neg : n_pos;
  int mpad = 1;
  while (mpad < max_segment && mpad < m) mpad <<= 1;  // (a segment is never longer than its class)
  VpArgs a;
  a.chan = chan, a.rs = chan_rs, a.w = w, a.sm = sm;
  a.sorted_idx = sort_neg ? neg_idx : pos_idx, a.other_idx = sort_neg ? pos_idx : neg_idx;
  a.sorted_off = sort_neg ? neg_off : pos_off, a.other_off = sort_neg ? pos_off : neg_off;
  a.pairs = reinterpret_cast<long long*>(pairs);
  a.k = k, a.n = n, a.s = s, a.m = m, a.r = n - m, a.v = v, a.mpad = mpad;
  a.sorted_is_neg = sort_neg ? 1 : 0;
  const size_t lds = (size_t)v * 8 + (((size_t)v + 2) & ~(size_t)1) * 4 + (size_t)mpad * 4;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(video_pairs_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int threads = mpad <= VP_SMALL_PAD ? VP_THREADS_SMALL : VP_THREADS_LARGE;
  hipLaunchKernelGGL(video_pairs_kernel, dim3((unsigned)(g * s * v)), dim3(threads), lds, (hipStream_t)stream, a);
  return ammc_launch_status();
}

int ammc_bootstrap_pairs_i64(const int64_t* pairs, int32_t m, int32_t v, const int32_t* mult, int32_t b, int64_t* out,
                             void* stream) {
  if (!pairs || !mult || !out) return AMMC_EINVAL;
  if (m < 1 || v < 1 || v > VP_MAX_VIDEOS || b < 1) return AMMC_EINVAL;
  if (((uintptr_t)pairs | (uintptr_t)out) & 7 || (uintptr_t)mult & 3) return AMMC_EINVAL;
  const int chunks = (b + BP_REPLICAS - 1) / BP_REPLICAS;
  if (chunks > 65535) return AMMC_EUNSUP;              // the grid's y dimension
  hipLaunchKernelGGL(bootstrap_pairs_kernel, dim3((unsigned)m, (unsigned)chunks), dim3(BP_REPLICAS), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(pairs), mult, reinterpret_cast<long long*>(out), m, v, b);
  return ammc_launch_status();
}

}  // extern "C"
