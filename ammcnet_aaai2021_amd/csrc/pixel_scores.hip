// Pixel-level evaluation: per sample of a score map and a ground-truth mask, the k-th largest map value inside the
// mask and the largest values inside and outside it (the definitions are in include/ammc_hip.h).  A stand-alone pass:
// map fp32 [batch][h * w], mask uint8 [batch][h * w], a sample contiguous, each with a batch stride of its own.
//
// NO floating-point operation touches a map value.  A value enters as its 32 bits and is compared through the
// order-preserving key of those bits,
//
//   key(b) = b has its sign bit ? ~b : b | 0x80000000        (negative values reversed below the non-negative ones)
//
// so key(x) < key(y) exactly when x < y for every pair of non-NaN values (with -0.0 one step below +0.0), denormals
// included, and an output is the inverse of a key: one of the stored values, bit for bit.
//
// One workgroup per sample, a radix select over the keys in PS_PASSES = 3 passes of 11, 11 and 10 bits, most
// significant first.  A pass re-reads the sample, counts the mask pixels whose key matches the prefix found so far in a
// histogram of PS_BINS LDS words by the digit of the pass (integer LDS atomics: a count has no order), and wave 0 then
// walks the counts from the top bin down to the bin that holds rank k: that digit joins the prefix, the count above
// it leaves k.  The first pass also takes the two maxima (integer maxima of keys) and the histogram's total is m, from
// which k follows.  After the last pass the prefix is the key itself.  Counts and integer maxima do not depend on
// which thread saw which pixel, so the outputs are a function of the sample's values and mask alone.
//
// A thread reads "quads", 4 consecutive pixels of the flat sample starting at a multiple of 4: one 16-byte map load and
// one 4-byte mask load where the bases and batch strides allow, scalar loads where not and in the ragged last quad;
// both forms hand the same registers to the same code.  Plain stores, workgroup barriers, nothing between workgroups.
#include "ammc_common.h"

namespace ammc_impl {

constexpr int PS_MAX_THREADS = 1024;
constexpr int PS_BINS = 2048;                          // 11 bits: the widest digit
constexpr int PS_PASSES = 3;
constexpr int PS_UNROLL = 4;                           // quads a thread has in flight
constexpr int PS_LANE_BINS = PS_BINS / AMMC_WAVE;      // bins a lane of wave 0 owns in the scan

__device__ __forceinline__ unsigned ps_key(unsigned bits) { return bits & 0x80000000u ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ unsigned ps_bits(unsigned key) { return key & 0x80000000u ? key ^ 0x80000000u : ~key; }

struct PsQuad {
  unsigned v[4];                                       // the map values' bits
  unsigned mk;                                         // byte j: the mask of pixel j
};

// quad q of a sample of n pixels; pixels past the end read as (0, outside) and are never counted (`cnt`)
template <bool MAPV, bool MASKV>
__device__ __forceinline__ void ps_load(const unsigned* __restrict__ map, const uint8_t* __restrict__ mask, int q, int n,
                                        PsQuad& o) {
  const int i = q * 4, cnt = min(4, n - i);
  if (MAPV && cnt == 4) {
    const ammc_u4 t = *reinterpret_cast<const ammc_u4*>(map + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = t[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = j < cnt ? map[i + j] : 0u;
  }
  if (MASKV && cnt == 4) {
    o.mk = *reinterpret_cast<const unsigned*>(mask + i);
  } else {
    o.mk = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) o.mk |= (unsigned)mask[i + j] << (8 * j);
  }
}

template <bool MAPV, bool MASKV>
__global__ __launch_bounds__(PS_MAX_THREADS) void pixel_scores_kernel(const float* __restrict__ map_f, int64_t map_bs,
                                                                      const uint8_t* __restrict__ mask_p, int64_t mask_bs,
                                                                      int n, int frac_num, int frac_den,
                                                                      int* __restrict__ m_out, float* __restrict__ kth,
                                                                      float* __restrict__ max_in,
                                                                      float* __restrict__ max_out) {
  __shared__ unsigned hist[PS_BINS];
  __shared__ unsigned s_max[2];                        // the largest key inside / outside the mask
  __shared__ unsigned s_m, s_digit, s_rank;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const unsigned* __restrict__ map = reinterpret_cast<const unsigned*>(map_f) + (int64_t)b * map_bs;
  const uint8_t* __restrict__ mask = mask_p + (int64_t)b * mask_bs;
  const int nq = (n + 3) / 4;
  const unsigned ninf = 0xff800000u;                   // -inf, the value of an empty set

  unsigned prefix = 0, rank = 0;                       // the key's digits found so far; the rank among the keys matching them
  int low = 32;                                        // bits below the prefix
#pragma unroll 1
  for (int pass = 0; pass < PS_PASSES; ++pass) {
    const int bits = pass == PS_PASSES - 1 ? 10 : 11;
    const int shift = low - bits;                      // 21, 10, 0
    for (int i = tid; i < PS_BINS; i += nt) hist[i] = 0u;
    if (pass == 0 && tid < 2) s_max[tid] = 0u;
    __syncthreads();
    unsigned best_in = 0u, best_out = 0u;              // key 0 is a NaN's: below the key of every value
    for (int q0 = tid; q0 < nq; q0 += nt * PS_UNROLL) {
      PsQuad quad[PS_UNROLL];
#pragma unroll
      for (int u = 0; u < PS_UNROLL; ++u) {
        const int q = q0 + u * nt;
        if (q < nq) ps_load<MAPV, MASKV>(map, mask, q, n, quad[u]);
      }
#pragma unroll
      for (int u = 0; u < PS_UNROLL; ++u) {
        const int q = q0 + u * nt;
        if (q >= nq) continue;
        const int cnt = min(4, n - q * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= cnt) continue;
          const unsigned key = ps_key(quad[u].v[j]);
          const bool in = (quad[u].mk >> (8 * j)) & 0xffu;
          if (pass == 0) {
            if (in) best_in = max(best_in, key); else best_out = max(best_out, key);
          }
          if (in && (unsigned)((unsigned long long)key >> low) == prefix)
            atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], 1u);
        }
      }
    }
    if (pass == 0) {
#pragma unroll
      for (int o = 1; o < AMMC_WAVE; o <<= 1) {
        best_in = max(best_in, (unsigned)__shfl_xor((int)best_in, o, AMMC_WAVE));
        best_out = max(best_out, (unsigned)__shfl_xor((int)best_out, o, AMMC_WAVE));
      }
      if (tid % AMMC_WAVE == 0) {
        atomicMax(&s_max[0], best_in);
        atomicMax(&s_max[1], best_out);
      }
    }
    __syncthreads();
    if (tid < AMMC_WAVE) {
      // lane l owns bins [l * 32, l * 32 + 32); it reads them rotated by l (a sum of counts has no order) so that the
      // lanes of one read fall into different banks
      unsigned own = 0u;
      for (int i = 0; i < PS_LANE_BINS; ++i) own += hist[tid * PS_LANE_BINS + ((i + tid) & (PS_LANE_BINS - 1))];
      unsigned from = own;                             // the count in the bins of lanes >= this one
#pragma unroll
      for (int o = 1; o < AMMC_WAVE; o <<= 1) {
        const unsigned t = (unsigned)__shfl_down((int)from, o, AMMC_WAVE);
        if (tid + o < AMMC_WAVE) from += t;
      }
      const unsigned total = (unsigned)__shfl((int)from, 0, AMMC_WAVE);
      unsigned want = rank;
      if (pass == 0) {
        // k = ceil(num * m / den) in integers; 1 <= k <= m for m >= 1 because 1 <= num <= den
        want = (unsigned)(((long long)total * frac_num + frac_den - 1) / frac_den);
        if (tid == 0) s_m = total;
      }
      const unsigned above = from - own;               // the count in the bins of the lanes above
      if (total > 0u && above < want && want <= from) {        // exactly one lane: the one whose bins hold rank `want`
        unsigned r = want - above;
        int bin = tid * PS_LANE_BINS + PS_LANE_BINS - 1;
        for (;; --bin) {
          const unsigned c = hist[bin];
          if (r <= c) break;
          r -= c;
        }
        s_digit = (unsigned)bin;
        s_rank = r;
      }
    }
    __syncthreads();
    if (s_m == 0u) break;                              // an empty mask: nothing to select (uniform: s_m is one LDS word)
    prefix = (prefix << bits) | s_digit;
    rank = s_rank;
    low = shift;
  }
  if (tid == 0) {
    const unsigned m = s_m;
    m_out[b] = (int)m;
    const unsigned* mx = s_max;
    reinterpret_cast<unsigned*>(kth)[b] = m ? ps_bits(prefix) : ninf;
    reinterpret_cast<unsigned*>(max_in)[b] = m ? ps_bits(mx[0]) : ninf;
    reinterpret_cast<unsigned*>(max_out)[b] = m < (unsigned)n ? ps_bits(mx[1]) : ninf;
  }
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_pixel_scores_f32(const float* map, int64_t map_bs, const uint8_t* mask, int64_t mask_bs, int32_t batch, int32_t h,
                          int32_t w, int32_t frac_num, int32_t frac_den, int32_t* m, float* kth, float* max_in,
                          float* max_out, void* stream) {
  if (!map || !mask || !m || !kth || !max_in || !max_out) return AMMC_EINVAL;
  if (batch < 1 || h < 1 || w < 1) return AMMC_EINVAL;
  const int64_t n = (int64_t)h * w;
  if (n > (1LL << 24)) return AMMC_EINVAL;
  if (frac_num < 1 || frac_den < frac_num || frac_den > 4096) return AMMC_EINVAL;
  if (batch > 1 && (map_bs < n || mask_bs < n)) return AMMC_EINVAL;
  if (((uintptr_t)map | (uintptr_t)m | (uintptr_t)kth | (uintptr_t)max_in | (uintptr_t)max_out) & 3) return AMMC_EINVAL;

  // 16-byte map loads / 4-byte mask loads: every quad of every sample starts on such a boundary
  const bool mapv = ((uintptr_t)map & 15) == 0 && (batch == 1 || (map_bs & 3) == 0);
  const bool maskv = ((uintptr_t)mask & 3) == 0 && (batch == 1 || (mask_bs & 3) == 0);
  const int64_t nq = (n + 3) / 4;
  int threads = (int)((nq + AMMC_WAVE - 1) / AMMC_WAVE) * AMMC_WAVE;
  threads = threads > PS_MAX_THREADS ? PS_MAX_THREADS : threads;
  const dim3 grid((unsigned)batch), block((unsigned)threads);
  hipStream_t s = (hipStream_t)stream;
#define AMMC_PS_LAUNCH(MV, KV)                                                                                           \
  hipLaunchKernelGGL((pixel_scores_kernel<MV, KV>), grid, block, 0, s, map, map_bs, mask, mask_bs, (int)n, frac_num, frac_den, \
                     m, kth, max_in, max_out)
  if (mapv && maskv) AMMC_PS_LAUNCH(true, true);
  else if (mapv) AMMC_PS_LAUNCH(true, false);
  else if (maskv) AMMC_PS_LAUNCH(false, true);
  else AMMC_PS_LAUNCH(false, false);
#undef AMMC_PS_LAUNCH
  return ammc_launch_status();
}

}  // extern "C"
