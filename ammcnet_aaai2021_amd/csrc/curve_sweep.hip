// Curve sweep: at every point of a (weight vector, smoothing pair) grid, what the equal error rate, the average precision
// and the precision-recall area of the fused score are made of - the two ROC vertices that bracket fpr + tpr = 1, their
// thresholds, the two precision sums, and the AUC numerator of fusion_sweep.hip.  The definition is in
// include/ammc_hip.h; the keys are fusion_sweep.hip's (sweep_keys.h), bit for bit.
//
// One launch, one workgroup per grid point, nothing passes between workgroups, no float atomics, no arrival counter.
//   1. the keys of the LARGER class (nb of them) are sorted in LDS by the bitonic network and written, ascending, to this
//      grid point's row of the workspace (plain coalesced stores);
//   2. the keys of the SMALLER class (ns) are sorted in the same LDS and stay there.  The barriers of the network stand
//      between the stores of 1. and every later load of the row; a workgroup-scope release before them and an acquire
//      after them order the two for the compiler and the memory model.  That is sufficient on gfx950 because a workgroup
//      lives on one CU, whose vector L1 is write-through and is the only cache the CU's own loads can hit in front of
//      the L2 its stores went to: the hazards of a hand-off through global memory are all between CUs (a stale L1 line
//      of ANOTHER CU's store).  Nobody else writes the row during the launch, and a launch starts with a clean L1;
//   3. pass A, one thread per position i of the row: two binary searches in LDS give the other class's counts
//      lb = #{small < key}, ub = #{small <= key}: the pair count of two_u, and - with the own class counted by position,
//      nb - i - the sign of G at i.  G by position is non-increasing in i and equals the true G at the head of a tie
//      run, so the first i with G <= 0, an integer minimum in LDS, is the first true one or lies inside the run in front
//      of it (one thread moves it to the run's end afterwards).  Where the larger class is the positive one, the head
//      of each tie run (key[i - 1] != key[i]) finds the run's end by a galloping search in the row and adds the run's
//      two precision terms in double;
//   4. pass B, one thread per position j of the LDS array: the same with the roles swapped - the other class's counts
//      from binary searches in the row (global memory, L2-resident), the own run's end from LDS;
//   5. vertex a is (n - lower bound) in both arrays at the smallest key with G <= 0, which are the two first positions
//      themselves; vertex b at the largest key below it, one more search each.
// The sums: each thread adds its runs in position order, the 64 lanes of a wave add by a xor tree, thread 0 adds the
// waves in order - an order fixed by the class sizes alone.
// LDS: 4 * nextpow2(nb) bytes dynamic, 128 KiB at nb = 32768, plus 400 bytes static.  256 threads up to a padded larger
// class of 4096, 1024 above.  Workspace: one row of nb words, rounded up to 64, per grid point.
// Frame indices are clamped to [0, n) as in the fusion sweep.  Contraction into FMAs is off for the whole file.
#include "sweep_keys.h"

namespace ammc_impl {

constexpr int CS_MAX_CLASS = 32768;
constexpr int CS_THREADS_SMALL = 256;
constexpr int CS_THREADS_LARGE = 1024;
constexpr int CS_SMALL_PAD = 4096;
constexpr int CS_MAX_WAVES = CS_THREADS_LARGE / AMMC_WAVE;
constexpr int CS_ROW_ALIGN = 64;                       // words

struct CsArgs {
  const float* chan;
  int64_t rs;
  const float* w;
  const float* sm;
  const int32_t* big_idx;                              // the larger class: nb frame indices
  const int32_t* small_idx;                            // the smaller class: ns frame indices
  long long* two_u;
  int32_t* pts;
  float* thr;
  double* sums;
  unsigned* ws;
  int64_t row_words;
  int k, n, s, nb, bpad, ns, spad;
  int big_is_pos;
};

// #{a[lo .. hi) < key} + lo in an ascending array
__device__ __forceinline__ int cs_lower(const unsigned* a, int lo, int hi, unsigned key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// #{a[lo .. hi) <= key} + lo in an ascending array
__device__ __forceinline__ int cs_upper(const unsigned* a, int lo, int hi, unsigned key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the end of the tie run of `key` in an ascending array whose words from lo on are >= key: doubling steps, then bisection
__device__ __forceinline__ int cs_run_end(const unsigned* a, int lo, int hi, unsigned key) {
  for (int st = 1; lo < hi; st <<= 1) {
    const int pr = lo + st - 1;
    if (pr >= hi) break;
    if (a[pr] == key) {
      lo = pr + 1;
    } else {
      hi = pr;
      break;
    }
  }
  return cs_upper(a, lo, hi, key);
}

// the two precision terms of one tie run of the positive class: mult positives at a value with TP, FP at or above it and
// TPgt, FPgt above it
__device__ __forceinline__ void cs_terms(int mult, int tp, int fp, int tpgt, int fpgt, double& s0, double& s1) {
  const double prec = (double)tp / (double)(tp + fp);
  const double last = tpgt > 0 ? (double)tpgt / (double)(tpgt + fpgt) : (fpgt > 0 ? 0.0 : 1.0);
  s0 += (double)mult * prec;
  s1 += 0.5 * (double)mult * (last + prec);
}

extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];

__global__ __launch_bounds__(CS_THREADS_LARGE) void curve_sweep_kernel(CsArgs p) {
  __shared__ long long red_u[CS_MAX_WAVES];
  __shared__ double red_s[2][CS_MAX_WAVES];
  __shared__ int first[2];                             // the first position with G <= 0 in the row and in LDS
  unsigned* __restrict__ keys = reinterpret_cast<unsigned*>(cs_smem);
  unsigned* row = p.ws + (int64_t)blockIdx.x * p.row_words;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int g = blockIdx.x / p.s, s = blockIdx.x - g * p.s;
  float w[FS_MAX_K];
#pragma unroll
  for (int c = 0; c < FS_MAX_K; ++c) w[c] = c < p.k ? p.w[(int64_t)g * p.k + c] : 0.f;
  const float a = p.sm[2 * s], b = p.sm[2 * s + 1];
  const int nb = p.nb, ns = p.ns;
  if (tid == 0) first[0] = nb, first[1] = ns;

  for (int j = tid; j < p.bpad; j += nt)
    keys[j] = j < nb ? fs_key(p.chan, p.rs, p.k, p.n, w, a, b, p.big_idx[j]) : FS_SENTINEL;
  __syncthreads();
  fs_bitonic_sort(keys, p.bpad, tid, nt);
  for (int j = tid; j < nb; j += nt) row[j] = keys[j];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();                                     // the row is stored, the LDS array is free

  for (int j = tid; j < p.spad; j += nt)
    keys[j] = j < ns ? fs_key(p.chan, p.rs, p.k, p.n, w, a, b, p.small_idx[j]) : FS_SENTINEL;
  __syncthreads();
  fs_bitonic_sort(keys, p.spad, tid, nt);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  const long long P = p.big_is_pos ? nb : ns, Q = p.big_is_pos ? ns : nb;
  const long long cb = p.big_is_pos ? Q : P, cs = p.big_is_pos ? P : Q;      // G = cb * (big count) + cs * (small count) - P Q
  long long acc = 0;
  double s0 = 0.0, s1 = 0.0;
  int mine = nb;
  for (int i = tid; i < nb; i += nt) {                 // pass A: the row
    const unsigned key = row[i];
    const int lb = cs_lower(keys, 0, ns, key);
    const int ub = cs_upper(keys, lb, ns, key);
    acc += p.big_is_pos ? (long long)lb + ub : 2LL * ns - lb - ub;
    if (cb * (nb - i) + cs * (ns - lb) - P * Q <= 0 && i < mine) mine = i;
    if (p.big_is_pos && (i == 0 || row[i - 1] != key)) {
      const int end = cs_run_end(row, i + 1, nb, key);
      cs_terms(end - i, nb - i, ns - lb, nb - end, ns - ub, s0, s1);
    }
  }
  if (mine < nb) atomicMin(&first[0], mine);
  mine = ns;
  for (int j = tid; j < ns; j += nt) {                 // pass B: the LDS array
    const unsigned key = keys[j];
    const int lb = cs_lower(row, 0, nb, key);
    if (cb * (nb - lb) + cs * (ns - j) - P * Q <= 0 && j < mine) mine = j;
    if (!p.big_is_pos && (j == 0 || keys[j - 1] != key)) {
      const int ub = cs_run_end(row, lb, nb, key);     // (lb == nb or row[lb] >= key: a run of `key` starts at lb or is empty)
      const int end = cs_run_end(keys, j + 1, ns, key);
      cs_terms(end - j, ns - j, nb - lb, ns - end, nb - ub, s0, s1);
    }
  }
  if (mine < ns) atomicMin(&first[1], mine);

#pragma unroll
  for (int o = 1; o < AMMC_WAVE; o <<= 1) {
    acc += __shfl_xor(acc, o, AMMC_WAVE);
    s0 += __shfl_xor(s0, o, AMMC_WAVE);
    s1 += __shfl_xor(s1, o, AMMC_WAVE);
  }
  if (tid % AMMC_WAVE == 0) red_u[tid / AMMC_WAVE] = acc, red_s[0][tid / AMMC_WAVE] = s0, red_s[1][tid / AMMC_WAVE] = s1;
  __syncthreads();
  if (tid != 0) return;

  for (int v = 1; v < nt / AMMC_WAVE; ++v) acc += red_u[v], s0 += red_s[0][v], s1 += red_s[1][v];
  // inside a tie run the position's G is below the run's: the first true position is then the run's end
  int ib = first[0], is = first[1];
  if (ib > 0 && ib < nb && row[ib - 1] == row[ib]) ib = cs_run_end(row, ib + 1, nb, row[ib]);
  if (is > 0 && is < ns && keys[is - 1] == keys[is]) is = cs_run_end(keys, is + 1, ns, keys[is]);
  // vertex a: the smallest key with G <= 0 is row[ib] or keys[is]; every key in front of ib and of is lies below it
  const bool has_a = ib < nb || is < ns;
  unsigned va = FS_SENTINEL;
  if (ib < nb) va = row[ib];
  if (is < ns && keys[is] < va) va = keys[is];
  // vertex b: the largest key below it (there is one: the smallest key of all has G = P Q > 0)
  unsigned vb = 0;
  if (ib > 0) vb = row[ib - 1];
  if (is > 0 && keys[is - 1] > vb) vb = keys[is - 1];
  const int lbb = cs_lower(row, 0, ib, vb), lbs = cs_lower(keys, 0, is, vb);
  const int big_a = nb - ib, small_a = ns - is, big_b = nb - lbb, small_b = ns - lbs;
  int32_t* __restrict__ pts = p.pts + 4 * (int64_t)blockIdx.x;
  pts[0] = p.big_is_pos ? big_a : small_a;
  pts[1] = p.big_is_pos ? small_a : big_a;
  pts[2] = p.big_is_pos ? big_b : small_b;
  pts[3] = p.big_is_pos ? small_b : big_b;
  p.thr[2 * (int64_t)blockIdx.x] = has_a ? fs_key_value(va) : __uint_as_float(0x7F800000u);
  p.thr[2 * (int64_t)blockIdx.x + 1] = fs_key_value(vb);
  p.two_u[blockIdx.x] = acc;
  p.sums[2 * (int64_t)blockIdx.x] = s0;
  p.sums[2 * (int64_t)blockIdx.x + 1] = s1;
}

static int64_t cs_row_words(int32_t n_pos, int32_t n_neg) {
  const int64_t nb = n_pos > n_neg ? n_pos : n_neg;
  return (nb + CS_ROW_ALIGN - 1) / CS_ROW_ALIGN * CS_ROW_ALIGN;
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_curve_sweep_max_class(void) { return CS_MAX_CLASS; }

int64_t ammc_curve_sweep_workspace_bytes(int32_t points, int32_t n_pos, int32_t n_neg) {
  if (points < 1 || n_pos < 1 || n_neg < 1 || n_pos > CS_MAX_CLASS || n_neg > CS_MAX_CLASS) return 0;
  return (int64_t)points * cs_row_words(n_pos, n_neg) * 4;
}

int ammc_curve_sweep_f32(const float* chan, int64_t chan_rs, int32_t k, int32_t n, const float* w, int32_t g, const float* sm,
                         int32_t s, const int32_t* pos_idx, int32_t n_pos, const int32_t* neg_idx, int32_t n_neg,
                         int64_t* two_u, int32_t* pts, float* thr, double* sums, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  if (!chan || !w || !sm || !pos_idx || !neg_idx || !two_u || !pts || !thr || !sums || !workspace) return AMMC_EINVAL;
  if (k < 1 || k > FS_MAX_K || n < 2 || g < 1 || s < 1 || n_pos < 1 || n_neg < 1) return AMMC_EINVAL;
  if ((int64_t)n_pos + (int64_t)n_neg != (int64_t)n || chan_rs < (int64_t)n) return AMMC_EINVAL;
  if (((uintptr_t)chan | (uintptr_t)w | (uintptr_t)sm | (uintptr_t)pos_idx | (uintptr_t)neg_idx | (uintptr_t)pts | (uintptr_t)thr |
       (uintptr_t)workspace) & 3)
    return AMMC_EINVAL;
  if (((uintptr_t)two_u | (uintptr_t)sums) & 7) return AMMC_EINVAL;
  if (n_pos > CS_MAX_CLASS || n_neg > CS_MAX_CLASS) return AMMC_EINVAL;
  if ((int64_t)g * s >= (1LL << 31)) return AMMC_EUNSUP;     // the grid's x dimension
  if (workspace_bytes < ammc_curve_sweep_workspace_bytes(g * s, n_pos, n_neg)) return AMMC_EINVAL;

  const bool big_pos = n_pos >= n_neg;
  CsArgs a;
  a.chan = chan, a.rs = chan_rs, a.w = w, a.sm = sm;
  a.big_idx = big_pos ? pos_idx : neg_idx;
  a.small_idx = big_pos ? neg_idx : pos_idx;
  a.two_u = reinterpret_cast<long long*>(two_u);
  a.pts = pts, a.thr = thr, a.sums = sums;
  a.ws = static_cast<unsigned*>(workspace);
  a.row_words = cs_row_words(n_pos, n_neg);
  a.k = k, a.n = n, a.s = s;
  a.nb = big_pos ? n_pos : n_neg, a.ns = n - a.nb;
  a.bpad = a.spad = 1;
  while (a.bpad < a.nb) a.bpad <<= 1;
  while (a.spad < a.ns) a.spad <<= 1;
  a.big_is_pos = big_pos ? 1 : 0;
  const size_t lds = (size_t)a.bpad * 4 > 16 ? (size_t)a.bpad * 4 : 16;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(curve_sweep_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int threads = a.bpad <= CS_SMALL_PAD ? CS_THREADS_SMALL : CS_THREADS_LARGE;
  hipLaunchKernelGGL(curve_sweep_kernel, dim3((unsigned)(g * s)), dim3(threads), lds, (hipStream_t)stream, a);
  return ammc_launch_status();
}

}  // extern "C"
