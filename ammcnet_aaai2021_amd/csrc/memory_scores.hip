// Per-clip memory-commit scores: the commitment distance of the memory module for every position of every clip, from a
// pass of its own over the bottleneck in front of the memory block (definitions in include/ammc_hip.h):
//
//   z[p][j]  = (sum_i x[p][i] * enc_w[j][i]) + enc_b[j]         the module's 1x1 `enc` (models/unet.py:318-331)
//   r[p][s]  = enorm[s] - 2 * sum_j z[p][j] * E[j][s]           the reference's `dist` without its row-constant |z|^2
//   idx[p]   = the k smallest keys, nearest first, equal keys in ascending slot order
//   s[p]     = sum_j (E[j][idx0] - z[p][j])^2                   directly from the fp32 data, j = 0, 1, ... in order
//   map      = s / d;   commit[b], worst[b], worst_idx[b] from the stored map of clip b (second launch)
//
// Two plain launches, no atomics, no arrival counter: every output has one writer.  A workgroup (256 threads, 4 waves)
// owns a tile of 64 positions of ONE clip; positions past the clip's end enter as zeros and are not stored.  What a
// position's values are made of is a function of (x[b], enc_w, enc_b, E, c, m, k) alone:
//
//   * phase 1, z: `c` goes through LDS in chunks of 32 channels (x tile and enc_w tile, double buffered); a wave owns one
//     32 x 32 quadrant (positions x outputs) and runs 16 v_mfma_f32_32x32x2_f32 per chunk - bitwise an fmaf chain in
//     channel order (the loads of a chunk are issued two chunks ahead).  Two chunks (64 channels) chain into a partial set that starts from 0 and is then ADDED to the
//     accumulators, so no chain is longer than 64 and the grouping depends on c only.  The bias is added last.  The
//     global loads are 16-byte where the bases and strides allow and 4-byte where they do not: the same values land in
//     the same LDS words;
//   * phase 2, keys: z stays in LDS; the slots go by in tiles of 64, a wave contracts 32 slots (MFMA rows, straight from
//     the [d][m] codebook, slot-contiguous) against 32 positions (MFMA columns) in ONE chain of 64 features from 0.  A
//     lane then holds 16 slots of one position in ascending order and keeps that position's running top-k (the next
//     tile's operands are in flight meanwhile); slots >= m enter as +inf keys, which never rank.  The four partial lists of a position meet in LDS and are merged by (key, slot);
//   * phase 3, s[p]: one thread per position, 64 sequential terms on the VALU, contraction off.
//
// NaN and +inf keys never enter a list; a position with fewer than k ranked keys reports slot m - 1 in the empty places.
#include "ammc_common.h"
#include <math.h>

namespace ammc_impl {

constexpr int MS_THREADS = 256;
constexpr int MS_TP = 64;            // positions per workgroup
constexpr int MS_D = 64;             // embedding width
constexpr int MS_KC = 32;            // channels per chunk
constexpr int MS_LD = MS_KC + 1;     // LDS row stride of a chunk tile (odd: the fragment reads are conflict free)
constexpr int MS_ZLD = MS_D + 1;     // LDS row stride of z
constexpr int MS_TAIL_THREADS = 256;
constexpr int MS_EMPTY = 0x7fffffff;

// sorted insertion by (key, slot); candidates of one list arrive in any order
template <int K>
__device__ __forceinline__ void ms_insert(float (&v)[K], int (&ix)[K], float c, int s) {
  if (c < v[K - 1] || (c == v[K - 1] && s < ix[K - 1])) {
    v[K - 1] = c;
    ix[K - 1] = s;
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      const bool sw = v[j] < v[j - 1] || (v[j] == v[j - 1] && ix[j] < ix[j - 1]);
      const float tv = sw ? v[j - 1] : v[j];
      const int ti = sw ? ix[j - 1] : ix[j];
      v[j - 1] = sw ? v[j] : v[j - 1];
      ix[j - 1] = sw ? ix[j] : ix[j - 1];
      v[j] = tv;
      ix[j] = ti;
    }
  }
}

// the same insertion when the candidates of a list arrive in ascending slot order (one lane's walk over the slots): a
// tie then always loses to the entry already held, so strict comparisons implement the (key, slot) order, branch-free
template <int K>
__device__ __forceinline__ void ms_insert_ordered(float (&v)[K], int (&ix)[K], float c, int s) {
  if (K == 2) {
    const bool lt0 = c < v[0], lt1 = c < v[1];
    v[1] = lt0 ? v[0] : (lt1 ? c : v[1]);
    ix[1] = lt0 ? ix[0] : (lt1 ? s : ix[1]);
    v[0] = lt0 ? c : v[0];
    ix[0] = lt0 ? s : ix[0];
  } else {
    const bool lt0 = c < v[0];
    v[0] = lt0 ? c : v[0];
    ix[0] = lt0 ? s : ix[0];
  }
}

// four consecutive floats at `p`: one 16-byte access or four 4-byte ones, the same values either way
template <bool VEC>
__device__ __forceinline__ f32x4 ms_load4(const float* __restrict__ p) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  const f32x4 v = {p[0], p[1], p[2], p[3]};
  return v;
}

__device__ __forceinline__ void ms_store4(float* __restrict__ p, const f32x4 v) {
  p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
}

template <int K, bool VEC>
__global__ __launch_bounds__(MS_THREADS) void memory_scores_kernel(
    const float* __restrict__ x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int hw, int w, int c, int tiles,
    const float* __restrict__ enc_w, const float* __restrict__ enc_b, const float* __restrict__ e_dm,
    const float* __restrict__ e_md, const float* __restrict__ enorm, int m, float* __restrict__ map, int64_t map_bs,
    int* __restrict__ idx_out) {
#pragma clang fp contract(off)
  __shared__ float xs[2][MS_TP * MS_LD];
  __shared__ float ws[2][MS_D * MS_LD];
  __shared__ float zs[MS_TP * MS_ZLD];
  __shared__ float cand_v[MS_TP][4][K];
  __shared__ int cand_i[MS_TP][4][K];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int p0 = tile * MS_TP;
  const int pr = wave & 1, qr = wave >> 1;       // quadrant: positions 32 pr .., outputs / slots 32 qr ..

  // ---- phase 1: z = x . enc_w^T ---------------------------------------------------------------------------------
  // staging: thread t moves quads t and t + 256 of each 64 x 32 tile: row (t >> 3), channels 4 (t & 7) ..
  const float* xsrc[2];
  const float* wsrc[2];
  bool xin[2];
  int ldst[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = tid + i * MS_THREADS;
    const int row = t >> 3, q = t & 7;
    const int p = p0 + row;
    xin[i] = p < hw;
    const int pc = xin[i] ? p : 0;
    const int y = pc / w, xx = pc - y * w;
    xsrc[i] = x + (int64_t)b * x_bs + (int64_t)y * x_rs + (int64_t)xx * x_ps + 4 * q;
    wsrc[i] = enc_w + (int64_t)row * c + 4 * q;
    ldst[i] = row * MS_LD + 4 * q;
  }
  // Chunk n waits in register set n & 1 while chunk n - 1 is contracted: its loads are issued TWO iterations ahead of
  // their LDS store, so a trip to L2 / HBM hides behind two chunks of MFMAs (one workgroup per CU at batch 16: there
  // is no second wave on a SIMD to hide it).
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int nch = c / MS_KC;
  auto gload = [&](int chn, f32x4(&ax)[2], f32x4(&aw)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ax[i] = xin[i] ? ms_load4<VEC>(xsrc[i] + chn * MS_KC) : zero4;
      aw[i] = ms_load4<VEC>(wsrc[i] + chn * MS_KC);
    }
  };
  auto lstore = [&](int buf, const f32x4(&ax)[2], const f32x4(&aw)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ms_store4(&xs[buf][ldst[i]], ax[i]);
      ms_store4(&ws[buf][ldst[i]], aw[i]);
    }
  };
  f32x4 ax0[2], aw0[2], ax1[2], aw1[2];
  gload(0, ax0, aw0);
  if (nch > 1) gload(1, ax1, aw1);
  lstore(0, ax0, aw0);
  __syncthreads();

  f32x16 acc, part;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f, part[r] = 0.f;
  const int arow = (32 * pr + l31) * MS_LD + hh, brow = (32 * qr + l31) * MS_LD + hh;
  // one chunk: loads of chunk ch + 2 into the set chunk ch came from, 16 MFMAs on LDS buffer ch & 1, the fold after an
  // odd (or the last) chunk, chunk ch + 1 from its set into the other LDS buffer
  auto step = [&](int ch, f32x4(&lx)[2], f32x4(&lw)[2], const f32x4(&sx)[2], const f32x4(&sw)[2]) {
    const int cur = ch & 1;
    if (ch + 2 < nch) gload(ch + 2, lx, lw);
    const float* __restrict__ xa = xs[cur] + arow;
    const float* __restrict__ wb = ws[cur] + brow;
#pragma unroll
    for (int kk = 0; kk < MS_KC / 2; ++kk)
      part = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * kk], wb[2 * kk], part, 0, 0, 0);
    if ((ch & 1) || ch + 1 == nch) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = acc[r] + part[r], part[r] = 0.f;
    }
    if (ch + 1 < nch) lstore(cur ^ 1, sx, sw);
    __syncthreads();
  };
  for (int ch = 0; ch < nch; ch += 2) {
    step(ch, ax0, aw0, ax1, aw1);
    if (ch + 1 < nch) step(ch + 1, ax1, aw1, ax0, aw0);
  }
  {
    // accumulator reg r of this lane: position 32 pr + (r & 3) + 8 (r >> 2) + 4 hh, output 32 qr + l31
    const int j = 32 * qr + l31;
    const float bj = enc_b[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = 32 * pr + (r & 3) + 8 * (r >> 2) + 4 * hh;
      zs[p * MS_ZLD + j] = acc[r] + bj;
    }
  }
  __syncthreads();

  // ---- phase 2: keys and the running top-k --------------------------------------------------------------------------
  float bv[K];
  int bi[K];
#pragma unroll
  for (int j = 0; j < K; ++j) bv[j] = INFINITY, bi[j] = MS_EMPTY;
  float zf[MS_D / 2];                              // this lane's B operands: z[32 pr + l31][2 kk + hh], all tiles
#pragma unroll
  for (int kk = 0; kk < MS_D / 2; ++kk) zf[kk] = zs[(32 * pr + l31) * MS_ZLD + 2 * kk + hh];
  const int mtiles = (m + 63) >> 6;
  // a tile's operands: 32 dwords of E (slot-contiguous rows of the [d][m] codebook) and the 16 |E_s|^2 of this lane's
  // accumulator rows.  Slots >= m are clamped to m - 1 for the loads and masked to a +inf key below.  The whole NEXT
  // tile is in flight while the current one is contracted (two register sets, the tile loop unrolled twice).
  auto tload = [&](int mt, float(&ef)[MS_D / 2], float(&en)[16]) {
    const int s0 = mt * 64 + 32 * qr;
    const float* __restrict__ ep = e_dm + (int64_t)hh * m + min(s0 + l31, m - 1);
#pragma unroll
    for (int kk = 0; kk < MS_D / 2; ++kk) ef[kk] = ep[(int64_t)(2 * kk) * m];
#pragma unroll
    for (int r = 0; r < 16; ++r) en[r] = enorm[min(s0 + (r & 3) + 8 * (r >> 2) + 4 * hh, m - 1)];
  };
  auto contract = [&](int mt, const float(&ef)[MS_D / 2], const float(&en)[16]) {
    const int s0 = mt * 64 + 32 * qr;
    f32x16 dot;
#pragma unroll
    for (int r = 0; r < 16; ++r) dot[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < MS_D / 2; ++kk) dot = __builtin_amdgcn_mfma_f32_32x32x2f32(ef[kk], zf[kk], dot, 0, 0, 0);
    // accumulator reg r of this lane: slot s0 + (r & 3) + 8 (r >> 2) + 4 hh (ascending in r), position 32 pr + l31
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      const float key = s < m ? en[r] - 2.f * dot[r] : INFINITY;
      ms_insert_ordered<K>(bv, bi, key, s);
    }
  };
  float ef0[MS_D / 2], en0[16], ef1[MS_D / 2], en1[16];
  tload(0, ef0, en0);
  for (int mt = 0; mt < mtiles; mt += 2) {
    if (mt + 1 < mtiles) tload(mt + 1, ef1, en1);
    contract(mt, ef0, en0);
    if (mt + 1 < mtiles) {
      if (mt + 2 < mtiles) tload(mt + 2, ef0, en0);
      contract(mt + 1, ef1, en1);
    }
  }
  {
    const int p = 32 * pr + l31, part_id = 2 * qr + hh;
#pragma unroll
    for (int j = 0; j < K; ++j) cand_v[p][part_id][j] = bv[j], cand_i[p][part_id][j] = bi[j];
  }
  __syncthreads();

  // ---- phase 3: merge, the commit distance of the nearest slot, stores ----------------------------------------------
  if (tid < MS_TP) {
    const int p = tid;
    float mv[K];
    int mi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) mv[j] = INFINITY, mi[j] = MS_EMPTY;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (cand_i[p][q][j] != MS_EMPTY) ms_insert<K>(mv, mi, cand_v[p][q][j], cand_i[p][q][j]);
#pragma unroll
    for (int j = 0; j < K; ++j) mi[j] = min(mi[j], m - 1);
    const float* __restrict__ er = e_md + (int64_t)mi[0] * MS_D;
    const float* __restrict__ zr = zs + p * MS_ZLD;
    float s = 0.f;
#pragma unroll 16
    for (int j = 0; j < MS_D; ++j) {
      const float df = er[j] - zr[j];
      s = s + df * df;
    }
    if (p0 + p < hw) {
      map[(int64_t)b * map_bs + p0 + p] = s / (float)MS_D;
      if (idx_out) {
        int* __restrict__ o = idx_out + ((int64_t)b * hw + p0 + p) * K;
#pragma unroll
        for (int j = 0; j < K; ++j) o[j] = mi[j];
      }
    }
  }
}

// per clip: thread y owns row y of the map (its sequential double sum, its largest value and where), thread 0 then
// adds the rows in order; maps of more than MS_TAIL_THREADS rows go through in chunks, still in index order
__global__ __launch_bounds__(MS_TAIL_THREADS) void memory_scores_tail_kernel(const float* __restrict__ map, int64_t map_bs,
                                                                            int h, int w, float* __restrict__ commit,
                                                                            float* __restrict__ worst,
                                                                            int* __restrict__ worst_idx) {
  __shared__ double row_sum[MS_TAIL_THREADS];
  __shared__ float row_best[MS_TAIL_THREADS];
  __shared__ int row_at[MS_TAIL_THREADS];
  const int b = blockIdx.x;
  const float* __restrict__ mp = map + (int64_t)b * map_bs;
  double total = 0.0;
  float best = 0.f;
  int at = 0;
  for (int base = 0; base < h; base += MS_TAIL_THREADS) {
    const int y = base + (int)threadIdx.x;
    if (y < h) {
      const int64_t o = (int64_t)y * w;
      double s = 0.0;
      float mx = mp[o];
      int mi = 0;
      for (int j = 0; j < w; ++j) {
        const float v = mp[o + j];
        s += (double)v;
        if (v > mx) mx = v, mi = j;                      // strict: the lowest index among equal values stays
      }
      row_sum[threadIdx.x] = s;
      row_best[threadIdx.x] = mx;
      row_at[threadIdx.x] = y * w + mi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = min(MS_TAIL_THREADS, h - base);
      for (int k = 0; k < cnt; ++k) {
        total += row_sum[k];
        if ((base == 0 && k == 0) || row_best[k] > best) best = row_best[k], at = row_at[k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    commit[b] = (float)(total / (double)((int64_t)h * w));
    worst[b] = best;
    worst_idx[b] = at;
  }
}

template <int K>
inline void ms_launch(bool vec, unsigned grid, hipStream_t s, const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int hw,
                      int w, int c, int tiles, const float* enc_w, const float* enc_b, const float* e_dm, const float* e_md,
                      const float* enorm, int m, float* map, int64_t map_bs, int* idx) {
  if (vec)
    hipLaunchKernelGGL((memory_scores_kernel<K, true>), dim3(grid), dim3(MS_THREADS), 0, s, x, x_bs, x_rs, x_ps, hw, w, c, tiles,
                       enc_w, enc_b, e_dm, e_md, enorm, m, map, map_bs, idx);
  else
    hipLaunchKernelGGL((memory_scores_kernel<K, false>), dim3(grid), dim3(MS_THREADS), 0, s, x, x_bs, x_rs, x_ps, hw, w, c, tiles,
                       enc_w, enc_b, e_dm, e_md, enorm, m, map, map_bs, idx);
}

}  // namespace ammc_impl
using namespace ammc_impl;

extern "C" {

int ammc_memory_scores_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t h, int32_t w,
                           int32_t c, const float* enc_w, const float* enc_b, const float* embed_dm, const float* embed_md,
                           const float* enorm, int32_t d, int32_t m, int32_t k, float* map, int64_t map_bs, int32_t* idx_topk,
                           float* commit, float* worst, int32_t* worst_idx, void* stream) {
  if (!x || !enc_w || !enc_b || !embed_dm || !embed_md || !enorm || !map || !commit || !worst || !worst_idx) return AMMC_EINVAL;
  if (batch <= 0 || h <= 0 || w <= 0 || c <= 0 || d <= 0 || m <= 0 || k <= 0) return AMMC_EINVAL;
  if (((uintptr_t)x | (uintptr_t)enc_w | (uintptr_t)enc_b | (uintptr_t)embed_dm | (uintptr_t)embed_md | (uintptr_t)enorm |
       (uintptr_t)map | (uintptr_t)idx_topk | (uintptr_t)commit | (uintptr_t)worst | (uintptr_t)worst_idx) & 3)
    return AMMC_EINVAL;
  // an NHWC view: pixel stride >= c, each outer stride >= the extent below it
  if (x_ps < c) return AMMC_EINVAL;
  const int64_t row = (int64_t)(w - 1) * x_ps + c;
  if (x_rs < row) return AMMC_EINVAL;
  if (x_bs < (int64_t)(h - 1) * x_rs + row) return AMMC_EINVAL;
  const int64_t hw = (int64_t)h * w;
  if (map_bs < hw) return AMMC_EINVAL;
  if (d != MS_D || k > 2 || c % MS_KC != 0 || c > 1024 || m < k) return AMMC_EUNSUP;
  // 32-bit position indices (worst_idx, y * w + x) and the 1-D grid; element offsets are 64-bit
  const int64_t tiles = (hw + MS_TP - 1) / MS_TP;
  if (hw > (1LL << 31) - MS_TP || (int64_t)batch * tiles >= (1LL << 31)) return AMMC_EUNSUP;

  // 16-byte loads: every quad of x (channels 4 q of a position) and of enc_w starts on a 16-byte boundary
  const bool vec = (((uintptr_t)x | (uintptr_t)enc_w) & 15) == 0 && ((x_bs | x_rs | x_ps) & 3) == 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)((int64_t)batch * tiles);
  if (k == 1)
    ms_launch<1>(vec, grid, s, x, x_bs, x_rs, x_ps, (int)hw, w, c, (int)tiles, enc_w, enc_b, embed_dm, embed_md, enorm, m, map,
                 map_bs, idx_topk);
  else
    ms_launch<2>(vec, grid, s, x, x_bs, x_rs, x_ps, (int)hw, w, c, (int)tiles, enc_w, enc_b, embed_dm, embed_md, enorm, m, map,
                 map_bs, idx_topk);
  int rc = ammc_launch_status();
  if (rc != AMMC_OK) return rc;
  hipLaunchKernelGGL(memory_scores_tail_kernel, dim3((unsigned)batch), dim3(MS_TAIL_THREADS), 0, s, map, map_bs, h, w, commit,
                     worst, worst_idx);
  return ammc_launch_status();
}

}  // extern "C"
