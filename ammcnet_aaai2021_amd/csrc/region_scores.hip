// Region-based evaluation: the connected components of a thresholded score map, scored against the ground-truth regions
// of a label image by intersection over union (the definitions are in include/ammc_hip.h).
//
// One workgroup per (sample, threshold) - per sample in ammc_label_regions_u8 - with a workspace slice of its own:
// `parent`, `area` and `inter`, int32 [h * w] each.  Labelling is a lock-free union-find over `parent`:
//
//   parent[i] = i for a foreground pixel, -1 for the background; a pixel is united with its foreground W / N neighbours
//   (4-connectivity) or, for 8-connectivity, by the decision tree "N alone; else W or else NW, and NE" (N present makes
//   the other three redundant: they are joined to N along their own rows).  unite(a, b) finds both roots and hangs the
//   LARGER root below the smaller with one atomicMin; when the atomicMin finds that the root was re-parented meanwhile
//   it goes on with the displaced parent, so no equivalence is lost.  parent[x] <= x at all times and only ever
//   decreases: every walk towards a root is strictly decreasing, so it ends within h * w steps whatever other threads
//   write, and the root of a finished component is its smallest flat index - its first pixel in raster order.
//
// Every loop has a bound known before it starts: walks h * w steps, unite h * w + 1 rounds (running out of them sets a
// flag that comes back as n_comp = -1 / count = -1), everything else is a strided pass over the pixels.  After the
// unions a pass points every pixel at its root; areas are integer atomicAdds per root; per ground-truth region present
// in the sample the intersections are atomicAdds per root, then the root's own thread makes the 64-bit match test.
// Atomics are integer and stay inside the workgroup's slice (or its LDS): counts have no order, so the outputs are a
// function of the map values, the label image and the threshold alone.  Workspace words are read and written with
// relaxed device-scope atomics between the workgroup's barriers.  Plain C++, vector stores only.
//
// The per-workgroup routines are templates over an execution policy: RsDev (a workgroup) here, and RsHost (one thread,
// no barrier) when the file is included with AMMC_REGION_HOST defined - tools/region_host_check.cpp runs them under the
// host sanitizers against a flood fill.
#ifndef AMMC_REGION_HOST
#include "ammc_common.h"
#define RS_FN __device__ __forceinline__
#else
#include <stdint.h>
#define RS_FN static inline
#endif

namespace ammc_impl {

constexpr int RS_MAX_REGIONS = 32;
constexpr int RS_MAX_THREADS = 1024;
constexpr int RS_MAX_PIXELS = 1 << 22;                 // h * w of one sample
constexpr int RS_MATCHED = 0x40000000;                 // flag in area[root]: the component matched a region (areas < 2^23)
constexpr int RS_WAVE = 64;

struct RsShared {
  int gsize[RS_MAX_REGIONS + 1];                       // pixels of ground-truth region r
  int n_px, n_comp, n_fp, fail;
  unsigned hit;
  int wsum[RS_MAX_THREADS / RS_WAVE];
};

template <class X>
RS_FN int rs_find(const X& x, int* parent, int n, int i) {
  int r = i;
  for (int s = 0; s < n; ++s) {                        // strictly decreasing: at most n - 1 steps
    const int p = x.ld(parent + r);
    if (p == r) break;
    r = p;
  }
  if (r != i) x.amin(parent + i, r);                   // a shortcut within the component; parent[i] only decreases
  return r;
}

template <class X>
RS_FN void rs_unite(const X& x, int* parent, int n, int a, int b, RsShared& sh) {
  for (int it = 0; it <= n; ++it) {
    a = rs_find(x, parent, n, a);
    b = rs_find(x, parent, n, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = x.amin(parent + a, b);
    if (old == a) return;                              // a was a root and now hangs below b
    a = old;                                           // a had been re-parented: its displaced parent joins b's set
  }
  x.sti(&sh.fail, 1);
}

// parent[i] = the smallest flat index of pixel i's component (-1: background), area[root] = its pixels, inter[] = 0
template <class X, class F>
RS_FN void rs_label(const X& x, F fg, int h, int w, int conn, int* parent, int* area, int* inter, RsShared& sh) {
  const int n = h * w, tid = x.tid(), nt = x.nt();
  int cnt = 0;
  for (int i = tid; i < n; i += nt) {
    const bool f = fg(i);
    cnt += f;
    x.st(parent + i, f ? i : -1);
    x.st(area + i, 0);
    x.st(inter + i, 0);
  }
  if (cnt) x.aadd(&sh.n_px, cnt);
  x.sync();
  for (int i = tid; i < n; i += nt) {
    if (x.ld(parent + i) < 0) continue;
    const int r = i / w, c = i - r * w;
    const bool W = c > 0 && x.ld(parent + i - 1) >= 0;
    const bool N = r > 0 && x.ld(parent + i - w) >= 0;
    if (conn == 4) {
      if (W) rs_unite(x, parent, n, i, i - 1, sh);
      if (N) rs_unite(x, parent, n, i, i - w, sh);
    } else if (N) {
      rs_unite(x, parent, n, i, i - w, sh);
    } else {
      const bool NW = r > 0 && c > 0 && x.ld(parent + i - w - 1) >= 0;
      const bool NE = r > 0 && c < w - 1 && x.ld(parent + i - w + 1) >= 0;
      if (W) rs_unite(x, parent, n, i, i - 1, sh);
      else if (NW) rs_unite(x, parent, n, i, i - w - 1, sh);
      if (NE) rs_unite(x, parent, n, i, i - w + 1, sh);
    }
  }
  x.sync();
  for (int i = tid; i < n; i += nt)
    if (x.ld(parent + i) >= 0) rs_find(x, parent, n, i);
  x.sync();
  for (int i = tid; i < n; i += nt) {
    const int p = x.ld(parent + i);
    if (p >= 0) x.aadd(area + p, 1);
  }
  x.sync();
}

template <class X>
RS_FN void rs_clear(const X& x, RsShared& sh) {
  for (int r = x.tid(); r <= RS_MAX_REGIONS; r += x.nt()) sh.gsize[r] = 0;
  if (x.tid() == 0) sh.n_px = sh.n_comp = sh.n_fp = sh.fail = 0, sh.hit = 0u;
  x.sync();
}

// one (sample, threshold): out = {n_px, n_comp, n_fp, hit}, valid on thread 0 after the call
template <class X>
RS_FN void rs_scores_one(const X& x, const float* map, const uint8_t* lab, float thr, int h, int w, int num, int den,
                         int min_area, int conn, int* parent, int* area, int* inter, RsShared& sh, int out[4]) {
  const int n = h * w, tid = x.tid(), nt = x.nt();
  rs_clear(x, sh);
  for (int i = tid; i < n; i += nt) {
    const int l = lab[i];
    if (l >= 1 && l <= RS_MAX_REGIONS) x.aadd(&sh.gsize[l], 1);
  }
  rs_label(x, [&](int i) { return map[i] >= thr; }, h, w, conn, parent, area, inter, sh);
  int cnt = 0;
  for (int i = tid; i < n; i += nt) cnt += x.ld(parent + i) == i && x.ld(area + i) >= min_area;
  if (cnt) x.aadd(&sh.n_comp, cnt);
  for (int r = 1; r <= RS_MAX_REGIONS; ++r) {
    const int g = sh.gsize[r];                         // one LDS word, settled before rs_label's barriers: uniform
    if (g == 0) continue;
    for (int i = tid; i < n; i += nt) {
      if (lab[i] != r) continue;
      const int p = x.ld(parent + i);
      if (p >= 0) x.aadd(inter + p, 1);
    }
    x.sync();
    for (int i = tid; i < n; i += nt) {                // pixel i is always this thread's: area[i] has one writer here
      if (x.ld(parent + i) != i) continue;
      const int it = x.ld(inter + i);
      if (it == 0) continue;
      x.st(inter + i, 0);
      const int af = x.ld(area + i), a = af & ~RS_MATCHED;
      if (a < min_area) continue;
      if ((long long)it * den >= (long long)num * ((long long)a + g - it)) {
        x.aor(&sh.hit, 1u << (r - 1));
        x.st(area + i, a | RS_MATCHED);
      }
    }
    x.sync();
  }
  cnt = 0;
  for (int i = tid; i < n; i += nt) {
    if (x.ld(parent + i) != i) continue;
    const int af = x.ld(area + i);
    cnt += !(af & RS_MATCHED) && af >= min_area;
  }
  if (cnt) x.aadd(&sh.n_fp, cnt);
  x.sync();
  if (tid == 0) {
    const bool bad = sh.fail != 0;
    out[0] = bad ? 0 : sh.n_px, out[1] = bad ? -1 : sh.n_comp, out[2] = bad ? 0 : sh.n_fp, out[3] = bad ? 0 : (int)sh.hit;
  }
}

// one sample: labels[i] = the raster rank (1..32, 0 beyond and for the background) of pixel i's kept component;
// returns the number of kept components (-1: the round bound was hit), valid on every thread
template <class X>
RS_FN int rs_number_one(const X& x, const uint8_t* mask, int h, int w, int min_area, int conn, uint8_t* labels, int* parent,
                        int* area, int* inter, RsShared& sh) {
  const int n = h * w, tid = x.tid(), nt = x.nt();
  rs_clear(x, sh);
  rs_label(x, [&](int i) { return mask[i] != 0; }, h, w, conn, parent, area, inter, sh);
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += nt) {                 // a prefix count of the kept-root flags, nt pixels at a time
    const int i = c0 + tid;
    const bool keep = i < n && x.ld(parent + i) == i && x.ld(area + i) >= min_area;
    int total;
    const int pre = x.scan(keep, sh, total);
    if (keep) x.st(inter + i, base + pre + 1);
    base += total;
  }
  x.sync();
  for (int i = tid; i < n; i += nt) {
    const int p = x.ld(parent + i);
    const int v = p >= 0 ? x.ld(inter + p) : 0;
    labels[i] = (uint8_t)(v >= 1 && v <= RS_MAX_REGIONS ? v : 0);
  }
  return sh.fail ? -1 : base;
}

#ifdef AMMC_REGION_HOST

struct RsHost {                                        // one thread is the whole workgroup
  int tid() const { return 0; }
  int nt() const { return 1; }
  void sync() const {}
  int ld(const int* p) const { return *p; }
  void st(int* p, int v) const { *p = v; }
  void sti(int* p, int v) const { *p = v; }
  int amin(int* p, int v) const { const int o = *p; if (v < o) *p = v; return o; }
  void aadd(int* p, int v) const { *p += v; }
  void aor(unsigned* p, unsigned v) const { *p |= v; }
  int scan(bool flag, RsShared&, int& total) const { total = flag; return 0; }
};

#else

struct RsDev {
  RS_FN int tid() const { return (int)threadIdx.x; }
  RS_FN int nt() const { return (int)blockDim.x; }
  RS_FN void sync() const { __threadfence(); __syncthreads(); }
  RS_FN int ld(const int* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  RS_FN void st(int* p, int v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  RS_FN void sti(int* p, int v) const { *(volatile int*)p = v; }       // an LDS flag that only ever becomes 1
  RS_FN int amin(int* p, int v) const { return atomicMin(p, v); }
  RS_FN void aadd(int* p, int v) const { atomicAdd(p, v); }
  RS_FN void aor(unsigned* p, unsigned v) const { atomicOr(p, v); }
  // the number of set flags among the threads below this one, and among all; every thread of the workgroup calls it
  RS_FN int scan(bool flag, RsShared& sh, int& total) const {
    const int lane = (int)threadIdx.x & (RS_WAVE - 1), wv = (int)threadIdx.x / RS_WAVE;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) sh.wsum[wv] = __popcll(b);
    __syncthreads();
    int below = 0, all = 0;
    const int nw = ((int)blockDim.x + RS_WAVE - 1) / RS_WAVE;
    for (int k = 0; k < nw; ++k) {
      const int v = sh.wsum[k];
      below += k < wv ? v : 0;
      all += v;
    }
    __syncthreads();
    total = all;
    return below + __popcll(b & ((1ull << lane) - 1ull));
  }
};

__global__ __launch_bounds__(RS_MAX_THREADS) void region_scores_kernel(const float* __restrict__ map, int64_t map_bs,
                                                                       const uint8_t* __restrict__ lab, int64_t lab_bs,
                                                                       const float* __restrict__ thr, int nthr, int h, int w,
                                                                       int num, int den, int min_area, int conn,
                                                                       int* __restrict__ n_px, int* __restrict__ n_comp,
                                                                       int* __restrict__ n_fp, int* __restrict__ hit,
                                                                       int64_t out_rs, int* __restrict__ ws) {
  __shared__ RsShared sh;
  const int b = (int)blockIdx.x / nthr, t = (int)blockIdx.x - b * nthr;
  const int64_t n = (int64_t)h * w;
  int* parent = ws + (int64_t)blockIdx.x * 3 * n;
  int out[4];
  rs_scores_one(RsDev(), map + b * map_bs, lab + b * lab_bs, thr[t], h, w, num, den, min_area, conn, parent, parent + n,
                parent + 2 * n, sh, out);
  if (threadIdx.x == 0) {
    const int64_t o = b * out_rs + t;
    n_px[o] = out[0], n_comp[o] = out[1], n_fp[o] = out[2], hit[o] = out[3];
  }
}

__global__ __launch_bounds__(RS_MAX_THREADS) void label_regions_kernel(const uint8_t* __restrict__ mask, int64_t mask_bs, int h,
                                                                       int w, int min_area, int conn,
                                                                       uint8_t* __restrict__ labels, int64_t labels_bs,
                                                                       int* __restrict__ count, int* __restrict__ ws) {
  __shared__ RsShared sh;
  const int b = (int)blockIdx.x;
  const int64_t n = (int64_t)h * w;
  int* parent = ws + (int64_t)b * 3 * n;
  const int c = rs_number_one(RsDev(), mask + b * mask_bs, h, w, min_area, conn, labels + b * labels_bs, parent, parent + n,
                              parent + 2 * n, sh);
  if (threadIdx.x == 0) count[b] = c;
}

static int rs_threads(int64_t n) {
  const int64_t t = (n + RS_WAVE - 1) / RS_WAVE * RS_WAVE;
  return (int)(t > RS_MAX_THREADS ? RS_MAX_THREADS : t);
}

static int64_t rs_workspace_bytes(int64_t batch, int64_t t, int64_t h, int64_t w) {
  if (batch < 1 || t < 1 || h < 1 || w < 1 || h * w > RS_MAX_PIXELS || batch * t > 0x7fffffffLL) return -1;
  return batch * t * 3 * h * w * (int64_t)sizeof(int);
}

#endif  // AMMC_REGION_HOST

}  // namespace ammc_impl

#ifndef AMMC_REGION_HOST
using namespace ammc_impl;

extern "C" {

int64_t ammc_region_workspace_bytes(int32_t batch, int32_t t, int32_t h, int32_t w) { return rs_workspace_bytes(batch, t, h, w); }

int ammc_label_regions_u8(const uint8_t* mask, int64_t mask_bs, int32_t batch, int32_t h, int32_t w, int32_t min_area,
                          int32_t connectivity, uint8_t* labels, int64_t labels_bs, int32_t* count, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  if (!mask || !labels || !count || !workspace) return AMMC_EINVAL;
  if (batch < 1 || h < 1 || w < 1 || min_area < 1) return AMMC_EINVAL;
  if (connectivity != 4 && connectivity != 8) return AMMC_EINVAL;
  const int64_t n = (int64_t)h * w;
  if (n > RS_MAX_PIXELS) return AMMC_EINVAL;
  if (batch > 1 && (mask_bs < n || labels_bs < n)) return AMMC_EINVAL;
  if (((uintptr_t)count | (uintptr_t)workspace) & 3) return AMMC_EINVAL;
  if (workspace_bytes < rs_workspace_bytes(batch, 1, h, w)) return AMMC_EINVAL;
  hipLaunchKernelGGL(label_regions_kernel, dim3((unsigned)batch), dim3((unsigned)rs_threads(n)), 0, (hipStream_t)stream, mask,
                     mask_bs, h, w, min_area, connectivity, labels, labels_bs, count, (int*)workspace);
  return ammc_launch_status();
}

int ammc_region_scores_f32(const float* map, int64_t map_bs, const uint8_t* labels, int64_t labels_bs, int32_t batch, int32_t h,
                           int32_t w, const float* thresholds, int32_t t, int32_t num, int32_t den, int32_t min_area,
                           int32_t connectivity, int32_t* n_px, int32_t* n_comp, int32_t* n_fp, int32_t* hit, int64_t out_rs,
                           void* workspace, int64_t workspace_bytes, void* stream) {
  if (!map || !labels || !thresholds || !n_px || !n_comp || !n_fp || !hit || !workspace) return AMMC_EINVAL;
  if (batch < 1 || h < 1 || w < 1 || t < 1 || min_area < 1) return AMMC_EINVAL;
  if (connectivity != 4 && connectivity != 8) return AMMC_EINVAL;
  if (num < 1 || den < num || den > 4096) return AMMC_EINVAL;
  const int64_t n = (int64_t)h * w;
  if (n > RS_MAX_PIXELS) return AMMC_EINVAL;
  if (batch > 1 && (map_bs < n || labels_bs < n || out_rs < t)) return AMMC_EINVAL;
  if (((uintptr_t)map | (uintptr_t)thresholds | (uintptr_t)n_px | (uintptr_t)n_comp | (uintptr_t)n_fp | (uintptr_t)hit |
       (uintptr_t)workspace) & 3)
    return AMMC_EINVAL;
  if ((int64_t)batch * t > 0x7fffffffLL) return AMMC_EUNSUP;
  if (workspace_bytes < rs_workspace_bytes(batch, t, h, w)) return AMMC_EINVAL;
  hipLaunchKernelGGL(region_scores_kernel, dim3((unsigned)(batch * t)), dim3((unsigned)rs_threads(n)), 0, (hipStream_t)stream,
                     map, map_bs, labels, labels_bs, thresholds, t, h, w, num, den, min_area, connectivity, n_px, n_comp, n_fp,
                     hit, out_rs, (int*)workspace);
  return ammc_launch_status();
}

}  // extern "C"
#endif
