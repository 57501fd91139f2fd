// Host build of the per-workgroup routines of csrc/region_scores.hip (one thread as the whole workgroup) against a
// breadth-first flood fill and the scores as the definitions state them, over the shapes of the GPU tests.  Meant for
// the host sanitizers: every bound of the labelling routine is checked without a device.
//
//   mkdir -p build
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/region_host_check.cpp -o build/region_host_check
//   build/region_host_check        # prints one line per case group, exits 0 when everything agrees
#define AMMC_REGION_HOST
#include "../ammcnet_aaai2021_amd/csrc/region_scores.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

using namespace ammc_impl;
typedef std::vector<uint8_t> Img;

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(rng_state >> 33);
}

// components of fg in raster order of their first pixel: comp[i] = 1.. (0: background); returns their sizes
static std::vector<int> flood(const Img& fg, int h, int w, int conn, std::vector<int>& comp) {
  comp.assign((size_t)h * w, 0);
  std::vector<int> sizes, queue;
  for (int s = 0; s < h * w; ++s) {
    if (!fg[s] || comp[s]) continue;
    const int id = (int)sizes.size() + 1;
    comp[s] = id;
    queue.assign(1, s);
    for (size_t q = 0; q < queue.size(); ++q) {
      const int y = queue[q] / w, x = queue[q] % w;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((!dy && !dx) || (conn == 4 && dy && dx)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
          const int j = yy * w + xx;
          if (fg[j] && !comp[j]) comp[j] = id, queue.push_back(j);
        }
    }
    sizes.push_back((int)queue.size());
  }
  return sizes;
}

static Img want_labels(const Img& mask, int h, int w, int conn, int min_area, int& count) {
  std::vector<int> comp;
  const std::vector<int> sizes = flood(mask, h, w, conn, comp);
  std::vector<int> rank(sizes.size() + 1, 0);
  count = 0;
  for (size_t c = 0; c < sizes.size(); ++c)
    if (sizes[c] >= min_area) rank[c + 1] = ++count;
  Img out((size_t)h * w, 0);
  for (int i = 0; i < h * w; ++i) {
    const int r = rank[comp[i]];
    out[i] = (uint8_t)(r >= 1 && r <= 32 ? r : 0);
  }
  return out;
}

static int failures = 0;
static void expect(bool ok, const std::string& what) {
  if (!ok) {
    std::printf("MISMATCH %s\n", what.c_str());
    ++failures;
  }
}

static void check(const std::string& name, const std::vector<float>& map, const Img& mask, int h, int w,
                  const std::vector<float>& thr) {
  const int n = h * w;
  std::vector<int> ws(3 * (size_t)n, -7);
  RsShared sh;
  for (int conn : {4, 8})
    for (int min_area : {1, 3}) {
      int want_count;
      const Img want = want_labels(mask, h, w, conn, min_area, want_count);
      Img got((size_t)n, 255);
      const int count = rs_number_one(RsHost(), mask.data(), h, w, min_area, conn, got.data(), ws.data(), ws.data() + n,
                                      ws.data() + 2 * n, sh);
      expect(count == want_count && got == want, name + " labels");
      for (float t : thr)
        for (int num : {1, 1, 3}) {
          const int den = num == 3 ? 4 : (min_area == 1 ? 10 : 1);
          Img fg((size_t)n);
          int n_px = 0;
          for (int i = 0; i < n; ++i) n_px += fg[i] = map[i] >= t;
          std::vector<int> comp;
          const std::vector<int> sizes = flood(fg, h, w, conn, comp);
          int n_comp = 0, n_fp = 0;
          unsigned hit = 0;
          std::vector<long long> gsize(33, 0);
          for (int i = 0; i < n; ++i)
            if (want[i]) ++gsize[want[i]];
          for (size_t c = 0; c < sizes.size(); ++c) {
            if (sizes[c] < min_area) continue;
            ++n_comp;
            bool any = false;
            for (int r = 1; r <= 32; ++r) {
              if (!gsize[r]) continue;
              long long inter = 0;
              for (int i = 0; i < n; ++i) inter += comp[i] == (int)c + 1 && want[i] == r;
              if (inter > 0 && inter * den >= num * (sizes[c] + gsize[r] - inter)) any = true, hit |= 1u << (r - 1);
            }
            n_fp += !any;
          }
          int out[4];
          rs_scores_one(RsHost(), map.data(), want.data(), t, h, w, num, den, min_area, conn, ws.data(), ws.data() + n,
                        ws.data() + 2 * n, sh, out);
          expect(out[0] == n_px && out[1] == n_comp && out[2] == n_fp && (unsigned)out[3] == hit, name + " scores");
        }
    }
}

static void shape_case(const std::string& name, const Img& fg, int h, int w) {
  // the picture as the mask and as the map (1 inside, 0 outside), and a smooth map against the picture's regions
  std::vector<float> map((size_t)h * w), smooth((size_t)h * w);
  for (int i = 0; i < h * w; ++i) {
    map[i] = fg[i] ? 1.f : 0.f;
    smooth[i] = 0.5f + 0.5f * std::sin(0.7f * (i / w)) * std::cos(0.45f * (i % w));
  }
  check(name, map, fg, h, w, {0.5f, 1.f, 0.f, 2.f});
  check(name + "/smooth", smooth, fg, h, w, {0.2f, 0.5f, 0.8f});
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 3}, {17, 23}, {33, 31}, {64, 64}};
  for (const auto& s : shapes) {
    const int h = s[0], w = s[1];
    for (int dens : {0, 10, 45, 60, 90, 100}) {
      Img fg((size_t)h * w);
      for (auto& v : fg) v = (int)(rnd() % 100) < dens ? (uint8_t)(1 + rnd() % 255) : 0;
      shape_case("random " + std::to_string(h) + "x" + std::to_string(w) + " @" + std::to_string(dens), fg, h, w);
    }
  }
  std::printf("random shapes done\n");
  {
    Img cb(64);
    for (int i = 0; i < 64; ++i) cb[i] = ((i / 8) + (i % 8)) % 2 == 0;
    shape_case("checkerboard", cb, 8, 8);
    const int h = 16, w = 16;
    Img spiral((size_t)h * w, 0), serp((size_t)h * w, 0), u((size_t)h * w, 0), comb((size_t)h * w, 0), diag((size_t)h * w, 0),
        ring((size_t)h * w, 0), many((size_t)33 * 31, 0);
    int y = 0, x = 0, dy = 0, dx = 1, y0 = 0, y1 = h - 1, x0 = 0, x1 = w - 1;          // a one-pixel-wide spiral, gaps of one
    for (int turn = 0; turn < 64 && y0 <= y1 && x0 <= x1; ++turn) {
      while (y >= y0 && y <= y1 && x >= x0 && x <= x1) spiral[y * w + x] = 1, y += dy, x += dx;
      y -= dy, x -= dx;
      if (dx == 1) y0 += 2; else if (dy == 1) x1 -= 2; else if (dx == -1) y1 -= 2; else x0 += 2;
      const int t = dy; dy = dx, dx = -t;
      y += dy, x += dx;
    }
    for (int r = 0; r < h; ++r)
      for (int c = 0; c < w; ++c) {
        if (r % 2 == 0 || c == (r % 4 == 1 ? w - 1 : 0)) serp[r * w + c] = 1;
        if (c == 2 || c == 13 || r == h - 1) u[r * w + c] = c >= 2 && c <= 13;
        if (c % 2 == 0 || r == h - 1) comb[r * w + c] = 1;
        if ((r < 8 && c < 8) || (r >= 8 && c >= 8)) diag[r * w + c] = 1;
        if (r == 0 || c == 0 || r == h - 1 || c == w - 1) ring[r * w + c] = 1;
      }
    shape_case("spiral", spiral, h, w);
    shape_case("serpentine", serp, h, w);
    shape_case("u", u, h, w);
    shape_case("comb", comb, h, w);
    shape_case("diagonal blobs", diag, h, w);
    shape_case("ring", ring, h, w);
    for (int r = 0; r < 33; r += 2)                                                    // more than 32 regions
      for (int c = 0; c < 31; c += 2) many[r * 31 + c] = 1;
    shape_case("many", many, 33, 31);
    // a 256 x 256 serpentine: the longest walks
    Img big((size_t)256 * 256, 0);
    for (int r = 0; r < 256; ++r)
      for (int c = 0; c < 256; ++c)
        if (r % 2 == 0 || c == (r % 4 == 1 ? 255 : 0)) big[r * 256 + c] = 1;
    std::vector<float> m((size_t)256 * 256);
    for (size_t i = 0; i < m.size(); ++i) m[i] = big[i];
    check("serpentine 256", m, big, 256, 256, {1.f});
  }
  std::printf("pictures done\n");
  {
    const int h = 5, w = 7;
    std::vector<float> v((size_t)h * w);
    const float kinds[] = {0.f, -0.f, -1.f, inf, -inf, nan, 0.25f, 1e-40f};
    for (auto& e : v) e = kinds[rnd() % 8];
    Img mask((size_t)h * w);
    for (auto& e : mask) e = rnd() % 3 == 0;
    check("values", v, mask, h, w, {0.f, -0.f, 0.25f, inf, -inf, nan, -1.f, 1e-40f});
  }
  std::printf("values done\n%s\n", failures ? "FAILED" : "all equal");
  return failures ? 1 : 0;
}
