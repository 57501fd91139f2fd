// Host build of the per-tile routine of csrc/fuse_maps.hip (one thread as the whole workgroup) against a plain loop
// restatement of the definitions, over the shapes of the GPU tests.  Meant for the host sanitizers: the tile's scratch
// arrays are heap blocks of exactly the size the routine states, so every index of every phase is checked without a
// device.
//
//   mkdir -p build
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/fuse_maps_host_check.cpp -o build/fuse_maps_host_check
//   build/fuse_maps_host_check        # prints one line per frame size, exits 0 when everything agrees
#define AMMC_FUSE_HOST
#include "../ammcnet_aaai2021_amd/csrc/fuse_maps.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace ammc_impl;

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static float rnd01() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((rng_state >> 40) & 0xffffff) / 16777216.0f;
}

static int fails = 0;
static void expect(bool ok, const char* what, int h, int w, int n_ch, int r, int p) {
  if (!ok) {
    ++fails;
    std::printf("MISMATCH %s at %d x %d, n_ch %d, radius %d, patch %d\n", what, h, w, n_ch, r, p);
  }
}

// ceil_grid: the coarse grids have ceil(h / cell) rows (else h / cell, at least 1: the last cells are reached by clamping)
static void run_case(int B, int h, int w, int n_ch, int radius, int patch, bool ceil_grid, int64_t pad) {
  const int cells[4] = {1, 1, 8, 8};
  std::vector<std::vector<float>> src(n_ch);
  FmArgs a = {};
  std::vector<float> coef(n_ch);
  for (int c = 0; c < n_ch; ++c) {
    const int cell = cells[c];
    int gh = ceil_grid ? (h + cell - 1) / cell : h / cell, gw = ceil_grid ? (w + cell - 1) / cell : w / cell;
    if (gh < 1) gh = 1;
    if (gw < 1) gw = 1;
    const int64_t bs = (int64_t)gh * gw + pad;
    src[c].resize((size_t)(bs * (B - 1) + (int64_t)gh * gw));
    for (float& v : src[c]) v = rnd01();
    int shift = -1;
    for (int s = 0; s < 31; ++s)
      if (cell == (1 << s)) shift = s;
    if (c == 1) shift = -1;                            // the division path of fm_cell, at cell 1
    a.src[c] = {src[c].data(), bs, gh, gw, cell, shift};
    coef[c] = 0.25f + rnd01();
  }
  const int ph = (h + patch - 1) / patch, pw = (w + patch - 1) / patch;
  const int tiles_y = (h + FM_TH - 1) / FM_TH, tiles_x = (w + FM_TW - 1) / FM_TW;
  const int64_t px_bs = (int64_t)h * w + pad, pm_bs = (int64_t)ph * pw + pad;
  std::vector<float> pixel((size_t)(px_bs * (B - 1) + (int64_t)h * w), -1.f), pmean((size_t)(pm_bs * (B - 1) + ph * pw), -1.f);
  std::vector<float> tmax((size_t)B * tiles_y * tiles_x, -1.f);
  a.coef = coef.data();
  a.n_ch = n_ch, a.h = h, a.w = w, a.radius = radius, a.patch = patch, a.ph = ph, a.pw = pw;
  a.tiles_x = tiles_x, a.tiles_y = tiles_y;
  a.pixel = pixel.data(), a.px_bs = px_bs, a.px_vec = (w % 4 == 0 && px_bs % 4 == 0);
  a.patch_mean = pmean.data(), a.pm_bs = pm_bs;
  a.tile_max = tmax.data();
  const int sh = FM_TH + 2 * radius, sw = FM_TW + 2 * radius;
  for (int b = 0; b < B; ++b)
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        std::vector<float> raw((size_t)sh * sw), hs((size_t)sh * FM_TW), qs(FM_QUADS), tm(FM_QUADS), rs((size_t)FM_TH * (FM_TW / patch));
        fm_tile(FmHost(), a, b, ty, tx, raw.data(), hs.data(), qs.data(), tm.data(), rs.data());
      }
  // the definitions, as plain loops in the order the header states
  for (int b = 0; b < B; ++b) {
    std::vector<float> raw((size_t)h * w);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        float v = 0.f;
        for (int c = 0; c < n_ch; ++c) {
          const FmSrc& s = a.src[c];
          int gy = y / s.cell, gx = x / s.cell;
          if (gy > s.gh - 1) gy = s.gh - 1;
          if (gx > s.gw - 1) gx = s.gw - 1;
          const float term = coef[c] * src[c][(size_t)(b * s.bs + (int64_t)gy * s.gw + gx)];
          v = c == 0 ? term : v + term;
        }
        raw[(size_t)y * w + x] = v;
      }
    float best = -INFINITY;
    bool pix_ok = true;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        float acc = 0.f;
        int rows = 0, cols = 0;
        for (int yy = y - radius; yy <= y + radius; ++yy) {
          if (yy < 0 || yy >= h) continue;
          float row = 0.f;
          cols = 0;
          for (int xx = x - radius; xx <= x + radius; ++xx) {
            if (xx < 0 || xx >= w) continue;
            row = cols == 0 ? raw[(size_t)yy * w + xx] : row + raw[(size_t)yy * w + xx];
            ++cols;
          }
          acc = rows == 0 ? row : acc + row;
          ++rows;
        }
        const float want = acc / (float)(rows * cols);
        pix_ok = pix_ok && pixel[(size_t)(b * px_bs + (int64_t)y * w + x)] == want;
        if (want > best) best = want;
      }
    expect(pix_ok, "pixel", h, w, n_ch, radius, patch);
    float got_best = -INFINITY;
    for (int t = 0; t < tiles_y * tiles_x; ++t) got_best = fm_max(got_best, tmax[(size_t)b * tiles_y * tiles_x + t]);
    expect(got_best == best, "frame_max", h, w, n_ch, radius, patch);
    bool pm_ok = true;
    for (int i = 0; i < ph; ++i)
      for (int j = 0; j < pw; ++j) {
        double s = 0.0;
        int n = 0;
        for (int y = i * patch; y < (i + 1) * patch && y < h; ++y)
          for (int x = j * patch; x < (j + 1) * patch && x < w; ++x, ++n) s += (double)pixel[(size_t)(b * px_bs + (int64_t)y * w + x)];
        const double want = s / n, got = (double)pmean[(size_t)(b * pm_bs + i * pw + j)];
        pm_ok = pm_ok && fabs(got - want) <= 1.01 * (n + 1) * ldexp(1.0, -24) * want;
      }
    expect(pm_ok, "patch_mean", h, w, n_ch, radius, patch);
  }
  if (pad)                                              // nothing written between the samples
    for (int b = 0; b + 1 < B; ++b)
      for (int64_t k = 0; k < pad; ++k) {
        expect(pixel[(size_t)(b * px_bs + (int64_t)h * w + k)] == -1.f, "pixel gap", h, w, n_ch, radius, patch);
        expect(pmean[(size_t)(b * pm_bs + ph * pw + k)] == -1.f, "patch_mean gap", h, w, n_ch, radius, patch);
      }
}

int main() {
  const int sizes[][2] = {{8, 8}, {17, 23}, {40, 72}, {64, 64}, {1, 1}, {33, 130}, {256, 256}};
  const int radii[] = {0, 1, 2, 4, 8}, patches[] = {8, 16, 32};
  for (const auto& hw : sizes) {
    int cases = 0;
    const bool big = hw[0] * hw[1] > 64 * 64;
    for (int n_ch = 1; n_ch <= 4; ++n_ch)
      for (int radius : radii)
        for (int patch : patches) {
          if (big && (n_ch != 4 || patch != 16)) continue;
          run_case(big ? 1 : 3, hw[0], hw[1], n_ch, radius, patch, false, (cases % 3 == 0) ? 0 : (cases % 3 == 1 ? 4 : 5));
          run_case(big ? 1 : 2, hw[0], hw[1], n_ch, radius, patch, true, 0);
          cases += 2;
        }
    std::printf("%3d x %3d: %d cases, %d mismatches so far\n", hw[0], hw[1], cases, fails);
  }
  std::printf(fails ? "FAILED\n" : "fuse_maps host check: all cases agree\n");
  return fails ? 1 : 0;
}
