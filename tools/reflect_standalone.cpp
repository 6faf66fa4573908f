// Stand-alone run of the reflect fill (mvn_set_pad_mode("reflect"), csrc/mvn_reflect.hpp) on the host emulation under
// AddressSanitizer + UBSan, on the shapes of the parity tests (tests/reflect_reference.py): a block, an odd last extent
// (row padding, 4-byte row copies), margins wider than the stack, an extent of 1 and an axis without a margin.  For
// each: the fill alone on a float32 and on a uint16 volume of exactly the volume's bytes (mvn_reflect_time - the
// sanitizer sees an access past it), and one "reflect" call of inplace_gpu_deconvolve on exactly-sized heap stacks,
// whose result must be finite and must differ from the "zero" call's.  Built with -fsanitize=address,undefined against
// the emulation built the same way (csrc/Makefile, target reflect-asan); exits non-zero on a failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "multiviewnative.h"
#include "mvn_engine_api.h"

struct Case {
  const char* name;
  int d[3], k[3];
  int ext[3];  // a volume the fill alone runs on (the window at (k - 1) / 2)
};

static int fail(const char* what, const char* name) {
  std::printf("FAILED %s: %s (%s)\n", name, what, mvn_last_error());
  return 1;
}

static int run(const Case& c) {
  const int V = 2;
  int dims[3] = {c.d[0], c.d[1], c.d[2]}, kd[3] = {c.k[0], c.k[1], c.k[2]};
  int ext[3] = {c.ext[0], c.ext[1], c.ext[2]}, off[3] = {(c.k[0] - 1) / 2, (c.k[1] - 1) / 2, (c.k[2] - 1) / 2};
  float ms[2];
  long long before[2], after[2];
  if (mvn_reflect_counters(before) < 0) return fail("counters", c.name);
  for (int u16 = 0; u16 < 2; ++u16)
    if (mvn_reflect_time(0, dims, ext, off, u16, 1, ms) < 0) return fail("the fill alone", c.name);
  const long n = (long)c.d[0] * c.d[1] * c.d[2], kn = (long)c.k[0] * c.k[1] * c.k[2];
  std::mt19937 rng(7u + (unsigned)n);
  std::uniform_real_distribution<float> px(1.f, 200.f), wt(0.1f, 0.5f);
  std::vector<float> kernel((size_t)kn);
  float ks = 0.f;
  for (long i = 0; i < kn; ++i) ks += kernel[(size_t)i] = 1.f + (float)(i % 5);
  for (float& k : kernel) k /= ks;
  std::vector<std::vector<float>> img((size_t)V), wts((size_t)V);
  std::vector<view_data> views((size_t)V);
  for (int v = 0; v < V; ++v) {
    img[(size_t)v].resize((size_t)n);
    wts[(size_t)v].resize((size_t)n);
    for (float& x : img[(size_t)v]) x = px(rng);
    for (float& x : wts[(size_t)v]) x = wt(rng);
    view_data& d = views[(size_t)v];
    d.image_ = img[(size_t)v].data(), d.weights_ = wts[(size_t)v].data();
    d.kernel1_ = d.kernel2_ = kernel.data();
    d.image_dims_ = d.weights_dims_ = dims;
    d.kernel1_dims_ = d.kernel2_dims_ = kd;
  }
  workspace ws;
  std::memset(&ws, 0, sizeof ws);
  ws.data_ = views.data(), ws.num_views_ = V, ws.lambda_ = 0.006, ws.minValue_ = 1e-4f, ws.num_iterations_ = 2;
  std::vector<float> psi[2];
  const char* modes[2] = {"zero", "reflect"};
  for (int m = 0; m < 2; ++m) {
    psi[m].assign((size_t)n, 50.f);
    if (mvn_set_pad_mode(modes[m]) < 0) return fail("mvn_set_pad_mode", c.name);
    inplace_gpu_deconvolve(psi[m].data(), ws, 0);
    if (*mvn_last_error()) return fail(modes[m], c.name);
    for (float x : psi[m])
      if (!std::isfinite(x)) return fail("a non-finite voxel", c.name);
  }
  mvn_set_pad_mode(nullptr);
  if (psi[0] == psi[1]) return fail("\"reflect\" gave what \"zero\" gives", c.name);
  // (the fill alone: a warm-up and one timed fill per element type; the call: psi, and image and weights of every view)
  if (mvn_reflect_counters(after) < 0 || after[1] - before[1] != 2 * 2 + 2 * V + 1) return fail("volumes filled", c.name);
  std::printf("%s: filled\n", c.name);
  return 0;
}

int main() {
  const Case cases[] = {
      {"block", {20, 18, 22}, {5, 5, 5}, {24, 24, 27}},
      {"odd last extent", {6, 10, 15}, {7, 3, 5}, {12, 12, 20}},
      {"margins wider than the stack", {3, 5, 2}, {9, 3, 7}, {12, 7, 8}},
      {"an extent of 1", {1, 12, 16}, {1, 5, 5}, {1, 16, 20}},
      {"an axis without a margin", {12, 16, 20}, {3, 3, 1}, {14, 18, 20}},
      {"uint16 rows of 16-byte groups", {5, 9, 20}, {3, 3, 5}, {7, 12, 24}},
  };
  int bad = 0;
  for (const Case& c : cases) bad += run(c);
  mvn_release_cached_engines();
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
