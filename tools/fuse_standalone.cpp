// Stand-alone run of the fusion (mvn_fuse_resampled and psi start, csrc/mvn_fuse.hpp) on the host emulation under
// AddressSanitizer + UBSan, at the (3, 5, 7) and (10, 14, 70) groups of tests/fuse_reference.py: an odd last extent, and
// a block larger than the kernel's tile on every axis by a non-multiple.  Raw stacks (view 0 uint16, view 1 float32) and
// outputs (float32 and uint16) are heap blocks of exactly their bytes, handed over once as host memory (uploads, a dense
// device volume, copies out) and once described as device memory, which the emulation lets any pointer be: the kernel
// then reads and writes the heap blocks themselves and the sanitizer sees an access past them.  Both routes must give
// the same bytes.  Then one mvn_deconvolve_resampled call with psi start 1 from a psi of NaNs, whose result must be
// finite.  Built with -fsanitize=address,undefined against the emulation built the same way (csrc/Makefile, target
// fuse-asan); exits non-zero on a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "multiviewnative.h"
#include "mvn_engine_api.h"

static const double C30 = 0.86602540378443864676, S30 = 0.5;

struct View {
  int m[3];
  double M[12];
  float border[3], range[3];
};
struct Group {
  const char* name;
  int block[3];
  View view[2];
};

static int fail(const char* what, const char* name) {
  std::printf("FAILED %s: %s (%s)\n", name, what, mvn_last_error());
  return 1;
}

static mvn_stack_desc dense(int dtype, int location, const int* n) {
  mvn_stack_desc d;
  d.dtype = dtype, d.location = location;
  d.stride[0] = (long long)n[1] * n[2], d.stride[1] = n[2], d.stride[2] = 1;
  return d;
}

static int run(const Group& g) {
  const int V = 2;
  std::mt19937 rng(11u);
  std::uniform_int_distribution<int> px(100, 3999);
  mvn_view_geometry geom[2];
  std::vector<uint16_t> raw0;
  std::vector<float> raw1;
  for (int v = 0; v < V; ++v) {
    const View& w = g.view[v];
    for (int k = 0; k < 3; ++k) geom[v].src_dims[k] = w.m[k], geom[v].blend_border[k] = w.border[k], geom[v].blend_range[k] = w.range[k];
    for (int i = 0; i < 12; ++i) geom[v].matrix[i] = w.M[i];
    const size_t n = (size_t)w.m[0] * w.m[1] * w.m[2];
    if (v == 0) {
      raw0.resize(n);
      for (uint16_t& x : raw0) x = (uint16_t)px(rng);
    } else {
      raw1.resize(n);
      for (float& x : raw1) x = (float)px(rng) + 0.25f;
    }
  }
  const void* raws[2] = {raw0.data(), raw1.data()};
  const size_t voxels = (size_t)g.block[0] * g.block[1] * g.block[2];
  long long before[2], after[2];
  if (mvn_fuse_counters(before) < 0) return fail("counters", g.name);
  for (int u16 = 0; u16 < 2; ++u16) {
    const size_t esz = u16 ? sizeof(uint16_t) : sizeof(float);
    std::vector<unsigned char> out[2];
    for (int loc = 0; loc < 2; ++loc) {  // MVN_HOST, MVN_DEVICE
      out[loc].assign(voxels * esz, 0xAB);
      const mvn_stack_desc od = dense(u16 ? MVN_U16 : MVN_F32, loc, g.block);
      const mvn_stack_desc rd[2] = {dense(MVN_U16, loc, g.view[0].m), dense(MVN_F32, loc, g.view[1].m)};
      if (mvn_fuse_resampled(out[loc].data(), &od, g.block, V, raws, rd, geom, 123.5f, nullptr, 0) < 0)
        return fail("mvn_fuse_resampled", g.name);
      size_t need = 0;
      if (mvn_fuse_memory_resampled(&od, g.block, V, rd, geom, 0, &need) < 0 || need == 0) return fail("memory", g.name);
    }
    if (out[0] != out[1]) return fail("host and device routes differ", g.name);
    bool filled = false, fused = false;
    for (size_t i = 0; i < voxels; ++i) {
      const float f = u16 ? (float)((const uint16_t*)out[0].data())[i] : ((const float*)out[0].data())[i];
      if (!std::isfinite(f)) return fail("a non-finite voxel", g.name);
      filled = filled || f == (u16 ? 124.f : 123.5f);
      fused = fused || f > 200.f;
    }
    if (!filled || !fused) return fail("no filled or no fused voxel", g.name);
  }
  if (mvn_fuse_counters(after) < 0 || after[0] - before[0] != 4 || after[1] != before[1]) return fail("launches", g.name);
  // psi start: the loop from the fusion of the engine's volumes, psi output only
  int kd[3] = {3, 3, 3};
  std::vector<float> kernel(27, 1.f / 27.f), psi(voxels, std::numeric_limits<float>::quiet_NaN());
  int dims[3] = {g.block[0], g.block[1], g.block[2]};
  view_data views[2];
  std::memset(views, 0, sizeof views);
  for (int v = 0; v < V; ++v) {
    views[v].image_ = (float*)raws[v];
    views[v].kernel1_ = views[v].kernel2_ = kernel.data();
    views[v].image_dims_ = views[v].weights_dims_ = dims;
    views[v].kernel1_dims_ = views[v].kernel2_dims_ = kd;
  }
  workspace ws;
  std::memset(&ws, 0, sizeof ws);
  ws.data_ = views, ws.num_views_ = V, ws.lambda_ = 0.006, ws.minValue_ = 1e-4f, ws.num_iterations_ = 2;
  const mvn_stack_desc id[2] = {dense(MVN_U16, MVN_HOST, g.view[0].m), dense(MVN_F32, MVN_HOST, g.view[1].m)};
  mvn_call_desc cd;
  std::memset(&cd, 0, sizeof cd);
  cd.psi = dense(MVN_F32, MVN_HOST, g.block);
  cd.image = id;
  const char* modes[2] = {"zero", "reflect"};
  for (int m = 0; m < 2; ++m) {
    psi.assign(voxels, std::numeric_limits<float>::quiet_NaN());
    if (mvn_set_pad_mode(modes[m]) < 0 || mvn_set_psi_start(1, 300.f) < 0) return fail("switches", g.name);
    const int rc = mvn_deconvolve_resampled(psi.data(), ws, &cd, geom, 1, 0);
    mvn_set_psi_start(0, 0.f);
    mvn_set_pad_mode(nullptr);
    if (rc < 0) return fail(modes[m], g.name);
    for (float x : psi)
      if (!std::isfinite(x)) return fail("psi start left a non-finite voxel", g.name);
  }
  if (mvn_fuse_counters(after) < 0 || after[1] - before[1] != 2) return fail("psi start launches", g.name);
  std::printf("%s: fused\n", g.name);
  return 0;
}

int main() {
  const Group groups[] = {
      {"(3, 5, 7)",
       {3, 5, 7},
       {{{5, 6, 7}, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {0, 1, 0.5f}, {1, 2, 1.5f}},
        {{5, 6, 7},
         {C30, 0, S30, 2 - C30 * 1 - S30 * 3, 0, 1, 0, 0.5, -S30, 0, C30, 3 + S30 * 1 - C30 * 3},
         {0, 0.25f, 0},
         {1, 1, 1.5f}}}},
      {"(10, 14, 70)",
       {10, 14, 70},
       {{{5, 6, 7}, {1.0 / 3, 0, 0, 0, 0, 0.35, 0, 0, 0, 0, 0.08, 0}, {0.5f, 0, 0.25f}, {1, 1.5f, 2}},
        {{5, 6, 7},
         {0.3 * C30, 0, 0.05 * S30, 2 - 0.3 * C30 * 4.5 - 0.05 * S30 * 34.5, 0, 0.38, 0, 0, -0.3 * S30, 0, 0.05 * C30,
          3 + 0.3 * S30 * 4.5 - 0.05 * C30 * 34.5},
         {0, 0, 0},
         {0.5f, 1, 1}}}},
  };
  int bad = 0;
  for (const Group& g : groups) bad += run(g);
  mvn_release_cached_engines();
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
