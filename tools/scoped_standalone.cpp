// Stand-alone run of the host code's error paths on the host emulation under AddressSanitizer + UBSan WITH leak
// detection: what csrc/mvn_backend.hpp's owning handles (DeviceBuffer, Stream, Event) are for.  The emulation refuses
// an allocation beyond MVN_EMU_TOTAL_MB per fake device (read at every allocation), so a cap set here makes a chosen
// allocation fail.  Needs MVN_EMU_DEVICES=2.
//   (a) every test and legacy utility that allocates scratch, once, at a shape whose first allocation fits the cap
//       and a later one does not: the call must fail, naming exhausted device memory
//   (b) a group of two slabs whose second engine cannot be built (device 1 is nearly full): what slab 0 created -
//       its engine, eight events, two streams - is released by the constructor's unwinding
//   (c) mvn_fft3_profile with the per-kind times (the profiler's event pool)
//   (d) one group that works: create, load, one sweep, destroy
//   (e) the engines' resident state, once each: an engine whose work volume does not fit, set_view on a live engine
//       whose PSF buffers do not fit, a streamed call (ring of two slots) and then one the planner refuses - the cached
//       engine with its ring goes -, a slab engine whose second exchange buffer does not fit
//   (f) a plan whose construction fails among the tables of its first axis
// Built with -fsanitize=address,undefined against the emulation built the same way (csrc/Makefile, target
// scoped-asan); exits non-zero on a failure, and LeakSanitizer reports at exit what was not released.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "multiviewnative.h"
#include "mvn_engine_api.h"

static int bad(const char* what) {
  std::printf("FAILED %s (%s)\n", what, mvn_last_error());
  return 1;
}

static void cap_mb(int mb) {
  if (mb > 0)
    setenv("MVN_EMU_TOTAL_MB", std::to_string(mb).c_str(), 1);
  else
    unsetenv("MVN_EMU_TOTAL_MB");
}

// the call must fail under the cap, with the emulation's message; `rc`: its return code, or for a void entry point 1
// after a message of another call's was put into mvn_last_error
static int must_exhaust(const char* name, int mb, const std::function<int()>& call,
                        const char* words = "device memory exhausted") {
  mvn_set_pad_mode("no such mode");  // (fails: mvn_last_error is this call's until the next failure)
  cap_mb(mb);
  const int rc = call();
  cap_mb(0);
  const std::string err = mvn_last_error();
  if (rc == 0 || err.rfind(name, 0) != 0 || err.find(words) == std::string::npos) return bad(name);
  std::printf("%s: refused\n", name);
  return 0;
}

int main() {
  const char* nd = std::getenv("MVN_EMU_DEVICES");
  if (!nd || std::atoi(nd) < 2) return bad("MVN_EMU_DEVICES must be >= 2");
  int fails = 0;
  // ---- (a): B = 126 x 64 x 64, a volume of 2016 KB with a Nyquist plane of 63 KB; the caps are what the same calls
  // need at 64^3, as in tests/test_emu_scoped.py
  int B[3] = {126, 64, 64}, K[3] = {3, 3, 3}, win[3] = {122, 60, 60}, off[3] = {2, 2, 2};
  const size_t n = (size_t)B[0] * B[1] * B[2], nspec = (size_t)B[0] * B[1] * (B[2] / 2 + 1);
  std::vector<float> a(3 * n), b(n), c(n), out(n), kernel(27, 1.f / 27.f), spec(3 * 2 * nspec), raw(8 * 8 * 8, 100.f);
  for (size_t i = 0; i < a.size(); ++i) a[i] = 1.f + (float)(i % 17) * 0.05f;
  for (size_t i = 0; i < n; ++i) b[i] = 2.f + (float)(i % 5), c[i] = 0.5f;
  mvn_view_geometry geom;
  std::memset(&geom, 0, sizeof geom);
  for (int k = 0; k < 3; ++k) geom.src_dims[k] = 8, geom.matrix[5 * k] = 0.1, geom.blend_range[k] = 2.f;
  float ms[2];
  fails += must_exhaust("mvn_tv_factor", 2, [&] { return mvn_tv_factor(0, B, a.data(), 0.005, 0.01, out.data()); });
  fails += must_exhaust("mvn_tv_time", 2, [&] { return mvn_tv_time(0, B, 1, ms); });
  fails += must_exhaust("mvn_reflect_time", 2, [&] { return mvn_reflect_time(0, win, B, off, 0, 1, ms); });
  fails += must_exhaust("mvn_resample_stack", 3,
                        [&] { return mvn_resample_stack(0, raw.data(), nullptr, &geom, B, out.data(), b.data()); });
  fails += must_exhaust("mvn_resample_time", 3, [&] { return mvn_resample_time(0, 0, &geom, B, 1, ms); });
  fails += must_exhaust("inplace_gpu_convolution", 3,
                        [&] { return inplace_gpu_convolution(a.data(), B, kernel.data(), K, 0), 1; });
  fails += must_exhaust("iterate_fft_plain", 5,
                        [&] { return iterate_fft_plain(a.data(), kernel.data(), out.data(), B, K, 0), 1; });
  fails += must_exhaust("compute_quotient", 2, [&] { return compute_quotient(a.data(), b.data(), n, 0), 1; });
  fails += must_exhaust("compute_final_values", 3,
                        [&] { return compute_final_values(a.data(), b.data(), c.data(), n, 1e-4f, 0.006, 0), 1; });
  fails += must_exhaust("mvn_fft3_r2c", 2, [&] { return mvn_fft3_r2c(0, B, a.data(), spec.data()); });
  fails += must_exhaust("mvn_fft3_many_r2c", 4, [&] { return mvn_fft3_many_r2c(0, B, 3, a.data(), spec.data()); });
  fails += must_exhaust("mvn_fft3_many_time", 4, [&] { return mvn_fft3_many_time(0, B, 3, 0, 1, ms); });

  // ---- (b): an engine of 64^3 on device 1 (two volumes of 1 MB and a Nyquist plane) under a cap of 3 MB leaves less
  // than the 1056 KB the first volume of a slab of 128 x 64 x 64 over two devices (64 + 2 planes) takes; slab 0, on
  // device 0, has room for its three
  {
    int E[3] = {64, 64, 64}, G[3] = {128, 64, 64}, devs[2] = {0, 1};
    mvn_engine* occupy = nullptr;
    mvn_group* g = nullptr;
    cap_mb(3);
    if (mvn_engine_create(1, E, 0, &occupy) < 0) fails += bad("the engine that occupies device 1");
    mvn_set_pad_mode("no such mode");
    const int rc = mvn_group_create(devs, 2, G, 1, 1, &g);
    const std::string err = mvn_last_error();
    cap_mb(0);
    if (rc == 0 || g || err.rfind("mvn_group_create", 0) != 0 || err.find("device memory exhausted") == std::string::npos)
      fails += bad("a group whose second slab cannot be built");
    else
      std::printf("mvn_group_create: refused\n");
    if (mvn_engine_destroy(occupy) < 0) fails += bad("mvn_engine_destroy");
  }

  // ---- (c)
  {
    int P[3] = {12, 10, 16};
    std::vector<double> per((size_t)mvn_kernel_kind_count(), -1.);
    if (mvn_fft3_profile(0, P, 0, 2, ms, per.data()) < 0 || !std::isfinite(ms[0]))
      fails += bad("mvn_fft3_profile");
    else
      std::printf("mvn_fft3_profile: ran\n");
  }

  // ---- (d)
  {
    int G[3] = {24, 8, 16}, KG[3] = {5, 3, 3}, devs[2] = {0, 1};
    const size_t gn = (size_t)G[0] * G[1] * G[2];
    std::vector<float> image(gn), weights(gn, 0.4f), psi(gn, 50.f), psf(45, 1.f / 45.f), got(gn, -1.f);
    for (size_t i = 0; i < gn; ++i) image[i] = 10.f + (float)(i % 23);
    view_data v;
    std::memset(&v, 0, sizeof v);
    v.image_ = image.data(), v.weights_ = weights.data(), v.kernel1_ = v.kernel2_ = psf.data();
    v.image_dims_ = v.weights_dims_ = G, v.kernel1_dims_ = v.kernel2_dims_ = KG;
    workspace ws;
    std::memset(&ws, 0, sizeof ws);
    ws.data_ = &v, ws.num_views_ = 1, ws.lambda_ = 0.006, ws.minValue_ = 1e-4f, ws.num_iterations_ = 1;
    mvn_group* g = nullptr;
    if (mvn_group_create(devs, 2, G, KG[0] / 2, 1, &g) < 0 || mvn_group_load(g, psi.data(), ws) < 0 ||
        mvn_group_iterate(g, 1, ws.lambda_, ws.minValue_, nullptr) < 0 || mvn_group_get_psi(g, got.data()) < 0)
      fails += bad("a group of two slabs");
    for (float x : got)
      if (!std::isfinite(x) || x < 0.f) {
        fails += bad("a voxel of the group's psi");
        break;
      }
    if (got == psi) fails += bad("the group's sweep changed nothing");
    if (mvn_group_destroy(g) < 0) fails += bad("mvn_group_destroy");
    if (!fails) std::printf("group: swept\n");
  }

  // ---- (e): shapes and caps of tests/test_emu_scoped.py, under the product's defaults (3 x 3 x 3 kernels are held in
  // the direct form: taps of 16 planes and a second work volume)
  {
    mvn_engine* e = nullptr;
    fails += must_exhaust("mvn_engine_create", 3, [&] { return mvn_engine_create(0, B, 0, &e); });  // psi fits
    if (e) fails += bad("an engine came back from the refused call");
    // the engine of 4 MB is built with no cap; under 9 MB view 0 gets its image, weights and taps, not the second work
    // volume
    if (mvn_engine_create(0, B, 2, &e) < 0) fails += bad("mvn_engine_create");
    fails += must_exhaust("mvn_engine_set_view", 9, [&] {
      int rc = 0;
      for (int v = 0; v < 2 && rc == 0; ++v)
        rc = mvn_engine_set_view(e, v, a.data(), c.data(), kernel.data(), K, kernel.data(), K);
      return rc;
    });
    if (mvn_engine_destroy(e) < 0) fails += bad("mvn_engine_destroy");
    // a call of two views at 64^3, one of them streamed; then the same at B under what that took: the planner refuses
    // it before anything is allocated (no cap reaches an allocation of a streamed call: the planner's figure is
    // exact), and drops the cached engine with its ring
    int S[3] = {64, 64, 64};
    const size_t sn = (size_t)S[0] * S[1] * S[2];
    view_data v[2];
    std::memset(v, 0, sizeof v);
    for (int i = 0; i < 2; ++i) {
      v[i].image_ = a.data() + i * sn, v[i].weights_ = c.data(), v[i].kernel1_ = v[i].kernel2_ = kernel.data();
      v[i].image_dims_ = v[i].weights_dims_ = S, v[i].kernel1_dims_ = v[i].kernel2_dims_ = K;
    }
    workspace ws;
    std::memset(&ws, 0, sizeof ws);
    ws.data_ = v, ws.num_views_ = 2, ws.lambda_ = 0.006, ws.minValue_ = 1e-4f, ws.num_iterations_ = 2;
    std::vector<float> psi(b.begin(), b.begin() + sn);
    if (mvn_set_pad_mode("none") < 0 || mvn_set_memory_mode("stream:1") < 0) fails += bad("the streamed call's modes");
    mvn_set_pad_mode("no such mode");
    inplace_gpu_deconvolve(psi.data(), ws, 0);
    if (std::string(mvn_last_error()).rfind("mvn_set_pad_mode", 0) != 0 || !std::isfinite(psi[0]) || psi[0] == b[0])
      fails += bad("a streamed call");
    for (int i = 0; i < 2; ++i) v[i].image_ = a.data() + i * n, v[i].image_dims_ = v[i].weights_dims_ = B;
    fails += must_exhaust("inplace_gpu_deconvolve", 15, [&] { return inplace_gpu_deconvolve(out.data(), ws, 0), 1; },
                          "memory constraints");
    if (mvn_set_memory_mode(nullptr) < 0 || mvn_set_pad_mode("zero") < 0) fails += bad("the modes' defaults");
    mvn_slab* slab = nullptr;
    fails += must_exhaust("mvn_slab_create", 3, [&] { return mvn_slab_create(0, B, 2, 0, 1, &slab); });  // own_a_ fits
    if (slab) fails += bad("a slab engine came back from the refused call");
  }

  // ---- (f): an engine of 72 x 80 x 64 on device 1 takes all but about 140 KB of a cap of 3 MB (two volumes of 1440
  // KB, a Nyquist plane of 45 KB, its plan's tables).  The last axis of 2 x 2 x 20480 has a twiddle table of 80 KB and
  // two index tables of 40 KB: the first two fit, the third does not, and the plan gives them back.
  {
    int E[3] = {72, 80, 64}, T[3] = {2, 2, 20480};
    mvn_engine* occupy = nullptr;
    cap_mb(3);
    if (mvn_engine_create(1, E, 0, &occupy) < 0) fails += bad("the engine that occupies device 1");
    fails += must_exhaust("mvn_plan_store_add", 3, [&] { return mvn_plan_store_add(1, T); });
    if (mvn_plan_store_has_key(1, T) != 0) fails += bad("the plan that could not be built is in the store");
    if (mvn_engine_destroy(occupy) < 0) fails += bad("mvn_engine_destroy");
  }

  if (mvn_release_cached_engines() < 0 || mvn_plan_store_clear() < 0) fails += bad("the clean-up");
  if (!fails) std::printf("ok\n");
  std::fflush(stdout);  // (LeakSanitizer's report at exit may end the process before the stream is flushed)
  return fails ? 1 : 0;
}
