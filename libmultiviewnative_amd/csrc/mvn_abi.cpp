// mvn_abi.cpp -- extern "C" boundary: the reference ABI (include/multiviewnative.h) and the
// engine ABI (include/mvn_engine_api.h).  Nothing escapes as an exception; failures leave the
// caller's in/out buffers untouched, print one diagnostic to stderr and never terminate the
// host process (SURVEY.md 8b "Errors").
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mvn_engine_api.h"
#include "mvn_engine.hpp"
#include "mvn_fixed_geom.hpp"
#include "mvn_multi.hpp"

using namespace mvn;

struct mvn_engine {
  std::unique_ptr<Engine> impl;
};

struct mvn_slab {
  std::unique_ptr<SlabEngine> impl;
};

struct mvn_group {
  std::unique_ptr<HaloGroup> impl;
};

static thread_local std::string g_last_error;

static bool trace_on() {
  const char* t = std::getenv("MVN_TRACE");
  return t && *t && std::strcmp(t, "0") != 0;
}

template <typename F>
static int guarded(const char* where, F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = std::string(where) + ": " + e.what();
  } catch (...) {
    g_last_error = std::string(where) + ": unknown failure";
  }
  std::fprintf(stderr, "[libmultiviewnative] %s\n", g_last_error.c_str());
  return -1;
}

// one ABI call at a time per device (the reference is not re-entrant, SURVEY.md 8b "Threading")
static std::mutex& device_mutex(int device) {
  static std::mutex table_mu;
  static std::map<int, std::unique_ptr<std::mutex>> table;
  std::lock_guard<std::mutex> lk(table_mu);
  auto& m = table[device];
  if (!m) m.reset(new std::mutex());
  return *m;
}

// One resident engine per device is kept between inplace_gpu_deconvolve calls: Fiji deconvolves
// block after block of the same shape, and allocating / freeing 4V+2 volumes per call costs more
// than uploading them.  A call with another shape, view count or residency plan
// (memory modes, plan_engine) replaces the cached engine.  MVN_ENGINE_CACHE=0 disables the cache;
// mvn_release_cached_engines() empties it.
// The map is process-wide while calls are serialised per DEVICE only (Fiji runs one host thread
// per GPU), so it has its own mutex, held just around find / erase / insert.
static std::mutex& engine_cache_mutex() {
  static std::mutex* m = new std::mutex();
  return *m;
}
static std::map<int, std::unique_ptr<Engine>>& engine_cache() {
  static std::map<int, std::unique_ptr<Engine>>* c = new std::map<int, std::unique_ptr<Engine>>();
  return *c;
}

static bool engine_cache_enabled() {
  const char* e = std::getenv("MVN_ENGINE_CACHE");
  return !(e && std::strcmp(e, "0") == 0);
}

// caller holds device_mutex(dev)
static std::unique_ptr<Engine> pop_cached_engine(int dev) {
  std::lock_guard<std::mutex> lk(engine_cache_mutex());
  auto& c = engine_cache();
  auto it = c.find(dev);
  if (it == c.end()) return nullptr;
  std::unique_ptr<Engine> e = std::move(it->second);
  c.erase(it);
  return e;
}

// ---------------------------------------------------------------------------------------------
// memory mode of inplace_gpu_deconvolve / mvn_deconvolve_submit
//   resident (default)  the check above: every stack on the device, or "memory constraints"
//   auto                Engine::memory_need decides: resident when the exact need fits; otherwise the
//                       fewest views s whose image and weights stay in host memory and cross PCIe into a
//                       ring of device slots for every view update (2 slots where they fit, else 1);
//                       "memory constraints" only when not even s = V with 1 slot fits (the reference's
//                       min-memory interleaved branch, src/gpu_deconvolve_methods.cuh:82-326)
//   stream              every view streamed: the smallest footprint
//   stream:N            exactly N views streamed (clamped to the view count; tests and measurements: the planner
//                       itself never streams one view, which costs as much as none with one ring slot)
// Selected by mvn_set_memory_mode(), else resident.  The planner may use min(free device memory,
// budget), budget = mvn_set_memory_budget() (ignored in resident mode).  Results are those of the resident call, bit for bit: same kernels, same order.
// ---------------------------------------------------------------------------------------------
enum { MVN_MEM_EXACT = -2, MVN_MEM_UNSET = -1, MVN_MEM_RESIDENT = 0, MVN_MEM_AUTO = 1, MVN_MEM_STREAM = 2 };
// a mode is stored as one int: MVN_MEM_STREAM + 1 + N for stream:N
static std::atomic<int> g_mem_mode{MVN_MEM_UNSET};
static std::atomic<long long> g_mem_budget{-1};

static int parse_memory_mode(const char* m) {
  if (!m || !*m) return MVN_MEM_UNSET;
  if (std::strcmp(m, "resident") == 0) return MVN_MEM_RESIDENT;
  if (std::strcmp(m, "auto") == 0) return MVN_MEM_AUTO;
  if (std::strcmp(m, "stream") == 0) return MVN_MEM_STREAM;
  if (std::strncmp(m, "stream:", 7) == 0 && m[7]) {
    char* end = nullptr;
    const long n = std::strtol(m + 7, &end, 10);
    if (*end == 0 && n >= 0 && n <= 65535) return MVN_MEM_STREAM + 1 + (int)n;
  }
  throw std::invalid_argument(std::string("unknown memory mode '") + m + "' (resident | auto | stream | stream:N)");
}

static int current_memory_mode() {
  const int m = g_mem_mode.load();
  return m == MVN_MEM_UNSET ? MVN_MEM_RESIDENT : m;
}

// the planner's cap below the free memory; 0 = none
static size_t current_memory_budget() {
  const long long b = g_mem_budget.load();
  return b > 0 ? (size_t)b : 0;
}

// ---- the switches of the loop (mvn_set_convergence, mvn_set_acceleration, mvn_set_regularization, mvn_set_background,
// mvn_set_likelihood): one process-wide value, which a call copies at its start and hands down ----
static std::mutex g_loop_mu;
static LoopOptions g_loop;
static LoopOptions current_loop() {
  std::lock_guard<std::mutex> lk(g_loop_mu);
  return g_loop;
}
// a setter: the edited value replaces the process-wide one if it is valid
template <typename F>
static void edit_loop(F&& edit) {
  std::lock_guard<std::mutex> lk(g_loop_mu);
  LoopOptions o = g_loop;
  edit(o);
  o.validate(LoopOptions::kAbi);
  g_loop = std::move(o);
}
// the last deconvolution this thread completed (inplace_gpu_deconvolve, or the wait of a ticket)
static thread_local LoopResult t_last_conv;
// the read-out of a record: min(rows, capacity) rows of `width` doubles; returns the rows there are
static int copy_rows(const std::vector<double>& from, int width, double* to, int capacity) {
  const int rows = (int)(from.size() / (size_t)width);
  const size_t n = (size_t)width * (size_t)std::min(rows, capacity);
  if (n) std::memcpy(to, from.data(), n * sizeof(double));
  return rows;
}

// ---- image storage (mvn_set_image_storage): captured at the start of a described call ----
static std::atomic<int> g_image_storage{0};
// per view: a described call in storage mode `mode` wants this image kept as uint16
static bool keeps_u16(const StackRef& image, int mode) { return mode == 1 && image.u16 && !image.broadcast(); }

// ---- psi start (mvn_set_psi_start): captured at the start of mvn_deconvolve_resampled ----
static std::mutex g_psi_start_mu;
static int g_psi_start_mode = 0;
static float g_psi_start_fill = 0.f;

static MemoryQuery memory_query(const shape_t& ext, const workspace& input, const LoopOptions& loop,
                                size_t embed_floats, const std::vector<char>& keep_u16) {
  MemoryQuery q;
  q.image_u16 = keep_u16;
  q.ext = ext;
  q.embed_floats = embed_floats;
  q.loop = loop;
  q.iterations = std::max(input.num_iterations_, 1);
  q.lambda = input.lambda_;
  q.kernels = call_kernels(input);
  return q;
}

// The PSF form rule (mvn_engine.hpp) for a volume of extents ext on device dev, before any engine exists: the
// switches in force now, and the plan an engine of these extents will run on - the one in the plan store where it
// has one (built with the MVN_NO_FIXED of its time), else one built now.  dev < 0: no stored plan is looked at.
static FormRule call_rule(const shape_t& ext, int dev) {
  const FormSwitches sw = FormSwitches::from_env();
  const std::shared_ptr<Plan3D> stored = dev >= 0 ? PlanStore::get().find(dev, ext) : nullptr;
  return FormRule(Layout(ext[0], ext[1], ext[2]), sw, stored ? stored->fixed : sw.fixed);
}

// A cached engine serves a call of its extents and view count whose PSF form rule it shares (switches, and the kernel
// family of its plan): then it holds the call's kernels in the forms call_extents and memory_need assumed.  (The
// switches are read when an engine is created; tests change them within a process.)
static bool reusable(const Engine& e, const shape_t& ext, int V) {
  const Layout& L = e.layout();
  if (!engine_cache_enabled() || L.d0 != ext[0] || L.d1 != ext[1] || L.d2 != ext[2] || e.num_views() != V) return false;
  const FormRule mine = e.form_rule(), call = call_rule(ext, e.device());
  return mine.sw == call.sw && mine.plan_fixed == call.plan_fixed;
}

// caller holds device_mutex(dev); the auto / stream modes of take_engine
static std::unique_ptr<Engine> plan_engine(int key, int dev, const shape_t& ext, size_t embed_floats,
                                           const workspace& input, const LoopOptions& loop, int mode,
                                           const std::vector<char>& keep_u16, bool use_budget = true) {
  const int V = input.num_views_;
  MemoryQuery q = memory_query(ext, input, loop, embed_floats, keep_u16);
  const FormRule rule = call_rule(ext, dev);
  auto need = [&](int s, int ring) {
    q.streamed = s;
    q.ring = ring;
    return Engine::memory_need(q, rule);
  };
  std::unique_ptr<Engine> cached = pop_cached_engine(key);
  if (cached && !reusable(*cached, ext, V))
    cached.reset();  // wrong shape or rule: free its memory before the free memory is read
  size_t free_b = 0, total_b = 0;
  be::device_mem_info(&free_b, &total_b);
  size_t avail = free_b;
  if (cached) {  // what re-planning would free: the cached engine as it stands, with the scratch it holds
    MemoryQuery held = q;
    held.embed_floats = cached->scratch_floats();
    held.streamed = cached->streamed_count();
    held.ring = cached->ring_size();
    held.image_u16 = cached->image_types();
    avail += Engine::memory_need(held, rule);
  }
  const size_t budget = use_budget ? current_memory_budget() : 0;
  if (budget) avail = std::min(avail, budget);
  int s = -1, ring = 0;
  const int first = mode == MVN_MEM_AUTO ? 0 : (mode == MVN_MEM_STREAM ? V : std::min(V, mode - MVN_MEM_STREAM - 1));
  const int last = mode == MVN_MEM_AUTO ? V : first;
  for (int c = first; c <= last && s < 0; ++c) {
    if (c == 0) {
      if (need(0, 0) <= avail) s = 0;
      continue;
    }
    for (int r = 2; r >= 1 && s < 0; --r)
      if (need(c, r) <= avail) {
        s = c;
        ring = r;
      }
  }
  if (trace_on())
    std::printf("[lmvn::inplace_gpu_deconvolve] memory plan: %.1f MB available (free %.1f MB, budget %.1f MB): %s\n",
                avail / 1048576.0, free_b / 1048576.0, budget / 1048576.0,
                s < 0 ? "does not fit"
                      : (std::to_string(s) + " of " + std::to_string(V) + " views streamed, ring of " +
                         std::to_string(ring) + ", " + std::to_string(need(s, ring) >> 20) + " MB")
                            .c_str());
  if (s < 0) throw std::runtime_error("FFT: Unable to run on GPU due to memory constraints");
  if (cached && cached->streamed_count() == s && cached->ring_size() == ring) return cached;
  cached.reset();  // another residency plan: free it before the new engine allocates
  std::unique_ptr<Engine> e(new Engine(dev, ext, V));
  e->set_residency(Engine::spread_views(V, s), ring);
  return e;
}

// caller holds device_mutex(dev).  The memory heuristic of src/multiviewnative.cu:94-119, restated
// for the resident layout (4 volumes per view -- view, weights, two spectra -- + psi + work + the
// spectrum scratch of the PSF preparation, + the host-shaped embedding scratch of the padded
// policies, + 2 % slack), is applied only when the call has to allocate: a cached engine of the same
// shape is re-used as it is (its memory is what the check would ask for, but for uint16 image slots that have to
// grow: see below), and a stale one of another
// shape is freed BEFORE the free memory is read -- so that "does not fit" is said here, before any
// work is queued, not by a failing hipMalloc on the staging thread.
static std::unique_ptr<Engine> take_engine(int key, int dev, const shape_t& ext, int V, size_t embed_floats,
                                           const workspace& input, const LoopOptions& loop, int mem_mode,
                                           const std::vector<char>& keep_u16) {
  // (MVN_MEM_EXACT: resident, priced by the exact model - a described call with stacks in device memory)
  if (mem_mode == MVN_MEM_EXACT)
    return plan_engine(key, dev, ext, embed_floats, input, loop, MVN_MEM_STREAM + 1, keep_u16, false);
  if (mem_mode != MVN_MEM_RESIDENT) return plan_engine(key, dev, ext, embed_floats, input, loop, mem_mode, keep_u16);
  std::unique_ptr<Engine> e = pop_cached_engine(key);  // key = device + lane * kLaneStride
  Layout L(ext[0], ext[1], ext[2]);
  if (e && reusable(*e, ext, V) && e->streamed_count() == 0) {
    // (image storage mode 1: a slot that holds a uint16 image grows by half a volume when this call brings it a
    //  float32 one - the one allocation a re-used engine still makes; it has to fit, or the engine goes and the
    //  check below speaks)
    const std::vector<char> held = e->image_types();
    size_t grow = 0;
    for (int v = 0; v < V; ++v)
      if (held[(size_t)v] && !(v < (int)keep_u16.size() && keep_u16[(size_t)v])) grow += L.real_floats() * 2;
    size_t free_b = 0, total_b = 0;
    if (grow) be::device_mem_info(&free_b, &total_b);
    if (grow == 0 || grow < free_b) return e;
  }
  e.reset();  // wrong shape or rule: free its memory before the new engine allocates
  const double need = ((4.0 * V + 3.0) * (double)L.B() + 4.0 * (double)embed_floats) * 1.02;
  size_t free_b = 0, total_b = 0;
  be::device_mem_info(&free_b, &total_b);
  if (trace_on())
    std::printf("[lmvn::inplace_gpu_deconvolve] FFT: %.1f MB (all-on-device), available on GPU: %.1f MB ... %s\n",
                need / 1048576.0, free_b / 1048576.0, need < free_b ? "all on device!" : "does not fit");
  if (need >= (double)free_b)
    throw std::runtime_error("FFT: Unable to run on GPU due to memory constraints");
  return std::unique_ptr<Engine>(new Engine(dev, ext, V));
}

static void give_back_engine(int dev, std::unique_ptr<Engine> e) {
  if (!engine_cache_enabled()) return;
  std::unique_ptr<Engine> old;  // destroyed outside the lock
  {
    std::lock_guard<std::mutex> lk(engine_cache_mutex());
    auto& slot = engine_cache()[dev];
    old = std::move(slot);
    slot = std::move(e);
  }
}

// ---------------------------------------------------------------------------------------------
// padding policy of inplace_gpu_deconvolve
//   MVN_PAD_ZERO (default)  the reference GPU entry's zero_padd (src/multiviewnative.cu:26-27,128;
//                           inc/padd_utils.h:121-138; src/gpu_deconvolve_methods.cuh:366-449,
//                           537-549): every stack is embedded at offset (kernel-1)/2 in a zero
//                           volume of extent >= image + kernel - 1 (maxima over views and both
//                           kernels), the loop runs cyclically on that volume, psi is cropped back
//                           on exit.  The padded extents grow to FFT-friendly sizes (see
//                           good_extent); the quotient is guarded (view == 0 -> 0) because the
//                           extra zeros lie beyond the PSF's reach.
//   MVN_PAD_ZERO_EXACT      the same with exactly image + kernel - 1 (the reference's extents; a
//                           prime factor such as 542 = 2 * 271 then goes the chirp-z route)
//   MVN_PAD_NONE            the reference CPU path's no_padd: cyclic on exactly image_dims_
//                           (inc/cpu_convolve.h:22-26) -- the parity target of the oracle tests
//   MVN_PAD_REFLECT         MVN_PAD_ZERO's volume, offset and guard, but the margins around image,
//                           weights and psi hold the stack's mirror image instead of zeros
//                           (whole-sample symmetric extension, mvn_reflect.hpp): the forward model
//                           no longer sees a black specimen just outside the stack.  One device.
// Selected by mvn_set_pad_mode() (a JVM host cannot easily change its environment per call),
// else by the environment variable MVN_PAD_MODE = zero | zero_exact | none | reflect (MVN_PAD_GOOD_SIZE=0
// turns "zero" into "zero_exact"), else MVN_PAD_ZERO.
// ---------------------------------------------------------------------------------------------
enum { MVN_PAD_UNSET = -1, MVN_PAD_ZERO = 0, MVN_PAD_ZERO_EXACT = 1, MVN_PAD_NONE = 2, MVN_PAD_REFLECT = 3 };
// the policies that grow the padded extents to FFT-friendly sizes and guard the quotient
static bool pad_grows(int pad_mode) { return pad_mode == MVN_PAD_ZERO || pad_mode == MVN_PAD_REFLECT; }
static std::atomic<int> g_pad_mode{MVN_PAD_UNSET};

static int parse_pad_mode(const char* m) {
  if (!m || !*m) return MVN_PAD_UNSET;
  if (std::strcmp(m, "zero") == 0) return MVN_PAD_ZERO;
  if (std::strcmp(m, "zero_exact") == 0) return MVN_PAD_ZERO_EXACT;
  if (std::strcmp(m, "none") == 0) return MVN_PAD_NONE;
  if (std::strcmp(m, "reflect") == 0) return MVN_PAD_REFLECT;
  throw std::invalid_argument(std::string("unknown padding mode '") + m + "' (zero | zero_exact | none | reflect)");
}

static int current_pad_mode() {
  int m = g_pad_mode.load();
  if (m == MVN_PAD_UNSET) m = parse_pad_mode(std::getenv("MVN_PAD_MODE"));
  if (m == MVN_PAD_UNSET) m = MVN_PAD_ZERO;
  if (m == MVN_PAD_ZERO) {
    const char* gs = std::getenv("MVN_PAD_GOOD_SIZE");
    if (gs && std::strcmp(gs, "0") == 0) m = MVN_PAD_ZERO_EXACT;
  }
  return m;
}

// Padded extent >= n for one axis.  Any 2^a 3^b 5^c 7^d length avoids the chirp-z route; the
// lengths served by the fixed-length kernels (mvn_fixed_geom.hpp) run ~1.45x faster per element
// than the run-time-radix ones, so a slightly longer fixed length can be the cheaper transform
// (542 -> 576 rather than 560; 270 -> 320).  Candidates up to 1.3 n are priced by
// length x (fixed ? 1 : 1.45).  The last axis (d2 = 2H) must be even to have fixed kernels.
static int good_extent(int n, bool last_axis) {
  int best = 0;
  double best_cost = 0;
  for (int c = n; c <= n + n * 3 / 10 + 8; ++c) {
    int m = c;
    for (int p : {2, 3, 5, 7})
      while (m % p == 0) m /= p;
    if (m != 1) continue;
    int T = 0, threads = 0;
    size_t lds = 0;
    const bool fixed = last_axis ? (c % 2 == 0 && fixed_rows_geom(c / 2, &T, &threads, &lds))
                                 : fixed_strided_geom(c, &T, &threads, &lds);
    const double cost = (double)c * (fixed ? 1.0 : 1.45);
    if (!best || cost < best_cost) {
      best = c;
      best_cost = cost;
    }
  }
  return best ? best : next_smooth(n);
}

static int pick_device(int device) {
  if (device < 0) device = selectDeviceWithHighestComputeCapability();
  const int n = be::device_count();
  if (device < 0 || device >= n)
    throw std::runtime_error("no usable GPU (requested device " + std::to_string(device) + ", " +
                             std::to_string(n) + " present)");
  return device;
}

static shape_t to_shape(const int* d) {
  shape_t s = {{d[0], d[1], d[2]}};
  return s;
}

// ---- what the test and bench utilities of the ABI share ------------------------------------------
// milliseconds per call of `body`, which enqueues on `s`: one call to warm up, then `reps` calls between two events
template <typename F>
static float time_on_stream(be::stream_t s, int reps, F&& body) {
  const be::Event a = be::Event::timing(), b = be::Event::timing();
  body();
  be::event_record(a.get(), s);
  for (int i = 0; i < reps; ++i) body();
  be::event_record(b.get(), s);
  be::event_sync(b.get());
  return be::event_elapsed_ms(a.get(), b.get()) / (float)reps;
}

// non-trivial contents for a timed volume (zeros flatter the clock: guide 5.4 rule 25): an LCG's values in [-0.5, 0.5)
static std::vector<float> lcg_fill(size_t n) {
  std::vector<float> host(n);
  unsigned x = 12345u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    host[i] = (float)(x >> 8) * (1.0f / 16777216.0f) - 0.5f;
  }
  return host;
}

// the epilogue of a plain convolution: the result is stored, unscaled
static EpilogueParams store_epilogue() {
  EpilogueParams e;
  std::memset(&e, 0, sizeof(e));
  e.mode = MVN_EPI_STORE;
  e.scale = 1.f;
  return e;
}

// On the device a spectrum is kept in POSITION order along every axis (digit-reversed, exactly as
// the decimation-in-frequency passes leave it; the PSF spectra are stored the same way, so the
// RL loop never permutes anything).  The host-buffer utilities translate to / from the
// natural FFTW/cuFFT bin order with this pair: bin (k0,k1,k2) lives at (inv0[k0], inv1[k1], inv2[k2]).
// f(index in the main spectrum, natural index) for every bin, nyq(row of the Nyquist plane, natural index) (even d2)
template <typename F, typename N>
static void for_each_bin(const Plan3D& plan, F&& f, N&& nyq) {
  const Layout& L = plan.L;
  const std::vector<int>&i0 = plan.ax0.host.inv, &i1 = plan.ax1.host.inv;
  const std::vector<int>& i2 = plan.ax2.host.inv;  // length L.h; used for even d2 only
  const size_t nc = (size_t)(L.d2 / 2 + 1);
  for (int k0 = 0; k0 < L.d0; ++k0)
    for (int k1 = 0; k1 < L.d1; ++k1) {
      const size_t row = (size_t)i0[k0] * L.d1 + (size_t)i1[k1], nat = ((size_t)k0 * L.d1 + k1) * nc;
      for (int k2 = 0; k2 < L.C; ++k2) f(row * L.C + (L.even ? i2[k2] : k2), nat + (size_t)k2);
      if (L.even) nyq(row, nat + (size_t)L.C);
    }
}

static void position_to_natural(const Plan3D& plan, const std::vector<cfloat>& main_h,
                                const std::vector<cfloat>& nyq_h, cfloat* out) {
  for_each_bin(
      plan, [&](size_t pos, size_t nat) { out[nat] = main_h[pos]; },
      [&](size_t row, size_t nat) { out[nat] = nyq_h[row]; });
}

static void natural_to_position(const Plan3D& plan, const cfloat* in, std::vector<cfloat>& main_h,
                                std::vector<cfloat>& nyq_h) {
  for_each_bin(
      plan, [&](size_t pos, size_t nat) { main_h[pos] = in[nat]; },
      [&](size_t row, size_t nat) { nyq_h[row] = in[nat]; });
}

// ---- derived kernels (mvn_psf.hpp; the arithmetic is stated at mvn_derive_kernels in include/mvn_engine_api.h) --------
namespace {

// B = A^-1 of the linear part of a row-major 3 x 4 matrix, in double, as adjugate over determinant
void psf_inverse(const double* M, const std::string& what, double B[9]) {
  double a[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      a[i][j] = M[4 * i + j];
      if (!std::isfinite(a[i][j])) throw std::invalid_argument(what + ": non-finite linear part");
    }
  double adj[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
      adj[i][j] = a[r0][c0] * a[r1][c1] - a[r0][c1] * a[r1][c0];  // cofactor (j, i): cyclic indices carry the sign
    }
  const double det = a[0][0] * adj[0][0] + a[0][1] * adj[1][0] + a[0][2] * adj[2][0];
  if (!std::isfinite(det) || det == 0.) throw std::invalid_argument(what + ": singular linear part");
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      B[3 * i + j] = adj[i][j] / det;
      if (!std::isfinite(B[3 * i + j])) throw std::invalid_argument(what + ": singular linear part");
    }
}

void psf_check_raw_dims(int V, const int* raw_dims) {
  if (V < 1) throw std::invalid_argument("num_views must be >= 1");
  if (!raw_dims) throw std::invalid_argument("null raw_dims");
  for (int i = 0; i < 3 * V; ++i)
    if (raw_dims[i] < 1 || !(raw_dims[i] & 1))
      throw std::invalid_argument("raw PSF " + std::to_string(i / 3) + ": extents must be odd and >= 1");
}

// K of mvn_psf_extents
void psf_extents(int V, const int* raw_dims, const mvn_view_geometry* geom, int K[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  psf_check_raw_dims(V, raw_dims);
  int best[3] = {0, 0, 0};
  for (int v = 0; v < V; ++v) {
    const int* r = raw_dims + 3 * v;
    if (!geom) {
      for (int k = 0; k < 3; ++k) best[k] = std::max(best[k], r[k]);
      continue;
    }
    double B[9];
    psf_inverse(geom[v].matrix, "geom " + std::to_string(v), B);
    const double cr[3] = {(double)((r[0] - 1) / 2), (double)((r[1] - 1) / 2), (double)((r[2] - 1) / 2)};
    for (int k = 0; k < 3; ++k) {
      const double p0 = std::fabs(B[3 * k]) * cr[0], p1 = std::fabs(B[3 * k + 1]) * cr[1], p2 = std::fabs(B[3 * k + 2]) * cr[2];
      const double s01 = p0 + p1;
      const double s = s01 + p2;
      const double h = std::ceil(s - 1e-6);
      if (!(h <= (double)(MVN_PSF_MAX / 2)))
        throw std::invalid_argument("the transformed PSF of view " + std::to_string(v) + " exceeds " +
                                    std::to_string(MVN_PSF_MAX) + " voxels along an axis");
      best[k] = std::max(best[k], 2 * (int)(h > 0. ? h : 0.) + 1);
    }
  }
  for (int k = 0; k < 3; ++k) {
    if (best[k] > MVN_PSF_MAX)
      throw std::invalid_argument("kernel extents above " + std::to_string(MVN_PSF_MAX));
    K[k] = best[k];
  }
}

// a derivation, everything checked that the host can check
struct PsfRequest {
  int V = 0, type = 0;
  int K[3] = {1, 1, 1};
  bool has_geom = false;
  std::vector<int> r;             // 3 per view
  std::vector<double> M;          // 12 per view: [A | t] (has_geom)
  std::vector<const float*> raw;  // host memory
  size_t n() const { return (size_t)K[0] * (size_t)K[1] * (size_t)K[2]; }
  size_t nA() const { return (size_t)(2 * K[0] - 1) * (size_t)(2 * K[1] - 1) * (size_t)(2 * K[2] - 1); }
  bool correlates() const { return V > 1 && (type == PSF_EFFICIENT_BAYESIAN || type == PSF_OPTIMIZATION_I); }
};

void psf_check_type(int type) {
  if (type < PSF_INDEPENDENT || type > PSF_OPTIMIZATION_II)
    throw std::invalid_argument("kernel type must be 0 (independent), 1 (efficient Bayesian), 2 (optimization I) or "
                                "3 (optimization II)");
}

PsfRequest psf_request(int V, const float* const* raw_psf, const int* raw_dims, const mvn_view_geometry* geom, int type,
                       const int* out_dims) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  PsfRequest q;
  psf_check_raw_dims(V, raw_dims);
  psf_check_type(type);
  if (!raw_psf) throw std::invalid_argument("null raw_psf");
  q.V = V, q.type = type, q.has_geom = geom != nullptr;
  q.r.assign(raw_dims, raw_dims + 3 * V);
  if (out_dims) {
    for (int k = 0; k < 3; ++k) {
      if (out_dims[k] < 1 || out_dims[k] > MVN_PSF_MAX || !(out_dims[k] & 1))
        throw std::invalid_argument("out_dims must be odd and between 1 and " + std::to_string(MVN_PSF_MAX));
      q.K[k] = out_dims[k];
    }
    if (geom)
      for (int v = 0; v < V; ++v) {
        double B[9];
        psf_inverse(geom[v].matrix, "geom " + std::to_string(v), B);
      }
  } else {
    psf_extents(V, raw_dims, geom, q.K);
  }
  for (int v = 0; v < V; ++v) {
    const float* p = raw_psf[v];
    if (!p) throw std::invalid_argument("raw PSF " + std::to_string(v) + ": null pointer");
    const int* r = raw_dims + 3 * v;
    const size_t count = (size_t)r[0] * (size_t)r[1] * (size_t)r[2];
    for (size_t i = 0; i < count; ++i)
      if (!std::isfinite(p[i])) throw std::invalid_argument("raw PSF " + std::to_string(v) + ": non-finite value");
    q.raw.push_back(p);
    if (!geom) continue;
    // t_k = cr_k - ((A[k][0] h_0 + A[k][1] h_1) + A[k][2] h_2): the centre of K lands on the centre of the raw PSF
    const double* A = geom[v].matrix;
    for (int k = 0; k < 3; ++k) {
      const double h0 = (double)((q.K[0] - 1) / 2), h1 = (double)((q.K[1] - 1) / 2), h2 = (double)((q.K[2] - 1) / 2);
      const double a = A[4 * k] * h0;
      const double b = A[4 * k + 1] * h1;
      const double ab = a + b;
      const double c = A[4 * k + 2] * h2;
      const double abc = ab + c;
      const double t = (double)((r[k] - 1) / 2) - abc;
      for (int j = 0; j < 3; ++j) q.M.push_back(A[4 * k + j]);
      q.M.push_back(t);
    }
  }
  return q;
}

// the device side of one derivation: buffers, job tables, and the launches in stream order
class PsfDerivation {
 public:
  PsfDerivation(const PsfRequest& q, be::stream_t s) : q_(q), L_(q.K[0], q.K[1], q.K[2]), n_(q.n()), nA_(q.nA()) {
    const size_t V = (size_t)q.V;
    size_t raw_floats = 0;
    for (size_t v = 0; v < V; ++v) {
      raw_off_.push_back(raw_floats);
      raw_floats += (size_t)q.r[3 * v] * (size_t)q.r[3 * v + 1] * (size_t)q.r[3 * v + 2];
    }
    raw_ = be::DeviceBuffer<float>(raw_floats * sizeof(float));
    if (q.has_geom) rs_ = be::DeviceBuffer<float>(L_.real_floats() * sizeof(float));
    k1_ = be::DeviceBuffer<float>(V * n_ * sizeof(float));
    k2_ = be::DeviceBuffer<float>(V * n_ * sizeof(float));
    partial_ = be::DeviceBuffer<double>(V * MVN_PSF_WG * sizeof(double));
    sums_ = be::DeviceBuffer<double>(2 * V * sizeof(double));
    for (size_t v = 0; v < V; ++v)
      be::h2d(raw_.get() + raw_off_[v], q.raw[v],
              (size_t)q.r[3 * v] * (size_t)q.r[3 * v + 1] * (size_t)q.r[3 * v + 2] * sizeof(float), s);
    if (!q.correlates()) return;
    const int* K = q.K;
    const int K2[3] = {2 * K[0] - 1, 2 * K[1] - 1, 2 * K[2] - 1};
    c_ = be::DeviceBuffer<float>(V * (V - 1) * n_ * sizeof(float));
    std::vector<PsfJob> ja, jc;
    if (q.type == PSF_EFFICIENT_BAYESIAN) {
      a_ = be::DeviceBuffer<float>(V * nA_ * sizeof(float));
      for (size_t w = 0; w < V; ++w)  // A_w = corr(flip(P_w), flip(P_w)): k2_ holds the flipped kernels then
        ja.push_back(job(k2_.get() + w * n_, K, k2_.get() + w * n_, K, a_.get() + w * nA_, K2));
    }
    for (size_t v = 0; v < V; ++v)
      for (size_t w = 0; w < V; ++w) {
        if (w == v) continue;
        float* out = c_.get() + (v * (V - 1) + (w < v ? w : w - 1)) * n_;
        if (q.type == PSF_EFFICIENT_BAYESIAN)
          jc.push_back(job(k1_.get() + v * n_, K, a_.get() + w * nA_, K2, out, K));
        else
          jc.push_back(job(k1_.get() + v * n_, K, k1_.get() + w * n_, K, out, K));
      }
    jobs_ = be::DeviceBuffer<PsfJob>((ja.size() + jc.size()) * sizeof(PsfJob));
    if (!ja.empty()) be::h2d(jobs_.get(), ja.data(), ja.size() * sizeof(PsfJob), s);
    be::h2d(jobs_.get() + ja.size(), jc.data(), jc.size() * sizeof(PsfJob), s);
    be::stream_sync(s);  // (the tables are locals)
    n_ja_ = (int)ja.size(), n_jc_ = (int)jc.size();
  }

  // the correlation launches alone (the buffers hold what the passes before them left)
  void correlations(be::stream_t s) const {
    if (!q_.correlates()) return;
    PsfCorrParams p;
    if (n_ja_) {
      p.jobs = jobs_.get(), p.njobs = n_ja_, p.blocks_per_job = (int)mvn_psf_blocks((long)nA_);
      be::launch_psf_correlate(p, s);
    }
    p.jobs = jobs_.get() + n_ja_, p.njobs = n_jc_, p.blocks_per_job = (int)mvn_psf_blocks((long)n_);
    be::launch_psf_correlate(p, s);
  }

  // every launch of the derivation
  void enqueue(be::stream_t s) const {
    const int V = q_.V;
    const int* K = q_.K;
    const long krow = K[2], kplane = (long)K[1] * K[2];
    if (!q_.has_geom) be::dzero(k1_.get(), (size_t)V * n_ * sizeof(float), s);
    for (int v = 0; v < V; ++v) {
      const int* r = &q_.r[3 * (size_t)v];
      const float* raw = raw_.get() + raw_off_[(size_t)v];
      float* dst = k1_.get() + (size_t)v * n_;
      if (q_.has_geom) {  // step 1: the resample pass on a volume of extents K, then its rows without their padding
        ResampleParams p;
        std::memset(&p, 0, sizeof(p));
        p.image = rs_.get(), p.weights = nullptr, p.RP = L_.RP, p.D0 = L_.d0, p.D1 = L_.d1;
        p.n0 = L_.d0, p.n1 = L_.d1, p.n2 = L_.d2;
        p.src = raw, p.s0 = (long long)r[1] * r[2], p.s1 = r[2], p.s2 = 1;
        for (int k = 0; k < 3; ++k) p.g.m[k] = r[k];
        for (int i = 0; i < 12; ++i) p.g.M[i] = q_.M[12 * (size_t)v + (size_t)i];
        be::launch_resample(p, false, s);
        be::launch_copy3d(dst, krow, kplane, rs_.get(), L_.RP, (long)L_.d1 * L_.RP, K[2], K[1], K[0], s);
      } else {  // the centred copy: per axis the whole raw PSF, or its central K elements
        int len[3];
        long so = 0, d_o = 0;
        const long sst[3] = {(long)r[1] * r[2], r[2], 1}, dst_st[3] = {kplane, krow, 1};
        for (int k = 0; k < 3; ++k) {
          const int cr = (r[k] - 1) / 2, h = (K[k] - 1) / 2;
          len[k] = std::min(r[k], K[k]);
          if (K[k] >= r[k])
            d_o += (long)(h - cr) * dst_st[k];
          else
            so += (long)(cr - h) * sst[k];
        }
        be::launch_copy3d(dst + d_o, krow, kplane, raw + so, sst[1], sst[0], len[2], len[1], len[0], s);
      }
    }
    PsfNormParams nm;  // step 2
    nm.src = k1_.get(), nm.dst = k1_.get(), nm.partial = partial_.get(), nm.sums = sums_.get(), nm.n = (long)n_, nm.count = V;
    be::launch_psf_normalize(nm, s);
    PsfPointParams pt;  // step 3
    pt.P = k1_.get(), pt.C = c_.get(), pt.T = k2_.get(), pt.n = (long)n_, pt.V = V, pt.type = PSF_INDEPENDENT;
    if (q_.correlates()) {
      if (q_.type == PSF_EFFICIENT_BAYESIAN) be::launch_psf_pointwise(pt, s);  // the flipped kernels the A_w are made of
      correlations(s);
    }
    pt.type = q_.type;
    be::launch_psf_pointwise(pt, s);
    if (q_.type == PSF_INDEPENDENT) return;
    nm.src = k2_.get(), nm.dst = k2_.get(), nm.sums = sums_.get() + V;
    be::launch_psf_normalize(nm, s);
  }

  // the sums checked, then the kernels into host memory (either may be null); blocks
  void download(std::vector<std::vector<float>>* k1, std::vector<std::vector<float>>* k2, be::stream_t s) const {
    const size_t V = (size_t)q_.V;
    std::vector<double> sums(2 * V, 1.0);
    be::d2h(sums.data(), sums_.get(), (q_.type == PSF_INDEPENDENT ? V : 2 * V) * sizeof(double), s);
    be::stream_sync(s);
    for (size_t i = 0; i < 2 * V; ++i)
      if (!std::isfinite(sums[i]) || !(sums[i] > 0.))
        throw std::invalid_argument(std::string("a kernel without mass: ") + (i < V ? "kernel1" : "kernel2") +
                                    " of view " + std::to_string(i % V) + " sums to " + std::to_string(sums[i]));
    for (size_t v = 0; v < V; ++v) {
      if (k1) be::d2h((*k1)[v].data(), k1_.get() + v * n_, n_ * sizeof(float), s);
      if (k2) be::d2h((*k2)[v].data(), k2_.get() + v * n_, n_ * sizeof(float), s);
    }
    be::stream_sync(s);
  }

 private:
  static PsfJob job(const float* a, const int* ea, const float* b, const int* eb, float* out, const int* eo) {
    PsfJob j;
    std::memset(&j, 0, sizeof(j));
    j.a = a, j.b = b, j.out = out;
    for (int k = 0; k < 3; ++k) j.ea[k] = ea[k], j.eb[k] = eb[k], j.eo[k] = eo[k];
    mvn_psf_job_check(j);
    return j;
  }

  const PsfRequest& q_;
  const Layout L_;
  const size_t n_, nA_;
  std::vector<size_t> raw_off_;
  be::DeviceBuffer<float> raw_, rs_, k1_, k2_, c_, a_;
  be::DeviceBuffer<double> partial_, sums_;
  be::DeviceBuffer<PsfJob> jobs_;
  int n_ja_ = 0, n_jc_ = 0;
};

// what a derivation leaves: the kernels of every view, in host memory
struct PsfKernels {
  int K[3];
  std::vector<std::vector<float>> k1, k2;
};

// the derivation cache: ONE entry, the last derivation of the process
struct PsfCacheEntry {
  int type = -1, V = 0;
  bool has_geom = false;
  std::vector<int> r;
  std::vector<double> A;  // 9 per view
  std::vector<std::vector<float>> raw;
  std::shared_ptr<const PsfKernels> out;
};
std::mutex g_psf_cache_mu;
PsfCacheEntry g_psf_cache;
std::atomic<long long> g_psf_computed{0}, g_psf_reused{0};

std::vector<double> psf_linear_parts(const PsfRequest& q) {
  std::vector<double> A;
  for (size_t v = 0; q.has_geom && v < (size_t)q.V; ++v)
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) A.push_back(q.M[12 * v + 4 * (size_t)k + (size_t)j]);
  return A;
}

bool psf_cache_hit(const PsfCacheEntry& e, const PsfRequest& q, const std::vector<double>& A) {
  if (!e.out || e.type != q.type || e.V != q.V || e.has_geom != q.has_geom || e.r != q.r) return false;
  if (std::memcmp(e.out->K, q.K, sizeof(q.K)) != 0) return false;
  if (A.size() != e.A.size() || (!A.empty() && std::memcmp(A.data(), e.A.data(), A.size() * sizeof(double)) != 0)) return false;
  for (size_t v = 0; v < (size_t)q.V; ++v)
    if (std::memcmp(e.raw[v].data(), q.raw[v], e.raw[v].size() * sizeof(float)) != 0) return false;
  return true;
}

// the kernels of a request: from the cache, or derived on `dev` (>= 0) and left there
std::shared_ptr<const PsfKernels> psf_derive(const PsfRequest& q, int dev) {
  std::lock_guard<std::mutex> cache_lk(g_psf_cache_mu);
  const std::vector<double> A = psf_linear_parts(q);
  if (psf_cache_hit(g_psf_cache, q, A)) {
    ++g_psf_reused;
    return g_psf_cache.out;
  }
  auto out = std::make_shared<PsfKernels>();
  std::memcpy(out->K, q.K, sizeof(q.K));
  out->k1.assign((size_t)q.V, std::vector<float>(q.n()));
  out->k2.assign((size_t)q.V, std::vector<float>(q.n()));
  {
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const be::Stream stream = be::Stream::create();
    const PsfDerivation d(q, stream.get());
    d.enqueue(stream.get());
    d.download(&out->k1, &out->k2, stream.get());
  }
  ++g_psf_computed;
  PsfCacheEntry e;
  e.type = q.type, e.V = q.V, e.has_geom = q.has_geom, e.r = q.r, e.A = A;
  for (size_t v = 0; v < (size_t)q.V; ++v) {
    const size_t count = (size_t)q.r[3 * v] * (size_t)q.r[3 * v + 1] * (size_t)q.r[3 * v + 2];
    e.raw.emplace_back(q.raw[v], q.raw[v] + count);
  }
  e.out = out;
  g_psf_cache = std::move(e);
  return out;
}

// mvn_set_kernel_derivation
std::mutex g_derivation_mu;
int g_derivation_mode = 0, g_derivation_type = 0;

}  // namespace

extern "C" {

const char* mvn_last_error(void) { return g_last_error.c_str(); }
const char* mvn_backend_name(void) { return be::backend_name(); }

// ---------------------------------------------------------------------------------------------
// device queries (inc/cuda_helpers.cuh:70-136)
// ---------------------------------------------------------------------------------------------
int getNumDevicesCUDA(void) {
  int n = 0;
  guarded("getNumDevicesCUDA", [&] { n = be::device_count(); });
  return n;
}

int getCUDAcomputeCapabilityMajorVersion(int devCUDA) {
  int major = 0, minor = 0;
  guarded("getCUDAcomputeCapabilityMajorVersion", [&] { be::device_arch(devCUDA, &major, &minor); });
  return major;
}

int getCUDAcomputeCapabilityMinorVersion(int devCUDA) {
  int major = 0, minor = 0;
  guarded("getCUDAcomputeCapabilityMinorVersion", [&] { be::device_arch(devCUDA, &major, &minor); });
  return minor;
}

void getNameDeviceCUDA(int devCUDA, char* name) {
  if (!name) return;
  std::memset(name, 0, 256);
  guarded("getNameDeviceCUDA", [&] { be::device_name(devCUDA, name); });
}

long long int getMemDeviceCUDA(int devCUDA) {
  long long v = 0;
  guarded("getMemDeviceCUDA", [&] { v = be::device_total_mem(devCUDA); });
  return v;
}

int selectDeviceWithHighestComputeCapability(void) {
  int value = -1;
  guarded("selectDeviceWithHighestComputeCapability", [&] {
    const int n = be::device_count();
    int best = 0;
    for (int d = 0; d < n; ++d) {  // first device with the highest 10*major+minor wins
      int major = 0, minor = 0;
      be::device_arch(d, &major, &minor);
      const int meta = 10 * major + minor;
      if (meta > best || value < 0) {
        best = meta;
        value = d;
      }
    }
  });
  return value;
}

// ---------------------------------------------------------------------------------------------
// reference hot path
// ---------------------------------------------------------------------------------------------
// Two LANES per device: a lane is what used to be "the device" for the blocking call -- its own
// mutex and its own cached resident engine (keys dev and dev + kLaneStride of device_mutex() /
// engine_cache()).  inplace_gpu_deconvolve and every other blocking entry point run on lane 0;
// mvn_deconvolve_submit alternates between the two, so that block k+1's stacks cross PCIe into the
// second engine while block k iterates in the first (the intent of
// inplace_gpu_deconvolve_iteration_interleaved, src/gpu_deconvolve_methods.cuh:82-326).  Uploads of
// the two lanes take turns (upload_mutex): one block at full PCIe rate starts iterating sooner than
// two at half rate each.
static const int kLaneStride = 1024;
static std::mutex& upload_mutex(int dev) { return device_mutex(2 * kLaneStride + dev); }

static void check_workspace(const imageType* psi, const workspace& input) {
  if (input.num_views_ < 0) throw std::invalid_argument("num_views_ must be >= 0");
  if (!psi || !input.data_) throw std::invalid_argument("null psi or workspace");
  for (int v = 0; v < input.num_views_; ++v) {  // before anything is dereferenced
    const view_data& d = input.data_[v];
    if (!d.image_ || !d.kernel1_ || !d.kernel2_ || !d.weights_ || !d.image_dims_ ||
        !d.kernel1_dims_ || !d.kernel2_dims_)
      throw std::invalid_argument("view " + std::to_string(v) + " has null members");
  }
}

// ---- MVN_DEVICES: one call, several devices ---------------------------------------------------
// MVN_DEVICES=0,1,2,3 makes inplace_gpu_deconvolve cut the (padded) volume into slabs of
// dim0 planes, one per listed device, and sweep them in the reference's view order with a halo exchange per
// convolution (mvn_multi.hpp) - the `device` argument is then ignored.  The call falls back to ONE device (its
// usual path) when the volume cannot be cut that way: a PSF deeper than 33 planes (no direct dim0 leg), fewer
// planes per slab than halo planes, an odd last extent, a slab that would hold padding only.  One group of slab
// engines is kept between calls like the single-device engine (mvn_release_cached_engines frees it).
static std::unique_ptr<HaloGroup>& multi_cache() {
  static std::unique_ptr<HaloGroup>* g = new std::unique_ptr<HaloGroup>();
  return *g;
}

static std::atomic<long> g_multi_calls{0};

static bool multi_device_call(imageType* psi, const workspace& input, const shape_t& dims, const shape_t& ext,
                              const int off[3], int pad_mode, const std::vector<int>& devs) {
  const int V = input.num_views_;
  int h = 1;
  for (int v = 0; v < V; ++v)
    h = std::max(h, std::max(input.data_[v].kernel1_dims_[0], input.data_[v].kernel2_dims_[0]) / 2);
  const int P = (int)devs.size();
  auto refuse = [&](const char* why) {
    if (trace_on()) std::printf("[lmvn::trace] MVN_DEVICES: %s - one device\n", why);
    return false;
  };
  if (!HaloGroup::feasible(P, ext, h)) return refuse("the volume cannot be cut into that many slabs");
  for (int r = 0; r < P; ++r) {  // every slab holds planes of the stacks, not padding only
    const int z0 = (int)((long)r * ext[0] / P), z1 = (int)((long)(r + 1) * ext[0] / P);
    if (std::min(z1, off[0] + dims[0]) <= std::max(z0, off[0])) return refuse("a slab would hold padding only");
  }
  std::vector<int> distinct(devs);
  std::sort(distinct.begin(), distinct.end());
  distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
  std::vector<std::unique_lock<std::mutex>> locks;  // ascending order: no two calls can wait for each other
  for (int d : distinct) locks.emplace_back(device_mutex(d));
  std::unique_ptr<HaloGroup> group;
  {
    std::lock_guard<std::mutex> lk(engine_cache_mutex());
    group = std::move(multi_cache());
  }
  if (group && !(engine_cache_enabled() && group->matches(devs, ext, h, V))) group.reset();
  if (!group) {
    for (int d : distinct) {  // the single-device engines cached on these devices would compete for the memory
      be::set_device(d);
      pop_cached_engine(d).reset();
    }
    try {
      group.reset(new HaloGroup(devs, ext, h, V));
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[libmultiviewnative] MVN_DEVICES ignored for this call: %s\n", e.what());
      return false;
    }
  }
  if (!group->all_direct(input)) {
    group.reset();
    return refuse("a PSF is not held in the direct dim0 form");
  }
  if (trace_on())
    std::printf("[lmvn::trace] MVN_DEVICES: %d slabs of %d x %d x %d, %d halo planes either side\n", P, ext[0], ext[1],
                ext[2], h);
  group->run(psi, input, dims, off, pad_mode == MVN_PAD_ZERO);  // (on failure the group is dropped)
  ++g_multi_calls;
  if (engine_cache_enabled()) {
    std::lock_guard<std::mutex> lk(engine_cache_mutex());
    multi_cache() = std::move(group);
  }
  return true;
}

// extents of the stacks, of the volume the call runs on (padding policy: see the block comment above good_extent())
// and the stacks' offset inside it; `dev`: the device the call runs on (call_rule)
static void call_extents(const workspace& input, int pad_mode, int dev, shape_t* dims_out, shape_t* ext_out,
                         int off[3]) {
  const int V = input.num_views_;
  const shape_t dims = to_shape(input.data_[0].image_dims_);
  for (int v = 0; v < V; ++v) {
    const view_data& d = input.data_[v];
    if (to_shape(d.image_dims_) != dims)
      throw std::invalid_argument("all views must share image_dims_ (view " + std::to_string(v) + ")");
    if (d.weights_dims_ && to_shape(d.weights_dims_) != dims)
      throw std::invalid_argument("weights_dims_ must equal image_dims_ (view " + std::to_string(v) + ")");
  }
  for (int d = 0; d < 3; ++d)
    if (dims[d] < 1) throw std::invalid_argument("image extents must be >= 1");
  shape_t ext = dims;  // padding policy: see the block comment above good_extent()
  off[0] = off[1] = off[2] = 0;
  if (pad_mode != MVN_PAD_NONE) {
    for (int d = 2; d >= 0; --d) {
      int kmax = 1;
      for (int v = 0; v < V; ++v) {
        kmax = std::max(kmax, input.data_[v].kernel1_dims_[d]);
        kmax = std::max(kmax, input.data_[v].kernel2_dims_[d]);
      }
      ext[d] = dims[d] + kmax - 1;
      off[d] = (kmax - 1) / 2;
      if (!pad_grows(pad_mode)) continue;
      // dim0 is not transformed when every PSF of the call is held in the direct dim0 form (mvn_dim0_direct.hpp):
      // it then keeps the reference's exact image + kernel - 1 (542 planes for a 512-block with 31^3 PSFs, not
      // 576: 6 % less volume in every pass) - provided the rows of a plane keep whole tiles of the fixed
      // last-axis kernels whatever the plane count (d1 a multiple of 16).  The engine takes the same decision
      // from the same rule, so it never holds a kernel of the call as a 3-D spectrum of an exact dim0 such as 542.
      if (d == 0 && ext[1] % 16 == 0 && call_rule(ext, dev).all_direct(call_kernels(input))) continue;
      ext[d] = good_extent(ext[d], d == 2);
    }
  }
  *dims_out = dims;
  *ext_out = ext;
}

static size_t embed_floats_of(const shape_t& dims, const shape_t& ext) {
  const bool embedded = ext[0] != dims[0] || ext[1] != dims[1] || ext[2] != dims[2];
  return embedded ? (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2] : 0;
}

// ---- the stacks of a call ----------------------------------------------------------------------------------------
// Every entry point hands deconvolve_call its stacks in this form: the described ones from their descriptors
// (mvn_deconvolve_described), the others as dense float32 stacks in host memory (workspace_stacks).
struct CallStacks {
  StackRef psi;
  std::vector<StackRef> image, weights;
  void* stream = nullptr;    // the caller's stream its device stacks were produced on
  bool any_device = false;
  bool need_scratch = false; // some stack passes through the host-shaped embedding scratch
  int storage = 0;              // the image storage mode the call captured (mvn_set_image_storage)
  std::vector<char> keep_u16;   // per view: keeps_u16 of its image; empty: none
  // mvn_deconvolve_resampled: the geometry of every view (image[v].geom points here; empty: no resampled call), and
  // whether its weights are computed from it (weights[v].ptr is then null) and normalised once all views are placed
  std::vector<ResampleGeom> geom;
  bool computed_weights = false;
  // mvn_set_psi_start as the call captured it: 1 = psi is output only, the loop starts from the fusion of the views
  int psi_start = 0;
  float psi_fill = 0.f;
};

// a descriptor and its pointer as a StackRef, everything about it checked that can be without touching the memory
static StackRef described_stack(const void* ptr, const mvn_stack_desc* d, const int* dims, const std::string& what,
                                bool may_u16, bool written) {
  if (!ptr) throw std::invalid_argument(what + ": null pointer");
  if (!d) return StackRef::dense_host((const float*)ptr, dims);
  if (d->dtype != MVN_F32 && d->dtype != MVN_U16) throw std::invalid_argument(what + ": unknown dtype " + std::to_string(d->dtype));
  if (d->dtype == MVN_U16 && !may_u16) throw std::invalid_argument(what + ": only images may be uint16");
  if (d->location != MVN_HOST && d->location != MVN_DEVICE)
    throw std::invalid_argument(what + ": unknown location " + std::to_string(d->location));
  StackRef r;
  r.ptr = ptr;
  r.u16 = d->dtype == MVN_U16;
  r.device = d->location == MVN_DEVICE;
  for (int k = 0; k < 3; ++k) {
    r.stride[k] = d->stride[k];
    if (r.stride[k] < 0) throw std::invalid_argument(what + ": negative stride");
  }
  if (written) {  // every element its own address
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return r.stride[a] < r.stride[b]; });
    long long reach = 0;  // largest element offset of the dimensions passed so far
    for (int k : order) {
      if (dims[k] == 1) continue;
      if (r.stride[k] <= reach) throw std::invalid_argument(what + ": strides must be positive and must not overlap");
      reach += r.stride[k] * (long long)(dims[k] - 1);
    }
  }
  return r;
}

// the pointer is where its descriptor says (the runtime's pointer attributes; nothing is read); *owner collects the
// device of the stacks in device memory
static void check_location(const StackRef& r, const std::string& what, int* owner) {
  const int where = be::pointer_device(r.ptr);
  if (r.device) {
    if (where == be::POINTER_HOST) throw std::invalid_argument(what + ": described as device memory, but it is host memory");
    if (where >= 0) {
      if (*owner >= 0 && *owner != where) throw std::invalid_argument(what + ": stacks on two different devices");
      *owner = where;
    }
  } else if (where >= 0) {
    throw std::invalid_argument(what + ": described as host memory, but it is device memory");
  }
}

static bool plain_stack(const StackRef& r, const int* dims) {
  const StackRef d = StackRef::dense_host(nullptr, dims);
  if (r.u16 || r.device) return false;
  for (int k = 0; k < 3; ++k)
    if (dims[k] > 1 && r.stride[k] != d.stride[k]) return false;
  return true;
}

// does the stack pass through the engine's host-shaped scratch when the call embeds its stacks?
static bool through_scratch(const StackRef& r) { return !r.device && !r.broadcast(); }

// the stacks of a workspace as the reference's entry points mean them: dense float32 in host memory (nothing is asked
// about the pointers)
static CallStacks workspace_stacks(const imageType* psi, const workspace& input) {
  check_workspace(psi, input);
  CallStacks cs;
  cs.need_scratch = true;
  if (input.num_views_ > 0) cs.psi = StackRef::dense_host(psi, input.data_[0].image_dims_);
  for (int v = 0; v < input.num_views_; ++v) {
    const view_data& d = input.data_[v];
    cs.image.push_back(StackRef::dense_host(d.image_, d.image_dims_));
    cs.weights.push_back(StackRef::dense_host(d.weights_, d.image_dims_));
  }
  return cs;
}

// (the caller has checked the workspace: check_workspace; loop: the switches as the call captured them at its start)
static void deconvolve_call(const workspace& input, const CallStacks& cs, int device, int lane, int pad_mode,
                            const LoopOptions& loop, LoopResult* conv) {
  *conv = LoopResult();
  {
    const int V = input.num_views_;
    if (V == 0 || input.num_iterations_ <= 0) return;  // 0 iterations returns psi unchanged
    loop.check_call(V, input.lambda_, LoopOptions::kAbi);  // (refused before psi is touched)
    shape_t dims, ext;
    int off[3] = {0, 0, 0};
    const std::vector<int> devs = lane == 0 ? multi_devices_from_env() : std::vector<int>();
    if (!devs.empty()) {  // (the second lane belongs to the block pipeline of mvn_deconvolve_submit)
      // the slab drivers know none of the loop's switches, and take dense float32 stacks in host memory only
      const char* why = loop.needs_single_device();
      if (!why && pad_mode == MVN_PAD_REFLECT) why = "reflect padding";
      if (!why && !cs.geom.empty()) why = "resampled views";
      bool plain = plain_stack(cs.psi, input.data_[0].image_dims_);
      for (int v = 0; plain && v < V; ++v)
        plain = plain_stack(cs.image[(size_t)v], input.data_[v].image_dims_) &&
                plain_stack(cs.weights[(size_t)v], input.data_[v].image_dims_);
      if (why || !plain) {
        if (trace_on())
          std::printf("[lmvn::trace] MVN_DEVICES: %s%s - one device\n", why ? why : "described stacks",
                      why ? " on" : "");
      } else {
        call_extents(input, pad_mode, -1, &dims, &ext, off);  // (the slabs run on plans of their own extents)
        if (multi_device_call((imageType*)cs.psi.ptr, input, dims, ext, off, pad_mode, devs)) return;
      }
    }
    const int dev = pick_device(device);
    call_extents(input, pad_mode, dev, &dims, &ext, off);
    // stacks in device memory: resident whatever the mode, priced by the exact model
    const int mem_mode = cs.any_device ? (int)MVN_MEM_EXACT : current_memory_mode();
    const int key = dev + lane * kLaneStride;
    std::lock_guard<std::mutex> lk(device_mutex(key));
    be::set_device(dev);
    const bool embedded = ext[0] != dims[0] || ext[1] != dims[1] || ext[2] != dims[2];
    // on failure the engine is simply dropped
    const bool scratch = cs.need_scratch;
    std::unique_ptr<Engine> eng_owner = take_engine(
        key, dev, ext, V, embedded && scratch ? (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2] : 0, input, loop,
        mem_mode, cs.keep_u16);
    Engine& eng = *eng_owner;
    eng.begin_call();
    eng.set_options(loop);  // (an engine that comes back from TV gives up the factor volume before it allocates)
    eng.set_image_storage(cs.storage);
    eng.plan_image_types(cs.keep_u16);
    // stacks are embedded into / cropped out of the padded volume by the transfers themselves
    // (strided device copies), so the padded modes keep the pipelined upload
    const int dims_i[3] = {dims[0], dims[1], dims[2]};
    eng.set_embedding(dims_i, off, scratch);
    // extra zeros beyond the PSF's reach: the blurred estimate is exactly or nearly 0 there and
    // the reference's pointwise math would give 0 * 1/0 = NaN; the one deliberate deviation
    eng.set_quotient_guard(pad_grows(pad_mode));
    eng.set_reflect(pad_mode == MVN_PAD_REFLECT);
    static const bool no_pipeline = [] {
      const char* e = std::getenv("MVN_NO_PIPELINE");
      return e && *e && std::strcmp(e, "0") != 0;
    }();
    if (no_pipeline && eng.streamed_count() == 0) {  // (streamed views need the uploader thread)
      eng.wait_for_caller(cs.stream);
      for (int v = 0; v < V; ++v) {
        const view_data& d = input.data_[v];
        eng.set_view(v, cs.image[(size_t)v], cs.weights[(size_t)v], d.kernel1_, d.kernel1_dims_, d.kernel2_,
                     d.kernel2_dims_);
      }
      if (cs.psi_start == 1) eng.fuse_psi(cs.psi_fill);  // (from the weights as they stand: before their normalisation)
      if (cs.computed_weights) eng.normalize_weights();
      if (cs.psi_start != 1) eng.set_psi(cs.psi);
      eng.iterate(input.num_iterations_, input.lambda_, input.minValue_, loop, conv);
      eng.sync();
      eng.get_psi(cs.psi);
      give_back_engine(key, std::move(eng_owner));
      return;
    }
    // stacks arrive view by view from a second host thread while the first iteration already
    // runs on the views that are in (the reference's interleaved driver)
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!trace_on()) return;
      auto t1 = std::chrono::steady_clock::now();
      std::printf("[lmvn::trace] %-28s %8.1f ms\n", what,
                  std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    eng.reserve_views(call_kernels(input));
    lap("allocate view buffers");
    std::unique_lock<std::mutex> pcie(upload_mutex(dev));  // handed to the uploader thread's scope below
    eng.wait_for_caller(cs.stream);
    if (cs.psi_start != 1) eng.set_psi(cs.psi);
    // views that are in device memory already: ingested on the compute stream, in view order; resampled views too,
    // wherever their raw stacks are (computed weights need every view in place before the loop's first read)
    for (int v = 0; v < V; ++v)
      if ((cs.image[(size_t)v].device && cs.weights[(size_t)v].device) || cs.image[(size_t)v].geom)
        eng.ingest_device_view(v, cs.image[(size_t)v], cs.weights[(size_t)v]);
    if (cs.psi_start == 1) eng.fuse_psi(cs.psi_fill);  // (every view of a resampled call is in place here)
    if (cs.computed_weights) eng.normalize_weights();
    lap("upload psi");
    std::exception_ptr up_err;
    std::thread uploader([&] {
      try {
        be::set_device(dev);
        auto u0 = std::chrono::steady_clock::now();
        for (int v = 0; v < V; ++v) {
          const view_data& d = input.data_[v];
          eng.stage_view(v, cs.image[(size_t)v], cs.weights[(size_t)v], d.kernel1_, d.kernel1_dims_, d.kernel2_,
                         d.kernel2_dims_);
        }
        eng.finish_staging();
        // out-of-core views: their stacks again for every later sweep, in sweep order, each as soon as its ring
        // slot is free (Engine::stream_view)
        for (int it = 1; it < input.num_iterations_ && eng.streamed_count() > 0; ++it)
          for (int v = 0; v < V; ++v)
            if (eng.is_streamed(v)) eng.stream_view(v, cs.image[(size_t)v], cs.weights[(size_t)v]);
        if (trace_on())
          std::printf("[lmvn::trace] %-28s %8.1f ms (uploader thread)\n", "stage all views",
                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count());
      } catch (...) {
        up_err = std::current_exception();
        eng.staging_failed();
      }
    });
    std::exception_ptr main_err;
    try {
      eng.iterate(input.num_iterations_, input.lambda_, input.minValue_, loop, conv);
      if (conv->ran < input.num_iterations_) eng.end_streaming();  // (an early stop)
    } catch (...) {
      main_err = std::current_exception();
      eng.abort_streaming();  // (an uploader waiting for a ring slot that will not be freed)
    }
    lap("enqueue iterations");
    uploader.join();
    pcie.unlock();  // the other lane's block may start crossing PCIe while this one iterates
    lap("join uploader");
    if (up_err) std::rethrow_exception(up_err);
    if (main_err) std::rethrow_exception(main_err);
    eng.sync();
    lap("wait for the device");
    eng.get_psi(cs.psi);
    lap("download psi");
    if (eng.streamed_count() > 0) Engine::count_streamed_call();
    give_back_engine(key, std::move(eng_owner));
  }
}

// the call of the reference's entry points (the record is empty again before the workspace is looked at)
static void workspace_call(imageType* psi, const workspace& input, int device, int lane, int pad_mode,
                           const LoopOptions& loop, LoopResult* conv) {
  *conv = LoopResult();
  deconvolve_call(input, workspace_stacks(psi, input), device, lane, pad_mode, loop, conv);
}

void inplace_gpu_deconvolve(imageType* psi, struct workspace input, int device) {
  guarded("inplace_gpu_deconvolve", [&] {
    const LoopOptions mode = current_loop();
    workspace_call(psi, input, device, 0, current_pad_mode(), mode, &t_last_conv);
  });
}

int mvn_deconvolve_described(void* psi, struct workspace input, const mvn_call_desc* desc, int device) {
  return guarded("mvn_deconvolve_described", [&] {
    const LoopOptions mode = current_loop();
    if (!desc) {
      workspace_call((imageType*)psi, input, device, 0, current_pad_mode(), mode, &t_last_conv);
      return;
    }
    check_workspace((const imageType*)psi, input);
    const int V = input.num_views_;
    if (V == 0) return;
    const int* dims = input.data_[0].image_dims_;
    for (int d = 0; d < 3; ++d)
      if (dims[d] < 1) throw std::invalid_argument("image extents must be >= 1");
    // everything about the descriptors is settled before any stack is touched
    CallStacks dc;
    dc.stream = desc->stream;
    dc.psi = described_stack(psi, &desc->psi, dims, "psi", false, true);
    int owner = -1;
    check_location(dc.psi, "psi", &owner);
    for (int v = 0; v < V; ++v) {
      const view_data& d = input.data_[v];
      const std::string n = std::to_string(v);
      dc.image.push_back(described_stack(d.image_, desc->image ? desc->image + v : nullptr, d.image_dims_, "image " + n, true, false));
      dc.weights.push_back(described_stack(d.weights_, desc->weights ? desc->weights + v : nullptr, d.image_dims_, "weights " + n, false, false));
      check_location(dc.image.back(), "image " + n, &owner);
      check_location(dc.weights.back(), "weights " + n, &owner);
    }
    dc.storage = g_image_storage.load();
    for (int v = 0; v < V; ++v) dc.keep_u16.push_back(keeps_u16(dc.image[(size_t)v], dc.storage) ? 1 : 0);
    dc.need_scratch = through_scratch(dc.psi);
    dc.any_device = dc.psi.device;
    for (int v = 0; v < V; ++v) {
      dc.need_scratch = dc.need_scratch || through_scratch(dc.image[(size_t)v]) || through_scratch(dc.weights[(size_t)v]);
      dc.any_device = dc.any_device || dc.image[(size_t)v].device || dc.weights[(size_t)v].device;
    }
    if (dc.any_device) {
      if (owner >= 0 && device >= 0 && device != owner)
        throw std::invalid_argument("the stacks live on device " + std::to_string(owner) + ", not on device " +
                                    std::to_string(device));
      if (owner >= 0) device = owner;
    }
    deconvolve_call(input, dc, device, 0, current_pad_mode(), mode, &t_last_conv);
  });
}

// ---- resampled views (mvn_resample.hpp) --------------------------------------------------------------------------
// a caller's geometry as the kernels take it, refused before anything is touched
static ResampleGeom checked_geometry(const mvn_view_geometry* g, const std::string& what) {
  if (!g) throw std::invalid_argument(what + ": null geometry");
  ResampleGeom r;
  for (int k = 0; k < 3; ++k) {
    if (g->src_dims[k] < 1) throw std::invalid_argument(what + ": src_dims must be >= 1");
    r.m[k] = g->src_dims[k];
    const float b = g->blend_border[k], w = g->blend_range[k];
    if (!std::isfinite(b) || !std::isfinite(w) || b < 0.f || w < 0.f)
      throw std::invalid_argument(what + ": blend border and range must be finite and >= 0");
    r.border[k] = b, r.range[k] = w;
  }
  for (int i = 0; i < 12; ++i) {
    if (!std::isfinite(g->matrix[i])) throw std::invalid_argument(what + ": non-finite matrix entry");
    r.M[i] = g->matrix[i];
  }
  return r;
}

// the views of a resampled call with every member check_workspace asks for (computed weights bring no weights_)
static std::vector<view_data> resampled_views(const workspace& input, int weights_mode) {
  if (weights_mode != 0 && weights_mode != 1) throw std::invalid_argument("weights_mode must be 0 (the caller's) or 1 (computed)");
  if (input.num_views_ < 0) throw std::invalid_argument("num_views_ must be >= 0");
  if (!input.data_) throw std::invalid_argument("null psi or workspace");
  std::vector<view_data> views(input.data_, input.data_ + input.num_views_);
  if (weights_mode == 1)
    for (view_data& d : views) d.weights_ = d.image_;  // (never read: the stacks of the call carry no weights)
  return views;
}

// mvn_set_kernel_derivation as a resampled call captures it
static void captured_derivation(int* mode, int* type) {
  std::lock_guard<std::mutex> lk(g_derivation_mu);
  *mode = g_derivation_mode, *type = g_derivation_type;
}

// Derivation mode 1: kernel1_ / kernel1_dims_ of the views are raw PSFs.  Their extents into `raw_dims`, and the members
// the mode ignores (kernel2_, kernel2_dims_) made whatever check_workspace wants to see.
static void raw_psf_views(std::vector<view_data>& views, std::vector<int>* raw_dims) {
  for (size_t v = 0; v < views.size(); ++v) {
    view_data& d = views[v];
    if (!d.kernel1_ || !d.kernel1_dims_) throw std::invalid_argument("view " + std::to_string(v) + " has null members");
    raw_dims->insert(raw_dims->end(), d.kernel1_dims_, d.kernel1_dims_ + 3);
    d.kernel2_ = d.kernel1_, d.kernel2_dims_ = d.kernel1_dims_;
  }
}

int mvn_deconvolve_resampled(void* psi, struct workspace input, const mvn_call_desc* desc, const mvn_view_geometry* geom,
                             int weights_mode, int device) {
  return guarded("mvn_deconvolve_resampled", [&] {
    const LoopOptions mode = current_loop();
    t_last_conv = LoopResult();
    if (!geom) throw std::invalid_argument("null geom");
    std::vector<view_data> views = resampled_views(input, weights_mode);
    input.data_ = views.data();
    int derive = 0, derive_type = 0;
    captured_derivation(&derive, &derive_type);
    std::vector<int> raw_psf_dims;
    if (derive) raw_psf_views(views, &raw_psf_dims);
    check_workspace((const imageType*)psi, input);
    const int V = input.num_views_;
    if (V == 0) return;
    const int* dims = input.data_[0].image_dims_;
    for (int d = 0; d < 3; ++d)
      if (dims[d] < 1) throw std::invalid_argument("image extents must be >= 1");
    // everything about descriptors and geometries is settled before any stack is touched
    CallStacks dc;
    dc.stream = desc ? desc->stream : nullptr;
    dc.computed_weights = weights_mode == 1;
    {
      std::lock_guard<std::mutex> lk(g_psi_start_mu);
      dc.psi_start = g_psi_start_mode, dc.psi_fill = g_psi_start_fill;
    }
    dc.psi = described_stack(psi, desc ? &desc->psi : nullptr, dims, "psi", false, true);
    int owner = -1;
    check_location(dc.psi, "psi", &owner);
    dc.geom.reserve((size_t)V);
    for (int v = 0; v < V; ++v) dc.geom.push_back(checked_geometry(geom + v, "geom " + std::to_string(v)));
    for (int v = 0; v < V; ++v) {
      const view_data& d = input.data_[v];
      const std::string n = std::to_string(v);
      StackRef im = described_stack(d.image_, desc && desc->image ? desc->image + v : nullptr, dc.geom[(size_t)v].m,
                                    "image " + n, true, false);
      im.geom = &dc.geom[(size_t)v];
      dc.image.push_back(im);
      check_location(dc.image.back(), "image " + n, &owner);
      if (dc.computed_weights) {
        dc.weights.push_back(StackRef());
      } else {
        dc.weights.push_back(described_stack(d.weights_, desc && desc->weights ? desc->weights + v : nullptr,
                                             d.image_dims_, "weights " + n, false, false));
        check_location(dc.weights.back(), "weights " + n, &owner);
      }
    }
    dc.storage = g_image_storage.load();  // (resampled images are float32 volumes: keep_u16 stays empty)
    dc.need_scratch = through_scratch(dc.psi);
    for (int v = 0; v < V && !dc.computed_weights; ++v)
      dc.need_scratch = dc.need_scratch || through_scratch(dc.weights[(size_t)v]);
    dc.any_device = true;  // resident on one device, as calls with device stacks are
    if (owner >= 0 && device >= 0 && device != owner)
      throw std::invalid_argument("the stacks live on device " + std::to_string(owner) + ", not on device " +
                                  std::to_string(device));
    if (owner >= 0) device = owner;
    // Derivation mode 1: both kernels of every view from its raw PSF and its linear part, on the call's device, before
    // an engine is looked up; from here on the call is the one that brings the derived arrays
    std::shared_ptr<const PsfKernels> derived;
    int derived_dims[3];
    if (derive) {
      std::vector<const float*> raw_psf;
      for (const view_data& d : views) raw_psf.push_back(d.kernel1_);
      const PsfRequest q = psf_request(V, raw_psf.data(), raw_psf_dims.data(), geom, derive_type, nullptr);
      device = pick_device(device);
      derived = psf_derive(q, device);
      std::memcpy(derived_dims, q.K, sizeof(q.K));
      for (size_t v = 0; v < (size_t)V; ++v) {
        views[v].kernel1_ = const_cast<float*>(derived->k1[v].data());
        views[v].kernel2_ = const_cast<float*>(derived->k2[v].data());
        views[v].kernel1_dims_ = views[v].kernel2_dims_ = derived_dims;
      }
    }
    deconvolve_call(input, dc, device, 0, current_pad_mode(), mode, &t_last_conv);
  });
}

// ---- asynchronous pair: mvn_deconvolve_submit / mvn_deconvolve_wait ---------------------------
extern "C++" {
namespace {
struct DeconvJob {
  std::thread worker;
  int rc = 0;
  std::string error;
  std::vector<view_data> views;  // the caller's view_data array and dims, copied at submit
  std::vector<int> dims;
  workspace ws;
  LoopOptions mode;  // the switches of the loop at submit
  LoopResult conv;   // moves into the waiting thread's record
};
std::mutex& jobs_mutex() {
  static std::mutex* m = new std::mutex();
  return *m;
}
std::map<long long, std::unique_ptr<DeconvJob>>& jobs() {  // leaked on purpose: no joinable thread is destroyed at exit
  static auto* j = new std::map<long long, std::unique_ptr<DeconvJob>>();
  return *j;
}
}  // namespace
}  // extern "C++"

int mvn_deconvolve_submit(imageType* psi, struct workspace input, int device, long long* ticket) {
  return guarded("mvn_deconvolve_submit", [&] {
    if (!ticket) throw std::invalid_argument("null ticket");
    *ticket = 0;
    check_workspace(psi, input);
    const int V = input.num_views_;
    std::unique_ptr<DeconvJob> job(new DeconvJob());
    job->views.assign(input.data_, input.data_ + V);
    job->dims.resize((size_t)V * 12);
    for (int v = 0; v < V; ++v) {  // the four int[3] of every view move into the job
      view_data& d = job->views[v];
      int* base = job->dims.data() + (size_t)v * 12;
      int** members[4] = {&d.image_dims_, &d.kernel1_dims_, &d.kernel2_dims_, &d.weights_dims_};
      for (int m = 0; m < 4; ++m) {
        if (!*members[m]) continue;  // weights_dims_ may be null
        std::memcpy(base + 3 * m, *members[m], 3 * sizeof(int));
        *members[m] = base + 3 * m;
      }
    }
    job->ws = input;
    job->ws.data_ = job->views.data();
    const int dev = pick_device(device);
    const int pad_mode = current_pad_mode();  // the policy in force at submit time
    job->mode = current_loop();                // ... and the switches of the loop
    static std::atomic<long long> next_ticket{1};
    const long long id = next_ticket.fetch_add(1);
    static std::mutex lane_mu;
    static std::map<int, int> lane_of;  // submits per device so far -> lanes alternate
    int lane;
    {
      std::lock_guard<std::mutex> lk(lane_mu);
      lane = lane_of[dev]++ & 1;
    }
    DeconvJob* j = job.get();
    // (the worker first, the map entry second: a thread that cannot be started leaves no job behind)
    j->worker = std::thread([j, psi, dev, lane, pad_mode] {
      j->rc = guarded("mvn_deconvolve_submit (worker)",
                      [&] { workspace_call(psi, j->ws, dev, lane, pad_mode, j->mode, &j->conv); });
      if (j->rc < 0) j->error = g_last_error;  // the worker's thread-local message travels with the job
    });
    try {
      std::lock_guard<std::mutex> lk(jobs_mutex());
      jobs()[id] = std::move(job);
    } catch (...) {
      j->worker.join();
      throw;
    }
    *ticket = id;
  });
}

int mvn_deconvolve_wait(long long ticket) {
  std::unique_ptr<DeconvJob> job;
  const int rc = guarded("mvn_deconvolve_wait", [&] {
    {
      std::lock_guard<std::mutex> lk(jobs_mutex());
      auto it = jobs().find(ticket);
      if (it == jobs().end()) throw std::invalid_argument("unknown or already awaited ticket");
      job = std::move(it->second);
      jobs().erase(it);
    }
    if (job->worker.joinable()) job->worker.join();
  });
  if (rc < 0) return rc;
  t_last_conv = std::move(job->conv);
  if (job->rc < 0) g_last_error = job->error;
  return job->rc;
}

int mvn_set_convergence(double tolerance) {
  return guarded("mvn_set_convergence", [&] {
    edit_loop([&](LoopOptions& o) { o.tolerance = tolerance < 0. ? -1. : tolerance; });
  });
}

int mvn_get_convergence(double* tolerance) {
  return guarded("mvn_get_convergence", [&] {
    if (!tolerance) throw std::invalid_argument("null tolerance");
    *tolerance = current_loop().tolerance;
  });
}

int mvn_last_convergence(int* iterations_run, double* stats, int capacity) {
  int rows = 0;
  const int rc = guarded("mvn_last_convergence", [&] {
    if (capacity < 0 || (capacity > 0 && !stats)) throw std::invalid_argument("bad statistics buffer");
    if (iterations_run) *iterations_run = t_last_conv.ran;
    rows = copy_rows(t_last_conv.rows, 3, stats, capacity);
  });
  return rc < 0 ? rc : rows;
}

int mvn_set_acceleration(int mode) {
  return guarded("mvn_set_acceleration", [&] { edit_loop([&](LoopOptions& o) { o.accel = mode; }); });
}

int mvn_get_acceleration(int* mode) {
  return guarded("mvn_get_acceleration", [&] {
    if (!mode) throw std::invalid_argument("null mode");
    *mode = current_loop().accel;
  });
}

int mvn_last_acceleration(double* alphas, int capacity) {
  int rows = 0;
  const int rc = guarded("mvn_last_acceleration", [&] {
    if (capacity < 0 || (capacity > 0 && !alphas)) throw std::invalid_argument("bad alpha buffer");
    rows = copy_rows(t_last_conv.alphas, 1, alphas, capacity);
  });
  return rc < 0 ? rc : rows;
}

// (epsilon belongs to total variation: the other kind keeps none)
static void set_regulariser(LoopOptions& o, int kind, double epsilon) {
  o.reg_kind = kind;
  o.epsilon = kind == MVN_REG_TV ? epsilon : 0.;
}

int mvn_set_regularization(int kind, double epsilon) {
  return guarded("mvn_set_regularization", [&] {
    edit_loop([&](LoopOptions& o) { set_regulariser(o, kind, epsilon); });
  });
}

int mvn_get_regularization(int* kind, double* epsilon) {
  return guarded("mvn_get_regularization", [&] {
    if (!kind || !epsilon) throw std::invalid_argument("null argument");
    const LoopOptions o = current_loop();
    *kind = o.reg_kind;
    *epsilon = o.epsilon;
  });
}

int mvn_set_background(const float* values, int count) {
  return guarded("mvn_set_background", [&] {
    if (count < 0) throw std::invalid_argument("negative count");
    if (!values) count = 0;
    edit_loop([&](LoopOptions& o) { o.background.assign(values, values + count); });
  });
}

int mvn_get_background(float* values, int capacity) {
  int count = 0;
  const int rc = guarded("mvn_get_background", [&] {
    if (capacity < 0 || (capacity > 0 && !values)) throw std::invalid_argument("bad background buffer");
    const LoopOptions o = current_loop();
    count = (int)o.background.size();
    for (int i = 0; i < std::min(count, capacity); ++i) values[i] = o.background[(size_t)i];
  });
  return rc < 0 ? rc : count;
}

int mvn_set_likelihood(int mode) {
  return guarded("mvn_set_likelihood", [&] { edit_loop([&](LoopOptions& o) { o.likelihood = mode; }); });
}

int mvn_get_likelihood(int* mode) {
  return guarded("mvn_get_likelihood", [&] {
    if (!mode) throw std::invalid_argument("null mode");
    *mode = current_loop().likelihood;
  });
}

int mvn_last_likelihood(int* iterations_run, int* num_views, double* stats, int capacity_rows) {
  int rows = 0;
  const int rc = guarded("mvn_last_likelihood", [&] {
    if (capacity_rows < 0 || (capacity_rows > 0 && !stats)) throw std::invalid_argument("bad statistics buffer");
    if (iterations_run) *iterations_run = t_last_conv.ran;
    if (num_views) *num_views = t_last_conv.views;
    rows = copy_rows(t_last_conv.like, 3, stats, capacity_rows);
  });
  return rc < 0 ? rc : rows;
}

long mvn_tv_launch_count(void) { return be::tv_launch_count(); }

// the pass of mvn_tv.hpp on a dense host volume: a test and bench utility
int mvn_tv_factor(int device, const int dims[3], const float* psi, double lambda, double epsilon, float* t) {
  return guarded("mvn_tv_factor", [&] {
    if (!dims || !psi || !t) throw std::invalid_argument("null argument");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) throw std::invalid_argument("extents must be positive");
    if (!LoopOptions::tv_epsilon_ok(epsilon)) throw std::invalid_argument("epsilon must be finite and > 0");
    LoopOptions::check_tv_lambda(lambda, LoopOptions::kAbi);
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const Layout L(dims[0], dims[1], dims[2]);
    const size_t bytes = L.real_floats() * sizeof(float), width = (size_t)L.d2 * sizeof(float),
                 pitch = (size_t)L.RP * sizeof(float);
    const be::DeviceBuffer<float> du(bytes), dt(bytes);
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    be::dzero(du.get(), bytes, s);
    be::h2d_2d(du.get(), pitch, psi, width, width, (size_t)L.rows, s);
    be::launch_tv(tv_params(L, du.get(), dt.get(), lambda, epsilon), s);
    be::d2h_2d(t, width, dt.get(), pitch, width, (size_t)L.rows, s);
    be::stream_sync(s);
  });
}

// ms[0]: the pass of mvn_tv.hpp on a resident volume of these extents, per launch over `reps` launches between two
// stream events; ms[1]: a plain streaming copy of the same volume (launch_copy3d: one read and one write), likewise
int mvn_tv_time(int device, const int dims[3], int reps, float* ms) {
  return guarded("mvn_tv_time", [&] {
    if (!dims || !ms) throw std::invalid_argument("null argument");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || reps < 1) throw std::invalid_argument("extents and reps must be positive");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const Layout L(dims[0], dims[1], dims[2]);
    const size_t bytes = L.real_floats() * sizeof(float);
    const be::DeviceBuffer<float> du(bytes), dt(bytes);
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    // a ramp with a ripple: finite gradients everywhere
    std::vector<float> h(L.real_floats());
    for (size_t i = 0; i < h.size(); ++i) h[i] = 1.f + 0.001f * (float)(i % 977) + 0.01f * (float)(i % 13);
    be::h2d(du.get(), h.data(), bytes, s);
    const TvParams p = tv_params(L, du.get(), dt.get(), 0.005, 0.01);
    const long plane = (long)L.d1 * L.RP;
    ms[0] = time_on_stream(s, reps, [&] { be::launch_tv(p, s); });
    ms[1] = time_on_stream(
        s, reps, [&] { be::launch_copy3d(dt.get(), L.RP, plane, du.get(), L.RP, plane, L.d2, L.d1, L.d0, s); });
  });
}

int mvn_reflect_counters(long long out[2]) {
  return guarded("mvn_reflect_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    be::reflect_counters(out);
  });
}

// ms[0]: the fill of mvn_reflect.hpp (all its launches) on a resident volume of extents ext around a window of extents
// dims at offset off, float32 or (u16) uint16, per fill over `reps` fills between two stream events; ms[1]: a plain
// streaming copy of that volume (launch_copy3d on its bytes: one read and one write), likewise
int mvn_reflect_time(int device, const int dims[3], const int ext[3], const int off[3], int u16, int reps, float* ms) {
  return guarded("mvn_reflect_time", [&] {
    if (!dims || !ext || !off || !ms) throw std::invalid_argument("null argument");
    if (reps < 1) throw std::invalid_argument("reps must be positive");
    for (int d = 0; d < 3; ++d)
      if (dims[d] < 1 || off[d] < 0 || (long)off[d] + dims[d] > ext[d])
        throw std::invalid_argument("the window does not fit the volume");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const Layout L(ext[0], ext[1], ext[2]);
    const size_t esz = u16 ? sizeof(uint16_t) : sizeof(float);
    const size_t bytes = L.real_floats() * esz;
    const be::DeviceBuffer<float> du(bytes), dt(bytes);
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    std::vector<unsigned char> h(bytes);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (unsigned char)(i % 251);
    be::h2d(du.get(), h.data(), bytes, s);
    ReflectParams p;
    p.vol = du.get(), p.RP = L.RP, p.D0 = L.d0, p.D1 = L.d1, p.D2 = L.d2;
    p.n0 = dims[0], p.n1 = dims[1], p.n2 = dims[2];
    p.o0 = off[0], p.o1 = off[1], p.o2 = off[2];
    p.axis = 2;
    // the copy moves the volume's bytes as rows of floats (a uint16 volume: RP / 2 of them, RP is even)
    const long row = u16 ? L.RP / 2 : L.RP, plane = (long)L.d1 * row;
    ms[0] = time_on_stream(s, reps, [&] { be::launch_reflect_fill(p, u16 != 0, s); });
    ms[1] = time_on_stream(
        s, reps, [&] { be::launch_copy3d(dt.get(), row, plane, du.get(), row, plane, (int)row, L.d1, L.d0, s); });
  });
}

int mvn_resample_counters(long long out[2]) {
  return guarded("mvn_resample_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    be::resample_counters(out);
  });
}

// the volumes of a stand-alone resample pass: dense extents dims, the window the whole volume
static ResampleParams resample_alone(const Layout& L, float* image, float* weights) {
  ResampleParams p;
  p.image = image, p.weights = weights, p.RP = L.RP, p.D0 = L.d0, p.D1 = L.d1;
  p.n0 = L.d0, p.n1 = L.d1, p.n2 = L.d2;
  p.o0 = p.o1 = p.o2 = 0;
  return p;
}

// the pass of mvn_resample.hpp alone, into dense host arrays: a test and bench utility
int mvn_resample_stack(int device, const void* src, const mvn_stack_desc* src_desc, const mvn_view_geometry* geom,
                       const int out_dims[3], float* image_out, float* weights_out) {
  return guarded("mvn_resample_stack", [&] {
    if (!src || !out_dims) throw std::invalid_argument("null argument");
    if (out_dims[0] < 1 || out_dims[1] < 1 || out_dims[2] < 1) throw std::invalid_argument("extents must be positive");
    const ResampleGeom g = checked_geometry(geom, "geom");
    StackRef st = described_stack(src, src_desc, g.m, "src", true, false);
    st.geom = &g;
    int owner = -1;
    check_location(st, "src", &owner);
    if (owner >= 0 && device >= 0 && device != owner) throw std::invalid_argument("src lives on another device");
    const int dev = pick_device(owner >= 0 ? owner : device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const Layout L(out_dims[0], out_dims[1], out_dims[2]);
    const size_t bytes = L.real_floats() * sizeof(float), width = (size_t)L.d2 * sizeof(float),
                 pitch = (size_t)L.RP * sizeof(float);
    const be::DeviceBuffer<float> di(bytes), dw(bytes);
    const be::Stream stream = be::Stream::create();
    const be::stream_t s = stream.get();
    Engine::resample_raw(resample_alone(L, di.get(), dw.get()), st, s);
    if (image_out) be::d2h_2d(image_out, width, di.get(), pitch, width, (size_t)L.rows, s);
    if (weights_out) be::d2h_2d(weights_out, width, dw.get(), pitch, width, (size_t)L.rows, s);
    be::stream_sync(s);
  });
}

// ms[0]: the pass of mvn_resample.hpp from a resident raw stack into resident volumes, per pass over `reps` passes
// between two stream events; ms[1]: streaming traffic of the output's size, one volume read and two written
// (launch_copy3d of a volume and a clear of a second one), likewise
int mvn_resample_time(int device, int u16, const mvn_view_geometry* geom, const int out_dims[3], int reps, float* ms) {
  return guarded("mvn_resample_time", [&] {
    if (!out_dims || !ms) throw std::invalid_argument("null argument");
    if (out_dims[0] < 1 || out_dims[1] < 1 || out_dims[2] < 1 || reps < 1)
      throw std::invalid_argument("extents and reps must be positive");
    const ResampleGeom g = checked_geometry(geom, "geom");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const Layout L(out_dims[0], out_dims[1], out_dims[2]);
    const size_t bytes = L.real_floats() * sizeof(float);
    const size_t esz = u16 ? sizeof(uint16_t) : sizeof(float);
    const size_t raw = (size_t)g.m[0] * (size_t)g.m[1] * (size_t)g.m[2];
    const be::DeviceBuffer<float> di(bytes), dw(bytes);
    const be::DeviceBuffer<> dr(raw * esz);
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    std::vector<unsigned char> h(raw * esz);
    if (u16)
      for (size_t i = 0; i < raw; ++i) ((uint16_t*)h.data())[i] = (uint16_t)(100u + i % 4001u);
    else
      for (size_t i = 0; i < raw; ++i) ((float*)h.data())[i] = 100.f + (float)(i % 4001u);
    be::h2d(dr.get(), h.data(), h.size(), s);
    be::dzero(di.get(), bytes, s);
    be::stream_sync(s);
    ResampleParams p = resample_alone(L, di.get(), dw.get());
    p.src = dr.get(), p.s0 = (long long)g.m[1] * g.m[2], p.s1 = g.m[2], p.s2 = 1;
    p.g = g;
    const long plane = (long)L.d1 * L.RP;
    ms[0] = time_on_stream(s, reps, [&] { be::launch_resample(p, u16 != 0, s); });
    ms[1] = time_on_stream(s, reps, [&] {
      be::launch_copy3d(dw.get(), L.RP, plane, di.get(), L.RP, plane, (int)L.RP, L.d1, L.d0, s);
      be::dzero(di.get(), bytes, s);
    });
  });
}

// ---- fusion (mvn_fuse.hpp) ---------------------------------------------------------------------------------------
int mvn_fuse_counters(long long out[2]) {
  return guarded("mvn_fuse_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    be::fuse_counters(out);
  });
}

int mvn_set_psi_start(int mode, float fill) {
  return guarded("mvn_set_psi_start", [&] {
    if (mode != 0 && mode != 1)
      throw std::invalid_argument("psi start mode must be 0 (the caller's psi) or 1 (the fusion of the views)");
    if (!std::isfinite(fill)) throw std::invalid_argument("fill must be finite");
    std::lock_guard<std::mutex> lk(g_psi_start_mu);
    g_psi_start_mode = mode, g_psi_start_fill = fill;
  });
}

int mvn_get_psi_start(int* mode, float* fill) {
  return guarded("mvn_get_psi_start", [&] {
    if (!mode || !fill) throw std::invalid_argument("null argument");
    std::lock_guard<std::mutex> lk(g_psi_start_mu);
    *mode = g_psi_start_mode, *fill = g_psi_start_fill;
  });
}

// ---- derived kernels (mvn_psf.hpp) ---------------------------------------------------------------------------------
int mvn_psf_extents(int num_views, const int* raw_dims, const mvn_view_geometry* geom, int out_dims[3]) {
  return guarded("mvn_psf_extents", [&] {
    if (!out_dims) throw std::invalid_argument("null out_dims");
    int K[3];
    psf_extents(num_views, raw_dims, geom, K);
    for (int k = 0; k < 3; ++k) out_dims[k] = K[k];
  });
}

int mvn_derive_kernels(int device, int num_views, const float* const* raw_psf, const int* raw_dims,
                       const mvn_view_geometry* geom, int type, const int out_dims[3], float* const* kernel1,
                       float* const* kernel2) {
  return guarded("mvn_derive_kernels", [&] {
    const PsfRequest q = psf_request(num_views, raw_psf, raw_dims, geom, type, out_dims);
    for (int v = 0; v < num_views; ++v)
      if ((kernel1 && !kernel1[v]) || (kernel2 && !kernel2[v]))
        throw std::invalid_argument("null output for view " + std::to_string(v));
    const std::shared_ptr<const PsfKernels> k = psf_derive(q, pick_device(device));
    for (size_t v = 0; v < (size_t)num_views; ++v) {
      if (kernel1) std::memcpy(kernel1[v], k->k1[v].data(), q.n() * sizeof(float));
      if (kernel2) std::memcpy(kernel2[v], k->k2[v].data(), q.n() * sizeof(float));
    }
  });
}

int mvn_set_kernel_derivation(int mode, int type) {
  return guarded("mvn_set_kernel_derivation", [&] {
    if (mode != 0 && mode != 1)
      throw std::invalid_argument("kernel derivation mode must be 0 (kernels handed in) or 1 (derived from raw PSFs)");
    psf_check_type(type);
    std::lock_guard<std::mutex> lk(g_derivation_mu);
    g_derivation_mode = mode, g_derivation_type = type;
  });
}

int mvn_get_kernel_derivation(int* mode, int* type) {
  return guarded("mvn_get_kernel_derivation", [&] {
    if (!mode || !type) throw std::invalid_argument("null argument");
    std::lock_guard<std::mutex> lk(g_derivation_mu);
    *mode = g_derivation_mode, *type = g_derivation_type;
  });
}

int mvn_derive_counters(long long out[3]) {
  return guarded("mvn_derive_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    out[0] = be::psf_correlate_launches(), out[1] = g_psf_computed.load(), out[2] = g_psf_reused.load();
  });
}

// ms[0]: every launch of a derivation of `type` for num_views resident PSFs of extents dims (no geometry: K = dims), per
// derivation over `reps` derivations between two stream events behind one that warms up; ms[1]: its correlation launches
// alone, likewise (0: the type has none)
int mvn_derive_time(int device, int num_views, const int dims[3], int type, int reps, float* ms) {
  return guarded("mvn_derive_time", [&] {
    if (!dims || !ms) throw std::invalid_argument("null argument");
    if (reps < 1 || num_views < 1) throw std::invalid_argument("reps and num_views must be positive");
    std::vector<int> r;
    for (int v = 0; v < num_views; ++v) r.insert(r.end(), dims, dims + 3);
    psf_check_raw_dims(num_views, r.data());
    for (int k = 0; k < 3; ++k)
      if (dims[k] > MVN_PSF_MAX) throw std::invalid_argument("extents above " + std::to_string(MVN_PSF_MAX));
    const size_t n = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
    std::vector<std::vector<float>> host;
    std::vector<const float*> ptrs;
    for (int v = 0; v < num_views; ++v) {  // random positives, peaked like a PSF: u^6 of an LCG's values
      host.push_back(lcg_fill(n));
      for (float& x : host.back()) {
        const float u = x + 0.5f + 1.0f / 1024.0f;
        x = (u * u) * (u * u) * (u * u);
        x += 1e-3f * (float)v;
      }
      ptrs.push_back(host.back().data());
    }
    const PsfRequest q = psf_request(num_views, ptrs.data(), r.data(), nullptr, type, nullptr);
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const be::Stream stream = be::Stream::create();
    const be::stream_t s = stream.get();
    const PsfDerivation d(q, s);
    ms[0] = time_on_stream(s, reps, [&] { d.enqueue(s); });
    ms[1] = q.correlates() ? time_on_stream(s, reps, [&] { d.correlations(s); }) : 0.f;
    d.download(nullptr, nullptr, s);  // (drains the stream; the sums say that the passes ran on sound values)
  });
}

// ---- bead PSFs (mvn_beads.hpp; the arithmetic is stated at mvn_extract_psf in include/mvn_engine_api.h) ---------------
extern "C++" {
namespace {
static_assert(MVN_BEADS_GROUP == MVN_BEADS_PER_GROUP, "the group size of the header is the passes'");

// an extraction, everything checked that can be without touching the stack (pointers == false: a memory query, which
// brings neither the stack nor the beads)
struct BeadRequest {
  int m[3] = {1, 1, 1}, r[3] = {1, 1, 1};
  int nbeads = 0, flags = 0;
  bool want_scores = false;
  StackRef raw;
  std::vector<BeadRec> recs;
  size_t raw_bytes = 0;  // the upload of a stack in host memory
  size_t n() const { return (size_t)r[0] * (size_t)r[1] * (size_t)r[2]; }
  size_t groups() const { return (size_t)mvn_beads_groups(nbeads); }
  size_t record_bytes() const { return (size_t)nbeads * sizeof(BeadRec); }
  size_t partial_bytes() const { return groups() * n() * sizeof(double); }
  size_t result_bytes() const { return n() * sizeof(float) + (MVN_BEADS_WG + 1) * sizeof(float); }
  size_t score_bytes() const {
    return want_scores ? (size_t)nbeads * (MVN_BEADS_WG * MVN_BEADS_SUMS + 1) * sizeof(double) : 0;
  }
  size_t bytes() const { return record_bytes() + partial_bytes() + result_bytes() + score_bytes() + raw_bytes; }
};

BeadRequest bead_request(const void* raw, const mvn_stack_desc* raw_desc, const int* src_dims, const double* beads,
                         int num_beads, const int* psf_dims, int flags, bool want_scores, bool pointers) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static const int placeholder = 0;  // (a memory query brings no pointers: nothing is read through this one)
  if (!src_dims || !psf_dims) throw std::invalid_argument("null dims");
  if (pointers && !beads) throw std::invalid_argument("null beads");
  BeadRequest q;
  for (int k = 0; k < 3; ++k) {
    if (src_dims[k] < 1 || src_dims[k] > 0x3fffffff) throw std::invalid_argument("src_dims must be in 1..2^30 - 1");
    if (psf_dims[k] < 1 || psf_dims[k] > MVN_BEADS_MAX || !(psf_dims[k] & 1))
      throw std::invalid_argument("psf_dims must be odd and between 1 and " + std::to_string(MVN_BEADS_MAX));
    q.m[k] = src_dims[k], q.r[k] = psf_dims[k];
  }
  if (num_beads < 1) throw std::invalid_argument("num_beads must be >= 1");
  if (flags & ~(int)MVN_BEADS_REMOVE_MIN) throw std::invalid_argument("unknown flag bits " + std::to_string(flags));
  q.nbeads = num_beads, q.flags = flags, q.want_scores = want_scores;
  q.raw = described_stack(pointers ? raw : &placeholder, raw_desc, q.m, "raw", true, false);
  Engine::check_raw_host(q.raw, q.m);
  if (!q.raw.device) {
    const size_t esz = q.raw.u16 ? sizeof(uint16_t) : sizeof(float);
    q.raw_bytes = q.raw.broadcast() ? esz : (size_t)q.m[0] * (size_t)q.m[1] * (size_t)q.m[2] * esz;
  }
  if (!pointers) return q;
  q.recs.resize((size_t)num_beads);
  for (int b = 0; b < num_beads; ++b) {
    BeadRec& rec = q.recs[(size_t)b];
    std::memset(&rec, 0, sizeof(rec));
    rec.interior = 1;
    for (int k = 0; k < 3; ++k) {
      const double p = beads[3 * (size_t)b + (size_t)k];
      if (!std::isfinite(p)) throw std::invalid_argument("bead " + std::to_string(b) + ": non-finite position");
      if (!(p >= 0. && p <= (double)(q.m[k] - 1)))
        throw std::invalid_argument("bead " + std::to_string(b) + ": position outside the raw stack");
      const int B = (int)p;  // floor: p >= 0
      const int h = (q.r[k] - 1) / 2;
      rec.B[k] = B;
      rec.f[k] = (float)(p - (double)B);
      if (B - h < 0 || (long long)B + h + 1 > (long long)q.m[k] - 1) rec.interior = 0;
    }
  }
  return q;
}

// the device side of one extraction: buffers, the bead table, and the launches in stream order
class BeadExtraction {
 public:
  // raw: the stack where the passes read it, in device memory (the caller's, or its temporary upload)
  BeadExtraction(const BeadRequest& q, const StackRef& raw, be::stream_t s)
      : q_(q),
        table_(q.record_bytes()),
        partial_(q.partial_bytes()),
        psf_(q.result_bytes()),
        records_(q.score_bytes() ? q.score_bytes() : sizeof(double)) {
    std::memset(&p_, 0, sizeof(p_));
    p_.src = raw.ptr, p_.s0 = raw.stride[0], p_.s1 = raw.stride[1], p_.s2 = raw.stride[2];
    for (int k = 0; k < 3; ++k) p_.m[k] = q.m[k], p_.r[k] = q.r[k];
    p_.beads = table_.get(), p_.nbeads = q.nbeads;
    p_.partial = partial_.get(), p_.psf = psf_.get();
    p_.minima = psf_.get() + q.n();
    p_.flag = (unsigned*)(psf_.get() + q.n() + MVN_BEADS_WG);
    if (q.want_scores) {
      p_.records = records_.get();
      p_.scores = records_.get() + (size_t)q.nbeads * MVN_BEADS_WG * MVN_BEADS_SUMS;
    }
    u16_ = raw.u16;
    mvn_beads_check(p_);
    be::h2d(table_.get(), q.recs.data(), q.record_bytes(), s);
  }

  // every launch of the extraction; scores are taken against the mean BEFORE its minimum is removed
  void enqueue(be::stream_t s) const {
    be::dzero(p_.flag, sizeof(unsigned), s);
    be::launch_beads_gather(p_, u16_, s);
    be::launch_beads_reduce(p_, s);
    if (q_.want_scores) be::launch_beads_score(p_, u16_, s);
    if (q_.flags & MVN_BEADS_REMOVE_MIN) be::launch_beads_remove_min(p_, s);
  }

  // the flag checked, then the results into host memory (either may be null); blocks
  void download(float* psf, double* scores, be::stream_t s) const {
    unsigned flag = 0;
    std::vector<float> h_psf(psf ? q_.n() : 0);
    std::vector<double> h_scores(scores && q_.want_scores ? (size_t)q_.nbeads : 0);
    be::d2h(&flag, p_.flag, sizeof(flag), s);
    if (!h_psf.empty()) be::d2h(h_psf.data(), p_.psf, h_psf.size() * sizeof(float), s);
    if (!h_scores.empty()) be::d2h(h_scores.data(), p_.scores, h_scores.size() * sizeof(double), s);
    be::stream_sync(s);
    if (flag) throw std::invalid_argument("a non-finite PSF (a non-finite sample under a bead, or a mean beyond float32)");
    if (!h_psf.empty()) std::memcpy(psf, h_psf.data(), h_psf.size() * sizeof(float));
    if (!h_scores.empty()) std::memcpy(scores, h_scores.data(), h_scores.size() * sizeof(double));
  }

 private:
  const BeadRequest& q_;
  BeadsParams p_;
  bool u16_ = false;
  be::DeviceBuffer<BeadRec> table_;
  be::DeviceBuffer<double> partial_;
  be::DeviceBuffer<float> psf_;  // the result, MVN_BEADS_WG minima and the flag word behind it
  be::DeviceBuffer<double> records_;
};

std::atomic<long long> g_extractions{0};
}  // namespace
}  // extern "C++"

int mvn_extract_psf(int device, const void* raw, const mvn_stack_desc* raw_desc, const int src_dims[3],
                    const double* beads, int num_beads, const int psf_dims[3], int flags, float* psf_out,
                    double* scores_out, void* stream) {
  return guarded("mvn_extract_psf", [&] {
    if (!psf_out) throw std::invalid_argument("null psf_out");
    const BeadRequest q = bead_request(raw, raw_desc, src_dims, beads, num_beads, psf_dims, flags, scores_out != nullptr, true);
    int owner = -1;
    check_location(q.raw, "raw", &owner);
    if (owner >= 0 && device >= 0 && device != owner) throw std::invalid_argument("raw lives on another device");
    const int dev = pick_device(owner >= 0 ? owner : device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    be::DeviceBuffer<char> upload;
    const be::Event caller = be::Event::sync_only();
    const be::Stream own = be::Stream::create();
    const be::stream_t s = own.get();
    if (stream) {  // the caller's device stack is complete behind what its stream holds now
      be::event_record(caller.get(), (be::stream_t)stream);
      be::stream_wait_event(s, caller.get());
    }
    StackRef there = q.raw;
    if (!q.raw.device) Engine::upload_raw(q.raw, q.m, upload, &there, s);
    const BeadExtraction x(q, there, s);
    x.enqueue(s);
    x.download(psf_out, scores_out, s);
    ++g_extractions;
  });
}

int mvn_extract_memory(const mvn_stack_desc* raw_desc, const int src_dims[3], int num_beads, const int psf_dims[3],
                       int want_scores, int device, size_t* bytes) {
  return guarded("mvn_extract_memory", [&] {
    if (!bytes) throw std::invalid_argument("null bytes");
    *bytes = 0;
    (void)device;
    *bytes = bead_request(nullptr, raw_desc, src_dims, nullptr, num_beads, psf_dims, 0, want_scores != 0, false).bytes();
  });
}

int mvn_extract_counters(long long out[3]) {
  return guarded("mvn_extract_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    be::beads_counters(out);
    out[2] = g_extractions.load();
  });
}

// ms[0]: every launch of an extraction (no scores, flags 0) of num_beads beads from a resident raw stack of src_dims,
// per extraction over `reps` extractions between two stream events behind one that warms up; ms[1]: num_beads launches
// of the resample pass on the same stack, image only, each into one volume of extents psf_dims through the identity
// plus the bead's offset, nothing summed, likewise; ms[2]: a plain copy of num_beads x prod psf_dims floats
int mvn_extract_time(int device, int u16, const int src_dims[3], int num_beads, const int psf_dims[3], int reps,
                     float* ms) {
  return guarded("mvn_extract_time", [&] {
    if (!src_dims || !psf_dims || !ms) throw std::invalid_argument("null argument");
    if (reps < 1 || num_beads < 1) throw std::invalid_argument("reps and num_beads must be positive");
    for (int k = 0; k < 3; ++k)
      if (psf_dims[k] >= 1 && src_dims[k] < psf_dims[k] + 2)
        throw std::invalid_argument("src_dims must be at least psf_dims + 2: the beads keep h + 1 from every face");
    // reproducible sub-voxel positions, at least h + 1 from every face: an LCG's values in [h + 1, m - 2 - h]
    std::vector<double> pos(3 * (size_t)num_beads);
    unsigned x = 2463534242u;
    for (size_t i = 0; i < pos.size(); ++i) {
      x = x * 1664525u + 1013904223u;
      const int k = (int)(i % 3);
      const double lo = (double)((psf_dims[k] - 1) / 2 + 1), hi = (double)(src_dims[k] - 1) - lo;
      pos[i] = lo + (hi - lo) * ((double)(x >> 8) * (1.0 / 16777216.0));
    }
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const size_t esz = u16 ? sizeof(uint16_t) : sizeof(float);
    const size_t raw = (size_t)src_dims[0] * (size_t)src_dims[1] * (size_t)src_dims[2];
    const be::DeviceBuffer<> dr(raw * esz);
    mvn_stack_desc desc;
    desc.dtype = u16 ? MVN_U16 : MVN_F32, desc.location = MVN_DEVICE;
    desc.stride[0] = (long long)src_dims[1] * src_dims[2], desc.stride[1] = src_dims[2], desc.stride[2] = 1;
    const BeadRequest q = bead_request(dr.get(), &desc, src_dims, pos.data(), num_beads, psf_dims, 0, false, true);
    const Layout L(q.r[0], q.r[1], q.r[2]);
    const size_t n = q.n();
    const be::DeviceBuffer<float> di(L.real_floats() * sizeof(float));
    const be::DeviceBuffer<float> ca((size_t)num_beads * n * sizeof(float)), cb((size_t)num_beads * n * sizeof(float));
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    std::vector<unsigned char> h(raw * esz);
    if (u16)
      for (size_t i = 0; i < raw; ++i) ((uint16_t*)h.data())[i] = (uint16_t)(100u + i % 4001u);
    else
      for (size_t i = 0; i < raw; ++i) ((float*)h.data())[i] = 100.f + (float)(i % 4001u);
    be::h2d(dr.get(), h.data(), h.size(), s);
    const std::vector<float> row = lcg_fill(n);
    for (int b = 0; b < num_beads; ++b) be::h2d(ca.get() + (size_t)b * n, row.data(), n * sizeof(float), s);
    be::stream_sync(s);
    const BeadExtraction ex(q, q.raw, s);
    ms[0] = time_on_stream(s, reps, [&] { ex.enqueue(s); });
    ex.download(nullptr, nullptr, s);  // (drains the stream; the flag says that the passes ran on sound values)
    ResampleParams rp = resample_alone(L, di.get(), nullptr);
    std::memset(&rp.g, 0, sizeof(rp.g));
    rp.src = dr.get(), rp.s0 = desc.stride[0], rp.s1 = desc.stride[1], rp.s2 = 1;
    for (int k = 0; k < 3; ++k) rp.g.m[k] = q.m[k], rp.g.M[4 * k + k] = 1.0;
    ms[1] = time_on_stream(s, reps, [&] {
      for (int b = 0; b < num_beads; ++b) {
        for (int k = 0; k < 3; ++k) rp.g.M[4 * k + 3] = pos[3 * (size_t)b + (size_t)k] - (double)((q.r[k] - 1) / 2);
        be::launch_resample(rp, u16 != 0, s);
      }
    });
    const long width = (long)n;
    ms[2] = time_on_stream(s, reps, [&] {
      be::launch_copy3d(cb.get(), width, width * num_beads, ca.get(), width, width * num_beads, (int)n, num_beads, 1, s);
    });
  });
}

// ---- bead detection (mvn_detect.hpp; the arithmetic is stated at mvn_detect_beads in include/mvn_engine_api.h) ---------
extern "C++" {
namespace {
static_assert(MVN_DETECT_MAX_RADIUS == MVN_DETECT_RMAX, "the largest radius of the header is the passes'");
static_assert(2 * MVN_DETECT_RMAX + 1 <= MVN_DETECT_TAPS, "a tap vector fits its place in the table");

// a detection, everything checked that can be without touching the stack (pointers == false: a memory query, which
// brings neither the stack nor the parameters)
struct DetectRequest {
  int m[3] = {1, 1, 1};
  int R[2][3] = {{0, 0, 0}, {0, 0, 0}};
  float threshold = 0.f;
  int flags = 0;
  long long capacity = 1;
  StackRef raw;
  std::vector<float> table;  // MVN_DETECT_TABLE floats
  size_t raw_bytes = 0;      // the upload of a stack in host memory
  size_t n() const { return (size_t)m[0] * (size_t)m[1] * (size_t)m[2]; }
  size_t volume_bytes() const { return n() * sizeof(float); }
  size_t table_bytes() const { return MVN_DETECT_TABLE * sizeof(float); }
  size_t list_bytes() const { return (size_t)capacity * sizeof(long long); }
  size_t result_bytes() const { return (size_t)capacity * (3 * sizeof(double) + sizeof(float) + 3 * sizeof(int)); }
  size_t bytes() const {
    return 4 * volume_bytes() + table_bytes() + sizeof(unsigned long long) + list_bytes() + result_bytes() + raw_bytes;
  }
  bool too_thin() const { return m[0] < 3 || m[1] < 3 || m[2] < 3; }  // no voxel has 26 neighbours
};

DetectRequest detect_request(const void* raw, const mvn_stack_desc* raw_desc, const int* src_dims,
                             const mvn_detect_params* prm, long long capacity, bool pointers) {
  static const int placeholder = 0;  // (a memory query brings no pointers: nothing is read through this one)
  if (!src_dims) throw std::invalid_argument("null dims");
  if (pointers && !prm) throw std::invalid_argument("null prm");
  DetectRequest q;
  for (int k = 0; k < 3; ++k) {
    if (src_dims[k] < 1 || src_dims[k] > 0x3fffffff) throw std::invalid_argument("src_dims must be in 1..2^30 - 1");
    q.m[k] = src_dims[k];
  }
  if (capacity < 1) throw std::invalid_argument("capacity must be >= 1");
  q.capacity = capacity;
  q.raw = described_stack(pointers ? raw : &placeholder, raw_desc, q.m, "raw", true, false);
  Engine::check_raw_host(q.raw, q.m);
  if (!q.raw.device) {
    const size_t esz = q.raw.u16 ? sizeof(uint16_t) : sizeof(float);
    q.raw_bytes = q.raw.broadcast() ? esz : q.n() * esz;
  }
  if (!pointers) return q;
  if (!std::isfinite(prm->threshold)) throw std::invalid_argument("a non-finite threshold");
  if (prm->flags & ~(int)MVN_DETECT_MINIMA) throw std::invalid_argument("unknown flag bits " + std::to_string(prm->flags));
  q.threshold = prm->threshold, q.flags = prm->flags;
  q.table.assign(MVN_DETECT_TABLE, 0.f);
  for (int a = 0; a < 2; ++a)
    for (int k = 0; k < 3; ++k) {
      const double sigma = a == 0 ? prm->sigma1[k] : prm->sigma2[k];
      if (!(sigma >= 0.0 && sigma <= 10.0))
        throw std::invalid_argument("sigma" + std::to_string(a + 1) + "[" + std::to_string(k) +
                                    "] must be finite and in 0..10");
      q.R[a][k] = mvn_detect_make_taps(sigma, q.table.data() + (size_t)(a * 3 + k) * MVN_DETECT_TAPS);
    }
  return q;
}

// the device side of one detection: buffers, the tap table, and the launches in stream order
class Detection {
 public:
  // raw: the stack where the passes read it, in device memory (the caller's, or its temporary upload)
  Detection(const DetectRequest& q, const StackRef& raw, be::stream_t s)
      : q_(q),
        volumes_(4 * q.volume_bytes()),
        table_(q.table_bytes()),
        count_(sizeof(unsigned long long)),
        list_(q.list_bytes()),
        results_(q.result_bytes()) {
    std::memset(&p_, 0, sizeof(p_));
    p_.src = raw.ptr, p_.s0 = raw.stride[0], p_.s1 = raw.stride[1], p_.s2 = raw.stride[2];
    for (int k = 0; k < 3; ++k) p_.m[k] = q.m[k], p_.R[0][k] = q.R[0][k], p_.R[1][k] = q.R[1][k];
    p_.taps = table_.get();
    p_.a[0] = volumes_.get(), p_.a[1] = volumes_.get() + q.n();
    p_.b[0] = volumes_.get() + 2 * q.n(), p_.b[1] = volumes_.get() + 3 * q.n();
    p_.threshold = q.threshold, p_.minima = (q.flags & MVN_DETECT_MINIMA) ? 1 : 0;
    p_.count = count_.get(), p_.list = list_.get(), p_.list_cap = q.capacity;
    p_.pos = (double*)results_.get();  // positions, then voxels, then values: every block aligned to its type
    p_.vox = (int*)(p_.pos + 3 * (size_t)q.capacity);
    p_.val = (float*)(p_.vox + 3 * (size_t)q.capacity);
    u16_ = raw.u16;
    mvn_detect_check_blur(p_);
    be::h2d(table_.get(), q.table.data(), q.table_bytes(), s);
  }

  void blur(be::stream_t s) const { be::launch_detect_blur(p_, u16_, s); }
  void extrema(be::stream_t s) const {
    be::dzero(p_.count, sizeof(unsigned long long), s);
    be::launch_detect_extrema(p_, s);
  }
  // the candidates the extremum pass counted (it may be above the capacity: the list then holds some of them); blocks
  unsigned long long found(be::stream_t s) const {
    unsigned long long c = 0;
    be::d2h(&c, p_.count, sizeof(c), s);
    be::stream_sync(s);
    return c;
  }
  // the list in ascending raster order, whatever order the workgroups appended in; blocks
  void sort(long long nfound, be::stream_t s) const {
    std::vector<long long> h((size_t)nfound);
    be::d2h(h.data(), p_.list, h.size() * sizeof(long long), s);
    be::stream_sync(s);
    std::sort(h.begin(), h.end());
    be::h2d(p_.list, h.data(), h.size() * sizeof(long long), s);
    be::stream_sync(s);  // (h leaves scope)
  }
  void refine(long long nfound, be::stream_t s) const {
    DetectParams p = p_;
    p.nfound = nfound;
    be::launch_detect_refine(p, s);
  }
  // the results of nfound candidates into host vectors; blocks
  void download(long long nfound, std::vector<double>* pos, std::vector<float>* val, std::vector<int>* vox,
                be::stream_t s) const {
    pos->resize(3 * (size_t)nfound), val->resize((size_t)nfound), vox->resize(3 * (size_t)nfound);
    be::d2h(pos->data(), p_.pos, pos->size() * sizeof(double), s);
    be::d2h(val->data(), p_.val, val->size() * sizeof(float), s);
    be::d2h(vox->data(), p_.vox, vox->size() * sizeof(int), s);
    be::stream_sync(s);
  }
  const float* dog() const { return p_.a[0]; }

 private:
  const DetectRequest& q_;
  DetectParams p_;
  bool u16_ = false;
  be::DeviceBuffer<float> volumes_;  // a[0], a[1], b[0], b[1]; D is a[0]
  be::DeviceBuffer<float> table_;
  be::DeviceBuffer<unsigned long long> count_;
  be::DeviceBuffer<long long> list_;
  be::DeviceBuffer<char> results_;
};

// the device and the stream of a call on one described raw stack, as mvn_extract_psf picks them; `body` runs with the
// stack where the passes read it
template <typename F>
void on_raw_stack(int device, const StackRef& raw, const int* m, void* stream, F&& body) {
  int owner = -1;
  check_location(raw, "raw", &owner);
  if (owner >= 0 && device >= 0 && device != owner) throw std::invalid_argument("raw lives on another device");
  const int dev = pick_device(owner >= 0 ? owner : device);
  std::lock_guard<std::mutex> lk(device_mutex(dev));
  be::set_device(dev);
  be::DeviceBuffer<char> upload;
  const be::Event caller = be::Event::sync_only();
  const be::Stream own = be::Stream::create();
  const be::stream_t s = own.get();
  if (stream) {  // the caller's device stack is complete behind what its stream holds now
    be::event_record(caller.get(), (be::stream_t)stream);
    be::stream_wait_event(s, caller.get());
  }
  StackRef there = raw;
  if (!raw.device) Engine::upload_raw(raw, m, upload, &there, s);
  body(there, s);
}

std::atomic<long long> g_detections{0};
}  // namespace
}  // extern "C++"

int mvn_detect_beads(int device, const void* raw, const mvn_stack_desc* raw_desc, const int src_dims[3],
                     const mvn_detect_params* prm, int capacity, int* num_found, double* positions_out,
                     float* values_out, int* voxels_out, void* stream) {
  return guarded("mvn_detect_beads", [&] {
    if (!num_found || !positions_out) throw std::invalid_argument("null num_found or positions_out");
    const DetectRequest q = detect_request(raw, raw_desc, src_dims, prm, capacity, true);
    if (q.too_thin()) {  // (the location is still checked: a wrong descriptor is an error at any extents)
      int owner = -1;
      check_location(q.raw, "raw", &owner);
      *num_found = 0;
      ++g_detections;
      return;
    }
    on_raw_stack(device, q.raw, q.m, stream, [&](const StackRef& there, be::stream_t s) {
      const Detection d(q, there, s);
      d.blur(s);
      d.extrema(s);
      const unsigned long long found = d.found(s);
      if (found > (unsigned long long)q.capacity) {
        *num_found = found > 0x7fffffffull ? 0x7fffffff : (int)found;
        throw std::invalid_argument(std::to_string(found) + " candidates exceed the capacity of " +
                                    std::to_string(q.capacity));
      }
      std::vector<double> pos;
      std::vector<float> val;
      std::vector<int> vox;
      if (found > 0) {
        d.sort((long long)found, s);
        d.refine((long long)found, s);
        d.download((long long)found, &pos, &val, &vox, s);
      }
      *num_found = (int)found;
      if (found > 0) {
        std::memcpy(positions_out, pos.data(), pos.size() * sizeof(double));
        if (values_out) std::memcpy(values_out, val.data(), val.size() * sizeof(float));
        if (voxels_out) std::memcpy(voxels_out, vox.data(), vox.size() * sizeof(int));
      }
      ++g_detections;
    });
  });
}

int mvn_detect_taps(double sigma, float* taps, int capacity, int* radius) {
  return guarded("mvn_detect_taps", [&] {
    if (!taps || !radius) throw std::invalid_argument("null argument");
    float w[2 * MVN_DETECT_RMAX + 1];
    const int R = mvn_detect_make_taps(sigma, w);
    if (capacity < 2 * R + 1)
      throw std::invalid_argument("capacity " + std::to_string(capacity) + " is below the " + std::to_string(2 * R + 1) +
                                  " taps of this sigma");
    std::memcpy(taps, w, (size_t)(2 * R + 1) * sizeof(float));
    *radius = R;
  });
}

int mvn_detect_dog(int device, const void* raw, const mvn_stack_desc* raw_desc, const int src_dims[3],
                   const mvn_detect_params* prm, float* dog_out) {
  return guarded("mvn_detect_dog", [&] {
    if (!dog_out) throw std::invalid_argument("null dog_out");
    const DetectRequest q = detect_request(raw, raw_desc, src_dims, prm, 1, true);
    on_raw_stack(device, q.raw, q.m, nullptr, [&](const StackRef& there, be::stream_t s) {
      const Detection d(q, there, s);
      d.blur(s);
      std::vector<float> h(q.n());
      be::d2h(h.data(), d.dog(), h.size() * sizeof(float), s);
      be::stream_sync(s);
      std::memcpy(dog_out, h.data(), h.size() * sizeof(float));
    });
  });
}

int mvn_detect_memory(const mvn_stack_desc* raw_desc, const int src_dims[3], int capacity, int device, size_t* bytes) {
  return guarded("mvn_detect_memory", [&] {
    if (!bytes) throw std::invalid_argument("null bytes");
    *bytes = 0;
    (void)device;
    *bytes = detect_request(nullptr, raw_desc, src_dims, nullptr, capacity, false).bytes();
  });
}

int mvn_detect_counters(long long out[3]) {
  return guarded("mvn_detect_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    be::detect_counters(out);
    out[2] = g_detections.load();
  });
}

// ms[0]: the blur passes, the extremum pass and the fit of the candidates a first run found (at most 2^20, unsorted),
// per repetition over `reps` repetitions between two stream events behind one that warms up; ms[1]: the blur passes
// alone, likewise; ms[2]: a plain copy of one float32 volume of src_dims
int mvn_detect_time(int device, int u16, const int src_dims[3], const mvn_detect_params* prm, int reps, float* ms) {
  return guarded("mvn_detect_time", [&] {
    if (!src_dims || !prm || !ms) throw std::invalid_argument("null argument");
    if (reps < 1) throw std::invalid_argument("reps must be positive");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    for (int k = 0; k < 3; ++k)
      if (src_dims[k] < 1 || src_dims[k] > 0x3fffffff) throw std::invalid_argument("src_dims must be in 1..2^30 - 1");
    const size_t esz = u16 ? sizeof(uint16_t) : sizeof(float);
    const size_t n = (size_t)src_dims[0] * (size_t)src_dims[1] * (size_t)src_dims[2];
    const be::DeviceBuffer<> dr(n * esz);
    mvn_stack_desc desc;
    desc.dtype = u16 ? MVN_U16 : MVN_F32, desc.location = MVN_DEVICE;
    desc.stride[0] = (long long)src_dims[1] * src_dims[2], desc.stride[1] = src_dims[2], desc.stride[2] = 1;
    const DetectRequest q = detect_request(dr.get(), &desc, src_dims, prm, 1 << 20, true);
    const be::DeviceBuffer<float> cb(n * sizeof(float));
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    {  // an LCG's values: 100 .. 4195 with no period the tiles share
      std::vector<unsigned char> h(n * esz);
      unsigned x = 2463534242u;
      for (size_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        if (u16)
          ((uint16_t*)h.data())[i] = (uint16_t)(100u + (x >> 20));
        else
          ((float*)h.data())[i] = 100.f + (float)(x >> 20);
      }
      be::h2d(dr.get(), h.data(), h.size(), s);
      be::stream_sync(s);
    }
    const Detection d(q, q.raw, s);
    d.blur(s);
    unsigned long long found = 0;
    if (!q.too_thin()) {
      d.extrema(s);
      found = d.found(s);
      if (found > (unsigned long long)q.capacity) found = (unsigned long long)q.capacity;
    }
    ms[0] = time_on_stream(s, reps, [&] {
      d.blur(s);
      if (!q.too_thin()) d.extrema(s);
      if (found > 0) d.refine((long long)found, s);
    });
    ms[1] = time_on_stream(s, reps, [&] { d.blur(s); });
    be::stream_sync(s);
    const long row = src_dims[2], plane = (long)src_dims[1] * src_dims[2];
    ms[2] = time_on_stream(s, reps, [&] {
      be::launch_copy3d(cb.get(), row, plane, d.dog(), row, plane, src_dims[2], src_dims[1], src_dims[0], s);
    });
  });
}

// ---- bead registration (mvn_register.hpp; the arithmetic is stated at mvn_register_beads in include/mvn_engine_api.h) ----
extern "C++" {
namespace {
static_assert(MVN_REGISTER_NEIGHBOURS == MVN_REG_NN, "the neighbours of the header are the passes'");
static_assert(MVN_REGISTER_MAX_BEADS == MVN_REG_MAX_BEADS, "the largest set of the header is the passes'");
static_assert(MVN_REGISTER_MAX_HYPOTHESES == MVN_REG_MAX_HYPOTHESES, "the hypotheses of the header are the passes'");

void register_check_count(int n, const char* name) {
  if (n < MVN_REG_NN + 1 || n > MVN_REGISTER_MAX_BEADS)
    throw std::invalid_argument(std::string(name) + " must be in 5.." + std::to_string(MVN_REGISTER_MAX_BEADS));
}

void register_check_points(const double* p, int n, const char* name) {
  if (!p) throw std::invalid_argument(std::string("null ") + name);
  register_check_count(n, (std::string("num_") + name).c_str());
  for (size_t i = 0; i < 3 * (size_t)n; ++i)
    if (!std::isfinite(p[i])) throw std::invalid_argument(std::string("a non-finite coordinate in ") + name);
}

void register_check_params(const mvn_register_params* prm) {
  if (!prm) throw std::invalid_argument("null prm");
  if (prm->flags & ~(int)MVN_REGISTER_PRIOR) throw std::invalid_argument("unknown flag bits " + std::to_string(prm->flags));
  if (prm->flags & MVN_REGISTER_PRIOR)
    for (int k = 0; k < 12; ++k)
      if (!std::isfinite(prm->prior[k])) throw std::invalid_argument("a non-finite prior entry");
  if (!(std::isfinite(prm->max_error) && prm->max_error > 0.0)) throw std::invalid_argument("max_error must be finite and > 0");
  if (!(std::isfinite(prm->ratio) && prm->ratio >= 1.0f)) throw std::invalid_argument("ratio must be finite and >= 1");
  if (prm->hypotheses < 1 || prm->hypotheses > MVN_REGISTER_MAX_HYPOTHESES)
    throw std::invalid_argument("hypotheses must be in 1.." + std::to_string(MVN_REGISTER_MAX_HYPOTHESES));
  if (prm->min_inliers < 4) throw std::invalid_argument("min_inliers must be >= 4");
}

// step 1: a' = T (a; 1) under the flag
std::vector<double> register_prior(const double* a, int n, const mvn_register_params* prm) {
  MVN_FP_EXACT
  std::vector<double> out(a, a + 3 * (size_t)n);
  if (!(prm->flags & MVN_REGISTER_PRIOR)) return out;
  const double* T = prm->prior;
  for (int i = 0; i < n; ++i) {
    const double z = a[3 * (size_t)i], y = a[3 * (size_t)i + 1], x = a[3 * (size_t)i + 2];
    for (int k = 0; k < 3; ++k) out[3 * (size_t)i + k] = ((T[4 * k] * z + T[4 * k + 1] * y) + T[4 * k + 2] * x) + T[4 * k + 3];
  }
  return out;
}

struct RegisterSizes {
  int na, nb, chunk, chunks, cap;
  RegisterSizes(int num_a, int num_b)
      : na(num_a), nb(num_b), chunk(mvn_reg_chunk(num_a, num_b)), chunks(mvn_reg_chunks(num_b, chunk)),
        cap(num_a < num_b ? num_a : num_b) {}
  size_t n() const { return (size_t)na + (size_t)nb; }
  size_t points_bytes() const { return n() * 3 * sizeof(double); }
  size_t nn_bytes() const { return n() * MVN_REG_NN * sizeof(int); }
  size_t desc_bytes() const { return n() * MVN_REG_DESC * sizeof(float); }
  size_t match_bytes() const { return (size_t)na * ((size_t)chunks + 1) * (2 * sizeof(float) + sizeof(int)); }
  size_t cand_bytes() const { return (size_t)cap * 6 * sizeof(double); }
  size_t bytes() const {
    return points_bytes() + nn_bytes() + desc_bytes() + match_bytes() + cand_bytes() + sizeof(unsigned long long);
  }
};

struct RegisterCandidate {
  int i, j;
  float d1, d2;
};

// the device side of one registration: buffers and the launches in stream order.  A's points are a' (step 1)
class Registration {
 public:
  Registration(int na, int nb)
      : z_(na, nb),
        points_(z_.points_bytes()),
        nn_(z_.nn_bytes()),
        desc_(z_.desc_bytes()),
        match_(z_.match_bytes()),
        cand_(z_.cand_bytes()),
        best_(sizeof(unsigned long long)) {}

  void upload(const double* a_prior, const double* b, be::stream_t s) const {
    be::h2d(points_.get(), a_prior, (size_t)z_.na * 3 * sizeof(double), s);
    be::h2d(points_.get() + 3 * (size_t)z_.na, b, (size_t)z_.nb * 3 * sizeof(double), s);
  }
  // steps 2 and 3 of set 0 (A) or 1 (B)
  void neighbours(int set, be::stream_t s) const {
    const size_t at = set ? (size_t)z_.na : 0;
    RegParams p;
    std::memset(&p, 0, sizeof(p));
    p.pts = points_.get() + 3 * at, p.n = set ? z_.nb : z_.na;
    p.nn = nn_.get() + MVN_REG_NN * at, p.desc = desc_.get() + MVN_REG_DESC * at;
    be::launch_register_neighbours(p, s);
  }
  void match(be::stream_t s) const { be::launch_register_match(match_params(), s); }
  void download_neighbours(int set, int* out, be::stream_t s) const {
    const size_t at = set ? (size_t)z_.na : 0;
    be::d2h(out, nn_.get() + MVN_REG_NN * at, (size_t)(set ? z_.nb : z_.na) * MVN_REG_NN * sizeof(int), s);
    be::stream_sync(s);
  }
  // step 4 behind the match pass: the ratio test and the uniqueness filter, on the host; blocks
  std::vector<RegisterCandidate> candidates(float ratio, be::stream_t s) const {
    MVN_FP_EXACT
    const size_t na = (size_t)z_.na;
    std::vector<float> d1(na), d2(na);
    std::vector<int> j1(na);
    const RegParams p = match_params();
    be::d2h(d1.data(), p.d1, na * sizeof(float), s);
    be::d2h(j1.data(), p.j1, na * sizeof(int), s);
    be::d2h(d2.data(), p.d2, na * sizeof(float), s);
    be::stream_sync(s);
    std::vector<int> claims((size_t)z_.nb, 0);
    std::vector<char> passes(na, 0);
    for (size_t i = 0; i < na; ++i) {
      const float scaled = d1[i] * ratio;
      if (!(scaled < d2[i])) continue;
      if (j1[i] < 0 || j1[i] >= z_.nb) throw std::runtime_error("mvn: register: a match outside B");
      passes[i] = 1;
      ++claims[(size_t)j1[i]];
    }
    std::vector<RegisterCandidate> out;
    for (size_t i = 0; i < na; ++i)
      if (passes[i] && claims[(size_t)j1[i]] == 1) out.push_back(RegisterCandidate{(int)i, j1[i], d1[i], d2[i]});
    return out;
  }
  // step 6 over `nc` records of (a, b); returns the best key; blocks
  unsigned long long ransac(const double* records, int nc, int hyps, unsigned long long seed, double maxerr2,
                            be::stream_t s) const {
    upload_records(records, nc, s);
    launch_ransac(nc, hyps, seed, maxerr2, s);
    unsigned long long key = 0;
    be::d2h(&key, best_.get(), sizeof(key), s);
    be::stream_sync(s);
    return key;
  }
  void launch_ransac(int nc, int hyps, unsigned long long seed, double maxerr2, be::stream_t s) const {
    if (nc > z_.cap) throw std::invalid_argument("mvn: register: more candidates than beads");
    RegParams p;
    std::memset(&p, 0, sizeof(p));
    p.cand = cand_.get(), p.nc = nc, p.hyps = hyps, p.seed = seed, p.maxerr2 = maxerr2, p.best = best_.get();
    be::dzero(best_.get(), sizeof(unsigned long long), s);
    be::launch_register_ransac(p, s);
  }
  void upload_records(const double* records, int nc, be::stream_t s) const {
    be::h2d(cand_.get(), records, (size_t)nc * 6 * sizeof(double), s);
  }
  const RegisterSizes& sizes() const { return z_; }

 private:
  // the match pass and its fold: the chunks' records, then the folded ones, for each of d1, j1, d2
  RegParams match_params() const {
    RegParams p;
    std::memset(&p, 0, sizeof(p));
    p.da = desc_.get(), p.db = desc_.get() + MVN_REG_DESC * (size_t)z_.na;
    p.na = z_.na, p.nb = z_.nb, p.chunk = z_.chunk;
    const size_t part = (size_t)z_.na * (size_t)z_.chunks;
    p.pd1 = match_.get(), p.d1 = p.pd1 + part;
    p.pj1 = (int*)(p.d1 + z_.na), p.j1 = p.pj1 + part;
    p.pd2 = (float*)(p.j1 + z_.na), p.d2 = p.pd2 + part;
    return p;
  }

  RegisterSizes z_;
  be::DeviceBuffer<double> points_;  // a', then b
  be::DeviceBuffer<int> nn_;
  be::DeviceBuffer<float> desc_;
  be::DeviceBuffer<float> match_;
  be::DeviceBuffer<double> cand_;
  be::DeviceBuffer<unsigned long long> best_;
};

// the candidates of step 4 as records (a, b) on the ORIGINAL a
std::vector<double> register_records(const std::vector<RegisterCandidate>& c, const double* a, const double* b) {
  std::vector<double> r(6 * c.size());
  for (size_t m = 0; m < c.size(); ++m)
    for (int k = 0; k < 3; ++k) {
      r[6 * m + k] = a[3 * (size_t)c[m].i + k];
      r[6 * m + 3 + k] = b[3 * (size_t)c[m].j + k];
    }
  return r;
}

std::vector<int> register_inliers(const std::vector<double>& rec, const double L[9], const double t[3], double maxerr2) {
  std::vector<int> in;
  for (size_t m = 0; m < rec.size() / 6; ++m)
    if (mvn_reg_residual2(L, t, &rec[6 * m], &rec[6 * m + 3]) <= maxerr2) in.push_back((int)m);
  return in;
}

// step 7 on the inliers `in` of the best hypothesis; false: no model
bool register_refit(const std::vector<double>& rec, std::vector<int>& in, int min_inliers, double maxerr2, double L[9],
                    double t[3]) {
  MVN_FP_EXACT
  for (int r = 1; r <= MVN_REGISTER_REFITS; ++r) {
    double ca[3], cb[3];
    for (int k = 0; k < 3; ++k) {
      double sa = rec[6 * (size_t)in[0] + k], sb = rec[6 * (size_t)in[0] + 3 + k];
      for (size_t m = 1; m < in.size(); ++m) sa = sa + rec[6 * (size_t)in[m] + k], sb = sb + rec[6 * (size_t)in[m] + 3 + k];
      ca[k] = sa / (double)in.size(), cb[k] = sb / (double)in.size();
    }
    double Saa[9], Sba[9];
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) {
        double saa = 0.0, sba = 0.0;
        for (size_t m = 0; m < in.size(); ++m) {
          const double* q = &rec[6 * (size_t)in[m]];
          const double al = q[l] - ca[l];
          const double paa = (q[k] - ca[k]) * al, pba = (q[3 + k] - cb[k]) * al;
          saa = m == 0 ? paa : saa + paa;
          sba = m == 0 ? pba : sba + pba;
        }
        Saa[3 * k + l] = saa, Sba[3 * k + l] = sba;
      }
    if (!mvn_reg_solve(Saa, Sba, L) || !mvn_reg_offset(L, ca, cb, t)) return false;
    std::vector<int> next = register_inliers(rec, L, t, maxerr2);
    if ((int)next.size() < min_inliers) return false;
    const bool same = next == in;
    in.swap(next);
    if (same) break;
  }
  return true;
}

// `body` with the device of a call on host lists picked, locked and current
template <typename F>
void on_register_device(int device, F&& body) {
  const int dev = pick_device(device);
  std::lock_guard<std::mutex> lk(device_mutex(dev));
  be::set_device(dev);
  body();
}

std::atomic<long long> g_registrations{0};
}  // namespace
}  // extern "C++"

int mvn_register_beads(int device, const double* a, int num_a, const double* b, int num_b,
                       const mvn_register_params* prm, double matrix_out[12], int* num_candidates, int* num_inliers,
                       int* pairs_out, double* errors_out, void* stream) {
  return guarded("mvn_register_beads", [&] {
    MVN_FP_EXACT
    (void)stream;  // (the lists are host memory: there is nothing to wait for)
    if (!matrix_out || !num_candidates || !num_inliers) throw std::invalid_argument("null matrix_out, num_candidates or num_inliers");
    register_check_points(a, num_a, "a");
    register_check_points(b, num_b, "b");
    register_check_params(prm);
    on_register_device(device, [&] {
      const std::vector<double> ap = register_prior(a, num_a, prm);
      std::vector<RegisterCandidate> cand;
      std::vector<double> rec;
      std::vector<int> in;
      double L[9], t[3];
      bool model = false;
      const double maxerr2 = prm->max_error * prm->max_error;
      {
        const Registration reg(num_a, num_b);
        const be::Stream own = be::Stream::create();
        const be::stream_t s = own.get();
        reg.upload(ap.data(), b, s);
        reg.neighbours(0, s);
        reg.neighbours(1, s);
        reg.match(s);
        cand = reg.candidates(prm->ratio, s);
        if (cand.size() >= 4) {
          rec = register_records(cand, a, b);
          const unsigned long long key = reg.ransac(rec.data(), (int)cand.size(), prm->hypotheses, prm->seed, maxerr2, s);
          const int score = mvn_reg_key_score(key);
          if (score >= prm->min_inliers) {
            if (!mvn_reg_hypothesis(rec.data(), (int)cand.size(), prm->seed, mvn_reg_key_h(key), L, t))
              throw std::runtime_error("mvn: register: the best hypothesis has no model on the host");
            in = register_inliers(rec, L, t, maxerr2);
            if ((int)in.size() != score) throw std::runtime_error("mvn: register: the host and the device disagree on a score");
            model = register_refit(rec, in, prm->min_inliers, maxerr2, L, t);
          }
        }
      }
      *num_candidates = (int)cand.size();
      if (!model) {
        *num_inliers = 0;
        ++g_registrations;
        return;
      }
      double sum = 0.0, worst = 0.0;
      for (size_t m = 0; m < in.size(); ++m) {
        const double e = std::sqrt(mvn_reg_residual2(L, t, &rec[6 * (size_t)in[m]], &rec[6 * (size_t)in[m] + 3]));
        sum = m == 0 ? e : sum + e;
        worst = e > worst ? e : worst;
      }
      for (int k = 0; k < 3; ++k) {
        for (int l = 0; l < 3; ++l) matrix_out[4 * k + l] = L[3 * k + l];
        matrix_out[4 * k + 3] = t[k];
      }
      *num_inliers = (int)in.size();
      if (pairs_out)
        for (size_t m = 0; m < in.size(); ++m) pairs_out[2 * m] = cand[(size_t)in[m]].i, pairs_out[2 * m + 1] = cand[(size_t)in[m]].j;
      if (errors_out) errors_out[0] = sum / (double)in.size(), errors_out[1] = worst;
      ++g_registrations;
    });
  });
}

int mvn_register_neighbours(int device, const double* p, int n, int* idx_out) {
  return guarded("mvn_register_neighbours", [&] {
    if (!idx_out) throw std::invalid_argument("null idx_out");
    register_check_points(p, n, "p");
    on_register_device(device, [&] {
      std::vector<int> h((size_t)n * MVN_REG_NN);
      {
        const Registration reg(n, n);
        const be::Stream own = be::Stream::create();
        const be::stream_t s = own.get();
        reg.upload(p, p, s);
        reg.neighbours(0, s);
        reg.download_neighbours(0, h.data(), s);
      }
      std::memcpy(idx_out, h.data(), h.size() * sizeof(int));
    });
  });
}

int mvn_register_candidates(int device, const double* a, int num_a, const double* b, int num_b,
                            const mvn_register_params* prm, int* num, int* pairs_out, float* d_out) {
  return guarded("mvn_register_candidates", [&] {
    if (!num || !pairs_out || !d_out) throw std::invalid_argument("null num, pairs_out or d_out");
    register_check_points(a, num_a, "a");
    register_check_points(b, num_b, "b");
    register_check_params(prm);
    on_register_device(device, [&] {
      const std::vector<double> ap = register_prior(a, num_a, prm);
      std::vector<RegisterCandidate> cand;
      {
        const Registration reg(num_a, num_b);
        const be::Stream own = be::Stream::create();
        const be::stream_t s = own.get();
        reg.upload(ap.data(), b, s);
        reg.neighbours(0, s);
        reg.neighbours(1, s);
        reg.match(s);
        cand = reg.candidates(prm->ratio, s);
      }
      *num = (int)cand.size();
      for (size_t m = 0; m < cand.size(); ++m) {
        pairs_out[2 * m] = cand[m].i, pairs_out[2 * m + 1] = cand[m].j;
        d_out[2 * m] = cand[m].d1, d_out[2 * m + 1] = cand[m].d2;
      }
    });
  });
}

int mvn_register_sample(unsigned long long seed, int h, int n, int out[4]) {
  return guarded("mvn_register_sample", [&] {
    if (!out) throw std::invalid_argument("null out");
    if (n < 4) throw std::invalid_argument("n must be >= 4");
    if (h < 0 || h >= MVN_REGISTER_MAX_HYPOTHESES) throw std::invalid_argument("h out of range");
    int s[4];
    mvn_reg_sample(seed, (unsigned)h, n, s);
    std::memcpy(out, s, sizeof(s));
  });
}

int mvn_register_memory(int num_a, int num_b, int hypotheses, size_t* bytes) {
  return guarded("mvn_register_memory", [&] {
    if (!bytes) throw std::invalid_argument("null bytes");
    register_check_count(num_a, "num_a");
    register_check_count(num_b, "num_b");
    if (hypotheses < 1 || hypotheses > MVN_REGISTER_MAX_HYPOTHESES)
      throw std::invalid_argument("hypotheses must be in 1.." + std::to_string(MVN_REGISTER_MAX_HYPOTHESES));
    *bytes = RegisterSizes(num_a, num_b).bytes();
  });
}

int mvn_register_counters(long long out[3]) {
  return guarded("mvn_register_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    be::register_counters(out);
    out[2] = g_registrations.load();
  });
}

// ms[0]: the neighbour and descriptor pass of both sets; ms[1]: the match pass and its fold; ms[2]: the RANSAC pass over
// min(num_a, num_b) records (pair i with i); each per repetition over `reps` repetitions behind one that warms up
int mvn_register_time(int device, int num_a, int num_b, int hypotheses, int reps, float* ms) {
  return guarded("mvn_register_time", [&] {
    if (!ms) throw std::invalid_argument("null ms");
    if (reps < 1) throw std::invalid_argument("reps must be positive");
    register_check_count(num_a, "num_a");
    register_check_count(num_b, "num_b");
    if (hypotheses < 1 || hypotheses > MVN_REGISTER_MAX_HYPOTHESES)
      throw std::invalid_argument("hypotheses must be in 1.." + std::to_string(MVN_REGISTER_MAX_HYPOTHESES));
    on_register_device(device, [&] {
      // an LCG's points in a box of 100 x 1000 x 1000; B: the same under a small affine map
      std::vector<double> a(3 * (size_t)num_a), b(3 * (size_t)num_b);
      unsigned x = 2463534242u;
      for (size_t i = 0; i < a.size(); ++i) {
        x = x * 1664525u + 1013904223u;
        a[i] = (double)(x >> 8) * (1.0 / 16777216.0) * (i % 3 == 0 ? 100.0 : 1000.0);
      }
      for (int j = 0; j < num_b; ++j) {
        const double* q = &a[3 * (size_t)(j % num_a)];
        b[3 * (size_t)j] = 1.01 * q[0] + 0.02 * q[1] + 1.5;
        b[3 * (size_t)j + 1] = 0.99 * q[1] - 0.02 * q[0] - 2.0;
        b[3 * (size_t)j + 2] = 1.005 * q[2] + 3.0;
      }
      const Registration reg(num_a, num_b);
      const int nc = reg.sizes().cap;
      std::vector<double> rec(6 * (size_t)nc);
      for (int m = 0; m < nc; ++m)
        for (int k = 0; k < 3; ++k) rec[6 * (size_t)m + k] = a[3 * (size_t)m + k], rec[6 * (size_t)m + 3 + k] = b[3 * (size_t)m + k];
      const be::Stream own = be::Stream::create();
      const be::stream_t s = own.get();
      reg.upload(a.data(), b.data(), s);
      reg.upload_records(rec.data(), nc, s);
      be::stream_sync(s);
      ms[0] = time_on_stream(s, reps, [&] {
        reg.neighbours(0, s);
        reg.neighbours(1, s);
      });
      ms[1] = time_on_stream(s, reps, [&] { reg.match(s); });
      ms[2] = time_on_stream(s, reps, [&] { reg.launch_ransac(nc, hypotheses, 1ull, 0.25, s); });
      be::stream_sync(s);
    });
  });
}

// what a fusion call is made of, everything checked that can be without its pointers (raw == NULL: a memory query)
extern "C++" {
namespace {
struct FuseCall {
  int dims[3];
  StackRef out;
  std::vector<ResampleGeom> geom;
  std::vector<StackRef> raw;
  size_t out_bytes = 0;  // the dense device volume of an output in host memory
  size_t raw_bytes = 0;  // the uploads of the raw stacks in host memory, all V at once
  size_t table_bytes = 0;
  size_t bytes() const { return out_bytes + raw_bytes + table_bytes; }
};
}  // namespace
static FuseCall fuse_call(const void* out, const mvn_stack_desc* out_desc, const int* out_dims, int num_views,
                          const void* const* raw, const mvn_stack_desc* raw_desc, const mvn_view_geometry* geom,
                          float fill, bool pointers) {
  static const int placeholder = 0;  // (a memory query brings no pointers: nothing is read through this one)
  if (!out_dims) throw std::invalid_argument("null out_dims");
  if (num_views < 1) throw std::invalid_argument("num_views must be >= 1");
  if (!geom) throw std::invalid_argument("null geom");
  if (pointers && !raw) throw std::invalid_argument("null raw");
  if (!std::isfinite(fill)) throw std::invalid_argument("fill must be finite");
  FuseCall c;
  for (int d = 0; d < 3; ++d) {
    if (out_dims[d] < 1) throw std::invalid_argument("extents must be positive");
    c.dims[d] = out_dims[d];
  }
  c.out = described_stack(pointers ? out : &placeholder, out_desc, c.dims, "out", true, true);
  const size_t voxels = (size_t)c.dims[0] * (size_t)c.dims[1] * (size_t)c.dims[2];
  if (!c.out.device) {
    if ((c.dims[2] > 1 && c.out.stride[2] != 1) || (c.dims[1] > 1 && c.out.stride[1] < c.dims[2]))
      throw std::invalid_argument("out: a stack in host memory needs contiguous rows that do not overlap");
    c.out_bytes = voxels * (c.out.u16 ? sizeof(uint16_t) : sizeof(float));
  }
  c.table_bytes = (size_t)num_views * sizeof(FuseView);
  c.geom.reserve((size_t)num_views);
  for (int v = 0; v < num_views; ++v) c.geom.push_back(checked_geometry(geom + v, "geom " + std::to_string(v)));
  for (int v = 0; v < num_views; ++v) {
    const ResampleGeom& g = c.geom[(size_t)v];
    StackRef r = described_stack(pointers ? raw[v] : &placeholder, raw_desc ? raw_desc + v : nullptr, g.m,
                                 "raw " + std::to_string(v), true, false);
    r.geom = &g;
    Engine::check_raw_host(r, g.m);
    if (!r.device) {
      const size_t esz = r.u16 ? sizeof(uint16_t) : sizeof(float);
      c.raw_bytes += r.broadcast() ? esz : (size_t)g.m[0] * (size_t)g.m[1] * (size_t)g.m[2] * esz;
    }
    c.raw.push_back(r);
  }
  return c;
}
}  // extern "C++"

int mvn_fuse_memory_resampled(const mvn_stack_desc* out_desc, const int out_dims[3], int num_views,
                              const mvn_stack_desc* raw_desc, const mvn_view_geometry* geom, int device, size_t* bytes) {
  return guarded("mvn_fuse_memory_resampled", [&] {
    if (!bytes) throw std::invalid_argument("null bytes");
    *bytes = 0;
    (void)device;
    *bytes = fuse_call(nullptr, out_desc, out_dims, num_views, nullptr, raw_desc, geom, 0.f, false).bytes();
  });
}

int mvn_fuse_resampled(void* out, const mvn_stack_desc* out_desc, const int out_dims[3], int num_views,
                       const void* const* raw, const mvn_stack_desc* raw_desc, const mvn_view_geometry* geom, float fill,
                       void* stream, int device) {
  return guarded("mvn_fuse_resampled", [&] {
    const FuseCall c = fuse_call(out, out_desc, out_dims, num_views, raw, raw_desc, geom, fill, true);
    const int V = num_views;
    int owner = -1;
    check_location(c.out, "out", &owner);
    for (int v = 0; v < V; ++v) check_location(c.raw[(size_t)v], "raw " + std::to_string(v), &owner);
    if (owner >= 0 && device >= 0 && device != owner)
      throw std::invalid_argument("the stacks live on device " + std::to_string(owner) + ", not on device " +
                                  std::to_string(device));
    const int dev = pick_device(owner >= 0 ? owner : device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const int* n = c.dims;
    const size_t esz = c.out.u16 ? sizeof(uint16_t) : sizeof(float);
    std::vector<be::DeviceBuffer<char>> uploads((size_t)V);
    be::DeviceBuffer<char> dout;
    if (c.out_bytes) dout = be::DeviceBuffer<char>(c.out_bytes);
    const be::DeviceBuffer<FuseView> table(c.table_bytes);
    std::vector<FuseView> records((size_t)V);
    const be::Event caller = be::Event::sync_only();
    const be::Stream own = be::Stream::create();
    const be::stream_t s = own.get();
    if (stream) {  // the caller's device stacks are complete behind what its stream holds now
      be::event_record(caller.get(), (be::stream_t)stream);
      be::stream_wait_event(s, caller.get());
    }
    for (int v = 0; v < V; ++v) {
      StackRef r = c.raw[(size_t)v];
      if (!r.device) Engine::upload_raw(c.raw[(size_t)v], c.geom[(size_t)v].m, uploads[(size_t)v], &r, s);
      FuseView& f = records[(size_t)v];
      std::memset(&f, 0, sizeof(f));
      f.src = r.ptr, f.s0 = r.stride[0], f.s1 = r.stride[1], f.s2 = r.stride[2];
      f.u16 = r.u16 ? 1 : 0;
      f.g = c.geom[(size_t)v];
    }
    be::h2d(table.get(), records.data(), c.table_bytes, s);
    FuseParams p;
    p.out_u16 = c.out.u16 ? 1 : 0;
    p.n0 = n[0], p.n1 = n[1], p.n2 = n[2];
    p.views = table.get(), p.V = V, p.fill = fill;
    if (c.out.device) {  // written where it lies
      p.out = (void*)c.out.ptr, p.q0 = c.out.stride[0], p.q1 = c.out.stride[1], p.q2 = c.out.stride[2];
    } else {
      p.out = dout.get(), p.q0 = (long long)n[1] * n[2], p.q1 = n[2], p.q2 = 1;
    }
    for (int d = 0; d < 3; ++d)  // (an extent of 1 makes no use of its stride)
      if (n[d] == 1) (d == 0 ? p.q0 : d == 1 ? p.q1 : p.q2) = 1;
    be::launch_fuse_resampled(p, s);
    if (!c.out.device) {
      const size_t width = (size_t)n[2] * esz;
      const size_t pitch = n[1] == 1 ? width : (size_t)c.out.stride[1] * esz;
      for (int z = 0; z < n[0]; ++z)
        be::d2h_2d((char*)out + (long long)z * c.out.stride[0] * (long long)esz, pitch,
                   dout.get() + (size_t)z * n[1] * width, width, width, (size_t)n[1], s);
    }
    be::stream_sync(s);
  });
}

// ms[0]: the fusion from V resident raw stacks of geom[v].src_dims (uint16, or float32) into a resident float32 volume
// of extents out_dims, per pass over `reps` passes between two stream events (one more pass warms up: the from-raw
// counter moves by reps + 1); ms[1]: V launches of the resample pass on the same stacks and geometries, image and
// weights volumes written, likewise; ms[2]: a plain copy of one volume
int mvn_fuse_time(int device, int u16, int num_views, const mvn_view_geometry* geom, const int out_dims[3], int reps,
                  float* ms) {
  return guarded("mvn_fuse_time", [&] {
    if (!out_dims || !ms || !geom) throw std::invalid_argument("null argument");
    if (out_dims[0] < 1 || out_dims[1] < 1 || out_dims[2] < 1 || reps < 1 || num_views < 1)
      throw std::invalid_argument("extents, reps and num_views must be positive");
    const int V = num_views;
    std::vector<ResampleGeom> g;
    for (int v = 0; v < V; ++v) g.push_back(checked_geometry(geom + v, "geom " + std::to_string(v)));
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const Layout L(out_dims[0], out_dims[1], out_dims[2]);
    const size_t bytes = L.real_floats() * sizeof(float);
    const size_t esz = u16 ? sizeof(uint16_t) : sizeof(float);
    const be::DeviceBuffer<float> di(bytes), dw(bytes);
    std::vector<be::DeviceBuffer<>> dr;
    const be::DeviceBuffer<FuseView> table((size_t)V * sizeof(FuseView));
    std::vector<FuseView> records((size_t)V);
    std::vector<unsigned char> h;
    for (int v = 0; v < V; ++v) dr.emplace_back((size_t)g[(size_t)v].m[0] * g[(size_t)v].m[1] * g[(size_t)v].m[2] * esz);
    const be::Stream st = be::Stream::create();
    const be::stream_t s = st.get();
    for (int v = 0; v < V; ++v) {
      const int* m = g[(size_t)v].m;
      const size_t raw = (size_t)m[0] * (size_t)m[1] * (size_t)m[2];
      h.resize(raw * esz);
      if (u16)
        for (size_t i = 0; i < raw; ++i) ((uint16_t*)h.data())[i] = (uint16_t)(100u + (i + 977u * (unsigned)v) % 4001u);
      else
        for (size_t i = 0; i < raw; ++i) ((float*)h.data())[i] = 100.f + (float)((i + 977u * (unsigned)v) % 4001u);
      be::h2d(dr[(size_t)v].get(), h.data(), h.size(), s);
      be::stream_sync(s);  // (h is filled again)
      FuseView& f = records[(size_t)v];
      std::memset(&f, 0, sizeof(f));
      f.src = dr[(size_t)v].get(), f.s0 = (long long)m[1] * m[2], f.s1 = m[2], f.s2 = 1;
      f.u16 = u16 ? 1 : 0;
      f.g = g[(size_t)v];
    }
    be::h2d(table.get(), records.data(), records.size() * sizeof(FuseView), s);
    be::dzero(di.get(), bytes, s);
    be::dzero(dw.get(), bytes, s);
    be::stream_sync(s);
    FuseParams p;
    p.out = di.get(), p.out_u16 = 0, p.q0 = (long long)L.d1 * L.RP, p.q1 = L.RP, p.q2 = 1;
    p.n0 = L.d0, p.n1 = L.d1, p.n2 = L.d2;
    p.views = table.get(), p.V = V, p.fill = 0.f;
    ms[0] = time_on_stream(s, reps, [&] { be::launch_fuse_resampled(p, s); });
    ms[1] = time_on_stream(s, reps, [&] {
      for (int v = 0; v < V; ++v) {
        ResampleParams r = resample_alone(L, di.get(), dw.get());
        const FuseView& f = records[(size_t)v];
        r.src = f.src, r.s0 = f.s0, r.s1 = f.s1, r.s2 = f.s2;
        r.g = f.g;
        be::launch_resample(r, u16 != 0, s);
      }
    });
    const long plane = (long)L.d1 * L.RP;
    ms[2] = time_on_stream(
        s, reps, [&] { be::launch_copy3d(dw.get(), L.RP, plane, di.get(), L.RP, plane, (int)L.RP, L.d1, L.d0, s); });
  });
}

int mvn_set_pad_mode(const char* mode) {
  return guarded("mvn_set_pad_mode", [&] { g_pad_mode.store(parse_pad_mode(mode)); });
}

const char* mvn_get_pad_mode(void) {
  switch (g_pad_mode.load()) {
    case MVN_PAD_ZERO: return "zero";
    case MVN_PAD_ZERO_EXACT: return "zero_exact";
    case MVN_PAD_NONE: return "none";
    case MVN_PAD_REFLECT: return "reflect";
    default: return "";
  }
}

int mvn_set_memory_mode(const char* mode) {
  return guarded("mvn_set_memory_mode", [&] { g_mem_mode.store(parse_memory_mode(mode)); });
}

const char* mvn_get_memory_mode(void) {
  static thread_local std::string name;
  const int m = g_mem_mode.load();
  switch (m) {
    case MVN_MEM_UNSET: return "";
    case MVN_MEM_RESIDENT: return "resident";
    case MVN_MEM_AUTO: return "auto";
    case MVN_MEM_STREAM: return "stream";
    default:
      name = "stream:" + std::to_string(m - MVN_MEM_STREAM - 1);
      return name.c_str();
  }
}

int mvn_set_memory_budget(long long bytes) {
  return guarded("mvn_set_memory_budget", [&] { g_mem_budget.store(bytes > 0 ? bytes : -1); });
}

// desc: the descriptors of a described call (their pointers are not looked at), or null
static void deconvolve_memory(struct workspace input, const mvn_call_desc* desc, int device, int streamed_views,
                              size_t* bytes) {
  if (!bytes) throw std::invalid_argument("null bytes");
  *bytes = 0;
  if (!input.data_ || input.num_views_ < 1) throw std::invalid_argument("no views");
  for (int v = 0; v < input.num_views_; ++v) {
    const view_data& d = input.data_[v];
    if (!d.image_dims_ || !d.kernel1_dims_ || !d.kernel2_dims_)
      throw std::invalid_argument("view " + std::to_string(v) + " has null dims");
  }
  if (streamed_views < 0 || streamed_views > input.num_views_)
    throw std::invalid_argument("streamed_views must be in [0, num_views_]");
  std::vector<char> keep;
  const int storage = g_image_storage.load();
  if (desc && desc->image && storage == 1)
    for (int v = 0; v < input.num_views_; ++v) {
      const mvn_stack_desc& d = desc->image[v];
      keep.push_back(d.dtype == MVN_U16 && (d.stride[0] != 0 || d.stride[1] != 0 || d.stride[2] != 0) ? 1 : 0);
    }
  const int dev = pick_device(device);
  shape_t dims, ext;
  int off[3];
  call_extents(input, current_pad_mode(), dev, &dims, &ext, off);
  // (outside a call: the process-wide switches, whatever calls other threads are running)
  MemoryQuery q = memory_query(ext, input, current_loop(), embed_floats_of(dims, ext), keep);
  q.streamed = streamed_views;
  q.ring = streamed_views > 0 ? 2 : 0;
  *bytes = Engine::memory_need(q, call_rule(ext, dev));
}

int mvn_deconvolve_memory(struct workspace input, int device, int streamed_views, size_t* bytes) {
  return guarded("mvn_deconvolve_memory", [&] { deconvolve_memory(input, nullptr, device, streamed_views, bytes); });
}

int mvn_deconvolve_memory_described(struct workspace input, const mvn_call_desc* desc, int device, int streamed_views,
                                    size_t* bytes) {
  return guarded("mvn_deconvolve_memory_described",
                 [&] { deconvolve_memory(input, desc, device, streamed_views, bytes); });
}

int mvn_deconvolve_memory_resampled(struct workspace input, const mvn_call_desc* desc, const mvn_view_geometry* geom,
                                    int weights_mode, int device, size_t* bytes) {
  return guarded("mvn_deconvolve_memory_resampled", [&] {
    if (!geom) throw std::invalid_argument("null geom");
    std::vector<view_data> views = resampled_views(input, weights_mode);
    input.data_ = views.data();
    int derive = 0, derive_type = 0, derived_dims[3];
    captured_derivation(&derive, &derive_type);
    if (derive) {  // the call is priced with the derived kernels' extents: dims and matrices are all that is read
      std::vector<int> raw_psf_dims;
      for (size_t v = 0; v < views.size(); ++v) {
        if (!views[v].kernel1_dims_) throw std::invalid_argument("view " + std::to_string(v) + " has null dims");
        raw_psf_dims.insert(raw_psf_dims.end(), views[v].kernel1_dims_, views[v].kernel1_dims_ + 3);
      }
      psf_extents(input.num_views_, raw_psf_dims.data(), geom, derived_dims);
      for (view_data& d : views) d.kernel1_dims_ = d.kernel2_dims_ = derived_dims;
    }
    // (images are float32 volumes: the figure of dense float32 stacks)
    deconvolve_memory(input, nullptr, device, 0, bytes);
    size_t upload = 0;  // one raw stack in host memory at a time
    for (int v = 0; v < input.num_views_; ++v) {
      const ResampleGeom g = checked_geometry(geom + v, "geom " + std::to_string(v));
      const mvn_stack_desc* d = desc && desc->image ? desc->image + v : nullptr;
      if (d && d->location == MVN_DEVICE) continue;
      const size_t esz = d && d->dtype == MVN_U16 ? sizeof(uint16_t) : sizeof(float);
      const bool one = d && d->stride[0] == 0 && d->stride[1] == 0 && d->stride[2] == 0;
      upload = std::max(upload, one ? esz : (size_t)g.m[0] * (size_t)g.m[1] * (size_t)g.m[2] * esz);
    }
    *bytes += upload;
  });
}

int mvn_set_image_storage(int mode) {
  return guarded("mvn_set_image_storage", [&] {
    if (mode != 0 && mode != 1)
      throw std::invalid_argument("image storage mode must be 0 (float32 on entry) or 1 (uint16 images kept as uint16)");
    g_image_storage.store(mode);
  });
}

int mvn_get_image_storage(int* mode) {
  return guarded("mvn_get_image_storage", [&] {
    if (!mode) throw std::invalid_argument("null mode");
    *mode = g_image_storage.load();
  });
}

int mvn_image_storage_counters(long long out[2]) {
  return guarded("mvn_image_storage_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    Engine::image_storage_counters(out);
  });
}

int mvn_stream_counters(long long out[3]) {
  return guarded("mvn_stream_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    Engine::stream_counters(out);
  });
}

// single convolution on the engine's kernels; shared by the three convolution entry points
static void convolve_host(float* im, const int* imDim, const float* kernel, const int* kernelDim,
                          int device) {
  if (!im || !imDim || !kernel || !kernelDim) throw std::invalid_argument("null argument");
  const int dev = pick_device(device);
  std::lock_guard<std::mutex> lk(device_mutex(dev));
  be::set_device(dev);
  std::shared_ptr<Plan3D> plan = PlanStore::get().add(dev, to_shape(imDim));
  const Layout& L = plan->L;
  const size_t kb = sizeof(float) * (size_t)kernelDim[0] * kernelDim[1] * kernelDim[2];
  be::DeviceBuffer<float> vol, spec, dk;
  be::DeviceBuffer<cfloat> nyq, snyq;
  const be::Stream st = be::Stream::create();
  const be::stream_t s = st.get();
  vol = be::DeviceBuffer<float>(plan->main_bytes());
  spec = be::DeviceBuffer<float>(plan->main_bytes());
  if (plan->nyq_bytes()) {
    nyq = be::DeviceBuffer<cfloat>(plan->nyq_bytes());
    snyq = be::DeviceBuffer<cfloat>(plan->nyq_bytes());
  }
  dk = be::DeviceBuffer<float>(kb);
  be::h2d(dk.get(), kernel, kb, s);
  be::dzero(vol.get(), plan->main_bytes(), s);
  be::h2d_2d(vol.get(), (size_t)L.RP * 4, im, (size_t)L.d2 * 4, (size_t)L.d2 * 4, L.rows, s);
  const float scale = (float)(1.0 / (double)L.logical());
  plan->psf_spectrum(dk.get(), kernelDim, scale, spec.get(), snyq.get(), s);
  plan->convolve(vol.get(), (cfloat*)vol.get(), nyq.get(), (const cfloat*)spec.get(), snyq.get(), vol.get(),
                 store_epilogue(), s);
  be::d2h_2d(im, (size_t)L.d2 * 4, vol.get(), (size_t)L.RP * 4, (size_t)L.d2 * 4, L.rows, s);
  be::stream_sync(s);
}

void inplace_gpu_convolution(imageType* im, int* imDim, imageType* kernel, int* kernelDim,
                             int device) {
  guarded("inplace_gpu_convolution", [&] { convolve_host(im, imDim, kernel, kernelDim, device); });
}

void convolution3DfftCUDAInPlace(imageType* im, int* imDim, imageType* kernel, int* kernelDim,
                                 int devCUDA) {
  guarded("convolution3DfftCUDAInPlace", [&] { convolve_host(im, imDim, kernel, kernelDim, devCUDA); });
}

// device-pointer convolution on an already selected device; the caller holds the device mutex
static void core_convolve_on_device(float* d_im, const int* imDim, const float* d_kernel,
                                    const int* kernelDim, int dev) {
  std::shared_ptr<Plan3D> plan = PlanStore::get().add(dev, to_shape(imDim));
  const Layout& L = plan->L;
  be::DeviceBuffer<float> spec, padded;  // padded: stays empty when the caller's volume is borrowed
  be::DeviceBuffer<cfloat> nyq, snyq;
  const be::Stream st = be::Stream::create();
  const be::stream_t s = st.get();
  spec = be::DeviceBuffer<float>(plan->main_bytes());
  if (plan->nyq_bytes()) {
    nyq = be::DeviceBuffer<cfloat>(plan->nyq_bytes());
    snyq = be::DeviceBuffer<cfloat>(plan->nyq_bytes());
  }
  float* vol = d_im;  // even d2: the caller's dense volume already is the engine layout
  if (L.RP != L.d2) {
    padded = be::DeviceBuffer<float>(plan->main_bytes());
    vol = padded.get();
    be::dzero(vol, plan->main_bytes(), s);
    be::d2d_2d(vol, (size_t)L.RP * 4, d_im, (size_t)L.d2 * 4, (size_t)L.d2 * 4, L.rows, s);
  }
  const float scale = (float)(1.0 / (double)L.logical());
  plan->psf_spectrum(d_kernel, kernelDim, scale, spec.get(), snyq.get(), s);
  plan->convolve(vol, (cfloat*)vol, nyq.get(), (const cfloat*)spec.get(), snyq.get(), vol, store_epilogue(), s);
  if (vol != d_im) be::d2d_2d(d_im, (size_t)L.d2 * 4, vol, (size_t)L.RP * 4, (size_t)L.d2 * 4, L.rows, s);
  be::stream_sync(s);
}

void convolution3DfftCUDAInPlace_core(imageType* d_im, int* imDim, imageType* d_kernel,
                                      int* kernelDim, int devCUDA) {
  guarded("convolution3DfftCUDAInPlace_core", [&] {
    if (!d_im || !imDim || !d_kernel || !kernelDim) throw std::invalid_argument("null argument");
    const int dev = pick_device(devCUDA);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    core_convolve_on_device(d_im, imDim, d_kernel, kernelDim, dev);
  });
}

// One Richardson-Lucy step on a single stack, the legacy demo entry points of
// src/multiviewnative.cu:395-506 (plain) and :508-600 (tikhonov): psi_0 = view = _input,
// kernel1 = _kernel, kernel2 = 0.1 everywhere (same extents), weights = 1; both convolutions are
// cyclic on _input_dims (they go through convolution3DfftCUDAInPlace_core there as here).
static void iterate_fft_legacy(const char* what, const float* input, const float* kernel,
                               float* output, const int* input_dims, const int* kernel_dims,
                               bool tikhonov, float min_value, double lambda, int device) {
  guarded(what, [&] {
    if (!input || !kernel || !output || !input_dims || !kernel_dims)
      throw std::invalid_argument("null argument");
    const size_t n = (size_t)input_dims[0] * input_dims[1] * input_dims[2];
    const size_t nk = (size_t)kernel_dims[0] * kernel_dims[1] * kernel_dims[2];
    if (n == 0 || nk == 0) throw std::invalid_argument("empty stack or kernel");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const be::DeviceBuffer<float> image(n * 4), initial(n * 4), weights(n * 4), dkernel(nk * 4);
    float *d_image = image.get(), *d_initial = initial.get(), *d_weights = weights.get(), *d_kernel = dkernel.get();
    std::vector<float> ones(n, 1.f), tenth(nk, .1f);
    be::h2d(d_weights, ones.data(), n * 4, nullptr);
    be::h2d(d_initial, input, n * 4, nullptr);
    be::h2d(d_image, input, n * 4, nullptr);
    be::h2d(d_kernel, kernel, nk * 4, nullptr);
    be::stream_sync(nullptr);
    int idims[3] = {input_dims[0], input_dims[1], input_dims[2]};
    int kdims[3] = {kernel_dims[0], kernel_dims[1], kernel_dims[2]};
    core_convolve_on_device(d_image, idims, d_kernel, kdims, dev);  // psi (*) kernel1
    be::launch_divide(d_initial, d_image, n, nullptr);              // view / blurred
    be::h2d(d_kernel, tenth.data(), nk * 4, nullptr);
    be::stream_sync(nullptr);
    core_convolve_on_device(d_image, idims, d_kernel, kdims, dev);  // (*) kernel2 -> integral
    if (tikhonov)
      be::launch_update_legacy_tikhonov(d_initial, d_image, d_weights, n, (float)lambda, min_value, nullptr);
    else
      be::launch_update(d_initial, d_image, d_weights, n, 0., min_value, nullptr);
    std::vector<float> tmp(n);
    be::d2h(tmp.data(), d_initial, n * 4, nullptr);
    be::stream_sync(nullptr);
    std::memcpy(output, tmp.data(), n * 4);
  });
}

void iterate_fft_plain(imageType* _input, imageType* _kernel, imageType* _output, int* _input_dims,
                       int* _kernel_dims, int _device) {
  // the reference hard-codes minValue = .0001f here (src/multiviewnative.cu:485-486)
  iterate_fft_legacy("iterate_fft_plain", _input, _kernel, _output, _input_dims, _kernel_dims,
                     false, .0001f, 0., _device);
}

void iterate_fft_tikhonov(imageType* _input, imageType* _kernel, imageType* _output,
                          int* _input_dims, int* _kernel_dims, size_t _size, float _minValue,
                          double _lambda, int _device) {
  (void)_size;  // unused by the reference too (the extent comes from _input_dims)
  iterate_fft_legacy("iterate_fft_tikhonov", _input, _kernel, _output, _input_dims, _kernel_dims,
                     true, _minValue, _lambda, _device);
}

void compute_quotient(imageType* _input, imageType* _output, size_t _size, int _device) {
  guarded("compute_quotient", [&] {
    if (!_input || !_output) throw std::invalid_argument("null argument");
    if (_size == 0) return;
    const int dev = pick_device(_device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const size_t bytes = _size * sizeof(float);
    const be::DeviceBuffer<float> d_in(bytes), d_out(bytes);
    be::h2d(d_in.get(), _input, bytes, nullptr);
    be::h2d(d_out.get(), _output, bytes, nullptr);
    be::launch_divide(d_in.get(), d_out.get(), _size, nullptr);
    std::vector<float> tmp(_size);
    be::d2h(tmp.data(), d_out.get(), bytes, nullptr);
    be::stream_sync(nullptr);
    std::memcpy(_output, tmp.data(), bytes);
  });
}

void compute_final_values(imageType* _image, imageType* _integral, imageType* _weight,
                          size_t _size, float _minValue, double _lambda, int _device) {
  guarded("compute_final_values", [&] {
    if (!_image || !_integral || !_weight) throw std::invalid_argument("null argument");
    if (_size == 0) return;
    const int dev = pick_device(_device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    be::set_device(dev);
    const size_t bytes = _size * sizeof(float);
    const be::DeviceBuffer<float> d_psi(bytes), d_int(bytes), d_w(bytes);
    be::h2d(d_psi.get(), _image, bytes, nullptr);
    be::h2d(d_int.get(), _integral, bytes, nullptr);
    be::h2d(d_w.get(), _weight, bytes, nullptr);
    be::launch_update(d_psi.get(), d_int.get(), d_w.get(), _size, _lambda, _minValue, nullptr);
    std::vector<float> tmp(_size);
    be::d2h(tmp.data(), d_psi.get(), bytes, nullptr);
    be::stream_sync(nullptr);
    std::memcpy(_image, tmp.data(), bytes);
  });
}

// ---------------------------------------------------------------------------------------------
// plan_store
// ---------------------------------------------------------------------------------------------
int mvn_release_cached_engines(void) {
  return guarded("mvn_release_cached_engines", [&] {
    std::vector<int> devs;
    {
      std::lock_guard<std::mutex> lk(engine_cache_mutex());
      for (auto& kv : engine_cache()) devs.push_back(kv.first);
    }
    for (int d : devs) {
      std::lock_guard<std::mutex> lk(device_mutex(d));  // not while a call on that device runs
      pop_cached_engine(d).reset();
    }
    std::unique_ptr<HaloGroup> group;
    {
      std::lock_guard<std::mutex> lk(engine_cache_mutex());
      group = std::move(multi_cache());
    }
    if (group) {
      std::vector<int> distinct(group->devices());
      std::sort(distinct.begin(), distinct.end());
      distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
      std::vector<std::unique_lock<std::mutex>> locks;
      for (int d : distinct) locks.emplace_back(device_mutex(d));
      group.reset();
    }
  });
}

long mvn_split_launch_count(void) { return be::split_launch_count(); }
long mvn_mid_fused_launch_count(void) { return be::mid_fused_launch_count(); }
long mvn_multi_device_calls(void) { return g_multi_calls.load(); }

// ---- resident group of slab engines (what MVN_DEVICES runs inside inplace_gpu_deconvolve) -----
int mvn_group_create(const int* devices, int ndevices, const int dims[3], int halo_planes, int num_views,
                     mvn_group** out) {
  return guarded("mvn_group_create", [&] {
    if (!devices || !dims || !out) throw std::invalid_argument("null argument");
    *out = nullptr;
    std::vector<int> devs(devices, devices + (ndevices > 0 ? ndevices : 0));
    for (int d : devs)
      if (d < 0 || d >= be::device_count()) throw std::invalid_argument("no such device");
    std::unique_ptr<mvn_group> g(new mvn_group());
    g->impl.reset(new HaloGroup(devs, to_shape(dims), halo_planes < 1 ? 1 : halo_planes, num_views));
    *out = g.release();
  });
}

int mvn_group_destroy(mvn_group* g) {
  return guarded("mvn_group_destroy", [&] { delete g; });
}

#define MVN_GROUP_CALL(where, ...)                                               \
  return guarded(where, [&] {                                                    \
    if (!g || !g->impl) throw std::invalid_argument("null group");               \
    HaloGroup& G = *g->impl;                                                     \
    __VA_ARGS__;                                                                 \
  })

int mvn_group_load(mvn_group* g, const float* psi, struct workspace input) {
  MVN_GROUP_CALL("mvn_group_load", {
    check_workspace(psi, input);
    if (input.num_views_ != G.num_views()) throw std::invalid_argument("view count of the group");
    for (int v = 0; v < input.num_views_; ++v)
      if (to_shape(input.data_[v].image_dims_) != G.extents())
        throw std::invalid_argument("stacks must have the extents the group was created for");
    if (!G.all_direct(input)) throw std::invalid_argument("every PSF must be held in the direct dim0 form (<= 33 planes)");
    const int off[3] = {0, 0, 0};
    G.load(psi, input, G.extents(), off, false);
  });
}

int mvn_group_iterate(mvn_group* g, int iterations, double lambda, float min_value, float* ms) {
  MVN_GROUP_CALL("mvn_group_iterate", {
    const double t = G.iterate(iterations, lambda, min_value);
    if (ms) *ms = (float)t;
  });
}

int mvn_group_get_psi(mvn_group* g, float* psi) {
  MVN_GROUP_CALL("mvn_group_get_psi", {
    if (!psi) throw std::invalid_argument("null psi");
    G.fetch(psi);
  });
}

int mvn_psf_cache_counters(long out[2]) {
  return guarded("mvn_psf_cache_counters", [&] {
    if (!out) throw std::invalid_argument("null out");
    out[0] = Engine::psf_cache_hits();
    out[1] = Engine::psf_cache_misses();
  });
}

int mvn_plan_store_add(int device, const int dims[3]) {
  return guarded("mvn_plan_store_add", [&] { PlanStore::get().add(pick_device(device), to_shape(dims)); });
}

int mvn_plan_store_has_key(int device, const int dims[3]) {
  int r = 0;
  int rc = guarded("mvn_plan_store_has_key",
                   [&] { r = PlanStore::get().has_key(pick_device(device), to_shape(dims)) ? 1 : 0; });
  return rc < 0 ? rc : r;
}

int mvn_plan_store_size(void) { return (int)PlanStore::get().size(); }
int mvn_plan_store_empty(void) { return PlanStore::get().empty() ? 1 : 0; }
int mvn_plan_store_clear(void) {
  return guarded("mvn_plan_store_clear", [&] {
    mvn_release_cached_engines();  // a cached engine would keep using its old plan
    PlanStore::get().clear();
  });
}

int mvn_plan_describe(int device, const int dims[3], int out[12]) {
  return guarded("mvn_plan_describe", [&] {
    std::shared_ptr<Plan3D> p = PlanStore::get().add(pick_device(device), to_shape(dims));
    out[0] = p->L.h;
    out[1] = p->L.C;
    out[2] = p->L.RP;
    out[3] = p->L.even ? 1 : 0;
    out[4] = p->g_rows.T;
    out[5] = p->g_ax1.T;
    out[6] = p->g_ax0.T;
    out[7] = p->ax2.view.nstages;
    out[8] = p->fx_rows ? 1 : 0;
    out[9] = p->fx_ax1 ? 1 : 0;
    out[10] = p->fx_ax0 ? 1 : 0;
    out[11] = 0;
  });
}

// ---------------------------------------------------------------------------------------------
// whole transforms on host buffers
// ---------------------------------------------------------------------------------------------
// `batch` zeroed volumes of one shape with their Nyquist planes (even d2), their cached plan and a stream
struct FftScratch {
  std::shared_ptr<Plan3D> plan;
  std::vector<be::DeviceBuffer<float>> vol;
  std::vector<be::DeviceBuffer<cfloat>> nyq;
  be::Stream stream;  // (behind the buffers: drained and destroyed before they are freed)
  be::stream_t s = nullptr;
  FftScratch(int dev, const int* dims, int batch = 1) {
    be::set_device(dev);
    plan = PlanStore::get().add(dev, to_shape(dims));
    stream = be::Stream::create();
    s = stream.get();
    for (int b = 0; b < batch; ++b) {
      vol.emplace_back(plan->main_bytes());
      be::dzero(v(b), plan->main_bytes(), s);
      nyq.emplace_back();
      if (plan->nyq_bytes()) {
        nyq.back() = be::DeviceBuffer<cfloat>(plan->nyq_bytes());
        be::dzero(n(b), plan->nyq_bytes(), s);
      }
    }
  }
  float* v(int b = 0) const { return vol[(size_t)b].get(); }
  cfloat* n(int b = 0) const { return nyq[(size_t)b].get(); }
  // direction 0: forward; otherwise backward, scaled to give the input back
  void transform(int b, int direction, Profiler* prof = nullptr) const {
    if (direction == 0)
      plan->forward(v(b), n(b), s, prof);
    else
      plan->backward(v(b), n(b), 1.0f / (float)plan->L.logical(), s, prof);
  }
};

int mvn_fft3_r2c(int device, const int dims[3], const float* real, float* spec) {
  return guarded("mvn_fft3_r2c", [&] {
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    FftScratch f(dev, dims);
    const Layout& L = f.plan->L;
    be::h2d_2d(f.v(), (size_t)L.RP * 4, real, (size_t)L.d2 * 4, (size_t)L.d2 * 4, L.rows, f.s);
    f.transform(0, 0);
    std::vector<cfloat> main_h(L.rows * (size_t)L.C), nyq_h(L.nyq_cplx());
    be::d2h(main_h.data(), f.v(), main_h.size() * sizeof(cfloat), f.s);
    if (L.even) be::d2h(nyq_h.data(), f.n(), nyq_h.size() * sizeof(cfloat), f.s);
    be::stream_sync(f.s);
    position_to_natural(*f.plan, main_h, nyq_h, reinterpret_cast<cfloat*>(spec));
  });
}

int mvn_fft3_c2r(int device, const int dims[3], const float* spec, float* real) {
  return guarded("mvn_fft3_c2r", [&] {
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    FftScratch f(dev, dims);
    const Layout& L = f.plan->L;
    std::vector<cfloat> main_h(L.rows * (size_t)L.C), nyq_h(L.nyq_cplx());
    natural_to_position(*f.plan, reinterpret_cast<const cfloat*>(spec), main_h, nyq_h);
    be::h2d(f.v(), main_h.data(), main_h.size() * sizeof(cfloat), f.s);
    if (L.even) be::h2d(f.n(), nyq_h.data(), nyq_h.size() * sizeof(cfloat), f.s);
    f.plan->backward(f.v(), f.n(), 1.f, f.s);
    be::d2h_2d(real, (size_t)L.d2 * 4, f.v(), (size_t)L.RP * 4, (size_t)L.d2 * 4, L.rows, f.s);
    be::stream_sync(f.s);
  });
}

int mvn_fft3_time(int device, const int dims[3], int direction, int reps, float* ms) {
  return mvn_fft3_profile(device, dims, direction, reps, ms, nullptr);
}

int mvn_fft3_profile(int device, const int dims[3], int direction, int reps, float* ms,
                     double* per_kind_ms) {
  return guarded("mvn_fft3_profile", [&] {
    if (reps < 1) throw std::invalid_argument("reps must be >= 1");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    FftScratch f(dev, dims);
    const Layout& L = f.plan->L;
    {
      const std::vector<float> host = lcg_fill(L.real_floats());
      be::h2d(f.v(), host.data(), host.size() * 4, f.s);
      be::stream_sync(f.s);
    }
    *ms = time_on_stream(f.s, reps, [&] { f.transform(0, direction); });
    if (per_kind_ms) {  // second, event-instrumented round: average launch time per kernel kind
      Profiler prof;
      prof.enabled = true;
      for (int i = 0; i < reps; ++i) f.transform(0, direction, &prof);
      be::stream_sync(f.s);
      prof.collect();
      for (int k = 0; k < KK_COUNT; ++k)
        per_kind_ms[k] = prof.count[k] ? prof.total_ms[k] / (double)prof.count[k] : 0.0;
    }
  });
}

// Batched transforms: `batch` stacks of one shape through ONE cached plan, back to back on one
// stream -- the counterpart of the cufftPlanMany path of bench/bench_gpu_many_nd_fft.cu:403-463.
int mvn_fft3_many_r2c(int device, const int dims[3], int batch, const float* real, float* spec) {
  return guarded("mvn_fft3_many_r2c", [&] {
    if (batch < 1 || !real || !spec) throw std::invalid_argument("bad batch or null buffers");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    FftScratch f(dev, dims, batch);
    const Layout& L = f.plan->L;
    const size_t nreal = (size_t)L.d0 * L.d1 * L.d2;
    const size_t nspec = (size_t)L.d0 * L.d1 * (size_t)(L.d2 / 2 + 1);
    for (int b = 0; b < batch; ++b)
      be::h2d_2d(f.v(b), (size_t)L.RP * 4, real + b * nreal, (size_t)L.d2 * 4, (size_t)L.d2 * 4, L.rows, f.s);
    for (int b = 0; b < batch; ++b) f.transform(b, 0);
    std::vector<cfloat> main_h(L.rows * (size_t)L.C), nyq_h(L.nyq_cplx());
    for (int b = 0; b < batch; ++b) {
      be::d2h(main_h.data(), f.v(b), main_h.size() * sizeof(cfloat), f.s);
      if (L.even) be::d2h(nyq_h.data(), f.n(b), nyq_h.size() * sizeof(cfloat), f.s);
      be::stream_sync(f.s);
      position_to_natural(*f.plan, main_h, nyq_h, reinterpret_cast<cfloat*>(spec) + b * nspec);
    }
  });
}

int mvn_fft3_many_time(int device, const int dims[3], int batch, int direction, int reps,
                       float* ms) {
  return guarded("mvn_fft3_many_time", [&] {
    if (batch < 1 || reps < 1 || !ms) throw std::invalid_argument("bad batch, reps or null ms");
    const int dev = pick_device(device);
    std::lock_guard<std::mutex> lk(device_mutex(dev));
    FftScratch f(dev, dims, batch);
    {
      const std::vector<float> host = lcg_fill(f.plan->L.real_floats());
      for (int b = 0; b < batch; ++b) be::h2d(f.v(b), host.data(), host.size() * 4, f.s);
      be::stream_sync(f.s);
    }
    *ms = time_on_stream(f.s, reps, [&] {
      for (int b = 0; b < batch; ++b) f.transform(b, direction);
    });
  });
}

// ---------------------------------------------------------------------------------------------
// resident engine
// ---------------------------------------------------------------------------------------------
int mvn_engine_create(int device, const int dims[3], int num_views, mvn_engine** out) {
  return guarded("mvn_engine_create", [&] {
    if (!out) throw std::invalid_argument("null out");
    *out = nullptr;
    std::unique_ptr<mvn_engine> h(new mvn_engine());
    h->impl.reset(new Engine(pick_device(device), to_shape(dims), num_views));
    *out = h.release();
  });
}

int mvn_engine_destroy(mvn_engine* e) {
  return guarded("mvn_engine_destroy", [&] { delete e; });
}

#define MVN_ENGINE_CALL(name, ...)                                 \
  return guarded(name, [&] {                                       \
    if (!e || !e->impl) throw std::invalid_argument("null engine"); \
    Engine& E = *e->impl;                                          \
    (void)E;                                                       \
    __VA_ARGS__;                                                   \
  })

// a stack of the engine entry points: a null descriptor means a dense float32 stack in host memory
static StackRef engine_stack(Engine& E, const void* ptr, const mvn_stack_desc* d, const char* what, bool may_u16,
                             bool written) {
  const Layout& L = E.layout();
  const int dims[3] = {L.d0, L.d1, L.d2};
  return described_stack(ptr, d, dims, what, may_u16, written);
}

// `checked` (here and in engine_psi): a described entry point - the pointers must be where their descriptors say, on
// the engine's device, and the engine waits for the caller's stream; the plain entry points ask nothing about theirs
static void engine_set_view(Engine& E, int v, const void* image, const mvn_stack_desc* image_desc, const void* weights,
                            const mvn_stack_desc* weights_desc, const float* kernel1, const int* k1dims,
                            const float* kernel2, const int* k2dims, void* stream, bool checked) {
  if (!kernel1 || !kernel2 || !k1dims || !k2dims) throw std::invalid_argument("null kernel");
  const StackRef im = engine_stack(E, image, image_desc, "image", true, false);
  const StackRef w = engine_stack(E, weights, weights_desc, "weights", false, false);
  if (checked) {
    int owner = -1;
    check_location(im, "image", &owner);
    check_location(w, "weights", &owner);
    if (owner >= 0 && owner != E.device()) throw std::invalid_argument("the stacks live on another device than the engine");
    E.wait_for_caller(stream);
  }
  E.set_image_storage(checked ? g_image_storage.load() : 0);  // (the plain entry point brings float32)
  E.set_view(v, im, w, kernel1, k1dims, kernel2, k2dims);
}

static StackRef engine_psi(Engine& E, const void* psi, const mvn_stack_desc* d, bool written, bool checked) {
  const StackRef r = engine_stack(E, psi, d, "psi", false, written);
  int owner = -1;
  if (checked) check_location(r, "psi", &owner);
  if (owner >= 0 && owner != E.device()) throw std::invalid_argument("psi lives on another device than the engine");
  return r;
}

int mvn_engine_set_view(mvn_engine* e, int v, const float* image, const float* weights,
                        const float* kernel1, const int k1dims[3], const float* kernel2,
                        const int k2dims[3]) {
  MVN_ENGINE_CALL("mvn_engine_set_view",
                  engine_set_view(E, v, image, nullptr, weights, nullptr, kernel1, k1dims, kernel2, k2dims, nullptr, false));
}

int mvn_engine_set_psi(mvn_engine* e, const float* psi) {
  MVN_ENGINE_CALL("mvn_engine_set_psi", E.set_psi(engine_psi(E, psi, nullptr, false, false)));
}

int mvn_engine_get_psi(mvn_engine* e, float* psi) {
  MVN_ENGINE_CALL("mvn_engine_get_psi", E.get_psi(engine_psi(E, psi, nullptr, true, false)));
}

int mvn_engine_set_view_described(mvn_engine* e, int v, const void* image, const mvn_stack_desc* image_desc,
                                  const void* weights, const mvn_stack_desc* weights_desc, const float* kernel1,
                                  const int k1dims[3], const float* kernel2, const int k2dims[3], void* stream) {
  MVN_ENGINE_CALL("mvn_engine_set_view_described", engine_set_view(E, v, image, image_desc, weights, weights_desc, kernel1,
                                                                   k1dims, kernel2, k2dims, stream, true));
}

int mvn_engine_set_view_resampled(mvn_engine* e, int v, const void* image, const mvn_stack_desc* image_desc,
                                  const mvn_view_geometry* geom, const void* weights, const mvn_stack_desc* weights_desc,
                                  const float* kernel1, const int k1dims[3], const float* kernel2, const int k2dims[3],
                                  void* stream) {
  MVN_ENGINE_CALL("mvn_engine_set_view_resampled", {
    if (!kernel1 || !kernel2 || !k1dims || !k2dims) throw std::invalid_argument("null kernel");
    if (E.has_halo_hook()) throw std::invalid_argument("resampled views are not for an engine with a halo hook");
    const ResampleGeom g = checked_geometry(geom, "geom");
    StackRef im = described_stack(image, image_desc, g.m, "image", true, false);
    im.geom = &g;
    const StackRef w = weights ? engine_stack(E, weights, weights_desc, "weights", false, false) : StackRef();
    int owner = -1;
    check_location(im, "image", &owner);
    if (weights) check_location(w, "weights", &owner);
    if (owner >= 0 && owner != E.device()) throw std::invalid_argument("the stacks live on another device than the engine");
    E.wait_for_caller(stream);
    E.set_view(v, im, w, kernel1, k1dims, kernel2, k2dims);
  });
}

int mvn_engine_normalize_weights(mvn_engine* e) {
  MVN_ENGINE_CALL("mvn_engine_normalize_weights", E.normalize_weights());
}

int mvn_engine_fuse_psi(mvn_engine* e, float fill) { MVN_ENGINE_CALL("mvn_engine_fuse_psi", E.fuse_psi(fill)); }

int mvn_engine_set_psi_described(mvn_engine* e, const void* psi, const mvn_stack_desc* d, void* stream) {
  MVN_ENGINE_CALL("mvn_engine_set_psi_described", {
    const StackRef r = engine_psi(E, psi, d, false, true);
    E.wait_for_caller(stream);
    E.set_psi(r);
  });
}

int mvn_engine_get_psi_described(mvn_engine* e, void* psi, const mvn_stack_desc* d) {
  MVN_ENGINE_CALL("mvn_engine_get_psi_described", {
    const StackRef r = engine_psi(E, psi, d, true, true);
    E.sync();
    E.get_psi(r);
  });
}

int mvn_engine_iterate(mvn_engine* e, int iterations, double lambda, float min_value) {
  MVN_ENGINE_CALL("mvn_engine_iterate", E.iterate(iterations, lambda, min_value));
}

// one iterate() under the options the engine holds plus what the call itself asks for; returns the sweeps run
static int engine_iterate(Engine& E, int iterations, double lambda, float min_value, double tolerance, int accel,
                          double* stats, double* alphas) {
  LoopOptions o = E.options();
  o.tolerance = tolerance, o.accel = accel;
  LoopResult r;
  E.iterate(iterations, lambda, min_value, o, &r);
  if (stats && !r.rows.empty()) std::memcpy(stats, r.rows.data(), r.rows.size() * sizeof(double));
  if (alphas && !r.alphas.empty()) std::memcpy(alphas, r.alphas.data(), r.alphas.size() * sizeof(double));
  return r.ran;
}

int mvn_engine_iterate_converge(mvn_engine* e, int iterations, double lambda, float min_value, double tolerance,
                                int* iterations_run, double* stats) {
  MVN_ENGINE_CALL("mvn_engine_iterate_converge", {
    if (tolerance >= 0. && !stats) throw std::invalid_argument("null statistics buffer");
    const int ran = engine_iterate(E, iterations, lambda, min_value, tolerance, 0, stats, nullptr);
    if (iterations_run) *iterations_run = ran;
  });
}

int mvn_engine_iterate_accelerated(mvn_engine* e, int iterations, double lambda, float min_value, double tolerance,
                                   int* iterations_run, double* stats, double* alphas) {
  MVN_ENGINE_CALL("mvn_engine_iterate_accelerated", {
    const int ran = engine_iterate(E, iterations, lambda, min_value, tolerance, 1, stats, alphas);
    if (iterations_run) *iterations_run = ran;
  });
}

int mvn_engine_set_regularization(mvn_engine* e, int kind, double epsilon) {
  MVN_ENGINE_CALL("mvn_engine_set_regularization", {
    LoopOptions o = E.options();
    set_regulariser(o, kind, epsilon);
    E.set_options(o);
  });
}

int mvn_engine_set_noise_model(mvn_engine* e, const float* background, int likelihood) {
  MVN_ENGINE_CALL("mvn_engine_set_noise_model", {
    LoopOptions o = E.options();
    o.background.assign(background, background + (background ? E.num_views() : 0));
    o.likelihood = likelihood;
    E.set_options(o);
  });
}

int mvn_engine_last_likelihood(mvn_engine* e, int* iterations_run, double* stats, int capacity_rows) {
  int rows = 0;
  const int rc = guarded("mvn_engine_last_likelihood", [&] {
    if (!e || !e->impl) throw std::invalid_argument("null engine");
    if (capacity_rows < 0 || (capacity_rows > 0 && !stats)) throw std::invalid_argument("bad statistics buffer");
    Engine& E = *e->impl;
    E.sync();
    const LoopResult& r = E.last_result();
    if (iterations_run) *iterations_run = r.like.empty() ? 0 : r.ran;
    rows = copy_rows(r.like, 3, stats, capacity_rows);
  });
  return rc < 0 ? rc : rows;
}

int mvn_engine_compute_delta(mvn_engine* e, double lambda, float min_value) {
  MVN_ENGINE_CALL("mvn_engine_compute_delta", E.compute_delta(lambda, min_value));
}

int mvn_engine_apply_delta(mvn_engine* e) {
  MVN_ENGINE_CALL("mvn_engine_apply_delta", E.apply_delta());
}

int mvn_engine_delta_chunks(mvn_engine* e, int wanted) {
  int n = 1;
  int rc = guarded("mvn_engine_delta_chunks", [&] {
    if (!e || !e->impl) throw std::invalid_argument("null engine");
    n = e->impl->delta_chunks(wanted);
  });
  return rc < 0 ? rc : n;
}

int mvn_engine_delta_chunk_range(mvn_engine* e, int c, int n, size_t* first_float, size_t* n_floats) {
  MVN_ENGINE_CALL("mvn_engine_delta_chunk_range", {
    if (!first_float || !n_floats) throw std::invalid_argument("null argument");
    E.delta_chunk_range(c, n, first_float, n_floats);
  });
}

int mvn_engine_compute_delta_head(mvn_engine* e, double lambda, float min_value) {
  MVN_ENGINE_CALL("mvn_engine_compute_delta_head", E.compute_delta_head(lambda, min_value));
}

int mvn_engine_compute_delta_chunk(mvn_engine* e, int c, int n) {
  MVN_ENGINE_CALL("mvn_engine_compute_delta_chunk", E.compute_delta_chunk(c, n));
}

int mvn_engine_apply_delta_chunk(mvn_engine* e, int c, int n, int feed_next) {
  MVN_ENGINE_CALL("mvn_engine_apply_delta_chunk", E.apply_delta_chunk(c, n, feed_next != 0));
}

int mvn_engine_delta_ptr(mvn_engine* e, void** dev_ptr, size_t* n_floats) {
  MVN_ENGINE_CALL("mvn_engine_delta_ptr", {
    *dev_ptr = E.delta_ptr();
    *n_floats = E.volume_floats();
  });
}

int mvn_engine_bind_delta(mvn_engine* e, void* dev_ptr) {
  MVN_ENGINE_CALL("mvn_engine_bind_delta", E.bind_delta((float*)dev_ptr));
}

int mvn_engine_set_halo_hook(mvn_engine* e, void (*fn)(void*, void*, int, int), void* user, int drain) {
  MVN_ENGINE_CALL("mvn_engine_set_halo_hook", E.set_halo_hook(fn, user, (drain & 1) != 0, (drain & 2) != 0));
}

int mvn_engine_would_be_direct(mvn_engine* e, const int kdims[3]) {
  int yes = 0;
  const int rc = guarded("mvn_engine_would_be_direct", [&] {
    if (!e || !e->impl || !kdims) throw std::invalid_argument("null argument");
    be::set_device(e->impl->device());
    yes = e->impl->would_be_direct(kdims) ? 1 : 0;
  });
  return rc < 0 ? rc : yes;
}

int mvn_engine_set_halo_planes(mvn_engine* e, int planes, int split) {
  MVN_ENGINE_CALL("mvn_engine_set_halo_planes", E.set_halo_planes(planes, split != 0));
}

int mvn_engine_poison_ptr(mvn_engine* e, void** dev_ptr) {
  MVN_ENGINE_CALL("mvn_engine_poison_ptr", {
    if (!dev_ptr) throw std::invalid_argument("null argument");
    *dev_ptr = E.poison_ptr();
  });
}

int mvn_engine_bind_poison(mvn_engine* e, void* dev_ptr) {
  MVN_ENGINE_CALL("mvn_engine_bind_poison", E.bind_poison((unsigned*)dev_ptr));
}

int mvn_engine_poison_get(mvn_engine* e, unsigned* value) {
  MVN_ENGINE_CALL("mvn_engine_poison_get", {
    if (!value) throw std::invalid_argument("null argument");
    *value = E.poison_get();
  });
}

int mvn_engine_poison_merge(mvn_engine* e, unsigned value) {
  MVN_ENGINE_CALL("mvn_engine_poison_merge", E.poison_merge(value));
}

int mvn_engine_copy_planes(mvn_engine* e, void* spectrum, int plane0, int nplanes, void* buffer, int to_buffer) {
  MVN_ENGINE_CALL("mvn_engine_copy_planes", E.copy_planes(spectrum, plane0, nplanes, buffer, (to_buffer & 1) != 0, (to_buffer & 2) != 0, (to_buffer & 4) == 0));
}

int mvn_engine_psi_ptr(mvn_engine* e, void** dev_ptr, size_t* n_floats) {
  MVN_ENGINE_CALL("mvn_engine_psi_ptr", {
    *dev_ptr = E.psi_ptr();
    *n_floats = E.volume_floats();
  });
}

int mvn_engine_stream(mvn_engine* e, void** hip_stream) {
  MVN_ENGINE_CALL("mvn_engine_stream", *hip_stream = E.stream());
}

int mvn_engine_sync(mvn_engine* e) { MVN_ENGINE_CALL("mvn_engine_sync", E.sync()); }

int mvn_engine_time_iterate(mvn_engine* e, int iterations, double lambda, float min_value,
                            float* ms) {
  MVN_ENGINE_CALL("mvn_engine_time_iterate", {
    be::set_device(E.device());
    const be::Event a = be::Event::timing(), b = be::Event::timing();
    be::event_record(a.get(), E.stream());
    E.iterate(iterations, lambda, min_value);
    be::event_record(b.get(), E.stream());
    be::event_sync(b.get());
    *ms = be::event_elapsed_ms(a.get(), b.get());
    E.sync();
  });
}

int mvn_engine_profile(mvn_engine* e, int enable) {
  MVN_ENGINE_CALL("mvn_engine_profile", {
    E.sync();
    E.profiler().reset();
    E.profiler().enabled = enable != 0;
    E.profiler().sample_every = enable > 1 ? enable : 1;
  });
}

int mvn_engine_profile_read(mvn_engine* e, int kind, double* total_ms, long* launches) {
  MVN_ENGINE_CALL("mvn_engine_profile_read", {
    if (kind < 0 || kind >= KK_COUNT) throw std::out_of_range("kernel kind");
    E.sync();
    *total_ms = E.profiler().total_ms[kind];
    *launches = E.profiler().count[kind];
  });
}

int mvn_kernel_kind_count(void) { return KK_COUNT; }
const char* mvn_kernel_kind_name(int kind) { return kernel_kind_name(kind); }

size_t mvn_engine_B(mvn_engine* e) { return (e && e->impl) ? e->impl->layout().B() : 0; }

// ---------------------------------------------------------------------------------------------
// slab-decomposed engine (sequential sweep across several GPUs)
// ---------------------------------------------------------------------------------------------
int mvn_slab_create(int device, const int dims[3], int nranks, int rank, int num_views,
                    mvn_slab** out) {
  return guarded("mvn_slab_create", [&] {
    if (!out || !dims) throw std::invalid_argument("null argument");
    *out = nullptr;
    std::unique_ptr<mvn_slab> h(new mvn_slab());
    h->impl.reset(new SlabEngine(pick_device(device), to_shape(dims), nranks, rank, num_views));
    *out = h.release();
  });
}

int mvn_slab_destroy(mvn_slab* e) {
  return guarded("mvn_slab_destroy", [&] { delete e; });
}

#define MVN_SLAB_CALL(name, ...)                                        \
  return guarded(name, [&] {                                            \
    if (!e || !e->impl) throw std::invalid_argument("null slab engine"); \
    SlabEngine& E = *e->impl;                                           \
    (void)E;                                                            \
    __VA_ARGS__;                                                        \
  })

int mvn_slab_set_view(mvn_slab* e, int v, const float* image_slab, const float* weights_slab,
                      const float* kernel1, const int k1dims[3], const float* kernel2,
                      const int k2dims[3]) {
  MVN_SLAB_CALL("mvn_slab_set_view", {
    if (!image_slab || !weights_slab || !kernel1 || !kernel2 || !k1dims || !k2dims)
      throw std::invalid_argument("null argument");
    E.set_view(v, image_slab, weights_slab, kernel1, k1dims, kernel2, k2dims);
  });
}

int mvn_slab_set_psi(mvn_slab* e, const float* psi_slab) {
  MVN_SLAB_CALL("mvn_slab_set_psi", {
    if (!psi_slab) throw std::invalid_argument("null argument");
    E.set_psi(psi_slab);
  });
}

int mvn_slab_get_psi(mvn_slab* e, float* psi_slab) {
  MVN_SLAB_CALL("mvn_slab_get_psi", {
    if (!psi_slab) throw std::invalid_argument("null argument");
    E.get_psi(psi_slab);
  });
}

int mvn_slab_buffer_sizes(mvn_slab* e, size_t* main_floats, size_t* nyq_floats) {
  MVN_SLAB_CALL("mvn_slab_buffer_sizes", {
    if (main_floats) *main_floats = E.main_floats();
    if (nyq_floats) *nyq_floats = E.nyq_floats();
  });
}

int mvn_slab_bind_buffers(mvn_slab* e, void* a_main, void* b_main, void* a_nyq, void* b_nyq) {
  MVN_SLAB_CALL("mvn_slab_bind_buffers",
                E.bind_buffers((float*)a_main, (float*)b_main, (float*)a_nyq, (float*)b_nyq));
}

int mvn_slab_buffers(mvn_slab* e, void** a_main, void** b_main, void** a_nyq, void** b_nyq) {
  MVN_SLAB_CALL("mvn_slab_buffers", {
    if (a_main) *a_main = E.a_main();
    if (b_main) *b_main = E.b_main();
    if (a_nyq) *a_nyq = E.a_nyq();
    if (b_nyq) *b_nyq = E.b_nyq();
  });
}

int mvn_slab_begin(mvn_slab* e) { MVN_SLAB_CALL("mvn_slab_begin", E.begin_sweeps()); }
int mvn_slab_pack(mvn_slab* e, int v, int conv) {
  MVN_SLAB_CALL("mvn_slab_pack", {
    if (conv != 0 && conv != 1) throw std::invalid_argument("conv must be 0 or 1");
    E.step_pack(v, conv);
  });
}
int mvn_slab_mid(mvn_slab* e, int v, int conv) {
  MVN_SLAB_CALL("mvn_slab_mid", {
    if (conv != 0 && conv != 1) throw std::invalid_argument("conv must be 0 or 1");
    E.step_mid(v, conv);
  });
}
int mvn_slab_unpack(mvn_slab* e, int v, int conv, double lambda, float min_value, int feed_next) {
  MVN_SLAB_CALL("mvn_slab_unpack", {
    if (conv != 0 && conv != 1) throw std::invalid_argument("conv must be 0 or 1");
    E.step_unpack(v, conv, lambda, min_value, feed_next != 0);
  });
}
int mvn_slab_sync(mvn_slab* e) { MVN_SLAB_CALL("mvn_slab_sync", E.sync()); }
int mvn_slab_stream(mvn_slab* e, void** hip_stream) {
  MVN_SLAB_CALL("mvn_slab_stream", {
    if (!hip_stream) throw std::invalid_argument("null argument");
    *hip_stream = (void*)E.stream();
  });
}

}  // extern "C"
