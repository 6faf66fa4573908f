// mvn_backend_emu.cpp -- TEST-ONLY host emulation of the device backend (-DMVN_HOST_EMU).
//
// Built into libmvn_emu.so, never into the product library.  "Device memory" is host memory;
// a launch runs the very same workgroup bodies (mvn_pass_bodies.hpp) one block after the other
// with a single work-item enumerator per block, so plans, tables, addressing and the RL driver
// can be validated against the oracle and numpy on a box without a GPU.  It says nothing about
// barriers or races -- those are covered by the -m gpu parity tests.
#ifndef MVN_HOST_EMU
#error "mvn_backend_emu.cpp is only for the MVN_HOST_EMU test build"
#endif

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "mvn_backend.hpp"
#include "mvn_fixed_geom.hpp"
#include "mvn_wave_rows.hpp"

namespace mvn {
namespace be {

const char* backend_name() { return "host-emulation (test only)"; }

// MVN_EMU_DEVICES=n pretends to have n devices (tests of the per-device engine cache and locking);
// the current device is per host thread, as in HIP
int device_count() {
  const char* e = std::getenv("MVN_EMU_DEVICES");
  const int n = e ? std::atoi(e) : 1;
  return n > 0 ? n : 1;
}
static thread_local int t_device = 0;
void set_device(int d) {  // as strict as hipSetDevice: a lane key or a stale id must not pass here either
  if (d < 0 || d >= device_count()) throw std::runtime_error("emu: invalid device ordinal " + std::to_string(d));
  t_device = d;
}
int get_device() { return t_device; }
void device_name(int, char* name256) {
  std::memset(name256, 0, 256);
  std::strcpy(name256, "mvn host emulation");
}
// "device memory" accounting per fake device: total = MVN_EMU_TOTAL_MB (default 8 GiB), free =
// total - live dmalloc bytes, so that the memory heuristic and the memory model of the ABI call can be tested
static std::mutex g_mem_mu;
static std::map<void*, std::pair<int, size_t>> g_live;  // pointer -> (device, bytes)
static std::map<int, size_t> g_used;
static size_t emu_total() {
  const char* e = std::getenv("MVN_EMU_TOTAL_MB");
  return e ? (size_t)std::atoll(e) << 20 : (size_t)8 << 30;
}
long long device_total_mem(int) { return (long long)emu_total(); }
void device_mem_info(size_t* f, size_t* t) {
  std::lock_guard<std::mutex> lk(g_mem_mu);
  const size_t total = emu_total(), used = g_used[t_device];
  *t = total;
  *f = used < total ? total - used : 0;
}
void device_arch(int, int* major, int* minor) {
  *major = 0;
  *minor = 0;
}

// an allocation beyond the total fails, as hipMalloc would: tests of the memory model (Engine::memory_need) run
// the ABI call with the total set to the model's figure
void* dmalloc(size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    if (g_used[t_device] + bytes > emu_total())
      throw std::runtime_error("emu: device memory exhausted (" + std::to_string(g_used[t_device]) + " + " +
                               std::to_string(bytes) + " bytes > MVN_EMU_TOTAL_MB)");
  }
  void* p = std::malloc(bytes ? bytes : 1);
  if (!p) throw std::bad_alloc();
  std::lock_guard<std::mutex> lk(g_mem_mu);
  g_live[p] = std::make_pair(t_device, bytes);
  g_used[t_device] += bytes;
  return p;
}
void dfree(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    auto it = g_live.find(p);
    if (it != g_live.end()) {
      g_used[it->second.first] -= it->second.second;
      g_live.erase(it);
    }
  }
  std::free(p);
}
void h2d(void* d, const void* h, size_t bytes, stream_t) { std::memcpy(d, h, bytes); }
void d2h(void* h, const void* d, size_t bytes, stream_t) { std::memcpy(h, d, bytes); }
void d2d(void* dst, const void* src, size_t bytes, stream_t) { std::memmove(dst, src, bytes); }
void h2d_2d(void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t height,
            stream_t) {
  for (size_t r = 0; r < height; ++r)
    std::memcpy((char*)d + r * dpitch, (const char*)h + r * hpitch, width);
}
void d2h_2d(void* h, size_t hpitch, const void* d, size_t dpitch, size_t width, size_t height,
            stream_t) {
  for (size_t r = 0; r < height; ++r)
    std::memcpy((char*)h + r * hpitch, (const char*)d + r * dpitch, width);
}
void d2d_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
            stream_t) {
  for (size_t r = 0; r < height; ++r)
    std::memmove((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
}
void dzero(void* d, size_t bytes, stream_t) { std::memset(d, 0, bytes); }
void enable_peer_access(int dev, int peer) {
  if (dev < 0 || dev >= device_count() || peer < 0 || peer >= device_count()) throw std::runtime_error("emu: invalid peer");
}
void copy_peer(void* dst, int, const void* src, int, size_t bytes, stream_t) { std::memmove(dst, src, bytes); }

int pointer_device(const void*) { return POINTER_ANY; }  // "device memory" is host memory here

stream_t stream_create() { return (stream_t)1; }
stream_t stream_create_upload() { return (stream_t)1; }
void stream_destroy(stream_t) {}
void stream_sync(stream_t) {}
void stream_wait_event(stream_t, event_t) {}

struct EmuEvent {
  std::chrono::steady_clock::time_point t;
};
event_t event_create() { return new EmuEvent(); }
event_t event_create_sync() { return new EmuEvent(); }
void event_destroy(event_t e) { delete (EmuEvent*)e; }
void event_record(event_t e, stream_t) { ((EmuEvent*)e)->t = std::chrono::steady_clock::now(); }
void event_sync(event_t) {}
float event_elapsed_ms(event_t a, event_t b) {
  return std::chrono::duration<float, std::milli>(((EmuEvent*)b)->t - ((EmuEvent*)a)->t).count();
}

bool graphs_supported() { return false; }
void capture_begin(stream_t) { throw std::runtime_error("mvn: no graphs in the host emulation"); }
graph_exec_t capture_end(stream_t) { throw std::runtime_error("mvn: no graphs in the host emulation"); }
void graph_launch(graph_exec_t, stream_t) { throw std::runtime_error("mvn: no graphs in the host emulation"); }
void graph_destroy(graph_exec_t) {}

// wave-row kernels (d2 = 512, mvn_wave_rows.hpp): a "grid" of about a third of the workgroups a
// one-sweep launch would have, so that the sweep loop and its ragged tail are exercised
// same knobs as the HIP backend, but read at every launch and with every pass enabled by default
// (the emulation exists to test them)
static bool emu_wave_rows(const RowsParams& p, int kind_bit) { return wr_rows_enabled(p, wr_rows_mask(31), kind_bit); }

template <int MODE, int EPI>
static void emu_wave_rows_run(const RowsParams& p) {
  typedef FxCtx<WrRegs, WrCfg::NT> Ctx;
  const long pairs = (p.rows + 1) / 2;
  const long full = (pairs + WrCfg::WAVES - 1) / WrCfg::WAVES;
  const long grid = full > 2 ? (full + 2) / 3 : full;
#pragma omp parallel
  {
    std::vector<char> lds(sizeof(cfloat) * WrCfg::lds_cfloats + 64);
    std::unique_ptr<Ctx> ctx(new Ctx());
#pragma omp for schedule(static)
    for (long b = 0; b < grid; ++b) wr_rows_body<MODE, EPI>(p, b, grid, (cfloat*)lds.data(), *ctx);
  }
}

// fixed-length kernels: every phase is run for all thread ids in turn (real thread mapping)
// "grid" of a fixed last-axis launch: one workgroup per tile, or for the walking configurations
// about a third as many, so that the tile loop is exercised
template <int H>
static long emu_rows_grid(long ntiles) {
  return FxRowsCfg<H>::WALK && ntiles > 2 ? (ntiles + 2) / 3 : ntiles;
}

// `grid` workgroups of a fixed last-axis launch (KIND: MvnPassKind), one register context per host thread
template <int H, int KIND, int EPI, bool LINES>
static void emu_rows_fixed_run(const RowsParams& p, long grid) {
  typedef FxCtx<FxRowsRegsFor<H, EPI>, FxRowsCfg<H>::NT> Ctx;
#pragma omp parallel
  {
    std::vector<char> lds(sizeof(cfloat) * FxRowsCfg<H>::lds_cfloats + 64);
    std::unique_ptr<Ctx> ctx(new Ctx());
#pragma omp for schedule(static)
    for (long t = 0; t < grid; ++t) fx_rows_workgroup<H, KIND, EPI, LINES>(p, t, grid, (cfloat*)lds.data(), *ctx);
  }
}

// the tiles of a run-time-radix launch, one "thread" per workgroup
template <int KIND, int T, int FORM>
static void emu_rows_generic_run(const RowsParams& p, bool even, long ntiles, size_t lds_bytes) {
#pragma omp parallel
  {
    std::vector<char> lds(lds_bytes + 64);
#pragma omp for schedule(static)
    for (long t = 0; t < ntiles; ++t) {
      cfloat* l = (cfloat*)lds.data();
      if constexpr (KIND == MVN_PASS_R2C) {
        if (even)
          rows_r2c_even_body<T>(p, t, 0, 1, l);
        else
          rows_r2c_odd_body<T>(p, t, 0, 1, l);
      } else if constexpr (KIND == MVN_PASS_C2R) {
        if (even)
          rows_c2r_even_body<T, false, FORM>(p, t, 0, 1, l);
        else
          rows_c2r_odd_body<T, FORM>(p, t, 0, 1, l);
      } else {
        rows_c2r_even_body<T, true, FORM>(p, t, 0, 1, l);  // (even extents only: Plan3D::rows_c2r_r2c)
      }
    }
  }
}

// The three last-axis passes, as in the product: the families in their order - line layout, wave rows, fixed length,
// run-time radix - each behind the one dispatch of the launch's mode (mvn_pass_bodies.hpp)
template <int KIND>
static void emu_rows(const RowsParams& p0, bool even, long ntiles, size_t lds_bytes) {
  RowsParams p = p0;
  if (KIND != MVN_PASS_R2C) mvn_arm_poison(p.epi);  // (the device kernels do this at their entry)
  const int mode = p.epi.mode;
  if (p.lines) {  // (H = 256: d2 = 512)
    fx_rows_lines_check(p, ntiles);
    return mvn_epi_dispatch<KIND>(mode, [&](auto epi) { emu_rows_fixed_run<256, KIND, decltype(epi)::value, true>(p, ntiles); });
  }
  if (emu_wave_rows(p, mvn_wave_rows_kind_bit(KIND, mode)))
    return mvn_epi_dispatch<KIND>(mode, [&](auto epi) { emu_wave_rows_run<KIND, decltype(epi)::value>(p); });
  if (p.fixed) {
    switch (p.h) {
#define X(H)                                                                                     \
  case H:                                                                                        \
    return mvn_epi_dispatch<KIND>(mode, [&](auto epi) {                                          \
      emu_rows_fixed_run<H, KIND, decltype(epi)::value, false>(p, emu_rows_grid<H>(ntiles));     \
    });
      MVN_FIXED_ROWS_LENGTHS(X)
#undef X
      default: throw std::invalid_argument("mvn: no fixed kernel");
    }
  }
  mvn_epi_dispatch<KIND, true>(mode, [&](auto form) {
    mvn_dispatch_tile_width(p.T, [&](auto t) {
      emu_rows_generic_run<KIND, decltype(t)::value, decltype(form)::value>(p, even, ntiles, lds_bytes);
    });
  });
}

void launch_rows_r2c(const RowsParams& p, bool even, long ntiles, int, size_t lds_bytes, stream_t) {
  emu_rows<MVN_PASS_R2C>(p, even, ntiles, lds_bytes);
}
void launch_rows_c2r(const RowsParams& p, bool even, long ntiles, int, size_t lds_bytes, stream_t) {
  emu_rows<MVN_PASS_C2R>(p, even, ntiles, lds_bytes);
}
void launch_rows_c2r_r2c(const RowsParams& p, long ntiles, int, size_t lds_bytes, stream_t) {
  emu_rows<MVN_PASS_C2R_R2C>(p, true, ntiles, lds_bytes);
}

static std::atomic<long> g_mid_fused_launches{0};
long mid_fused_launch_count() { return g_mid_fused_launches.load(); }

// the fused middle pass (mvn_mid_fused.hpp), one workgroup after the other
template <int K>
static void emu_mid_fused(const MidFusedParams& p) {
  typedef FxCtx<MfRegs<K>, MF_NT> Ctx;
  const long blocks = mf_blocks(p);
#pragma omp parallel
  {
    std::vector<cfloat> lds(MF_LDS_CFLOATS + 8);
    std::unique_ptr<Ctx> ctx(new Ctx());
#pragma omp for schedule(static)
    for (long b = 0; b < blocks; ++b) mf_body<K>(p, b, lds.data(), *ctx);
  }
}
void launch_mid_fused(const MidFusedParams& p, stream_t) {
  mf_check(p);
  if (p.mode == MF_TAPS) {
    typedef FxCtx<MfRegs<1>, MF_NT> Ctx;
    const long blocks = mf_blocks(p);
#pragma omp parallel
    {
      std::vector<cfloat> lds(MF_LDS_CFLOATS + 8);
      std::unique_ptr<Ctx> ctx(new Ctx());
#pragma omp for schedule(static)
      for (long b = 0; b < blocks; ++b) mf_taps_body(p, b, lds.data(), *ctx);
    }
    return;
  }
  ++g_mid_fused_launches;
  switch (mvn_dim0_taps_template(p.k)) {
#define X(K) case K: emu_mid_fused<K>(p); break;
    MVN_MF_TAP_COUNTS(X)
#undef X
    default: throw std::invalid_argument("mvn: no fused middle pass for this tap count");
  }
}

template <int N, int MODE>
static void emu_strided_fixed_mode(const StridedParams& p0, long nblocks) {
  typedef FxStridedSel<N, MODE> Sel;
  typedef typename Sel::Ctx Ctx;
  StridedParams p = p0;
  p.nblocks = nblocks;
  // a "grid" of about half as many workgroups as tiles, so that the tile loop and its
  // prefetching are exercised (each workgroup walks over 1-2 tiles)
  const long grid = nblocks > 1 ? (nblocks + 1) / 2 : 1;
#pragma omp parallel
  {
    std::vector<char> lds(sizeof(cfloat) * FxStridedCfg<N>::lds_cfloats + 64);
    std::unique_ptr<Ctx> ctx(new Ctx());
#pragma omp for schedule(static)
    for (long b = 0; b < grid; ++b) Sel::run(p, b, nblocks, grid, (cfloat*)lds.data(), *ctx);
  }
}

static std::atomic<long> g_split_launches{0};
long split_launch_count() { return g_split_launches.load(); }

template <int N>
static bool emu_try_split(int mode, const StridedParams& p, long nblocks) {
  StridedParams q;
  if (!fx_split_retile<N>(mode, p, nblocks, q)) return false;
  if constexpr (FxSplitCfg<N>::USE) {
    typedef FxSplitCfg<N> C;
    const long nb = q.nblocks;
    ++g_split_launches;
    const long grid = nb > 1 ? (nb + 1) / 2 : 1;
    typedef FxCtx<FxSplitRegs<N>, C::NT> Ctx;
#pragma omp parallel
    {
      std::vector<char> lds(sizeof(cfloat) * C::lds_cfloats + 64);
      std::unique_ptr<Ctx> ctx(new Ctx());
#pragma omp for schedule(static)
      for (long b = 0; b < grid; ++b) {
        if (mode == MVN_ST_FWD)
          fx_strided_split_body<N, MVN_ST_FWD>(q, b, nb, grid, (cfloat*)lds.data(), *ctx);
        else
          fx_strided_split_body<N, MVN_ST_INV>(q, b, nb, grid, (cfloat*)lds.data(), *ctx);
      }
    }
  }
  return true;
}

template <int N>
static void emu_strided_fixed(int mode, const StridedParams& p, long nblocks) {
  if (emu_try_split<N>(mode, p, nblocks)) return;
  if (mode == MVN_ST_FWD) emu_strided_fixed_mode<N, MVN_ST_FWD>(p, nblocks);
  if (mode == MVN_ST_INV) emu_strided_fixed_mode<N, MVN_ST_INV>(p, nblocks);
  if (mode == MVN_ST_FWD_MUL_INV) emu_strided_fixed_mode<N, MVN_ST_FWD_MUL_INV>(p, nblocks);
}

static bool emu_strided_fixed_dispatch(int mode, const StridedParams& p, long nblocks) {
  switch (p.ax.n) {
#define X(N) case N: emu_strided_fixed<N>(mode, p, nblocks); return true;
    MVN_FIXED_STRIDED_LENGTHS(X)
#undef X
    default: return false;
  }
}

void launch_convergence_reduce(const double* rec, const unsigned* counts, int nviews, long cap, double* out,
                               stream_t) {
  double lds[3];
  mvn_convergence_reduce_body(rec, counts, nviews, cap, out, lds, 0, 1);
}

void launch_nm_reduce(const double* rec, const unsigned* counts, int nviews, long cap, double* out, stream_t) {
  double lds[3];
  for (long v = 0; v < nviews; ++v) mvn_nm_reduce_body(rec + 3 * v * cap, counts + v, cap, out + 3 * v, lds, 0, 1);
}

void launch_strided(int mode, const StridedParams& p, long nblocks, int, size_t lds_bytes,
                    stream_t, const StridedParams* rider, size_t rider_lds) {
  mvn_strided_rider_check(mode, p, rider, rider_lds);
  if (p.fixed) {
    if (!emu_strided_fixed_dispatch(mode, p, nblocks)) throw std::invalid_argument("mvn: no fixed kernel");
    if (rider) {  // the workgroups behind the walkers: one line each
      const long lines = rider->tiles_per_outer;
#pragma omp parallel
      {
        std::vector<char> lds(rider_lds + 64);
#pragma omp for schedule(static)
        for (long b = 0; b < lines; ++b) {
          cfloat* l = (cfloat*)lds.data();
          if (mode == MVN_ST_FWD)
            strided_body<MVN_ST_FWD, 1, true>(*rider, b, 0, 1, l);
          else
            strided_body<MVN_ST_INV, 1, true>(*rider, b, 0, 1, l);
        }
      }
    }
    return;
  }
  mvn_dispatch_tile_width(p.T, [&](auto tt) {
    constexpr int T = decltype(tt)::value;
#pragma omp parallel
    {
      std::vector<char> lds(lds_bytes + 64);
#pragma omp for schedule(static)
      for (long b = 0; b < nblocks; ++b) {
        cfloat* l = (cfloat*)lds.data();
        if (mode == MVN_ST_FWD) strided_body<MVN_ST_FWD, T, true>(p, b, 0, 1, l);
        if (mode == MVN_ST_INV) strided_body<MVN_ST_INV, T, true>(p, b, 0, 1, l);
        if (mode == MVN_ST_FWD_MUL_INV) strided_body<MVN_ST_FWD_MUL_INV, T, true>(p, b, 0, 1, l);
      }
    }
  });
}

void launch_dim0_direct(const Dim0DirectParams& p, stream_t) {
  mvn_dim0_check(p);
  if (p.packed) {
#pragma omp parallel
    {
      std::vector<cfloat> lds(2 * (size_t)p.d0 + 2 * (size_t)p.k);
#pragma omp for schedule(static)
      for (int pair = 0; pair < mvn_dim0_pairs(p.d1); ++pair) {
        for (int t = 0; t < 256; ++t) mvn_dim0_dc_load(p, pair, lds.data(), t, 256);
        for (int t = 0; t < 256; ++t) mvn_dim0_dc_compute(p, pair, lds.data(), t, 256);
      }
    }
  }
  switch (mvn_dim0_taps_template(p.k)) {
#define X(K)                                                                        \
  case K: {                                                                         \
    const long nblocks = mvn_dim0_blocks(p).blocks;                                 \
    _Pragma("omp parallel for schedule(static)")                                    \
    for (long blk = 0; blk < nblocks; ++blk)                                        \
      for (int t = 0; t < MVN_D0_WG; ++t) {                                         \
        Dim0DirectParams q;                                                         \
        long b;                                                                     \
        int zs, nout;                                                               \
        if (mvn_dim0_job(p, blk, t, q, b, zs, nout)) mvn_dim0_direct_column<K, MVN_D0_PF>(q, b, zs, nout); \
      }                                                                             \
  } break;
    MVN_D0_TAP_COUNTS(X)
#undef X
    default: throw std::invalid_argument("mvn: no direct dim0 kernel for this tap count");
  }
}

void launch_scatter_psf(const float* kernel, int k0, int k1, int k2, float* target, int D0,
                        int D1, int D2, long pitch, float scale, stream_t) {
  const long total = (long)k0 * k1 * k2;
  for (long i = 0; i < total; ++i) mvn_scatter_psf_item(kernel, k0, k1, k2, target, D0, D1, D2, pitch, scale, i);
}

void launch_copy3d(float* dst, long drow, long dplane, const float* src, long srow, long splane,
                   int nx, int ny, int nz, stream_t) {
  for (long z = 0; z < nz; ++z)
    for (long y = 0; y < ny; ++y)
      std::memcpy(dst + z * dplane + y * drow, src + z * splane + y * srow, sizeof(float) * (size_t)nx);
}

void launch_ingest3d(const IngestParams& p, bool u16, stream_t, bool dst_u16) {
  if (dst_u16 && (!u16 || p.use_value)) throw std::invalid_argument("mvn: a uint16 volume takes a uint16 stack");
  const long nblocks = mvn_ingest_blocks(p.rows);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_INGEST_WG; ++t) {
      if (dst_u16)
        mvn_ingest_rows<uint16_t, uint16_t>(p, blk, t);
      else if (u16)
        mvn_ingest_rows<uint16_t>(p, blk, t);
      else
        mvn_ingest_rows<float>(p, blk, t);
    }
}

void launch_extract3d(const ExtractParams& p, stream_t) {
  const long nblocks = mvn_extract_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_INGEST_WG; ++t) mvn_extract_rows(p, blk, t);
}

static std::atomic<long long> g_reflect_launches{0}, g_reflect_volumes{0};
void reflect_counters(long long out[2]) {
  out[0] = g_reflect_launches.load();
  out[1] = g_reflect_volumes.load();
}

void launch_reflect_fill(const ReflectParams& p0, bool u16, stream_t) {
  mvn_reflect_check(p0);
  ReflectParams p = p0;
  for (int axis = 2; axis >= 0; --axis) {
    p.axis = axis;
    const long nblocks = mvn_ingest_blocks(mvn_reflect_rows_of(p));
    if (nblocks < 1) continue;  // (no margin along this axis)
    ++g_reflect_launches;
#pragma omp parallel for schedule(static)
    for (long blk = 0; blk < nblocks; ++blk)
      for (int t = 0; t < MVN_INGEST_WG; ++t) {
        if (u16)
          mvn_reflect_rows<uint16_t>(p, blk, t);
        else
          mvn_reflect_rows<float>(p, blk, t);
      }
  }
  ++g_reflect_volumes;
}

static std::atomic<long long> g_resample_launches{0}, g_normalize_launches{0};
void resample_counters(long long out[2]) {
  out[0] = g_resample_launches.load();
  out[1] = g_normalize_launches.load();
}

void launch_resample(const ResampleParams& p, bool u16, stream_t) {
  mvn_resample_check(p);
  const long nblocks = mvn_resample_blocks(p);
  ++g_resample_launches;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_RS_WG; ++t) {
      if (u16)
        mvn_resample_tile<uint16_t>(p, blk, t);
      else
        mvn_resample_tile<float>(p, blk, t);
    }
}

void launch_weights_normalize(const NormalizeParams& p, stream_t) {
  mvn_normalize_check(p);
  const long nblocks = mvn_normalize_blocks(p);
  ++g_normalize_launches;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_INGEST_WG; ++t) mvn_normalize_rows(p, blk, t);
}

static std::atomic<long long> g_fuse_raw_launches{0}, g_fuse_volumes_launches{0};
void fuse_counters(long long out[2]) {
  out[0] = g_fuse_raw_launches.load();
  out[1] = g_fuse_volumes_launches.load();
}

void launch_fuse_resampled(const FuseParams& p, stream_t) {
  mvn_fuse_check(p);
  const long nblocks = mvn_fuse_blocks(p);
  ++g_fuse_raw_launches;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_RS_WG; ++t) mvn_fuse_tile(p, blk, t);
}

void launch_fuse_volumes(const FuseVolumesParams& p, stream_t) {
  mvn_fuse_volumes_check(p);
  const long nblocks = mvn_fuse_volumes_blocks(p);
  ++g_fuse_volumes_launches;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_INGEST_WG; ++t) mvn_fuse_rows(p, blk, t);
}

static std::atomic<long long> g_psf_correlate_launches{0};
long long psf_correlate_launches() { return g_psf_correlate_launches.load(); }

void launch_psf_normalize(const PsfNormParams& p, stream_t) {
  mvn_psf_norm_check(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < (long)p.count; ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_sum_item(p, blk, t);
  const long nblocks = p.count * mvn_psf_blocks(p.n);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_scale_item(p, blk, t);
}

void launch_psf_pointwise(const PsfPointParams& p, stream_t) {
  mvn_psf_point_check(p);
  const long nblocks = p.V * mvn_psf_blocks(p.n);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_pointwise_item(p, blk, t);
}

void launch_psf_correlate(const PsfCorrParams& p, stream_t) {
  mvn_psf_corr_check(p);
  ++g_psf_correlate_launches;
  const long nblocks = (long)p.njobs * p.blocks_per_job;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_correlate_item(p, blk, t);
}

static std::atomic<long long> g_beads_gather_launches{0}, g_beads_score_launches{0};
void beads_counters(long long out[2]) {
  out[0] = g_beads_gather_launches.load();
  out[1] = g_beads_score_launches.load();
}

void launch_beads_gather(const BeadsParams& p, bool u16, stream_t) {
  mvn_beads_check(p);
  const long nblocks = (long)mvn_beads_groups(p.nbeads) * mvn_beads_tiles(p);
  ++g_beads_gather_launches;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) {
      if (u16)
        mvn_beads_gather_item<uint16_t>(p, blk, t);
      else
        mvn_beads_gather_item<float>(p, blk, t);
    }
}

void launch_beads_reduce(const BeadsParams& p, stream_t) {
  mvn_beads_check(p);
  const long nblocks = mvn_beads_tiles(p);
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_reduce_item(p, blk, t);
}

void launch_beads_remove_min(const BeadsParams& p, stream_t) {
  mvn_beads_check(p);
  if (!p.minima) throw std::invalid_argument("mvn: beads: null pointer");
  for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_min_item(p, t);
  const long nblocks = mvn_beads_tiles(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_sub_item(p, blk, t);
}

void launch_beads_score(const BeadsParams& p, bool u16, stream_t) {
  mvn_beads_check(p);
  if (!p.records || !p.scores) throw std::invalid_argument("mvn: beads: null pointer");
  ++g_beads_score_launches;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < (long)p.nbeads; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) {
      if (u16)
        mvn_beads_score_item<uint16_t>(p, blk, t);
      else
        mvn_beads_score_item<float>(p, blk, t);
    }
  const long folds = ((long)p.nbeads + MVN_BEADS_WG - 1) / MVN_BEADS_WG;
  for (long blk = 0; blk < folds; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_score_fold_item(p, blk, t);
}

static std::atomic<long long> g_detect_blur_launches{0}, g_detect_extrema_launches{0};
void detect_counters(long long out[2]) {
  out[0] = g_detect_blur_launches.load();
  out[1] = g_detect_extrema_launches.load();
}

void launch_detect_blur(const DetectParams& p, bool u16, stream_t) {
  mvn_detect_check_blur(p);
  g_detect_blur_launches += 3;
  if (u16)
    mvn_detect_rows_host<uint16_t>(p);
  else
    mvn_detect_rows_host<float>(p);
  mvn_detect_lines_host<1>(p);
  mvn_detect_lines_host<0>(p);
}

void launch_detect_extrema(const DetectParams& p, stream_t) {
  mvn_detect_check_list(p);
  ++g_detect_extrema_launches;
  mvn_detect_extrema_host(p);
}

void launch_detect_refine(const DetectParams& p, stream_t) {
  mvn_detect_check_list(p);
  if (p.nfound < 1 || p.nfound > p.list_cap || !p.pos || !p.val || !p.vox)
    throw std::invalid_argument("mvn: detect: nothing to refine");
  mvn_detect_refine_host(p);
}

static std::atomic<long long> g_register_match_launches{0}, g_register_ransac_launches{0};
void register_counters(long long out[2]) {
  out[0] = g_register_match_launches.load();
  out[1] = g_register_ransac_launches.load();
}

void launch_register_neighbours(const RegParams& p, stream_t) {
  mvn_reg_check_neighbours(p);
  mvn_reg_neighbours_host(p);
}

void launch_register_match(const RegParams& p, stream_t) {
  mvn_reg_check_match(p);
  ++g_register_match_launches;
  mvn_reg_match_host(p);
}

void launch_register_ransac(const RegParams& p, stream_t) {
  mvn_reg_check_ransac(p);
  ++g_register_ransac_launches;
  mvn_reg_ransac_host(p);
}

static std::atomic<long> g_tv_launches{0};
long tv_launch_count() { return g_tv_launches.load(); }
void launch_tv(const TvParams& p0, stream_t) {
  TvParams p = p0;
  mvn_tv_geometry(p);
  if (p.d0 < 1 || p.d1 < 1 || p.d2 < 1 || p.RP < p.d2 || (long)p.d1 * p.RP > 0x7fffffffL)
    throw std::invalid_argument("mvn: total-variation pass outside its range");
  ++g_tv_launches;
  mvn_tv_host(p);
}

void launch_accel_a(const AccelParams& p, stream_t) { mvn_accel_host_a(p); }
void launch_accel_reduce(const double* rec, long nrec, float* alpha, stream_t) { mvn_accel_host_reduce(rec, nrec, alpha); }
void launch_accel_b(const AccelParams& p, stream_t) { mvn_accel_host_b(p); }

void launch_divide(const float* view, float* inout, size_t n, stream_t) {
  for (size_t i = 0; i < n; ++i) inout[i] = mvn_quotient(view[i], inout[i]);
}

void launch_update(float* psi, const float* integral, const float* weights, size_t n,
                   double lambda, float min_value, stream_t) {
  const float linv = lambda > 0 ? (float)(1.f / lambda) : 0.f;
  for (size_t i = 0; i < n; ++i) {
    float last = psi[i];
    float next = mvn_next_value(last, integral[i], lambda, linv, min_value);
    psi[i] = weights[i] * (next - last) + last;
  }
}

void launch_update_legacy_tikhonov(float* image, const float* integral, const float* weights,
                                   size_t n, float lambda_f, float min_value, stream_t) {
  for (size_t i = 0; i < n; ++i)
    image[i] = mvn_legacy_tikhonov_value(image[i], integral[i], weights[i], lambda_f, min_value);
}

void launch_axpy1(float* psi, const float* delta, size_t n, stream_t) {
  for (size_t i = 0; i < n; ++i) psi[i] += delta[i];
}

}  // namespace be
}  // namespace mvn
