// mvn_engine.cpp -- see mvn_engine.hpp
#include "mvn_engine.hpp"

#include <algorithm>
#include <cmath>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "mvn_fixed_geom.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace mvn {

static const size_t kLdsSoftBudget = 80 * 1024;   // two workgroups per CU (160 KiB LDS)
static const size_t kLdsHardBudget = 160 * 1024;  // one workgroup may own the whole CU
static const size_t kSideMinBytes = 16u << 20;    // volumes above this use the side stream (see Engine::conv_pair)

const char* kernel_kind_name(int k) {
  static const char* names[KK_COUNT] = {"rows_r2c",    "rows_c2r",  "rows_fused_div",
                                        "rows_fused_upd", "axis1_fwd", "axis1_inv",
                                        "axis0_fused", "axis0_fwd",  "axis0_inv",
                                        "nyquist",     "other",     "axis0_direct", "mid_fused",
                                        "tv_factor"};
  return (k >= 0 && k < KK_COUNT) ? names[k] : "?";
}

// ---------------------------------------------------------------------------------------------
// Profiler
// ---------------------------------------------------------------------------------------------
be::Event Profiler::get_event() {
  if (pool_.empty()) return be::Event::timing();
  be::Event e = std::move(pool_.back());
  pool_.pop_back();
  return e;
}

void Profiler::begin(int kind, be::stream_t s) {
  if (!enabled) return;
  Rec r;
  r.kind = kind;
  r.a = get_event();
  r.b = get_event();
  be::event_record(r.a.get(), s);
  recs_.push_back(std::move(r));
}

void Profiler::end(be::stream_t s) {
  if (!enabled || recs_.empty()) return;
  be::event_record(recs_.back().b.get(), s);
}

void Profiler::collect() {
  for (size_t i = 0; i < recs_.size(); ++i) {
    be::event_sync(recs_[i].b.get());
    total_ms[recs_[i].kind] += be::event_elapsed_ms(recs_[i].a.get(), recs_[i].b.get());
    count[recs_[i].kind] += 1;
    pool_.push_back(std::move(recs_[i].a));
    pool_.push_back(std::move(recs_[i].b));
  }
  recs_.clear();
}

void Profiler::reset() {
  collect();
  for (int k = 0; k < KK_COUNT; ++k) {
    total_ms[k] = 0;
    count[k] = 0;
  }
}

Profiler::~Profiler() {
  try {
    collect();
  } catch (...) {
  }
}

struct ProfScope {
  Profiler* p;
  be::stream_t s;
  ProfScope(Profiler* p_, int kind, be::stream_t s_) : p(p_), s(s_) {
    if (p) p->begin(kind, s);
  }
  ~ProfScope() {
    if (p) p->end(s);
  }
};

// ---------------------------------------------------------------------------------------------
// DevAxis / Plan3D
// ---------------------------------------------------------------------------------------------
template <typename T>
static be::DeviceBuffer<T> upload(const std::vector<T>& src) {
  be::DeviceBuffer<T> d(sizeof(T) * src.size());
  be::h2d(d.get(), src.data(), sizeof(T) * src.size(), nullptr);
  return d;
}

DevAxis::DevAxis(int n, bool composite) : host(n, composite) {
  tw = upload(host.tw);  // nfft entries
  rev = upload(host.rev);
  inv = upload(host.inv);
  if (!host.tws.empty()) tws = upload(host.tws);
  if (host.bluestein) {
    chirp = upload(host.chirp);
    bhat = upload(host.bhat);
  }
  be::stream_sync(nullptr);
  view = host.view(tw.get(), rev.get(), inv.get(), tws.get(), chirp.get(), bhat.get());
}

static int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}

PassGeom Plan3D::pick_geom(int n, bool generic, bool rows, int max_t) {
  static const int cand[5] = {16, 8, 4, 2, 1};
  PassGeom g;
  bool found = false;
  for (int pass = 0; pass < 2 && !found; ++pass) {
    const size_t budget = pass == 0 ? kLdsSoftBudget : kLdsHardBudget;
    for (int i = 0; i < 5; ++i) {
      const int T = cand[i];
      if (T > max_t) continue;
      const int TP = rows ? (T | 1) : T;  // odd pitch keeps the row transpose conflict-free
      const size_t one = (size_t)n * (size_t)TP * sizeof(cfloat);
      const size_t twb = (size_t)n * sizeof(cfloat);  // LDS copy of the twiddle table
      const size_t bytes = one * (generic ? 2 : 1) + twb;
      if (bytes <= budget) {
        g.T = T;
        g.TP = TP;
        g.lds_bytes = bytes;
        g.lds_alt = generic ? (long)n * TP : 0;
        g.lds_tw = (long)n * TP * (generic ? 2 : 1);
        found = true;
        break;
      }
    }
  }
  if (!found)
    throw std::invalid_argument("mvn: axis length " + std::to_string(n) +
                                " does not fit the single-pass LDS FFT (160 KiB)");
  // long strided axes: 32-byte row segments (T = 4) waste HBM bursts; one workgroup per CU with
  // 64-byte segments is the better trade (measured at n = 1920: 5.2 -> 4.1 ms per pass)
  if (!rows && g.T < 8 && max_t >= 8) {
    const size_t one = (size_t)n * 8 * sizeof(cfloat);
    const size_t bytes = one * (generic ? 2 : 1) + (size_t)n * sizeof(cfloat);
    if (bytes <= kLdsHardBudget - 4096) {
      g.T = g.TP = 8;
      g.lds_bytes = bytes;
      g.lds_alt = generic ? (long)n * 8 : 0;
      g.lds_tw = (long)n * 8 * (generic ? 2 : 1);
    }
  }
  // one radix-8 butterfly per thread and stage when the tile is big enough
  const long work = (long)n * g.T / 8;
  g.threads = work >= 512 ? 512 : (work >= 256 ? 256 : (work >= 128 ? 128 : 64));
  return g;
}

// ---- the PSF form rule (mvn_engine.hpp) -------------------------------------------------------
// MVN_DIM0_DIRECT_MAX: most PSF planes the direct dim0 leg takes on (MVN_D0_MAX_TAPS = 33 are instantiated);
// measured at 512^3 x 6 views on MI355X (profiles/r03_dim0_direct.md) the whole iteration is 6.7 / 4.1 % faster
// than with the fused FFT pass at 15 / 31 planes.  MVN_DIM0_DIRECT_MIN_PLANE: work items a launch should have
// (columns are cut into pieces below that, default 131072); MVN_DIM0_DIRECT_MIN_ITEMS: fewest work items for which
// the leg is used at all (default 0: it wins at every size measured, profiles/r03_shapes.txt - 32^3 0.098 -> 0.062
// ms per view update, 128^3 0.132 -> 0.079, 256^3 0.311 -> 0.245, 512^3 2.31 -> 2.16, 1024^3 19.9 -> 17.4 - on
// small volumes because the packed Nyquist layout it allows removes 6 of 14 launches).
FormSwitches FormSwitches::from_env() {
  FormSwitches sw;
  sw.direct = env_int("MVN_DIM0_DIRECT", 1) != 0;
  sw.direct_max = env_int("MVN_DIM0_DIRECT_MAX", MVN_D0_MAX_TAPS);
  sw.min_plane = env_int("MVN_DIM0_DIRECT_MIN_PLANE", 131072);
  sw.min_items = env_int("MVN_DIM0_DIRECT_MIN_ITEMS", 0);
  sw.mid_fused = env_int("MVN_MID_FUSED", 1);
  sw.fixed = env_int("MVN_NO_FIXED", 0) == 0;
  return sw;
}

bool rows_fixed(const Layout& L, bool fixed) {
  int T = 0, threads = 0;
  size_t lds = 0;
  return fixed && L.even && fixed_rows_geom(L.h, &T, &threads, &lds) && L.rows % (size_t)T == 0;
}
bool ax1_fixed(const Layout& L, bool fixed) {
  int T = 0, threads = 0;
  size_t lds = 0;
  return fixed && fixed_strided_geom(L.d1, &T, &threads, &lds) && L.C % T == 0;
}
bool ax0_fixed(const Layout& L, bool fixed) {
  int T = 0, threads = 0;
  size_t lds = 0;
  return fixed && fixed_strided_geom(L.d0, &T, &threads, &lds) && ((long)L.d1 * L.C) % T == 0;
}

// (d1 = MF_N1 = 512 is a power of two: its dim1 transform is a plain radix one of length 512, never chirp-z)
bool lines_capable(const Layout& L, bool fixed) {
  int T = 0, threads = 0;
  size_t lds = 0;
  return rows_fixed(L, fixed) && fixed_rows_geom(L.h, &T, &threads, &lds) && T == 16 && L.h == 256 && L.C == 256 &&
         L.d1 == MF_N1;
}

bool FormRule::direct(const int* kdims) const {
  if (!sw.direct || kdims[0] > sw.direct_max || !mvn_dim0_direct_possible(kdims[0], L.d0) ||
      mvn_dim0_items_for(kdims[0], L.d0, (long)L.d1 * L.C, sw.min_plane) < sw.min_items)
    return false;
  const Layout T(taps_depth(kdims[0]), L.d1, L.d2);  // (C, RP and parity: same d2 as L)
  return rows_fixed(T, sw.fixed) == rows_fixed(L, plan_fixed) && ax1_fixed(T, sw.fixed) == ax1_fixed(L, plan_fixed);
}

bool FormRule::lines_taps(const int* kdims) const {
  return sw.mid_fused != 0 && lines_capable(L, plan_fixed) && direct(kdims) &&
         lines_capable(Layout(taps_depth(kdims[0]), L.d1, L.d2), sw.fixed) && mvn_dim0_taps_template(kdims[0]) <= 31;
}

// A whole column walks d0 + K - 1 steps for d0 outputs (the first K - 1 fill the filter's window).  Measured per view
// update on (d0, 512, 512) volumes (tools/mid_fused_planes.py, profiles/r04_mid_fused.md): with 31-plane PSFs the two
// forms meet at 96 - 128 planes (48: +10 %, 256: -15 %, 512: -18 %), with 15 planes the fused pass is ahead from 32
// planes on (-2 %; 256: -24 %), with 5 planes always (-12 .. -30 %): three PSF depths of planes.
bool FormRule::lines_worth(int k0) const { return sw.mid_fused >= 2 || L.d0 >= 3 * k0; }

bool FormRule::all_direct(const kernel_list_t& k) const {
  for (const std::array<int, 3>& d : k)
    if (!direct(d.data())) return false;
  return true;
}

bool FormRule::all_lines(const kernel_list_t& k) const {
  for (const std::array<int, 3>& d : k)
    if (!lines(d.data())) return false;
  return true;
}

Plan3D::Plan3D(int dev, int d0, int d1, int d2, bool fixed_allowed)
    : device(dev), L(d0, d1, d2), fixed(fixed_allowed), ax2(L.h, rows_fixed(L, fixed)), ax1(d1, ax1_fixed(L, fixed)),
      ax0(d0, ax0_fixed(L, fixed)) {
  // the word an epilogue that follows no direct dim0 leg compares with (EpilogueParams::poison is never null
  // on the device): zero, against the epoch 0xffffffff no leg ever has
  no_poison = be::DeviceBuffer<unsigned>(64);
  be::dzero(no_poison.get(), 64, nullptr);
  be::stream_sync(nullptr);
  if (L.even) {
    std::vector<cfloat> roots((size_t)L.h / 2 + 1);
    for (size_t k = 0; k < roots.size(); ++k) {
      double a = -2.0 * M_PI * (double)k / (double)d2;
      roots[k].x = (float)std::cos(a);
      roots[k].y = (float)std::sin(a);
    }
    twr = be::DeviceBuffer<cfloat>(sizeof(cfloat) * roots.size());
    be::h2d(twr.get(), roots.data(), sizeof(cfloat) * roots.size(), nullptr);
    be::stream_sync(nullptr);
  }
  // LDS rows per tile = length of the radix transform (the chirp-z length for bluestein axes)
  // widest tile 16 for all three pass families (the fused pass on MI355X at 512^3: T=16 0.46 ms, T=8 0.63 ms)
  g_rows = pick_geom(ax2.host.nfft, ax2.host.generic, true, 16);
  g_ax1 = pick_geom(ax1.host.nfft, ax1.host.generic, false, 16);
  g_ax0 = pick_geom(ax0.host.nfft, ax0.host.generic, false, 16);
  g_nyq1 = g_ax1;
  g_nyq0 = g_ax0;
  g_nyq1_line = pick_geom(ax1.host.nfft, ax1.host.generic, false, 1);  // one line per workgroup (riders)
  // fixed-length fast path: full tiles, 16-byte aligned rows
  {
    int T = 0, threads = 0;
    size_t lds = 0;
    if (rows_fixed(L, fixed)) {
      fixed_rows_geom(L.h, &T, &threads, &lds);
      fx_rows = true;
      gx_rows.T = T;
      gx_rows.threads = threads;
      gx_rows.lds_bytes = lds;
    }
    if (ax1_fixed(L, fixed)) {
      fixed_strided_geom(d1, &T, &threads, &lds);
      fx_ax1 = true;
      gx_ax1.T = gx_ax1.TP = T;
      gx_ax1.threads = threads;
      gx_ax1.lds_bytes = lds;
    }
    if (ax0_fixed(L, fixed)) {
      fixed_strided_geom(d0, &T, &threads, &lds);
      fx_ax0 = true;
      gx_ax0.T = gx_ax0.TP = T;
      gx_ax0.threads = threads;
      gx_ax0.lds_bytes = lds;
    }
  }
}

// a range of rows of a last-axis pass: whole tiles where the kernels need them
static long rows_in_range(const Plan3D& P, long row0, long nrows) {
  const long all = (long)P.L.rows;
  const long n = nrows < 0 ? all - row0 : nrows;
  if (row0 < 0 || n < 1 || row0 + n > all) throw std::out_of_range("mvn: row range of a last-axis pass");
  if (P.rows_need_full_tiles() && (row0 % P.rows_tile() || n % P.rows_tile()))
    throw std::logic_error("mvn: a row range of the fixed last-axis kernels must be whole tiles");
  return n;
}

// a last-axis pass on the line layout: the complex pointer stays at the volume's first element, the kernel gets the
// first row instead
static void lines_args(const Plan3D& P, RowsParams& p, long row0, const void* nyq, const void* real_side,
                       const void* cplx_side) {
  if (!P.lines_capable()) throw std::logic_error("mvn: this shape has no line-layout last-axis passes");
  if (nyq) throw std::logic_error("mvn: the line layout keeps the Nyquist bins in the DC column");
  if (real_side && real_side == cplx_side) throw std::logic_error("mvn: a plain last-axis pass on the line layout is out of place");
  p.lines = 1;
  p.lines_d1 = P.L.d1;
  p.row_base = row0;
  p.nyq_packed = 1;
}

void Plan3D::rows_r2c(const float* in_real, cfloat* out, cfloat* out_nyq, be::stream_t s,
                      Profiler* prof, long row0, long nrows, bool lines) const {
  const long R = rows_in_range(*this, row0, nrows);
  const void* real0 = in_real;
  in_real += row0 * L.RP;
  if (!lines) out += row0 * L.C;
  if (out_nyq) out_nyq += row0;
  RowsParams p;
  std::memset(&p, 0, sizeof(p));
  p.ax = ax2.view;
  p.twr = twr.get();
  p.d2 = L.d2;
  p.h = L.h;
  p.C = L.C;
  p.RP = L.RP;
  p.rows = R;
  p.T = g_rows.T;
  p.TP = g_rows.TP;
  p.lds_alt = g_rows.lds_alt;
  p.lds_tw = g_rows.lds_tw;
  p.hmul = mvn_fastdiv_mul((unsigned)L.h);
  p.Cmul = mvn_fastdiv_mul((unsigned)L.C);
  p.in_real = in_real;
  p.out_cplx = out;
  p.out_nyq = out_nyq;
  p.nyq_packed = (L.even && !out_nyq) ? 1 : 0;  // no Nyquist plane given: DC + i Nyquist in column 0
  if (lines) lines_args(*this, p, row0, out_nyq, real0, out);
  ProfScope ps(prof, KK_ROWS_R2C, s);
  if (fx_rows) {
    p.fixed = 1;
    p.T = gx_rows.T;
    be::launch_rows_r2c(p, true, R / p.T, gx_rows.threads, gx_rows.lds_bytes, s);
    return;
  }
  const long ntiles = (R + p.T - 1) / p.T;
  be::launch_rows_r2c(p, L.even, ntiles, g_rows.threads, g_rows.lds_bytes, s);
}

void Plan3D::rows_c2r(const cfloat* in, const cfloat* in_nyq, float* out_real,
                      const EpilogueParams& epi_all, be::stream_t s, Profiler* prof, long row0,
                      long nrows, bool lines, const MvnStatsParams* st) const {
  const long R = rows_in_range(*this, row0, nrows);
  const void* cplx0 = in;
  const void* real0 = out_real;
  if (!lines) in += row0 * L.C;
  if (in_nyq) in_nyq += row0;
  if (out_real) out_real += row0 * L.RP;
  EpilogueParams epi = epi_all;
  const long eoff = row0 * L.RP;
  // (the offsets below are in floats: a uint16 view is only ever divided by whole-volume launches, Engine::set_halo_hook)
  if (mvn_epi_u16(epi.mode) && row0 != 0) throw std::logic_error("mvn: a row range on a uint16 image volume");
  if (epi.view) epi.view += eoff;
  if (epi.psi) epi.psi += eoff;
  if (epi.weights) epi.weights += eoff;
  if (epi.delta) epi.delta += eoff;
  if (epi.tv) epi.tv += eoff;
  RowsParams p;
  std::memset(&p, 0, sizeof(p));
  p.ax = ax2.view;
  p.twr = twr.get();
  p.d2 = L.d2;
  p.h = L.h;
  p.C = L.C;
  p.RP = L.RP;
  p.rows = R;
  p.T = g_rows.T;
  p.TP = g_rows.TP;
  p.lds_alt = g_rows.lds_alt;
  p.lds_tw = g_rows.lds_tw;
  p.hmul = mvn_fastdiv_mul((unsigned)L.h);
  p.Cmul = mvn_fastdiv_mul((unsigned)L.C);
  p.in_cplx = in;
  p.in_nyq = in_nyq;
  p.nyq_packed = (L.even && !in_nyq) ? 1 : 0;
  if (lines) lines_args(*this, p, row0, in_nyq, real0, cplx0);
  p.out_real = out_real;
  p.epi = epi;
  if (!p.epi.poison) {
    p.epi.poison = no_poison.get();
    p.epi.poison_epoch = 0xffffffffu;
  }
  if (st) {
    p.st = *st;
    p.st.row0 = row0;
  }
  ProfScope ps(prof, KK_ROWS_C2R, s);
  if (fx_rows) {
    p.fixed = 1;
    p.T = gx_rows.T;
    be::launch_rows_c2r(p, true, R / p.T, gx_rows.threads, gx_rows.lds_bytes, s);
    return;
  }
  const long ntiles = (R + p.T - 1) / p.T;
  be::launch_rows_c2r(p, L.even, ntiles, g_rows.threads, g_rows.lds_bytes, s);
}

void Plan3D::rows_c2r_r2c(cfloat* data, cfloat* nyq, const EpilogueParams& epi_all, be::stream_t s,
                          Profiler* prof, long row0, long nrows, bool lines, const MvnStatsParams* st) const {
  if (!L.even) throw std::logic_error("mvn: rows_c2r_r2c needs an even last extent");
  const long R = rows_in_range(*this, row0, nrows);
  if (!lines) data += row0 * L.C;
  if (nyq) nyq += row0;
  EpilogueParams epi = epi_all;
  const long eoff = row0 * L.RP;
  // (the offsets below are in floats: a uint16 view is only ever divided by whole-volume launches, Engine::set_halo_hook)
  if (mvn_epi_u16(epi.mode) && row0 != 0) throw std::logic_error("mvn: a row range on a uint16 image volume");
  if (epi.view) epi.view += eoff;
  if (epi.psi) epi.psi += eoff;
  if (epi.weights) epi.weights += eoff;
  if (epi.delta) epi.delta += eoff;
  if (epi.tv) epi.tv += eoff;
  RowsParams p;
  std::memset(&p, 0, sizeof(p));
  p.ax = ax2.view;
  p.twr = twr.get();
  p.d2 = L.d2;
  p.h = L.h;
  p.C = L.C;
  p.RP = L.RP;
  p.rows = R;
  p.in_cplx = data;
  p.in_nyq = nyq;
  p.out_cplx = data;
  p.out_nyq = nyq;
  p.nyq_packed = nyq ? 0 : 1;
  if (lines) lines_args(*this, p, row0, nyq, nullptr, nullptr);
  p.epi = epi;
  if (!p.epi.poison) {
    p.epi.poison = no_poison.get();
    p.epi.poison_epoch = 0xffffffffu;
  }
  if (st) {
    p.st = *st;
    p.st.row0 = row0;
  }
  ProfScope ps(prof, mvn_epi_reads_psi(epi.mode) ? KK_ROWS_FUSED_UPD : KK_ROWS_FUSED, s);
  if (fx_rows) {
    p.fixed = 1;
    p.T = gx_rows.T;
    be::launch_rows_c2r_r2c(p, R / p.T, gx_rows.threads, gx_rows.lds_bytes, s);
    return;
  }
  p.T = g_rows.T;
  p.TP = g_rows.TP;
  p.lds_alt = g_rows.lds_alt;
  p.lds_tw = g_rows.lds_tw;
  p.hmul = mvn_fastdiv_mul((unsigned)L.h);
  p.Cmul = mvn_fastdiv_mul((unsigned)L.C);
  const long ntiles = (R + p.T - 1) / p.T;
  be::launch_rows_c2r_r2c(p, ntiles, g_rows.threads, g_rows.lds_bytes, s);
}

void Plan3D::mid_fused(const cfloat* in, cfloat* out, const cfloat* taps, int k, int kd, unsigned* poison,
                       unsigned poison_epoch, be::stream_t s, Profiler* prof, int zbeg, int zcount, int n_peers,
                       unsigned* const* peers) const {
  if (!lines_capable()) throw std::logic_error("mvn: this shape has no fused middle pass");
  MidFusedParams p;
  std::memset(&p, 0, sizeof(p));
  p.in = in;
  p.out = out;
  p.taps = taps;
  p.kd = kd;
  p.tw = ax1.view.tw;
  p.d0 = L.d0;
  p.H = L.C;
  p.k = k;
  p.h = k / 2;
  p.seg = 0;  // whole columns: C = 256 workgroups, one per CU of an MI355X
  p.mode = MF_CONV;
  p.packed = 1;
  p.poison = poison;
  p.poison_epoch = poison_epoch;
  p.zbeg = zbeg;
  p.zcount = zcount;
  p.n_peers = n_peers;
  p.poison_peers = peers;
  ProfScope ps(prof, KK_MID_FUSED, s);
  be::launch_mid_fused(p, s);
}

void Plan3D::taps_to_lines(cfloat* taps, be::stream_t s) const {
  if (!lines_capable()) throw std::logic_error("mvn: this shape has no fused middle pass");
  MidFusedParams p;
  std::memset(&p, 0, sizeof(p));
  p.in = taps;
  p.out = taps;
  p.tw = ax1.view.tw;
  p.d0 = L.d0;
  p.H = L.C;
  p.mode = MF_TAPS;
  be::launch_mid_fused(p, s);
}

static StridedParams make_strided(const DevAxis& ax, const PassGeom& g, cfloat* data,
                                  const cfloat* spec, long ostride, long estride, long cstride,
                                  int ncols) {
  StridedParams p;
  std::memset(&p, 0, sizeof(p));
  p.ax = ax.view;
  p.data = data;
  p.spec = spec;
  p.ostride = ostride;
  p.estride = estride;
  p.cstride = cstride;
  p.ncols = ncols;
  p.T = g.T;
  p.TP = g.TP;
  p.lds_alt = g.lds_alt;
  p.lds_tw = g.lds_tw;
  p.tiles_per_outer = (ncols + g.T - 1) / g.T;
  return p;
}

void SideStream::create() {
  s = be::Stream::create();
  fork = be::Event::sync_only();
  join = be::Event::sync_only();
}

void SideStream::fork_from(be::stream_t main) {
  be::event_record(fork.get(), main);
  be::stream_wait_event(s.get(), fork.get());
}

void SideStream::join_into(be::stream_t main) {
  be::event_record(join.get(), s.get());
  be::stream_wait_event(main, join.get());
}

void Plan3D::axis1(int mode, cfloat* data, cfloat* nyq, be::stream_t s, Profiler* prof,
                   be::stream_t s_nyq, int z0, int nz) const {
  if (!s_nyq) s_nyq = s;
  if (nz < 0) nz = L.d0 - z0;
  if (z0 < 0 || nz < 1 || z0 + nz > L.d0) throw std::out_of_range("mvn: plane range of a dim1 pass");
  data += (size_t)z0 * L.d1 * L.C;
  if (nyq) nyq += (size_t)z0 * L.d1;
  const bool ride = nyq_rides() && L.even && nyq;
  {
    // main array [d0][d1][C]: lines along d1, tiles of neighbouring bins
    const PassGeom& g = fx_ax1 ? gx_ax1 : g_ax1;
    StridedParams p = make_strided(ax1, g, data, nullptr, (long)L.d1 * L.C, L.C, 1, L.C);
    p.fixed = fx_ax1 ? 1 : 0;
    ProfScope ps(prof, mode == MVN_ST_FWD ? KK_AXIS1_FWD : KK_AXIS1_INV, s);
    if (ride) {
      // the Nyquist plane [d0][d1] rides in the same launch: its nz lines (contiguous along d1), one per workgroup
      StridedParams r = make_strided(ax1, g_nyq1_line, nyq, nullptr, 0, 1, L.d1, nz);
      r.is_nyq = 1;
      be::launch_strided(mode, p, (long)nz * p.tiles_per_outer, g.threads, g.lds_bytes, s, &r, g_nyq1_line.lds_bytes);
    } else {
      be::launch_strided(mode, p, (long)nz * p.tiles_per_outer, g.threads, g.lds_bytes, s);
    }
  }
  if (L.even && nyq && !ride) {  // (no plane: the Nyquist bins are packed into column 0 of the main array)
    // Nyquist plane [d0][d1]: lines along d1 are contiguous, neighbouring lines d1 apart
    StridedParams p = make_strided(ax1, g_nyq1, nyq, nullptr, 0, 1, L.d1, nz);
    p.is_nyq = 1;
    ProfScope ps(s_nyq == s ? prof : nullptr, KK_NYQ, s_nyq);
    be::launch_strided(mode, p, p.tiles_per_outer, g_nyq1.threads, g_nyq1.lds_bytes, s_nyq);
  }
}

void Plan3D::retile_spectrum(const cfloat* natural, cfloat* tiled, be::stream_t s) const {
  const long cols = (long)L.d1 * L.C;
  const int T = gx_ax0.T;
  // tiled[(tile * d0 + row) * T + c] = natural[row * cols + tile * T + c], in floats for copy3d
  be::launch_copy3d((float*)tiled, 2L * T, 2L * T * L.d0, (const float*)natural, 2L * cols, 2L * T, 2 * T,
                    L.d0, (int)(cols / T), s);
}

void Plan3D::axis0(int mode, cfloat* data, cfloat* nyq, const cfloat* spec,
                   const cfloat* spec_nyq, be::stream_t s, Profiler* prof, be::stream_t s_nyq,
                   const cfloat* src, const cfloat* src_nyq, bool spec_tiled) const {
  if (!s_nyq) s_nyq = s;
  const int kind = mode == MVN_ST_FWD ? KK_AXIS0_FWD
                                      : (mode == MVN_ST_INV ? KK_AXIS0_INV : KK_AXIS0_FUSED);
  {
    // main array viewed as [d0][d1*C]: lines along d0, all (d1, bin) columns are contiguous
    const long cols = (long)L.d1 * L.C;
    if (cols > 0x7fffffffL) throw std::invalid_argument("mvn: d1*d2 too large");
    const PassGeom& g = fx_ax0 ? gx_ax0 : g_ax0;
    StridedParams p = make_strided(ax0, g, data, spec, 0, cols, 1, (int)cols);
    p.fixed = fx_ax0 ? 1 : 0;
    p.src = src;
    if (spec_tiled && !fx_ax0) throw std::logic_error("mvn: tile-contiguous spectra need the fixed dim0 kernels");
    p.spec_tiled = spec_tiled ? 1 : 0;
    ProfScope ps(prof, kind, s);
    be::launch_strided(mode, p, p.tiles_per_outer, g.threads, g.lds_bytes, s);
  }
  if (L.even) {
    StridedParams p = make_strided(ax0, g_nyq0, nyq, spec_nyq, 0, L.d1, 1, L.d1);
    p.is_nyq = 1;
    p.src = src_nyq;
    ProfScope ps(s_nyq == s ? prof : nullptr, KK_NYQ, s_nyq);
    be::launch_strided(mode, p, p.tiles_per_outer, g_nyq0.threads, g_nyq0.lds_bytes, s_nyq);
  }
}

void Plan3D::forward(float* vol, cfloat* nyq, be::stream_t s, Profiler* prof) const {
  rows_r2c(vol, (cfloat*)vol, nyq, s, prof);
  axis1(MVN_ST_FWD, (cfloat*)vol, nyq, s, prof);
  axis0(MVN_ST_FWD, (cfloat*)vol, nyq, nullptr, nullptr, s, prof);
}

void Plan3D::backward(float* vol, cfloat* nyq, float scale, be::stream_t s,
                      Profiler* prof) const {
  axis0(MVN_ST_INV, (cfloat*)vol, nyq, nullptr, nullptr, s, prof);
  axis1(MVN_ST_INV, (cfloat*)vol, nyq, s, prof);
  EpilogueParams e;
  std::memset(&e, 0, sizeof(e));
  e.mode = MVN_EPI_STORE;
  e.scale = scale;
  rows_c2r((const cfloat*)vol, nyq, vol, e, s, prof);
}

void Plan3D::middle_passes(cfloat* work, cfloat* work_nyq, const cfloat* spec,
                           const cfloat* spec_nyq, be::stream_t s, Profiler* prof,
                           SideStream* side, bool spec_tiled) const {
  be::stream_t sn = s;
  // (where the plane's dim1 transforms ride in the main launches, its dim0 launch runs in line between them)
  if (side && side->s.get() && L.even && !nyq_rides()) {
    side->fork_from(s);  // the plane was written by the last-axis pass just enqueued on s
    sn = side->s.get();
  }
  axis1(MVN_ST_FWD, work, work_nyq, s, prof, sn);
  axis0(MVN_ST_FWD_MUL_INV, work, work_nyq, spec, spec_nyq, s, prof, sn, nullptr, nullptr, spec_tiled);
  axis1(MVN_ST_INV, work, work_nyq, s, prof, sn);
  if (sn != s) side->join_into(s);  // the next last-axis pass on s reads the plane
}

void Plan3D::convolve(const float* in_real, cfloat* work, cfloat* work_nyq, const cfloat* spec,
                      const cfloat* spec_nyq, float* out_real, const EpilogueParams& epi,
                      be::stream_t s, Profiler* prof) const {
  rows_r2c(in_real, work, work_nyq, s, prof);
  axis1(MVN_ST_FWD, work, work_nyq, s, prof);
  axis0(MVN_ST_FWD_MUL_INV, work, work_nyq, spec, spec_nyq, s, prof);
  axis1(MVN_ST_INV, work, work_nyq, s, prof);
  rows_c2r(work, work_nyq, out_real, epi, s, prof);
}

void Plan3D::psf_spectrum(const float* d_kernel, const int* kdims, float scale, float* spec_vol,
                          cfloat* spec_nyq, be::stream_t s) const {
  for (int i = 0; i < 3; ++i) {
    const int D = i == 0 ? L.d0 : (i == 1 ? L.d1 : L.d2);
    if (kdims[i] < 1 || kdims[i] > D)
      throw std::invalid_argument("mvn: kernel extent must be in [1, image extent]");
  }
  be::dzero(spec_vol, main_bytes(), s);
  be::launch_scatter_psf(d_kernel, kdims[0], kdims[1], kdims[2], spec_vol, L.d0, L.d1, L.d2, L.RP,
                         scale, s);
  forward(spec_vol, spec_nyq, s, nullptr);
}

// ---------------------------------------------------------------------------------------------
// PlanStore
// ---------------------------------------------------------------------------------------------
PlanStore& PlanStore::get() {
  static PlanStore* inst = new PlanStore();  // leaked on purpose: outlives static destructors
  return *inst;
}

static std::array<int, 4> plan_key(int device, const shape_t& s) {
  std::array<int, 4> k = {{device, s[0], s[1], s[2]}};
  return k;
}

std::shared_ptr<Plan3D> PlanStore::add(int device, const shape_t& shape) {
  std::lock_guard<std::mutex> lk(mu_);
  auto key = plan_key(device, shape);
  auto it = plans_.find(key);
  if (it != plans_.end()) return it->second;
  const int prev = be::get_device();
  be::set_device(device);
  std::shared_ptr<Plan3D> p(new Plan3D(device, shape[0], shape[1], shape[2], FormSwitches::from_env().fixed));
  be::set_device(prev);
  plans_[key] = p;
  return p;
}

bool PlanStore::has_key(int device, const shape_t& shape) {
  std::lock_guard<std::mutex> lk(mu_);
  return plans_.count(plan_key(device, shape)) != 0;
}

std::shared_ptr<Plan3D> PlanStore::lookup(int device, const shape_t& shape) {
  std::lock_guard<std::mutex> lk(mu_);
  auto it = plans_.find(plan_key(device, shape));
  if (it == plans_.end())
    throw std::runtime_error("mvn::PlanStore: no plan for " + std::to_string(shape[0]) + "x" +
                             std::to_string(shape[1]) + "x" + std::to_string(shape[2]));
  return it->second;
}

std::shared_ptr<Plan3D> PlanStore::find(int device, const shape_t& shape) {
  std::lock_guard<std::mutex> lk(mu_);
  auto it = plans_.find(plan_key(device, shape));
  return it == plans_.end() ? nullptr : it->second;
}

bool PlanStore::empty() {
  std::lock_guard<std::mutex> lk(mu_);
  return plans_.empty();
}

size_t PlanStore::size() {
  std::lock_guard<std::mutex> lk(mu_);
  return plans_.size();
}

void PlanStore::clear() {
  std::lock_guard<std::mutex> lk(mu_);
  plans_.clear();
}

// ---------------------------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------------------------
Engine::Engine(int device, const shape_t& dims, int num_views) : Engine(device) {
  // zero views: a rank of a view-sharded run that got none (6 views on 8 GPUs) still keeps a
  // replica of psi and takes part in the all-reduce with a zero correction
  if (num_views < 0) throw std::invalid_argument("mvn: num_views must be >= 0");
  be::set_device(device_);
  plan_ = PlanStore::get().add(device_, dims);
  stream_ = be::Stream::create();
  side_.create();
  const size_t mb = plan_->main_bytes();
  psi_ = be::DeviceBuffer<float>(mb);
  work_own_[0] = be::DeviceBuffer<float>(mb);
  work_ = work_own_[0].get();
  be::dzero(psi_.get(), mb, stream_.get());
  be::dzero(work_, mb, stream_.get());
  if (plan_->nyq_bytes()) work_nyq_own_[0] = be::DeviceBuffer<cfloat>(plan_->nyq_bytes());
  work_nyq_ = work_nyq_own_[0].get();
  poison_own_ = be::DeviceBuffer<unsigned>(256);  // the words, and at bytes 64 / 128 the tables of the peers' words
  be::dzero(poison_own_.get(), 256, stream_.get());
  poison_ = poison_own_.get();
  views_.resize((size_t)num_views);
  stream_pos_.assign((size_t)num_views, -1);
  want_u16_.assign((size_t)num_views, 0);
  spec_tiled_ = plan_->tiles_spectra();
  sw_ = FormSwitches::from_env();  // read per engine (tests)
  d0_stagger_ = env_int("MVN_D0_STAGGER", 64);
  packed_allowed_ = packed_default_ = packed_layout_for(plan_->main_bytes()) && mvn_dim0_packed_possible(dims[0]);
  for (int d = 0; d < 3; ++d) host_dims_[d] = dims[d];
  be::stream_sync(stream_.get());
}

// Packed Nyquist layout (mvn_dim0_direct.hpp): MVN_NYQ_PACKED = 1 always / 0 never / unset: for volumes up to
// 256 MB.  Small volumes are bound by launches and latency and the layout's single
// launch chain wins (one view update, round 4, against the split layout with its Nyquist lines riding in the dim1
// launches: 64^3 0.055 / 0.062 ms, 128^3 0.082 / 0.089, 256^3 0.246 / 0.262; 320^3 and 384^3 even).  At 512^3 it
// is 6 % SLOWER (2.24 / 2.11 ms): the DC column's 2 x 257 dim0 columns are 8-byte accesses one row apart in every
// plane, and the leg takes 0.27 instead of 0.23 ms (profiles/r04_layouts.md).
bool Engine::packed_layout_for(size_t volume_bytes) {
  const int sw = env_int("MVN_NYQ_PACKED", -1);
  return sw > 0 || (sw < 0 && volume_bytes <= ((size_t)256 << 20));
}

Engine::~Engine() {
  try {
    be::set_device(device_);
    if (stream_.get()) be::stream_sync(stream_.get());
  } catch (...) {
  }
}

void Engine::set_embedding(const int dims[3], const int off[3], bool scratch) {
  be::set_device(device_);
  const Layout& L = plan_->L;
  const int ext[3] = {L.d0, L.d1, L.d2};
  bool dense = true, same = true;
  for (int d = 0; d < 3; ++d) {
    if (dims[d] < 1 || off[d] < 0 || off[d] + dims[d] > ext[d])
      throw std::invalid_argument("mvn: embedded stack does not fit the engine volume");
    dense = dense && dims[d] == ext[d];
    same = same && host_dims_[d] == dims[d] && host_off_[d] == off[d];
  }
  if (same && embedded_ == !dense) {
    if (embedded_ && scratch && !embed_scratch_.get()) embed_scratch_ = be::DeviceBuffer<float>(host_floats() * sizeof(float));
    if (!scratch && embed_scratch_.get()) {
      be::stream_sync(stream_.get());
      embed_scratch_.reset();
    }
    return;
  }
  be::stream_sync(stream_.get());
  // the interior moves: what used to be interior may now be padding and must read zero
  for (size_t v = 0; v < views_.size(); ++v) {
    if (views_[v].image.get()) be::dzero(views_[v].image.get(), image_bytes(views_[v].image_u16), stream_.get());
    if (views_[v].weights.get()) be::dzero(views_[v].weights.get(), plan_->main_bytes(), stream_.get());
  }
  for (size_t r = 0; r < ring_.size(); ++r) {
    if (ring_[r].image.get()) be::dzero(ring_[r].image.get(), image_bytes(ring_[r].image_u16), stream_.get());
    be::dzero(ring_[r].weights.get(), plan_->main_bytes(), stream_.get());
  }
  be::stream_sync(stream_.get());
  margins_mirrored_ = false;
  embed_scratch_.reset();
  for (int d = 0; d < 3; ++d) {
    host_dims_[d] = dims[d];
    host_off_[d] = off[d];
  }
  embedded_ = !dense;
  if (embedded_ && scratch) embed_scratch_ = be::DeviceBuffer<float>(host_floats() * sizeof(float));
}

// ---- stacks in and out (mvn_ingest.hpp) -------------------------------------------------------------
// rows of a host stack as 2-D copies: [n0][n1] rows of `width` bytes, source pitches in bytes, destination pitches
// drow / dplane bytes; one copy where the source's planes continue its row pitch, else one per plane
static void host_rows_to_device(char* dst, size_t drow, size_t dplane, const char* src, long long s0b, long long s1b,
                                size_t width, const int* n, be::stream_t s) {
  if (n[1] == 1) {  // (one row per plane: its row stride means nothing)
    for (int z = 0; z < n[0]; ++z) be::h2d(dst + z * dplane, src + z * s0b, width, s);
    return;
  }
  if (n[0] == 1 || (s0b == (long long)n[1] * s1b && dplane == (size_t)n[1] * drow)) {
    be::h2d_2d(dst, drow, src, (size_t)s1b, width, (size_t)n[0] * n[1], s);
    return;
  }
  for (int z = 0; z < n[0]; ++z) be::h2d_2d(dst + z * dplane, drow, src + z * s0b, (size_t)s1b, width, (size_t)n[1], s);
}

static void check_host_rows(const StackRef& st, const int* n) {
  if (n[2] > 1 && st.stride[2] != 1)
    throw std::invalid_argument("mvn: a stack in host memory needs contiguous rows (stride[2] == 1); gather it or hand it over in device memory");
  if ((n[1] > 1 && st.stride[1] < n[2]) || (n[0] > 1 && st.stride[0] < 0))
    throw std::invalid_argument("mvn: rows of a stack in host memory must not overlap (stride[1] >= extent[2])");
}

static std::atomic<long long> g_u16_divides{0}, g_u16_ingests{0};
void Engine::image_storage_counters(long long out[2]) {
  out[0] = g_u16_divides.load();
  out[1] = g_u16_ingests.load();
}

void Engine::set_reflect(bool on) {
  be::set_device(device_);
  if (!on && margins_mirrored_) {  // back to margins of zeros, as set_embedding leaves them
    be::stream_sync(stream_.get());
    for (size_t v = 0; v < views_.size(); ++v) {
      if (views_[v].image.get()) be::dzero(views_[v].image.get(), image_bytes(views_[v].image_u16), stream_.get());
      if (views_[v].weights.get()) be::dzero(views_[v].weights.get(), plan_->main_bytes(), stream_.get());
    }
    for (size_t r = 0; r < ring_.size(); ++r) {
      if (ring_[r].image.get()) be::dzero(ring_[r].image.get(), image_bytes(ring_[r].image_u16), stream_.get());
      be::dzero(ring_[r].weights.get(), plan_->main_bytes(), stream_.get());
    }
    be::stream_sync(stream_.get());
    margins_mirrored_ = false;
  }
  reflect_ = on;
  if (on && embedded_) margins_mirrored_ = true;
}

long long Engine::ingest_stack(float* dst, const StackRef& st, float* scratch, bool dst_dirty, be::stream_t s,
                               bool dst_u16) {
  const long long bytes = place_stack(dst, st, scratch, dst_dirty, s, dst_u16);
  mirror_margins(dst, dst_u16, s);
  return bytes;
}

void Engine::mirror_margins(float* dst, bool dst_u16, be::stream_t s) {
  if (!reflect_ || !embedded_) return;
  const Layout& L = plan_->L;
  ReflectParams p;
  p.vol = dst, p.RP = L.RP, p.D0 = L.d0, p.D1 = L.d1, p.D2 = L.d2;
  p.n0 = host_dims_[0], p.n1 = host_dims_[1], p.n2 = host_dims_[2];
  p.o0 = host_off_[0], p.o1 = host_off_[1], p.o2 = host_off_[2];
  p.axis = 2;
  be::launch_reflect_fill(p, dst_u16, s);
}

long long Engine::place_stack(float* dst, const StackRef& st, float* scratch, bool dst_dirty, be::stream_t s,
                              bool dst_u16) {
  const Layout& L = plan_->L;
  const int* n = host_dims_;
  if (!st.ptr) throw std::invalid_argument("mvn: null stack");
  if (st.geom) throw std::invalid_argument("mvn: only the image of a view can be a raw stack with a geometry");
  if (dst_u16 && (!st.u16 || st.broadcast())) throw std::logic_error("mvn: a uint16 volume takes a uint16 stack");
  for (int d = 0; d < 3; ++d)
    if (st.stride[d] < 0) throw std::invalid_argument("mvn: negative stride");
  IngestParams p;
  p.dst = dst, p.RP = L.RP, p.D1 = L.d1, p.rows = (long)L.rows;
  p.n0 = n[0], p.n1 = n[1], p.n2 = n[2];
  p.o0 = host_off_[0], p.o1 = host_off_[1], p.o2 = host_off_[2];
  p.src = st.ptr, p.s0 = st.stride[0], p.s1 = st.stride[1], p.s2 = st.stride[2];
  p.use_value = 0, p.value = 0.f;
  if (st.device) {  // read where it lies
    be::launch_ingest3d(p, st.u16, s, dst_u16);
    if (dst_u16) ++g_u16_ingests;
    return 0;
  }
  if (st.broadcast()) {  // one value in host memory: it travels as a kernel argument
    p.use_value = 1;
    p.value = st.u16 ? (float)*(const uint16_t*)st.ptr : *(const float*)st.ptr;
    p.src = nullptr;
    be::launch_ingest3d(p, false, s);
    return 0;
  }
  check_host_rows(st, n);
  const size_t esz = st.u16 ? sizeof(uint16_t) : sizeof(float);
  const long long bytes = (long long)(host_floats() * esz);
  const bool dense = (n[1] == 1 || st.stride[1] == n[2]) && (n[0] == 1 || st.stride[0] == (long long)n[1] * n[2]);
  if (!embedded_ && (!st.u16 || dst_u16)) {  // into a volume of its own extents and element type: the copy itself places it
    if (dst_dirty && L.RP != L.d2) be::dzero(dst, image_bytes(dst_u16), s);
    if (!dense)
      host_rows_to_device((char*)dst, (size_t)L.RP * esz, (size_t)L.d1 * L.RP * esz, (const char*)st.ptr,
                          st.stride[0] * (long long)esz, st.stride[1] * (long long)esz, (size_t)n[2] * esz, n, s);
    else if (L.RP == L.d2)
      be::h2d(dst, st.ptr, (size_t)bytes, s);
    else
      be::h2d_2d(dst, (size_t)L.RP * esz, st.ptr, (size_t)L.d2 * esz, (size_t)L.d2 * esz, L.rows, s);
    return bytes;
  }
  if (!scratch) throw std::logic_error("mvn: no scratch for a host stack");
  // (a float32 stack is copied into its window only: margins that are no longer the zeros of their allocation go first)
  if (!st.u16 && dst_dirty) be::dzero(dst, plan_->main_bytes(), s);
  if (dense)
    be::h2d(scratch, st.ptr, (size_t)bytes, s);
  else
    host_rows_to_device((char*)scratch, (size_t)n[2] * esz, (size_t)n[1] * n[2] * esz, (const char*)st.ptr,
                        st.stride[0] * (long long)esz, st.stride[1] * (long long)esz, (size_t)n[2] * esz, n, s);
  if (!st.u16) {  // float32 into its window: a strided device copy
    be::launch_copy3d(dst + ((size_t)host_off_[0] * L.d1 + host_off_[1]) * L.RP + host_off_[2], L.RP, (long)L.d1 * L.RP,
                      scratch, n[2], (long)n[1] * n[2], n[2], n[1], n[0], s);
    return bytes;
  }
  p.src = scratch, p.s0 = (long long)n[1] * n[2], p.s1 = n[2], p.s2 = 1;
  be::launch_ingest3d(p, true, s, dst_u16);
  if (dst_u16) ++g_u16_ingests;
  return bytes;
}

long long Engine::ingest_pair(float* image_dst, float* weights_dst, const StackRef& image, const StackRef& weights,
                              be::stream_t s, bool image_u16) {
  if (weights.u16) throw std::invalid_argument("mvn: weights are float32");
  if (image.geom) {
    if (image_u16) throw std::logic_error("mvn: a resampled image is a float32 volume");
    return resample_pair(image_dst, weights_dst, image, weights, s);
  }
  float* scr = embed_scratch_.get();
  bool dirty = false;
  if (!image_u16 && !scr && !image.device && !image.broadcast() && image.u16) {
    // (no embedding, so no scratch: the raw uint16 stack lands in the view's weights volume, which is filled next,
    //  on the same stream)
    scr = weights_dst;
    dirty = true;
  }
  long long bytes = ingest_stack(image_dst, image, scr, false, s, image_u16);
  bytes += ingest_stack(weights_dst, weights, embed_scratch_.get(), dirty, s);
  return bytes;
}

long long Engine::resample_pair(float* image_dst, float* weights_dst, const StackRef& image, const StackRef& weights,
                                be::stream_t s) {
  const Layout& L = plan_->L;
  if (halo_fn_) throw std::invalid_argument("mvn: resampled views are not for an engine with a halo hook");
  ResampleParams p;
  p.image = image_dst, p.weights = weights.ptr ? nullptr : weights_dst;
  p.RP = L.RP, p.D0 = L.d0, p.D1 = L.d1;
  p.n0 = host_dims_[0], p.n1 = host_dims_[1], p.n2 = host_dims_[2];
  p.o0 = host_off_[0], p.o1 = host_off_[1], p.o2 = host_off_[2];
  long long bytes = resample_raw(p, image, s);
  mirror_margins(image_dst, false, s);
  // (computed weights are mirrored behind their normalisation: normalize_weights)
  if (weights.ptr) bytes += ingest_stack(weights_dst, weights, embed_scratch_.get(), false, s);
  return bytes;
}

void Engine::check_raw_host(const StackRef& image, const int* m) {
  if (!image.device && !image.broadcast()) check_host_rows(image, m);
}

long long Engine::upload_raw(const StackRef& image, const int* m, be::DeviceBuffer<char>& tmp, StackRef* there,
                             be::stream_t s) {
  const size_t esz = image.u16 ? sizeof(uint16_t) : sizeof(float);
  *there = image;
  there->device = true;
  long long bytes;
  if (image.broadcast()) {
    bytes = (long long)esz;
    tmp = be::DeviceBuffer<char>(esz);
    be::h2d(tmp.get(), image.ptr, esz, s);
  } else {
    check_host_rows(image, m);
    bytes = (long long)m[0] * m[1] * m[2] * (long long)esz;
    tmp = be::DeviceBuffer<char>((size_t)bytes);
    const bool dense = (m[1] == 1 || image.stride[1] == m[2]) && (m[0] == 1 || image.stride[0] == (long long)m[1] * m[2]);
    if (dense)
      be::h2d(tmp.get(), image.ptr, (size_t)bytes, s);
    else
      host_rows_to_device(tmp.get(), (size_t)m[2] * esz, (size_t)m[1] * m[2] * esz, (const char*)image.ptr,
                          image.stride[0] * (long long)esz, image.stride[1] * (long long)esz, (size_t)m[2] * esz, m, s);
    there->stride[0] = (long long)m[1] * m[2], there->stride[1] = m[2], there->stride[2] = 1;
  }
  there->ptr = tmp.get();
  return bytes;
}

long long Engine::resample_raw(ResampleParams p, const StackRef& image, be::stream_t s) {
  if (!image.ptr || !image.geom) throw std::invalid_argument("mvn: null stack");
  const ResampleGeom& g = *image.geom;
  for (int d = 0; d < 3; ++d) {
    if (image.stride[d] < 0) throw std::invalid_argument("mvn: negative stride");
    if (g.m[d] < 1) throw std::invalid_argument("mvn: extents of a raw stack must be >= 1");
  }
  p.src = image.ptr, p.s0 = image.stride[0], p.s1 = image.stride[1], p.s2 = image.stride[2];
  p.g = g;
  be::DeviceBuffer<char> tmp;
  long long bytes = 0;
  try {
    if (!image.device) {  // the raw stack crosses PCIe as it is, into a dense temporary
      StackRef there;
      bytes = upload_raw(image, g.m, tmp, &there, s);
      p.src = there.ptr, p.s0 = there.stride[0], p.s1 = there.stride[1], p.s2 = there.stride[2];
    }
    be::launch_resample(p, image.u16, s);
    if (tmp.get()) be::stream_sync(s);
  } catch (...) {
    if (tmp.get()) be::drain_quietly(s);  // the caller's stream: what it holds of tmp's is over before tmp goes
    throw;
  }
  return bytes;
}

void Engine::normalize_weights() {
  be::set_device(device_);
  if (halo_fn_) throw std::invalid_argument("mvn: resampled views are not for an engine with a halo hook");
  const Layout& L = plan_->L;
  const size_t V = views_.size();
  weights_tab_host_.assign(V, nullptr);
  for (size_t v = 0; v < V; ++v) {
    if (stream_pos_[v] >= 0 || !views_[v].weights.get()) throw std::logic_error("mvn: normalize_weights needs every view resident and placed");
    weights_tab_host_[v] = views_[v].weights.get();
  }
  if (!weights_tab_.get()) weights_tab_ = be::DeviceBuffer<float*>(V * sizeof(float*));
  be::h2d(weights_tab_.get(), weights_tab_host_.data(), V * sizeof(float*), stream_.get());
  NormalizeParams p;
  p.vols = weights_tab_.get(), p.V = (int)V, p.RP = L.RP, p.D1 = L.d1;
  p.n0 = host_dims_[0], p.n1 = host_dims_[1], p.n2 = host_dims_[2];
  p.o0 = host_off_[0], p.o1 = host_off_[1], p.o2 = host_off_[2];
  be::launch_weights_normalize(p, stream_.get());
  for (size_t v = 0; v < V; ++v) mirror_margins(views_[v].weights.get(), false, stream_.get());
  be::stream_sync(stream_.get());
}

void Engine::fuse_psi(float fill) {
  be::set_device(device_);
  if (halo_fn_) throw std::invalid_argument("mvn: fusion into psi is not for an engine with a halo hook");
  if (!streamed_order_.empty()) throw std::invalid_argument("mvn: fusion into psi needs every view resident");
  if (!std::isfinite(fill)) throw std::invalid_argument("mvn: fill must be finite");
  const Layout& L = plan_->L;
  const size_t V = views_.size();
  if (V < 1) throw std::invalid_argument("mvn: fusion into psi needs a view");
  fuse_tab_host_.assign(2 * V, nullptr);
  for (size_t v = 0; v < V; ++v) {
    if (!views_[v].image.get() || !views_[v].weights.get()) throw std::invalid_argument("mvn: fusion into psi needs every view placed");
    if (views_[v].image_u16) throw std::invalid_argument("mvn: fusion into psi is not for an engine that holds a uint16 image volume");
    fuse_tab_host_[v] = views_[v].image.get();
    fuse_tab_host_[V + v] = views_[v].weights.get();
  }
  if (!fuse_tab_.get()) fuse_tab_ = be::DeviceBuffer<const float*>(2 * V * sizeof(float*));
  be::h2d(fuse_tab_.get(), fuse_tab_host_.data(), 2 * V * sizeof(float*), stream_.get());
  psi_spec_valid_ = false;
  // (the loop has written the margins of an embedded psi; the row padding of an odd last extent reads zero)
  if (embedded_ || L.RP != L.d2) be::dzero(psi_.get(), plan_->main_bytes(), stream_.get());
  FuseVolumesParams p;
  p.psi = psi_.get(), p.vols = fuse_tab_.get(), p.V = (int)V, p.RP = L.RP, p.D1 = L.d1;
  p.n0 = host_dims_[0], p.n1 = host_dims_[1], p.n2 = host_dims_[2];
  p.o0 = host_off_[0], p.o1 = host_off_[1], p.o2 = host_off_[2];
  p.fill = fill;
  be::launch_fuse_volumes(p, stream_.get());
  mirror_margins(psi_.get(), false, stream_.get());
  be::stream_sync(stream_.get());
}

void Engine::wait_for_caller(void* caller_stream) {
  if (!caller_stream) return;
  be::set_device(device_);
  if (!caller_ev_.get()) caller_ev_ = be::Event::sync_only();
  be::event_record(caller_ev_.get(), (be::stream_t)caller_stream);
  be::stream_wait_event(stream_.get(), caller_ev_.get());
  if (upload_stream_.get()) be::stream_wait_event(upload_stream_.get(), caller_ev_.get());
}

void Engine::alloc_view(ViewSlot& s) {
  const size_t mb = plan_->main_bytes();
  const size_t v = (size_t)(&s - views_.data());
  if (stream_pos_[v] >= 0) return;  // (streamed views: the ring's slots)
  const bool u16 = want_u16_[v] != 0;
  if (s.image.get() && s.image_u16 != u16) {  // the slot held the other element type: its image alone is re-allocated
    be::stream_sync(stream_.get());
    s.image.reset();
    ++graph_gen_;
  }
  const bool new_image = !s.image.get(), new_weights = !s.weights.get();
  if (new_image) {
    s.image = be::DeviceBuffer<float>(image_bytes(u16));
    s.image_u16 = u16;
  }
  if (new_weights) s.weights = be::DeviceBuffer<float>(mb);
  // the PSF buffers (3-D spectra or direct-form taps) are allocated by prepare_psf, which knows the form
  if ((new_image || new_weights) && (plan_->L.RP != plan_->L.d2 || embedded_)) {  // odd d2 / embedded stacks: the padding must hold zeros
    if (new_image) be::dzero(s.image.get(), image_bytes(u16), stream_.get());
    if (new_weights) be::dzero(s.weights.get(), mb, stream_.get());
    be::stream_sync(stream_.get());
  }
}

static std::atomic<long> g_psf_hits{0}, g_psf_misses{0};
long Engine::psf_cache_hits() { return g_psf_hits.load(); }
long Engine::psf_cache_misses() { return g_psf_misses.load(); }

// The spectra of a slot stay valid for as long as the engine (shape, scale and layout are fixed
// per engine): compare the incoming kernel with the host copy of the one they were made from.
// A bytewise comparison of ~100 kB, not a hash: a false match would silently change results.
// MVN_PSF_CACHE=0 always prepares.
bool Engine::psf_resident(ViewSlot& s, int i, const float* kernel, const int* kdims) {
  static const bool enabled = [] {
    const char* e = std::getenv("MVN_PSF_CACHE");
    return !(e && std::strcmp(e, "0") == 0);
  }();
  const size_t n = (size_t)kdims[0] * (size_t)kdims[1] * (size_t)kdims[2];
  const bool same = enabled && s.set && s.kcopy[i].size() == n && s.kdims[i][0] == kdims[0] &&
                    s.kdims[i][1] == kdims[1] && s.kdims[i][2] == kdims[2] &&
                    std::memcmp(s.kcopy[i].data(), kernel, n * sizeof(float)) == 0;
  if (same) {
    ++g_psf_hits;
    return true;
  }
  ++g_psf_misses;
  s.kcopy[i].assign(kernel, kernel + n);
  for (int d = 0; d < 3; ++d) s.kdims[i][d] = kdims[d];
  return false;
}

void Engine::make_spectrum(const float* d_kernel, const int* kdims, float scale, float* spec,
                           cfloat* nyq, float* scratch, be::stream_t s) {
  if (!spec_tiled_) {
    plan_->psf_spectrum(d_kernel, kdims, scale, spec, nyq, s);
    return;
  }
  plan_->psf_spectrum(d_kernel, kdims, scale, scratch, nyq, s);  // the Nyquist plane stays as it is
  plan_->retile_spectrum((const cfloat*)scratch, (cfloat*)spec, s);
}

// the (kd, d1, d2) plan of the tap arrays, built with the engine's switches (FormRule::direct)
Plan3D* Engine::taps_plan(int kd) {
  auto it = taps_plans_.find(kd);
  if (it != taps_plans_.end()) return it->second.get();
  std::unique_ptr<Plan3D> p(new Plan3D(device_, kd, plan_->L.d1, plan_->L.d2, sw_.fixed));
  Plan3D* raw = p.get();
  taps_plans_[kd] = std::move(p);
  return raw;
}

void Engine::prepare_psf(ViewSlot& s, int i, const float* d_kernel, const int* kdims, float* scratch,
                         bool staging, be::stream_t st) {
  const Layout& L = plan_->L;
  for (int d = 0; d < 3; ++d) {
    const int D = d == 0 ? L.d0 : (d == 1 ? L.d1 : L.d2);
    if (kdims[d] < 1 || kdims[d] > D) throw std::invalid_argument("mvn: kernel extent must be in [1, image extent]");
  }
  ++graph_gen_;  // a captured sweep holds the PSF buffers, their form and depth
  const FormRule rule = form_rule();
  if (rule.direct(kdims)) {
    const int kd = taps_depth(kdims[0]);
    Plan3D* tp = taps_plan(kd);
    if (s.tap_kd[i] != kd) {  // (re)allocate for this depth; the previous arrays may still be read by the stream
      be::stream_sync(st);
      be::stream_sync(stream_.get());
      s.tap_kd[i] = 0;  // (none held, should an allocation below fail)
      s.taps[i].reset();
      s.taps_nyq[i].reset();
      s.taps[i] = be::DeviceBuffer<float>(tp->main_bytes());
      if (tp->nyq_bytes()) s.taps_nyq[i] = be::DeviceBuffer<cfloat>(tp->nyq_bytes());
      s.taps_l[i].reset();
      s.tap_kd[i] = kd;
    }
    s.taps_l_ok[i] = false;
    s.tap_k[i] = 0;  // not valid until the launches below are enqueued
    // dims 1 and 2 are transformed (un-normalised, both ways), dim0 is not: 1 / (d1 d2)
    const float scale = (float)(1.0 / ((double)L.d1 * (double)L.d2));
    be::dzero(s.taps[i].get(), tp->main_bytes(), st);
    be::launch_scatter_psf(d_kernel, kdims[0], kdims[1], kdims[2], s.taps[i].get(), kd, L.d1, L.d2, tp->L.RP, scale, st);
    tp->rows_r2c(s.taps[i].get(), (cfloat*)s.taps[i].get(), s.taps_nyq[i].get(), st, nullptr);
    tp->axis1(MVN_ST_FWD, (cfloat*)s.taps[i].get(), s.taps_nyq[i].get(), st, nullptr);
    if (rule.lines_taps(kdims)) {
      // the same planes for the fused middle pass: line layout, Nyquist bins packed, its own bin order along dim1
      // (wherever the kernel could take the pass: decide_lines() asks whether it is worth it)
      if (!s.taps_l[i].get()) s.taps_l[i] = be::DeviceBuffer<float>(tp->main_bytes());
      if (taps_scr_bytes_ < tp->main_bytes()) {  // one scratch per engine, as large as the deepest tap array
        be::stream_sync(st);
        be::stream_sync(stream_.get());
        taps_scr_bytes_ = 0;
        taps_scr_.reset();
        taps_scr_ = be::DeviceBuffer<float>(tp->main_bytes());
        taps_scr_bytes_ = tp->main_bytes();
      }
      be::dzero(taps_scr_.get(), tp->main_bytes(), st);
      be::launch_scatter_psf(d_kernel, kdims[0], kdims[1], kdims[2], taps_scr_.get(), kd, L.d1, L.d2, tp->L.RP, scale, st);
      tp->rows_r2c(taps_scr_.get(), (cfloat*)s.taps_l[i].get(), nullptr, st, nullptr, 0, -1, true);
      tp->taps_to_lines((cfloat*)s.taps_l[i].get(), st);
      s.taps_l_ok[i] = true;
    }
    s.tap_k[i] = kdims[0];
    return;
  }
  // 3-D spectrum for the fused FFT pass
  if (!s.spec[i].get()) {
    s.spec[i] = be::DeviceBuffer<float>(plan_->main_bytes());
    if (plan_->nyq_bytes()) s.nyq[i] = be::DeviceBuffer<cfloat>(plan_->nyq_bytes());
  }
  s.tap_k[i] = 0;
  s.taps_l_ok[i] = false;
  if (spec_tiled_ && !scratch) {
    if (!staging) throw std::logic_error("mvn: spectrum scratch missing");
    if (!stage_spec_scratch_) {  // the main thread iterates on the work volume meanwhile: own scratch, freed
                                 // with the other staging scratch once the upload stream has drained
      stage_scratch_.emplace_back(plan_->main_bytes());
      stage_spec_scratch_ = stage_scratch_.back().get();
    }
    scratch = stage_spec_scratch_;
  }
  const float scale = (float)(1.0 / (double)L.logical());  // inc/cpu_convolve.h:271-274
  make_spectrum(d_kernel, kdims, scale, s.spec[i].get(), s.nyq[i].get(), scratch, st);
}

void Engine::ensure_work2() {
  if (work2_) return;
  work_own_[1] = be::DeviceBuffer<float>(plan_->main_bytes());
  if (plan_->nyq_bytes()) work_nyq_own_[1] = be::DeviceBuffer<cfloat>(plan_->nyq_bytes());
  work2_ = work_own_[1].get();
  work2_nyq_ = work_nyq_own_[1].get();
}

// the dim0 leg with the direct form of kernel i: in -> out (never in place).  Packed layout: one launch, the
// DC + i Nyquist column separated inside it.  Split layout: main array and Nyquist plane in ONE launch on the
// engine's stream
void Engine::dim0_conv(const ViewSlot& s, int i, const cfloat* in, const cfloat* in_nyq, cfloat* out,
                       cfloat* out_nyq, Profiler* prof, int zbeg, int zcount, bool first) {
  const Layout& L = plan_->L;
  if (zcount < 0 || zbeg < 0 || zbeg + zcount > L.d0) throw std::out_of_range("mvn: plane range of a dim0 leg");
  Dim0DirectParams p;
  std::memset(&p, 0, sizeof(p));
  p.in = in;
  p.out = out;
  p.taps = (const cfloat*)s.taps[i].get();
  p.d0 = L.d0;
  p.k = s.tap_k[i];
  p.kd = s.tap_kd[i];
  p.h = s.tap_k[i] / 2;
  p.plane = (long)L.d1 * L.C;
  p.stagger = d0_stagger_;
  p.zbeg = zbeg;
  p.zcount = zcount;
  p.seg1 = mvn_dim0_piece_len(p.k, zcount > 0 ? zcount : L.d0, p.plane, sw_.min_plane);
  p.C = L.C;
  p.d1 = L.d1;
  // non-finite inputs are reported under this leg's epoch (never 0, never a value the word may still hold); the
  // launches of one leg (a slab's interior planes, then those next to its halos) share it
  if (first && ++epoch_ == 0x7fffffffu) {
    be::dzero(poison_, poison_bytes(), stream_.get());
    epoch_ = 1;
  }
  armed_epoch_ = epoch_;
  p.poison = poison_word(epoch_);
  p.poison_epoch = epoch_;
  p.n_peers = (int)poison_peers_.size();
  p.poison_peers = poison_table(epoch_);
  if (packed_) {
    p.packed = 1;
    p.taps2 = s.taps_nyq[i].get();
    p.inv1 = plan_->ax1.view.inv;
    ProfScope ps(prof, KK_AXIS0_DIRECT, stream_.get());
    be::launch_dim0_direct(p, stream_.get());
    return;
  }
  p.in2 = L.even ? in_nyq : nullptr;
  p.out2 = L.even ? out_nyq : nullptr;
  p.taps2 = L.even ? s.taps_nyq[i].get() : nullptr;
  p.plane2 = L.even ? L.d1 : 0;
  p.seg2 = 16;
  ProfScope ps(prof, KK_AXIS0_DIRECT, stream_.get());
  be::launch_dim0_direct(p, stream_.get());
}

void Engine::arm(EpilogueParams& e) {
  e.poison = armed_epoch_ ? poison_word(armed_epoch_) : nullptr;
  e.poison_epoch = armed_epoch_;
  armed_epoch_ = 0;
}

void Engine::bind_poison(unsigned* external) {
  // (an engine with peers keeps two words of its own, poison_word: a caller-bound word of 4 bytes cannot be one)
  if (external && !poison_peers_.empty()) throw std::logic_error("mvn: bind_poison on an engine with poison peers");
  be::set_device(device_);
  be::stream_sync(stream_.get());
  sweep_graph_.reset();  // a captured sweep holds the word's address
  poison_ = external ? external : poison_own_.get();
  be::dzero(poison_own_.get(), sizeof(unsigned), stream_.get());
  be::stream_sync(stream_.get());
}

unsigned Engine::poison_get() {
  be::set_device(device_);
  unsigned v[2] = {0, 0};
  be::d2h(v, poison_, poison_bytes(), stream_.get());
  be::stream_sync(stream_.get());
  return v[0] > v[1] ? v[0] : v[1];  // (with peers: the later report of the two words)
}

// word = max(word, value): epochs only grow, so the larger one is the later report
void Engine::poison_merge(unsigned value) {
  if (value > poison_get()) {
    be::h2d(poison_word(value), &value, sizeof(value), stream_.get());
    be::stream_sync(stream_.get());  // (`value` is a stack variable)
  }
}

void Engine::add_poison_peer(unsigned* word) {
  if (!word) throw std::invalid_argument("mvn: null poison word");
  if ((int)poison_peers_.size() >= MVN_D0_MAX_PEERS) throw std::invalid_argument("mvn: too many poison peers");
  if (poison_ != poison_own_.get()) throw std::logic_error("mvn: poison peers on an engine with a caller-bound word");
  be::set_device(device_);
  be::stream_sync(stream_.get());
  poison_peers_.push_back(word);
  std::vector<unsigned*> odd(poison_peers_);  // the peers' words of the odd epochs (poison_word)
  for (size_t i = 0; i < odd.size(); ++i) ++odd[i];
  be::h2d(poison_own_.get() + 16, poison_peers_.data(), poison_peers_.size() * sizeof(unsigned*), stream_.get());
  be::h2d(poison_own_.get() + 32, odd.data(), odd.size() * sizeof(unsigned*), stream_.get());
  be::stream_sync(stream_.get());
}

// every view's two kernels are held in the direct form: the Nyquist bins can ride in the DC column
bool Engine::all_direct() const {
  if (views_.empty()) return false;
  for (size_t v = 0; v < views_.size(); ++v)
    if (!views_[v].set || !views_[v].tap_k[0] || !views_[v].tap_k[1]) return false;
  return true;
}

void Engine::decide_layout() {
  const bool allowed = layout_override_ < 0 ? packed_allowed_ : (layout_override_ > 0 && mvn_dim0_packed_possible(plan_->L.d0));
  const bool want = allowed && plan_->L.even && plan_->nyq_bytes() > 0;
  const bool was = packed_;
  packed_ = want && (pipelined_ ? packed_hint_ : all_direct());
  if (was != packed_) ++graph_gen_;  // ... and the layout
  lines_ = false;  // (only the sequential sweep asks for the line layout: decide_lines())
}

// The sequential sweep takes the fused middle pass when the shape has it, every kernel is held in the form it
// reads and nothing else lays claim to the layout of the work volumes (halo exchanges copy planes of the row-major
// spectrum).  Decided per iterate() call, behind decide_layout().
void Engine::decide_lines() {
  const bool was = lines_last_sweep_;
  const FormRule rule = form_rule();
  bool all = rule.sw.mid_fused != 0 && plan_->lines_capable() && !views_.empty();
  if (halo_fn_ || halo_planes_ > 0)  // slabs: the common decision of whoever drives them, on plane ranges
    all = all && halo_fn_ && lines_override_ == 1 && halo_ranged() && halo_nyq_aware_;
  if (all) {
    if (pipelined_) {
      all = lines_hint_;
    } else {
      for (size_t v = 0; v < views_.size() && all; ++v)
        all = views_[v].set && views_[v].tap_k[0] && views_[v].tap_k[1] && views_[v].taps_l_ok[0] && views_[v].taps_l_ok[1] &&
              rule.lines_worth(views_[v].tap_k[0]) && rule.lines_worth(views_[v].tap_k[1]);
    }
  }
  lines_ = lines_last_sweep_ = all;
  if (was != lines_) ++graph_gen_;  // (a captured sweep holds the form of its passes)
}

// the three middle passes of convolution i as ONE: work_ -> work2_ (line layout), the volumes swap roles
void Engine::mid_fused_conv(const ViewSlot& s, int i, Profiler* prof, int zbeg, int zcount) {
  if (!s.taps_l_ok[i] || !s.tap_k[i]) throw std::logic_error("mvn: fused middle pass with a kernel that is not in its form");
  ensure_work2();
  if (++epoch_ == 0x7fffffffu) {
    be::dzero(poison_, poison_bytes(), stream_.get());
    epoch_ = 1;
  }
  armed_epoch_ = epoch_;
  plan_->mid_fused((const cfloat*)work_, (cfloat*)work2_, (const cfloat*)s.taps_l[i].get(), s.tap_k[i], s.tap_kd[i],
                   poison_word(epoch_), epoch_, stream_.get(), prof, zbeg, zcount, (int)poison_peers_.size(),
                   poison_table(epoch_));
  std::swap(work_, work2_);
  std::swap(work_nyq_, work2_nyq_);
}

void Engine::middle(const ViewSlot& s, int i, Profiler* prof, SideStream* side, const RowsProducer* produce) {
  const Plan3D& P = *plan_;
  if (lines_) {
    if (!halo_fn_) {
      if (produce && *produce) (*produce)(0, -1);
      mid_fused_conv(s, i, prof);
      return;
    }
    // Halo mode on the line layout: the first and last H planes of the slab are the neighbours'.  The last-axis pass
    // that produces this convolution's input runs on the own planes [H, d0 - H) - the H planes at either end of them
    // FIRST, then the call that lets the neighbours pull them (planes are contiguous in the line layout as they are
    // in the row-major one), then the interior beside the copies -, the second call waits for the halos, and ONE
    // middle pass walks every column from plane 0 to produce the own planes (it never wraps: its window fills on
    // the lower halo).  Same calls, same order as the three-pass form below.
    const int H = halo_planes_, own = P.L.d0 - 2 * H, view = (int)(&s - views_.data());
    const long d1 = P.L.d1;
    auto rows = [&](int z0, int nz) {
      if (produce && *produce) (*produce)((long)z0 * d1, (long)nz * d1);
    };
    auto call = [&](int what) {
      if (halo_drain_) be::stream_sync(stream_.get());
      halo_fn_(halo_user_, work_, view, what);
    };
    if (produce && boundary_first()) {
      rows(H, H);
      rows(own, H);
      call(i);
      rows(2 * H, own - 2 * H);
    } else {
      rows(H, own);
      call(i);
    }
    if (halo_split_) call(i + 4);
    mid_fused_conv(s, i, prof, H, own);
    if (halo_post_) call(i + 2);
    return;
  }
  // One launch chain on stream_.get() - dim1 forward, direct leg, dim1 inverse, three launches - wherever the Nyquist bins
  // need no launches of their own: packed into the DC column, or (split layout) riding in the dim1 launches and in
  // the leg's.
  const bool one_chain = packed_ || (s.tap_k[i] != 0 && (!P.L.even || P.nyq_rides()));
  if (one_chain) {
    if (!s.tap_k[i]) throw std::logic_error("mvn: packed Nyquist layout with a kernel that is not in the direct form");
    if (halo_fn_ && !packed_ && !halo_nyq_aware_)
      throw std::logic_error("mvn: this halo hook exchanges the main array only: it needs the packed Nyquist layout");
    // Halo mode: the first and last H planes of the volume are the neighbours'.  No pass computes them - the
    // last-axis and dim1 passes run on the own planes [H, d0 - H) only, the leg produces only those - and the leg
    // runs in two parts: the planes that do not depend on the halos first, so that the exchange (the hook's
    // business) can go on beside them, then - behind the hook's second call - the H planes next to either halo.
    const int H = halo_ranged() ? halo_planes_ : 0;
    const int own = P.L.d0 - 2 * H;
    const int view = (int)(&s - views_.data());
    const long d1 = P.L.d1;
    auto rows = [&](int z0, int nz) {  // the pass that produces the planes [z0, z0 + nz) of this convolution's input
      if (produce && *produce) (*produce)(H > 0 ? (long)z0 * d1 : 0, H > 0 ? (long)nz * d1 : -1);
    };
    if (produce && boundary_first()) {
      // the planes the neighbours need FIRST - last-axis pass and dim1 pass of the H planes at either end of the own
      // range -, then the call that lets them pull, then the interior: their copies run beside these two passes'
      // interior and the leg's, not beside the leg's alone
      rows(H, H);
      rows(own, H);
      P.axis1(MVN_ST_FWD, (cfloat*)work_, wn(), stream_.get(), prof, stream_.get(), H, H);
      P.axis1(MVN_ST_FWD, (cfloat*)work_, wn(), stream_.get(), nullptr, stream_.get(), own, H);
      if (halo_drain_) be::stream_sync(stream_.get());
      halo_fn_(halo_user_, work_, view, i);
      rows(2 * H, own - 2 * H);
      P.axis1(MVN_ST_FWD, (cfloat*)work_, wn(), stream_.get(), nullptr, stream_.get(), 2 * H, own - 2 * H);
    } else {
      rows(H, own);
      P.axis1(MVN_ST_FWD, (cfloat*)work_, wn(), stream_.get(), prof, stream_.get(), H, own);
      if (halo_fn_) {  // the neighbours' planes arrive in the halo planes of the leg's input
        if (halo_drain_) be::stream_sync(stream_.get());
        halo_fn_(halo_user_, work_, view, i);
      }
    }
    ensure_work2();
    const cfloat* in = (const cfloat*)work_;
    const cfloat* in_n = packed_ ? nullptr : work_nyq_;
    cfloat* out = (cfloat*)work2_;
    cfloat* out_n = packed_ ? nullptr : work2_nyq_;
    if (H == 0) {
      if (halo_fn_ && halo_split_) {  // (no ranges, e.g. rows that do not end on tile boundaries: one part)
        if (halo_drain_) be::stream_sync(stream_.get());
        halo_fn_(halo_user_, work_, view, i + 4);
      }
      dim0_conv(s, i, in, in_n, out, out_n, prof);
    } else if (halo_split_ && own > 2 * H) {
      dim0_conv(s, i, in, in_n, out, out_n, prof, 2 * H, own - 2 * H, true);
      if (halo_drain_) be::stream_sync(stream_.get());
      halo_fn_(halo_user_, work_, view, i + 4);  // the halo planes must be in place behind this call
      dim0_conv(s, i, in, in_n, out, out_n, nullptr, H, H, false);
      dim0_conv(s, i, in, in_n, out, out_n, nullptr, own, H, false);
    } else {
      if (halo_split_) {
        if (halo_drain_) be::stream_sync(stream_.get());
        halo_fn_(halo_user_, work_, view, i + 4);
      }
      dim0_conv(s, i, in, in_n, out, out_n, prof, H, own, true);
    }
    std::swap(work_, work2_);
    std::swap(work_nyq_, work2_nyq_);
    P.axis1(MVN_ST_INV, (cfloat*)work_, wn(), stream_.get(), prof, stream_.get(), H, own);
    if (halo_fn_ && halo_post_) {  // the slabs merge their reports of non-finite inputs under the dim1 pass
      if (halo_drain_) be::stream_sync(stream_.get());
      halo_fn_(halo_user_, work_, view, i + 2);
    }
    return;
  }
  if (halo_fn_)
    throw std::logic_error("mvn: halo mode needs every PSF in the direct form (<= 33 planes) and Nyquist bins that need no "
                           "launches of their own (packed, or riding in the fixed-length dim1 kernels)");
  if (produce && *produce) (*produce)(0, -1);  // (no plane ranges outside halo mode)
  if (!s.tap_k[i]) {
    P.middle_passes((cfloat*)work_, work_nyq_, (const cfloat*)s.spec[i].get(), s.nyq[i].get(),
                    stream_.get(), prof, side, spec_tiled_);
    return;
  }
  // The folded dim0 leg needs two fork / join pairs per convolution (17 - 20 us of cross-queue latency each):
  // below 256 MB the Nyquist plane's two dim1 launches cost less in line
  // (256^3 per view update: 0.329 ms with the side stream, 0.312 with the fused FFT pass)
  const bool use_side = side && side->s.get() && P.L.even && P.main_bytes() > ((size_t)256 << 20) && !P.nyq_rides();
  be::stream_t sn = use_side ? side->s.get() : stream_.get();
  // the Nyquist plane's dim1 launches go on the side stream; its dim0 leg rides in the main launch, so the side
  // stream joins before that launch and forks again behind it
  if (use_side) side->fork_from(stream_.get());  // the plane was written by the last-axis pass just enqueued on stream_.get()
  P.axis1(MVN_ST_FWD, (cfloat*)work_, work_nyq_, stream_.get(), prof, sn);
  ensure_work2();
  if (use_side) side->join_into(stream_.get());
  dim0_conv(s, i, (const cfloat*)work_, work_nyq_, (cfloat*)work2_, work2_nyq_, prof);
  if (use_side) side->fork_from(stream_.get());
  std::swap(work_, work2_);
  std::swap(work_nyq_, work2_nyq_);
  P.axis1(MVN_ST_INV, (cfloat*)work_, work_nyq_, stream_.get(), prof, sn);
  if (use_side) side->join_into(stream_.get());  // the next last-axis pass on stream_.get() reads the plane
}

void Engine::set_view(int v, const StackRef& image, const StackRef& weights, const float* kernel1, const int* k1dims,
                      const float* kernel2, const int* k2dims) {
  if (v < 0 || v >= (int)views_.size()) throw std::out_of_range("mvn: view index");
  be::set_device(device_);
  if (stream_pos_[(size_t)v] >= 0) throw std::logic_error("mvn: a streamed view is staged by the pipelined call only");
  ViewSlot& s = views_[(size_t)v];
  // (halo mode divides row ranges, whose offsets are in floats: the image stays float32 under a hook)
  want_u16_[(size_t)v] = image_storage_ == 1 && image.u16 && !image.broadcast() && !halo_fn_ && !image.geom;
  alloc_view(s);
  ingest_pair(s.image.get(), s.weights.get(), image, weights, stream_.get(), s.image_u16);
  be::stream_sync(stream_.get());  // the sources have been consumed
  prepare_psfs(s, kernel1, k1dims, kernel2, k2dims, false, stream_.get());
  s.set = true;
}

void Engine::prepare_psfs(ViewSlot& s, const float* kernel1, const int* k1dims, const float* kernel2, const int* k2dims,
                          bool staging, be::stream_t st) {
  const float* ks[2] = {kernel1, kernel2};
  const int* kd[2] = {k1dims, k2dims};
  for (int i = 0; i < 2; ++i) {
    if (psf_resident(s, i, ks[i], kd[i])) continue;
    const size_t kb = sizeof(float) * (size_t)kd[i][0] * (size_t)kd[i][1] * (size_t)kd[i][2];
    be::DeviceBuffer<float> own(kb);
    float* dk = own.get();
    if (staging) stage_scratch_.push_back(std::move(own));  // freed in finish_staging(), after the stream has drained
    be::h2d(dk, ks[i], kb, st);
    try {
      // nothing else runs on this engine during a blocking set_view: the work volume is the scratch
      if (!staging) work_has_psi_spectrum_ = false;
      prepare_psf(s, i, dk, kd[i], staging ? nullptr : work_, staging, st);
      // the direct leg's second work volume: allocated here, not inside a sweep (reserve_views has, when staging)
      if (!staging && s.tap_k[i]) ensure_work2();
      if (!staging) be::stream_sync(st);
    } catch (...) {
      if (!staging) be::drain_quietly(st);
      s.kcopy[i].clear();  // the resident form is in an unknown state: never a cache hit
      throw;
    }
  }
}

// ---- pipelined staging ------------------------------------------------------------------------
void Engine::reserve_views(const kernel_list_t& kernels) {
  be::set_device(device_);
  for (size_t v = 0; v < views_.size(); ++v) alloc_view(views_[v]);
  if (sw_.direct) ensure_work2();  // (not inside the first sweep: the direct dim0 leg is out of place)
  if (!upload_stream_.get()) upload_stream_ = be::Stream::create_upload();
  staged_ev_.resize(views_.size());
  for (size_t v = 0; v < views_.size(); ++v)
    if (!staged_ev_[v].get()) staged_ev_[v] = be::Event::sync_only();
  staged_.assign(views_.size(), 0);
  pre_ingested_.assign(views_.size(), 0);
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    uploads_ = consumed_ = 0;
    stream_abort_ = false;
    stream_done_ = false;
  }
  // the loop starts before the last view has been staged: will every kernel of the call be held in the direct dim0
  // form (then the Nyquist bins ride in the DC column) and take the fused middle pass?
  const FormRule rule = form_rule();
  packed_hint_ = rule.all_direct(kernels);
  lines_hint_ = rule.all_lines(kernels);
  pipelined_ = true;
}

void Engine::ingest_device_view(int v, const StackRef& image, const StackRef& weights) {
  be::set_device(device_);
  ViewSlot& s = views_[(size_t)v];
  if (stream_pos_[(size_t)v] >= 0) throw std::logic_error("mvn: a call with stacks in device memory runs resident");
  ingest_pair(s.image.get(), s.weights.get(), image, weights, stream_.get(), s.image_u16);
  pre_ingested_[(size_t)v] = 1;
}

// uploader thread: the stacks and the PSFs of view v on the upload stream, then the view is staged
void Engine::stage_view(int v, const StackRef& image, const StackRef& weights, const float* kernel1, const int* k1dims,
                        const float* kernel2, const int* k2dims) {
  be::set_device(device_);  // the HIP device is per host thread
  ViewSlot& s = views_[(size_t)v];
  if (stream_pos_[(size_t)v] >= 0)
    ring_upload(v, image, weights);
  else if (!pre_ingested_[(size_t)v])
    ingest_pair(s.image.get(), s.weights.get(), image, weights, upload_stream_.get(), s.image_u16);
  prepare_psfs(s, kernel1, k1dims, kernel2, k2dims, true, upload_stream_.get());
  be::event_record(staged_ev_[(size_t)v].get(), upload_stream_.get());
  s.set = true;
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    staged_[(size_t)v] = 1;
  }
  stage_cv_.notify_all();
}

void Engine::staging_failed() {
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    for (size_t v = 0; v < staged_.size(); ++v)
      if (staged_[v] == 0) staged_[v] = -1;
    stream_abort_ = true;  // (a main thread waiting for a ring slot's upload)
  }
  stage_cv_.notify_all();
}

void Engine::finish_staging() {
  be::set_device(device_);
  if (upload_stream_.get()) be::stream_sync(upload_stream_.get());
  stage_scratch_.clear();
  stage_spec_scratch_ = nullptr;
}

// main thread: block until the uploader has enqueued view v, then make the compute stream wait
// for the upload stream's event
void Engine::wait_staged(int v) {
  std::unique_lock<std::mutex> lk(stage_mu_);
  stage_cv_.wait(lk, [&] { return staged_[(size_t)v] != 0; });
  if (staged_[(size_t)v] < 0) throw std::runtime_error("mvn: staging of view " + std::to_string(v) + " failed");
  lk.unlock();
  be::stream_wait_event(stream_.get(), staged_ev_[(size_t)v].get());
}

// ---- out-of-core views ---------------------------------------------------------------------------
// Upload k of the call (stream order: the streamed views of sweep 0, then of sweep 1, ...) lands in ring slot
// k % R.  The uploader waits on the host until view update k - R - the slot's previous reader - has been enqueued,
// then makes the upload stream wait for that update's `freed` event; the main thread waits on the host until
// upload k has been enqueued, then makes the compute stream wait for its `filled` event.  Both counters move
// under stage_mu_, so neither event is re-recorded before the wait that refers to its last record was enqueued.
static std::atomic<long long> g_stream_calls{0}, g_stream_updates{0}, g_stream_bytes{0};

void Engine::stream_counters(long long out[3]) {
  out[0] = g_stream_calls.load();
  out[1] = g_stream_updates.load();
  out[2] = g_stream_bytes.load();
}

void Engine::count_streamed_call() { ++g_stream_calls; }

std::vector<int> Engine::spread_views(int V, int s) {
  std::vector<int> out;
  for (int j = 0; j < s; ++j) out.push_back((int)(((2L * j + 1) * V) / (2L * s)));
  return out;
}

std::vector<char> Engine::kept_u16(const std::vector<char>& want, const std::vector<int>& streamed, int V) {
  std::vector<char> out((size_t)V, 0);
  if (want.empty()) return out;
  if ((int)want.size() != V) throw std::invalid_argument("mvn: one image storage wish per view");
  for (int v = 0; v < V; ++v) out[(size_t)v] = want[(size_t)v] ? 1 : 0;
  bool all = true;
  for (int v : streamed) all = all && out[(size_t)v];
  if (!all)
    for (int v : streamed) out[(size_t)v] = 0;
  return out;
}

void Engine::plan_image_types(const std::vector<char>& want) {
  be::set_device(device_);
  want_u16_ = kept_u16(want, streamed_order_, (int)views_.size());
  if (ring_.empty()) return;
  const bool u16 = want_u16_[(size_t)streamed_order_[0]] != 0;  // (all streamed views, or none)
  if (ring_[0].image.get() && ring_[0].image_u16 == u16) return;
  alloc_ring_images(u16);
}

// the ring's image volumes (again): zeroed once, the padded rows and the embedding margins are never written
void Engine::alloc_ring_images(bool u16) {
  be::stream_sync(stream_.get());
  for (RingSlot& r : ring_) r.image.reset();
  for (RingSlot& r : ring_) {
    r.image = be::DeviceBuffer<float>(image_bytes(u16));
    r.image_u16 = u16;
    be::dzero(r.image.get(), image_bytes(u16), stream_.get());
  }
  be::stream_sync(stream_.get());
}

int Engine::u16_views() const {
  int n = 0;
  for (const ViewSlot& s : views_) n += (s.image.get() && s.image_u16) ? 1 : 0;
  return n;
}

void Engine::divide_epilogue(EpilogueParams& e, const ViewStacks& in) const {
  e.view = in.image;
  e.mode = MVN_EPI_DIVIDE;
  if (in.image_u16) {
    e.view16 = (const unsigned short*)in.image;
    e.mode = MVN_EPI_DIVIDE_U16;
    ++g_u16_divides;
  }
}

void Engine::set_residency(const std::vector<int>& streamed, int ring) {
  if (!streamed_order_.empty() || !ring_.empty()) throw std::logic_error("mvn: the residency plan is set once");
  for (size_t v = 0; v < views_.size(); ++v)
    if (views_[v].image.get()) throw std::logic_error("mvn: the residency plan is set before the views are allocated");
  if (streamed.empty()) {
    if (ring != 0) throw std::invalid_argument("mvn: a ring without streamed views");
    return;
  }
  if (ring < 1 || ring > 2) throw std::invalid_argument("mvn: ring of 1 or 2 slots");
  be::set_device(device_);
  for (size_t j = 0; j < streamed.size(); ++j) {
    const int v = streamed[j];
    if (v < 0 || v >= (int)views_.size() || stream_pos_[(size_t)v] >= 0 || (j && v < streamed[j - 1]))
      throw std::invalid_argument("mvn: streamed views must be distinct view indices in sweep order");
    stream_pos_[(size_t)v] = (int)j;
    streamed_order_.push_back(v);
  }
  const size_t mb = plan_->main_bytes();
  ring_.resize((size_t)ring);
  for (RingSlot& r : ring_) {  // zeroed once: the padded rows and the embedding margins are never written
    // (the image volumes come with the call's image types: plan_image_types)
    r.weights = be::DeviceBuffer<float>(mb);
    be::dzero(r.weights.get(), mb, stream_.get());
    r.filled = be::Event::sync_only();
    r.freed = be::Event::sync_only();
  }
  be::stream_sync(stream_.get());
}

void Engine::ring_upload(int v, const StackRef& image, const StackRef& weights) {
  if (stream_pos_[(size_t)v] < 0) throw std::logic_error("mvn: view " + std::to_string(v) + " is resident");
  const long R = (long)ring_.size();
  long k;
  {
    std::unique_lock<std::mutex> lk(stage_mu_);
    k = uploads_;
    stage_cv_.wait(lk, [&] { return stream_abort_ || stream_done_ || consumed_ >= k - R + 1; });
    if (stream_abort_) throw std::runtime_error("mvn: streamed call abandoned");
    if (stream_done_) return;  // (the loop stopped early: no later sweep reads this upload)
  }
  RingSlot& r = ring_[(size_t)(k % R)];
  if (k >= R) be::stream_wait_event(upload_stream_.get(), r.freed.get());
  if (image.device || weights.device) throw std::logic_error("mvn: a call with stacks in device memory runs resident");
  if (!r.image.get()) throw std::logic_error("mvn: the ring has no image volumes (plan_image_types)");
  g_stream_bytes += ingest_pair(r.image.get(), r.weights.get(), image, weights, upload_stream_.get(), r.image_u16);
  be::event_record(r.filled.get(), upload_stream_.get());
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    ++uploads_;
  }
  stage_cv_.notify_all();
}

void Engine::stream_view(int v, const StackRef& image, const StackRef& weights) {
  if (v < 0 || v >= (int)views_.size()) throw std::out_of_range("mvn: view index");
  be::set_device(device_);
  ring_upload(v, image, weights);
}

void Engine::abort_streaming() {
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    stream_abort_ = true;
  }
  stage_cv_.notify_all();
}

ViewStacks Engine::ring_acquire() {
  long k;
  {
    std::unique_lock<std::mutex> lk(stage_mu_);
    k = consumed_;
    stage_cv_.wait(lk, [&] { return uploads_ > k || stream_abort_; });
    if (uploads_ <= k) throw std::runtime_error("mvn: upload of a streamed view failed");
  }
  const RingSlot& r = ring_[(size_t)(k % (long)ring_.size())];
  be::stream_wait_event(stream_.get(), r.filled.get());
  return ViewStacks{r.image.get(), r.image_u16, r.weights.get()};
}

// the view update that reads the pair has been enqueued whole (its last reader is the update pass ending
// conv_pair): the slot is free behind it
void Engine::ring_release() {
  const long k = consumed_;  // (written by this thread only)
  be::event_record(ring_[(size_t)(k % (long)ring_.size())].freed.get(), stream_.get());
  ++g_stream_updates;
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    ++consumed_;
  }
  stage_cv_.notify_all();
}

// ---- memory model -------------------------------------------------------------------------------
// Plan tables (a few twiddle and index arrays per axis), the poison words of the plans and allocator rounding are
// not listed one by one: every allocation is rounded up to 4 KiB and a fixed slack covers the rest.
static const size_t kMemSlack = (size_t)1 << 20;
static size_t alloc_rounded(size_t b) { return (b + 4095) & ~(size_t)4095; }

// The table of the loop state: which buffers the switches of a call need, and how large (a buffer of 0 bytes is not
// needed).  Read by Engine::memory_need and by Engine::iterate alike.
void LoopState::bytes_of(const Layout& L, int V, int iterations, double lambda, const LoopOptions& o,
                         size_t bytes[N_BUFFERS]) {
  const size_t mb = L.real_floats() * sizeof(float), n = (size_t)std::max(iterations, 0);
  const size_t records = 3 * sizeof(double) * (size_t)record_cap(L) * (size_t)V, counts = sizeof(unsigned) * (size_t)V;
  std::fill(bytes, bytes + N_BUFFERS, (size_t)0);
  if (o.stats_on()) {
    bytes[STAT_REC] = records, bytes[STAT_COUNT] = counts;
    bytes[STAT_OUT] = 3 * sizeof(double) * std::max(n, (size_t)1);
  }
  if (n == 0) return;  // (the other switches add nothing to a call without sweeps)
  if (o.noise_model_on()) {
    bytes[NM_REC] = records, bytes[NM_COUNT] = counts;
    bytes[NM_OUT] = 3 * sizeof(double) * n * (size_t)V;
  }
  if (o.accel_on()) {
    bytes[X_PREV] = bytes[G_PREV] = bytes[Y_SAVE] = mb;
    bytes[ACCEL_REC] = 2 * sizeof(double) * (size_t)accel_records(L);
    bytes[ALPHA] = sizeof(float) * n;
  }
  if (o.tv_on(lambda)) bytes[TV] = mb;
}

void LoopState::allocate(const size_t bytes[N_BUFFERS]) {
  for (int b = 0; b < N_BUFFERS; ++b)
    if (bytes[b] && !buf[b].get()) buf[b] = be::DeviceBuffer<>(bytes[b]);
}

void LoopState::release(int first, int last) {
  for (int b = first; b < last; ++b) buf[b].reset();
}

size_t Engine::memory_need(const MemoryQuery& q, const FormRule& rule) {
  const Layout& L = rule.L;
  if (L.d0 != q.ext[0] || L.d1 != q.ext[1] || L.d2 != q.ext[2]) throw std::logic_error("mvn: memory query of other extents");
  const int V = (int)(q.kernels.size() / 2);
  if (q.kernels.size() % 2 || q.streamed < 0 || q.streamed > V || q.ring < 0 || q.ring > 2 ||
      (q.streamed > 0) != (q.ring > 0))
    throw std::invalid_argument("mvn: memory query: bad residency plan");
  const size_t mb = L.real_floats() * sizeof(float), nb = L.nyq_cplx() * sizeof(cfloat);
  size_t total = kMemSlack;
  auto add = [&](size_t bytes, size_t n) {
    if (bytes) total += n * alloc_rounded(bytes);
  };
  add(mb, 1);                                     // psi
  add(mb, 1), add(nb, 1);                         // work volume
  if (rule.sw.direct) add(mb, 1), add(nb, 1);      // second work volume (reserve_views)
  add(256, 1);                                    // poison words
  add(q.embed_floats * sizeof(float), 1);         // embedding scratch of the padded policies
  // image + weights of the resident views, ring slots of the streamed ones; an image held as uint16 (kept_u16) is
  // the same element grid at 2 bytes per voxel
  const std::vector<int> sv = spread_views(V, q.streamed);
  const std::vector<char> kept = kept_u16(q.image_u16, sv, V);
  std::vector<char> streams((size_t)V, 0);
  for (int v : sv) streams[(size_t)v] = 1;
  for (int v = 0; v < V; ++v)
    if (!streams[(size_t)v]) add(kept[(size_t)v] ? mb / 2 : mb, 1), add(mb, 1);
  if (q.ring) add(kept[(size_t)sv[0]] ? mb / 2 : mb, (size_t)q.ring), add(mb, (size_t)q.ring);
  size_t scr = 0;
  bool spectra = false;
  for (const std::array<int, 3>& k : q.kernels) {
    add(sizeof(float) * (size_t)k[0] * k[1] * k[2], 1);  // the kernel's device copy, until staging has drained
    if (rule.direct(k.data())) {
      const Layout T(taps_depth(k[0]), L.d1, L.d2);
      const size_t tb = T.real_floats() * sizeof(float);
      add(tb, 1), add(T.nyq_cplx() * sizeof(cfloat), 1);  // taps
      if (rule.lines_taps(k.data())) {
        add(tb, 1);  // the fused middle pass's taps
        scr = std::max(scr, tb);
      }
    } else {
      add(mb, 1), add(nb, 1);  // 3-D spectrum
      spectra = true;
    }
  }
  add(scr, 1);                                        // the engine's one tap scratch
  if (spectra && ax0_fixed(L, rule.plan_fixed)) add(mb, 1);  // re-tiling scratch of the staging thread
  size_t loop[LoopState::N_BUFFERS];  // what the switches of the loop add (Engine::iterate)
  LoopState::bytes_of(L, V, q.iterations, q.lambda, q.loop, loop);
  for (size_t b : loop) add(b, 1);
  // (psi_spec_.get() and delta_ belong to the simultaneous steps of the view-sharded drivers: never allocated here)
  return total;
}

void Engine::set_psi(const StackRef& st) {
  if (st.u16) throw std::invalid_argument("mvn: psi is float32");
  be::set_device(device_);
  psi_spec_valid_ = false;
  ingest_stack(psi_.get(), st, embed_scratch_.get(), embedded_, stream_.get());  // (the loop has written the margins of an embedded psi)
  be::stream_sync(stream_.get());
}

void Engine::get_psi(const StackRef& st) {
  if (st.u16) throw std::invalid_argument("mvn: psi is float32");
  be::set_device(device_);
  const Layout& L = plan_->L;
  const int* n = host_dims_;
  for (int d = 0; d < 3; ++d)
    if (n[d] > 1 && st.stride[d] <= 0) throw std::invalid_argument("mvn: psi needs positive strides");
  ExtractParams e;
  e.src = psi_.get(), e.RP = L.RP, e.D1 = L.d1;
  e.n0 = n[0], e.n1 = n[1], e.n2 = n[2];
  e.o0 = host_off_[0], e.o1 = host_off_[1], e.o2 = host_off_[2];
  if (st.device) {  // straight into the caller's memory
    e.dst = (float*)st.ptr, e.s0 = st.stride[0], e.s1 = st.stride[1], e.s2 = st.stride[2];
    be::launch_extract3d(e, stream_.get());
    be::stream_sync(stream_.get());
    return;
  }
  check_host_rows(st, n);
  if (embedded_ && !embed_scratch_.get()) throw std::logic_error("mvn: no scratch for a host stack");
  const bool dense = (n[1] == 1 || st.stride[1] == n[2]) && (n[0] == 1 || st.stride[0] == (long long)n[1] * n[2]);
  const char* src = (const char*)psi_.get();
  size_t srow = (size_t)L.RP * sizeof(float), splane = (size_t)L.d1 * srow;
  if (embedded_) {  // the window into the scratch first: a strided device copy for dense rows, the extract pass else
    if (dense) {
      be::launch_copy3d(embed_scratch_.get(), n[2], (long)n[1] * n[2],
                        psi_.get() + ((size_t)host_off_[0] * L.d1 + host_off_[1]) * L.RP + host_off_[2], L.RP,
                        (long)L.d1 * L.RP, n[2], n[1], n[0], stream_.get());
    } else {
      e.dst = embed_scratch_.get(), e.s0 = (long long)n[1] * n[2], e.s1 = n[2], e.s2 = 1;
      be::launch_extract3d(e, stream_.get());
    }
    src = (const char*)embed_scratch_.get();
    srow = (size_t)n[2] * sizeof(float), splane = (size_t)n[1] * srow;
  }
  const size_t width = (size_t)n[2] * sizeof(float);
  if (dense && srow == width)
    be::d2h((void*)st.ptr, src, host_floats() * sizeof(float), stream_.get());
  else if (dense)
    be::d2h_2d((void*)st.ptr, width, src, srow, width, L.rows, stream_.get());
  else
    for (int z = 0; z < n[0]; ++z)
      be::d2h_2d((char*)st.ptr + (long long)z * st.stride[0] * 4, n[1] == 1 ? width : (size_t)st.stride[1] * 4,
                 src + z * splane, srow, width, (size_t)n[1], stream_.get());
  be::stream_sync(stream_.get());
}

// one (view, iteration): the reference's steps 1-4, src/gpu_deconvolve_methods.cuh:491-532.
//   psi (*) kernel1 -> view / blurred -> (*) kernel2 -> psi update
// With a fixed-length plan the two last-axis passes that meet between the convolutions
// (c2r + divide, then r2c) run as ONE kernel, and so do the update pass and the forward
// last-axis pass of the NEXT (view, iteration) when `feed_next` is set: 8 full passes instead of 10.
void Engine::conv_pair(int v, const ViewStacks& in, double lambda, float min_value, int final_mode, int accumulate,
                       bool feed_next) {
  const ViewSlot& s = views_[(size_t)v];
  if (!s.set) throw std::runtime_error("mvn: view " + std::to_string(v) + " was never set");
  Profiler* prof = nullptr;
  if (prof_.enabled && (pair_counter_++ % (prof_.sample_every > 0 ? prof_.sample_every : 1)) == 0)
    prof = &prof_;
  const Plan3D& P = *plan_;
  const bool fuse = P.can_fuse_rows();

  EpilogueParams e1;
  std::memset(&e1, 0, sizeof(e1));
  e1.scale = 1.f;  // 1/N already lives in the PSF spectrum
  divide_epilogue(e1, in);
  e1.guard_zero_view = quotient_guard_ ? 1 : 0;
  // noise model: the same pass with the view's background in the forward model and the statistics of the window
  const bool nm = nm_records().on() && final_mode == MVN_EPI_UPDATE;
  const MvnStatsParams st1 = nm ? params_for(nm_records(), v) : MvnStatsParams();
  if (nm) {
    e1.mode = e1.mode == MVN_EPI_DIVIDE_U16 ? MVN_EPI_DIVIDE_NM_U16 : MVN_EPI_DIVIDE_NM;
    e1.background = loop_.o.background_of(v);
  }

  EpilogueParams e2;
  std::memset(&e2, 0, sizeof(e2));
  const bool stats = stat_records().on() && final_mode == MVN_EPI_UPDATE;
  const MvnStatsParams st2 = stats ? params_for(stat_records(), v) : MvnStatsParams();
  e2.mode = stats ? MVN_EPI_UPDATE_STATS : final_mode;
  // total variation: the factor of psi as it stands now - psi does not change before this view's update pass -
  // multiplies the integral there; lambda is the TV weight and the Tikhonov branch stays off
  const bool tv = tv_volume() && final_mode == MVN_EPI_UPDATE;
  if (tv) {
    ProfScope ps(prof, KK_TV, stream_.get());
    be::launch_tv(tv_params(P.L, psi_.get(), tv_volume(), lambda, loop_.o.epsilon), stream_.get());
    e2.mode = stats ? MVN_EPI_UPDATE_STATS_TV : MVN_EPI_UPDATE_TV;
    e2.tv = tv_volume();
    lambda = 0.;
  }
  e2.scale = 1.f;
  e2.psi = psi_.get();
  e2.weights = in.weights;
  e2.delta = delta_;
  e2.accumulate = accumulate;
  e2.lambda = lambda;
  e2.lambda_inv = lambda > 0 ? (float)(1.f / lambda) : 0.f;
  e2.min_value = min_value;

  // convolution 1: psi (*) kernel1
  // The Nyquist-plane launches run on a second stream under the full-volume passes - except for
  // small volumes, where the two event waits per convolution cost more than three more 4 us
  // launches in line (measured per view update: 64^3 0.095 -> 0.074 ms, 96^3 0.124 -> 0.105 ms,
  // 128^3 0.143 -> 0.134 ms in line; 256^3 0.308 -> 0.340 ms, so the switch sits in between).
  SideStream* side = P.main_bytes() <= kSideMinBytes ? nullptr : &side_;
  // The last-axis pass that PRODUCES a convolution's input is handed to middle() as a function of a row range: in
  // halo mode with a split leg the planes next to the halos are produced (and dim1-transformed) FIRST, so that the
  // neighbours can pull them while this slab still works on its interior (middle()); otherwise it is called once.
  // (work_ / work_nyq_ are read when a producer is BUILT: the direct dim0 leg swaps the two work volumes, and a
  // producer runs before the next leg.)
  const Plan3D* Pp = plan_.get();
  be::stream_t st = stream_.get();
  RowsProducer p1;
  if (pending_rows_) {  // the previous view update's fused update + forward pass, deferred (boundary-first order)
    p1 = std::move(pending_rows_);
    pending_rows_ = nullptr;
  } else if (!work_has_psi_spectrum_) {
    const float* psi = psi_.get();
    cfloat* w = (cfloat*)work_;
    cfloat* wnq = wn();
    const bool ln = lines_;
    p1 = [=](long r0, long nr) { Pp->rows_r2c(psi, w, ln ? nullptr : wnq, st, prof, r0, nr, ln); };
  }
  work_has_psi_spectrum_ = false;
  middle(s, 0, prof, side, p1 ? &p1 : nullptr);
  arm(e1);
  // view / blurred, handed to convolution 2 as its last-axis spectrum
  {
    float* w = work_;
    cfloat* wnq = wn();
    const bool ln = lines_;
    RowsProducer p2 = [=](long r0, long nr) {
      const MvnStatsParams* s1 = nm ? &st1 : nullptr;
      if (ln) {
        Pp->rows_c2r_r2c((cfloat*)w, nullptr, e1, st, prof, r0, nr, true, s1);
      } else if (fuse) {
        Pp->rows_c2r_r2c((cfloat*)w, wnq, e1, st, prof, r0, nr, false, s1);
      } else {
        Pp->rows_c2r((const cfloat*)w, wnq, w, e1, st, prof, r0, nr, false, s1);
        Pp->rows_r2c(w, (cfloat*)w, wnq, st, prof, r0, nr);
      }
    };
    // convolution 2: quotient (*) kernel2, then the psi update fused into the last pass
    middle(s, 1, prof, side, &p2);
  }
  arm(e2);
  // (halo mode: the rows of the own planes only)
  const long r0 = halo_ranged() ? (long)halo_planes_ * P.L.d1 : 0;
  const long nr = halo_ranged() ? (long)(P.L.d0 - 2 * halo_planes_) * P.L.d1 : -1;
  if (fuse && feed_next && final_mode == MVN_EPI_UPDATE) {  // (with or without the statistics)
    float* w = work_;
    cfloat* wnq = wn();
    const bool ln = lines_;
    RowsProducer upd = [=](long a, long n) {
      Pp->rows_c2r_r2c((cfloat*)w, ln ? nullptr : wnq, e2, st, prof, a, n, ln, stats ? &st2 : nullptr);
    };
    if (boundary_first())
      pending_rows_ = std::move(upd);  // runs as the producer of the NEXT convolution, boundary planes first
    else
      upd(r0, nr);
    work_has_psi_spectrum_ = true;
  } else {
    P.rows_c2r((const cfloat*)work_, lines_ ? nullptr : wn(), psi_.get(), e2, stream_.get(), prof, r0, nr, lines_,
               stats ? &st2 : nullptr);
  }
}

// a deferred producer also WRITES psi (the update epilogue): whoever leaves the loop runs it
void Engine::flush_pending_rows() {
  if (!pending_rows_) return;
  const long d1 = plan_->L.d1;
  const bool rg = halo_ranged();
  pending_rows_(rg ? (long)halo_planes_ * d1 : 0, rg ? (long)(plan_->L.d0 - 2 * halo_planes_) * d1 : -1);
  pending_rows_ = nullptr;
}

// the leg runs in two parts and the slab has planes that do not depend on its halos: boundary planes first
bool Engine::boundary_first() const {
  return halo_fn_ && halo_split_ && halo_ranged() && plan_->L.d0 - 2 * halo_planes_ > 2 * halo_planes_;
}

// Sweeps 2 .. n-1 of a call are identical launch sequences (every view update starts from the
// last-axis transform the previous one left and leaves one itself).  Where a sweep is
// launch-bound -- a 64^3 view update is 14 launches of ~6 us kernels -- it can be captured once
// as a graph and replayed.  Measured on MI355X (`tools/graph_probe.py`
// (removed; see git history before this change)): 64^3 0.091 -> 0.081 ms, 128^3 0.132 -> 0.120 ms,
// 256^3 0.308 -> 0.305 ms per view update, against ~11 ms for capture and instantiation, which only
// a long-lived engine (thousands of small view updates) earns back.  Hence opt-in: MVN_GRAPH=1
// enables it, MVN_GRAPH_MAX_MB (default 160) bounds the volume.
// the records of view v's pass in r, and their window: the stacks inside the padded volume, or all of it
MvnStatsParams Engine::params_for(const RecordSet& r, int v) const {
  const Layout& L = plan_->L;
  MvnStatsParams p;
  std::memset(&p, 0, sizeof(p));
  p.d1 = L.d1;
  p.o0 = embedded_ ? host_off_[0] : 0;
  p.o1 = embedded_ ? host_off_[1] : 0;
  p.o2 = embedded_ ? host_off_[2] : 0;
  p.n0 = (unsigned)(embedded_ ? host_dims_[0] : L.d0);
  p.n1 = (unsigned)(embedded_ ? host_dims_[1] : L.d1);
  p.n2 = (unsigned)(embedded_ ? host_dims_[2] : L.d2);
  p.rec = r.rec + 3 * (size_t)r.cap * (size_t)v;
  p.count = r.count + v;
  p.cap = r.cap;
  return p;
}

bool LoopOptions::tv_epsilon_ok(double epsilon) { return epsilon > 0. && std::isfinite(epsilon); }

void LoopOptions::check_tv_lambda(double lambda, const Voice& who) {
  if (!(lambda >= 0. && lambda < 1. / 12.))
    throw std::invalid_argument(std::string(who.prefix) + "total-variation regularisation needs 0 <= " + who.lambda +
                                " < 1/12");
}

void LoopOptions::validate(const Voice& who) const {
  const std::string p = who.prefix;
  // (the first three are arguments of C entry points under either API, and have always been reported in their words)
  if (std::isnan(tolerance)) throw std::invalid_argument("tolerance is NaN");
  if (accel != 0 && accel != 1)
    throw std::invalid_argument("acceleration mode must be 0 (off) or 1 (vector extrapolation)");
  if (likelihood != 0 && likelihood != 1) throw std::invalid_argument("likelihood mode must be 0 (off) or 1 (on)");
  if (reg_kind != 0 && reg_kind != 1)
    throw std::invalid_argument(p + "regularisation kind must be 0 (Tikhonov) or 1 (total variation)");
  if (reg_kind == 1 && !tv_epsilon_ok(epsilon))
    throw std::invalid_argument(p + "total-variation regularisation needs a finite epsilon > 0");
  for (float b : background)
    if (!(b >= 0.f && std::isfinite(b))) throw std::invalid_argument(p + "background values must be finite and >= 0");
}

void LoopOptions::check_call(int V, double lambda, const Voice& who) const {
  if (reg_kind == 1) check_tv_lambda(lambda, who);
  const size_t n = background.size();
  if (n > 1 && n != (size_t)V)
    throw std::invalid_argument(who.prefix + std::to_string(n) + " background values (mvn_set_background) for a call of "
                                + std::to_string(V) + " views");
}

const char* LoopOptions::needs_single_device() const {
  if (stats_on()) return "convergence statistics";
  if (accel_on()) return "acceleration";
  if (reg_kind == 1) return "total variation";
  return noise_model_on() ? "noise model" : nullptr;
}

void LoopOptions::refuse(const char* what) const {
  const struct {
    bool on;
    const char *name, *held, *tail;
  } switches[] = {{noise_model_on(), "noise model", "a noise model (background or likelihood)", " (halo mode)"},
                  {reg_kind == 1, "total-variation regularisation", "total-variation regularisation", " (halo mode)"},
                  {accel_on(), "acceleration", "acceleration", " (halo mode)"},
                  {stats_on(), "convergence statistics", "convergence statistics", ""}};
  for (const auto& s : switches) {
    if (!s.on) continue;
    if (what) throw std::logic_error(std::string("mvn: ") + what + " with " + s.held);
    throw std::logic_error(std::string("mvn: no ") + s.name + " on a slab of a multi-device group" + s.tail);
  }
}

void Engine::set_options(const LoopOptions& o) {
  o.validate(LoopOptions::kEngine);
  if (halo_fn_) o.refuse();
  be::set_device(device_);
  if (o.reg_kind == 0) tv_free();
  held_ = o;
}

void Engine::end_streaming() {
  {
    std::lock_guard<std::mutex> lk(stage_mu_);
    stream_done_ = true;
  }
  stage_cv_.notify_all();
}

void Engine::tv_free() {
  if (!tv_volume()) return;
  be::stream_sync(stream_.get());  // (a pass that reads it may still be in flight)
  // a captured sweep of a TV call holds the volume's address (the pass's store target and the update's operand):
  // it goes with the volume, as in bind_poison, and the key below holds the address as well
  sweep_graph_.reset();
  loop_.release(LoopState::TV, LoopState::TV + 1);
}

// psi = x_k -> psi = y_k (mvn_extrapolate.hpp); a_k stays in ALPHA[k - 1]
void Engine::accel_extrapolate(int k, float min_value) {
  const Layout& L = plan_->L;
  AccelParams p;
  std::memset(&p, 0, sizeof(p));
  p.psi = psi_.get(), p.ysave = loop_.at<float>(LoopState::Y_SAVE), p.g = loop_.at<float>(LoopState::G_PREV);
  p.xprev = loop_.at<float>(LoopState::X_PREV);
  p.n = (long)L.real_floats();
  p.RP = L.RP, p.d2 = L.d2;
  p.first = k == 1;
  p.rec = loop_.at<double>(LoopState::ACCEL_REC);
  float* const alpha = loop_.at<float>(LoopState::ALPHA) + (k - 1);
  p.alpha = alpha;
  p.min_value = min_value;
  be::launch_accel_a(p, stream_.get());
  be::launch_accel_reduce(p.rec, LoopState::accel_records(L), alpha, stream_.get());
  be::launch_accel_b(p, stream_.get());
}

int Engine::iterate(int iterations, double lambda, float min_value, const LoopOptions& o, LoopResult* result) {
  be::set_device(device_);
  const int V = (int)views_.size();
  o.validate(LoopOptions::kEngine);
  o.check_call(V, lambda, LoopOptions::kEngine);
  if (halo_fn_) o.refuse();
  last_ = LoopResult();
  last_.views = V;
  size_t bytes[LoopState::N_BUFFERS];
  LoopState::bytes_of(plan_->L, V, iterations, lambda, o, bytes);
  if (!bytes[LoopState::TV]) tv_free();
  // the record sets and the extrapolation state live for this call: once the passes that use them are done, they go
  struct CallScope {
    Engine& e;
    ~CallScope() {
      bool held = false;
      for (int b = 0; b < LoopState::kKept; ++b) held = held || e.loop_.buf[b].get();
      if (!held) return;
      be::drain_quietly(e.stream_.get());
      e.loop_.release(0, LoopState::kKept);
    }
  } scope{*this};
  loop_.o = o;
  loop_.allocate(bytes);
  last_.ran = iterate_sweeps(iterations, lambda, min_value);
  if (result) *result = last_;
  return last_.ran;
}

int Engine::iterate_sweeps(int iterations, double lambda, float min_value) {
  const LoopOptions& o = loop_.o;
  const double tolerance = o.tolerance;
  const RecordSet st = stat_records(), nm = nm_records();
  const bool accel = accel_running();
  work_has_psi_spectrum_ = false;  // psi may have been replaced since the last call
  pending_rows_ = nullptr;
  psi_spec_valid_ = false;
  decide_layout();
  decide_lines();
  const int V = (int)views_.size();
  static const bool graphs_on = env_int("MVN_GRAPH", 0) != 0 && be::graphs_supported();
  static const size_t graph_max_bytes = (size_t)env_int("MVN_GRAPH_MAX_MB", 160) << 20;
  // (a captured sweep holds buffer addresses: the two work volumes must be back in their roles after it,
  // i.e. the sweep must contain an even number of direct dim0 legs)
  bool use_graph = graphs_on && !halo_fn_ && iterations >= 3 && !prof_.enabled && plan_->can_fuse_rows() &&
                   plan_->main_bytes() <= graph_max_bytes && streamed_order_.empty() && !st.on() && !accel &&
                   !nm.on();  // (a captured sweep would bake in the backgrounds and the records' addresses)
  std::vector<double>& rows = last_.rows;  // {S, M, P} of the sweeps run
  int ran = 0;
  if (accel) be::d2d(loop_.buf[LoopState::Y_SAVE].get(), psi_.get(), plan_->main_bytes(), stream_.get());  // y_0
  for (int it = 0; it < iterations; ++it) {
    if (use_graph && it == 1) {  // every view has been staged by now: its PSF forms are known
      int swaps = 0;
      for (int v = 0; v < V; ++v) swaps += (views_[(size_t)v].tap_k[0] != 0) + (views_[(size_t)v].tap_k[1] != 0);
      use_graph = swaps % 2 == 0;
    }
    if (use_graph && it >= 1 && it < iterations - 1) {
      if (sweep_graph_.get() && (graph_lambda_ != lambda || graph_min_ != min_value ||
                           graph_guard_ != quotient_guard_ || graph_captured_gen_ != graph_gen_ ||
                           graph_reg_kind_ != o.reg_kind || graph_reg_eps_ != o.epsilon ||
                           graph_tv_ != tv_volume() ||
                           graph_work_ != work_)) {
        sweep_graph_.reset();
      }
      if (sweep_graph_.get()) g_u16_divides += u16_views();  // (a replay; the capture below counts through conv_pair)
      if (!sweep_graph_.get()) {
        // all views were used by sweep 0, so none is still being staged
        const float* work_at_capture = work_;
        be::capture_begin(stream_.get());
        try {
          // (a replay reports under the epochs of the capture: the word must not still hold one of them)
          be::dzero(poison_, poison_bytes(), stream_.get());
          for (int v = 0; v < V; ++v) conv_pair(v, views_[(size_t)v].stacks(), lambda, min_value, MVN_EPI_UPDATE, 0, true);
        } catch (...) {
          try {
            be::GraphExec(be::capture_end(stream_.get()));
          } catch (...) {
          }
          throw;
        }
        sweep_graph_.reset(be::capture_end(stream_.get()));
        graph_lambda_ = lambda;
        graph_reg_kind_ = o.reg_kind;
        graph_reg_eps_ = o.epsilon;
        graph_tv_ = tv_volume();
        graph_min_ = min_value;
        graph_guard_ = quotient_guard_;
        graph_captured_gen_ = graph_gen_;
        graph_work_ = work_at_capture;  // (the two work volumes swap roles at every direct leg)
      }
      be::graph_launch(sweep_graph_.get(), stream_.get());
      continue;
    }
    for (int v = 0; v < V; ++v) {
      if (pipelined_ && it == 0) wait_staged(v);  // the uploader thread may still be busy with v
      const bool last = (it == iterations - 1) && (v == V - 1);
      const bool streamed = stream_pos_[(size_t)v] >= 0;
      const ViewStacks in = streamed ? ring_acquire() : views_[(size_t)v].stacks();
      // (acceleration: psi changes between the sweeps, so the last view update leaves no spectrum of it behind
      // and the next sweep starts from rows_r2c of the new psi, as the first sweep of a call does.  Not after
      // sweep 1: y_1 = x_1, psi stays, and so does the fused pass - 2 iterations are the plain loop's launches.
      // The fused pass has written all of psi when pass A reads it: pending_rows_ is only ever set under
      // boundary_first(), which needs a halo hook, and an engine with one refuses acceleration)
      conv_pair(v, in, lambda, min_value, MVN_EPI_UPDATE, 0, !last && !(accel && v == V - 1 && it >= 1));
      if (streamed) ring_release();
    }
    ran = it + 1;
    if (nm.on()) be::launch_nm_reduce(nm.rec, nm.count, V, nm.cap, nm.out + 3 * (size_t)V * (size_t)it, stream_.get());
    if (st.on()) {
      be::launch_convergence_reduce(st.rec, st.count, V, st.cap, st.out + 3 * (size_t)it, stream_.get());
      if (tolerance > 0.) {
        // (no sweep is enqueued ahead: after a stop psi is the estimate of the sweeps run)
        double r[3];
        be::d2h(r, st.out + 3 * (size_t)it, sizeof(r), stream_.get());
        be::stream_sync(stream_.get());
        rows.insert(rows.end(), r, r + 3);
        if (r[0] / r[2] <= tolerance) break;  // (NaN never stops the loop)
      }
    }
    // (no extrapolation after the last sweep run: psi stays x_k)
    if (accel && it < iterations - 1) accel_extrapolate(it + 1, min_value);
  }
  flush_pending_rows();
  work_has_psi_spectrum_ = false;
  if (st.on() && tolerance == 0. && ran > 0) {
    rows.resize(3 * (size_t)ran);
    be::d2h(rows.data(), st.out, rows.size() * sizeof(double), stream_.get());
    be::stream_sync(stream_.get());
  }
  if (nm.on() && ran > 0) {  // {D, Y, M} per (sweep, view) of the sweeps run
    last_.like.resize(3 * (size_t)V * (size_t)ran);
    be::d2h(last_.like.data(), nm.out, last_.like.size() * sizeof(double), stream_.get());
    be::stream_sync(stream_.get());
  }
  if (accel) {  // a_1 .. a_ran; the last sweep run was not followed by an extrapolation
    last_.alphas.assign((size_t)ran, 0.);
    if (ran > 1) {
      std::vector<float> a((size_t)ran - 1);
      be::d2h(a.data(), loop_.buf[LoopState::ALPHA].get(), a.size() * sizeof(float), stream_.get());
      be::stream_sync(stream_.get());
      for (size_t k = 0; k < a.size(); ++k) last_.alphas[k] = (double)a[k];
    }
  }
  return ran;
}

float* Engine::delta_ptr() {
  if (!delta_) {
    be::set_device(device_);
    delta_own_ = be::DeviceBuffer<float>(plan_->main_bytes());
    delta_ = delta_own_.get();
    be::dzero(delta_, plan_->main_bytes(), stream_.get());
  }
  return delta_;
}

// the rows of the own planes start and end on tile boundaries of the last-axis passes
bool Engine::halo_ranged() const {
  if (!halo_fn_ || halo_planes_ < 1) return false;
  if (!plan_->rows_need_full_tiles()) return true;
  const long T = plan_->rows_tile(), d1 = plan_->L.d1;
  return ((long)halo_planes_ * d1) % T == 0 && ((long)(plan_->L.d0 - 2 * halo_planes_) * d1) % T == 0;
}

void Engine::set_halo_planes(int planes, bool split) {
  if (planes < 0 || 2 * planes >= plan_->L.d0) throw std::invalid_argument("mvn: halo planes must leave own planes");
  halo_planes_ = planes;
  halo_split_ = split && planes > 0;
}

void Engine::set_halo_hook(halo_fn_t fn, void* user, bool drain, bool post) {
  if (fn) {
    held_.refuse("no halo hook on an engine");
    // halo mode divides ranges of rows, whose operand offsets are in floats (Plan3D::rows_c2r*)
    if (u16_views() > 0)
      throw std::invalid_argument("mvn: no halo hook on an engine that holds a uint16 image volume (image storage mode 1)");
    if (!plan_->L.even || !mvn_dim0_packed_possible(plan_->L.d0))
      throw std::invalid_argument("mvn: halo mode needs an even last extent and at most 4062 planes per rank");
    packed_allowed_ = true;  // (a hook that also exchanges the Nyquist plane says so: set_halo_nyq_aware)
  }
  halo_nyq_aware_ = false;
  halo_fn_ = fn;
  halo_user_ = user;
  halo_drain_ = drain;
  halo_post_ = post && fn;
  if (!fn) {  // back to the engine's own decisions
    halo_planes_ = 0;
    halo_split_ = false;
    layout_override_ = -1;
    lines_override_ = -1;
    packed_allowed_ = packed_default_;
  }
}

void Engine::copy_planes(void* spectrum, int plane0, int nplanes, void* buffer, bool to_buffer, bool host_buffer,
                         bool wait) {
  be::set_device(device_);
  const Layout& L = plan_->L;
  if (!spectrum || !buffer || plane0 < 0 || nplanes < 1 || plane0 + nplanes > L.d0)
    throw std::invalid_argument("mvn: copy_planes out of range");
  const size_t pb = (size_t)L.d1 * (size_t)L.C * sizeof(cfloat);
  char* p = (char*)spectrum + (size_t)plane0 * pb;
  const size_t n = (size_t)nplanes * pb;
  if (host_buffer) {
    if (to_buffer)
      be::d2h(buffer, p, n, stream_.get());
    else
      be::h2d(p, buffer, n, stream_.get());
  } else if (to_buffer) {
    be::d2d(buffer, p, n, stream_.get());
  } else {
    be::d2d(p, buffer, n, stream_.get());
  }
  if (wait) be::stream_sync(stream_.get());
}

void Engine::bind_delta(float* external) {
  be::set_device(device_);
  be::stream_sync(stream_.get());
  delta_own_.reset();
  delta_ = external;
}

// Simultaneous (Jacobi) step.  psi is not touched while the local views are swept, so its
// forward last-axis and dim1 passes are done ONCE and every view's first convolution starts at
// the (out-of-place) dim0 pass: 7 full passes per view instead of 9.
void Engine::compute_delta(double lambda, float min_value) {
  compute_delta_head(lambda, min_value);
  compute_delta_chunk(0, 1);
}

// planes [z0, z0 + nz) of chunk c of n
void Engine::chunk_planes(int c, int n, int* z0, int* nz) const {
  const int d0 = plan_->L.d0;
  if (n < 1 || n > d0 || c < 0 || c >= n) throw std::out_of_range("mvn: delta chunk index");
  const int a = (int)((long)c * d0 / n), b = (int)((long)(c + 1) * d0 / n);
  *z0 = a;
  *nz = b - a;
}

// the largest chunk count <= wanted whose plane boundaries fall on tile boundaries of the
// last-axis passes (the fixed-length kernels work on whole tiles of T rows)
int Engine::delta_chunks(int wanted) const {
  const Layout& L = plan_->L;
  int n = wanted < 1 ? 1 : (wanted > L.d0 ? L.d0 : wanted);
  if (!plan_->rows_need_full_tiles()) return n;
  const int T = plan_->rows_tile();
  for (; n > 1; --n) {
    bool ok = true;
    for (int c = 1; c < n && ok; ++c) ok = (((long)c * L.d0 / n) * L.d1) % T == 0;
    if (ok) break;
  }
  return n;
}

void Engine::delta_chunk_range(int c, int n, size_t* first_float, size_t* n_floats) const {
  int z0 = 0, nz = 0;
  chunk_planes(c, n, &z0, &nz);
  const size_t plane = (size_t)plan_->L.d1 * (size_t)plan_->L.RP;
  *first_float = (size_t)z0 * plane;
  *n_floats = (size_t)nz * plane;
}

void Engine::compute_delta_head(double lambda, float min_value) {
  held_.refuse("no simultaneous (delta) step on an engine");
  be::set_device(device_);
  delta_ptr();
  tail_pending_ = false;
  tail_prof_ = nullptr;
  work_has_psi_spectrum_ = false;
  const int V = (int)views_.size();
  if (V == 0) return;  // a rank without views contributes a zero correction (compute_delta_chunk)
  {
    const bool was = packed_;
    decide_layout();
    decide_lines();
    // the chunk-fed spectrum of psi is in the other layout
    if (was != packed_ || (psi_spec_valid_ && psi_spec_lines_ != lines_)) psi_spec_valid_ = false;
  }
  const Plan3D& P = *plan_;
  // event pairs around every launch cost ~3 % of a sweep: sample like iterate() does
  const int every = prof_.sample_every > 0 ? prof_.sample_every : 1;
  Profiler* prof = (prof_.enabled && (pair_counter_++ % every) == 0) ? &prof_ : nullptr;
  if (!psi_spec_.get()) {
    psi_spec_ = be::DeviceBuffer<float>(P.main_bytes());
    if (P.nyq_bytes()) psi_spec_nyq_ = be::DeviceBuffer<cfloat>(P.nyq_bytes());
    psi_spec_valid_ = false;
  }
  const bool fuse = P.can_fuse_rows();
  const bool use_side = side_.s.get() && P.L.even && P.main_bytes() > kSideMinBytes && !packed_ && !P.nyq_rides();
  be::stream_t sn = use_side ? side_.s.get() : stream_.get();
  if (!psi_spec_valid_) {  // else: left there chunk by chunk by apply_delta_chunk(.., feed_next)
    if (lines_) {  // line layout: the fused middle pass transforms along dim1 itself
      P.rows_r2c(psi_.get(), (cfloat*)psi_spec_.get(), nullptr, stream_.get(), prof, 0, -1, true);
    } else {
      P.rows_r2c(psi_.get(), (cfloat*)psi_spec_.get(), pn(), stream_.get(), prof);
      if (use_side) side_.fork_from(stream_.get());
      P.axis1(MVN_ST_FWD, (cfloat*)psi_spec_.get(), pn(), stream_.get(), prof, sn);
    }
    psi_spec_lines_ = lines_;
  }
  psi_spec_valid_ = false;  // consumed by this step; psi changes when the correction is applied
  for (int v = 0; v < V; ++v) {
    const ViewSlot& s = views_[(size_t)v];
    if (!s.set) throw std::runtime_error("mvn: view " + std::to_string(v) + " was never set");
    prof = (prof_.enabled && (pair_counter_++ % every) == 0) ? &prof_ : nullptr;
    EpilogueParams e1;
    std::memset(&e1, 0, sizeof(e1));
    e1.scale = 1.f;
    divide_epilogue(e1, s.stacks());
    e1.guard_zero_view = quotient_guard_ ? 1 : 0;
    EpilogueParams e2;
    std::memset(&e2, 0, sizeof(e2));
    e2.mode = MVN_EPI_DELTA;
    e2.scale = 1.f;
    e2.psi = psi_.get();
    e2.weights = s.weights.get();
    e2.delta = delta_;
    e2.accumulate = v == 0 ? 0 : 1;
    e2.lambda = lambda;
    e2.lambda_inv = lambda > 0 ? (float)(1.f / lambda) : 0.f;
    e2.min_value = min_value;
    if (lines_) {
      // line layout: psi's last-axis spectrum -> ONE middle pass -> fused divide -> ONE middle pass -> correction
      if (!s.taps_l_ok[0] || !s.tap_k[0]) throw std::logic_error("mvn: fused middle pass with a kernel that is not in its form");
      if (++epoch_ == 0x7fffffffu) {
        be::dzero(poison_, poison_bytes(), stream_.get());
        epoch_ = 1;
      }
      armed_epoch_ = epoch_;
      P.mid_fused((const cfloat*)psi_spec_.get(), (cfloat*)work_, (const cfloat*)s.taps_l[0].get(), s.tap_k[0], s.tap_kd[0],
                  poison_word(epoch_), epoch_, stream_.get(), prof);
      arm(e1);
      P.rows_c2r_r2c((cfloat*)work_, nullptr, e1, stream_.get(), prof, 0, -1, true);
      mid_fused_conv(s, 1, prof);
      arm(e2);
      if (v + 1 < V) {
        P.rows_c2r((const cfloat*)work_, nullptr, psi_.get(), e2, stream_.get(), prof, 0, -1, true);
      } else {
        tail_epi_ = e2;
        tail_prof_ = prof;
        tail_pending_ = true;
      }
      continue;
    }
    // convolution 1 from the shared spectrum of psi; the Nyquist-plane launches ride on the side
    // stream (forked per view: the previous view's last pass still reads work_nyq_, and the
    // chunk-fed spectrum of psi was written on the main stream)
    if (s.tap_k[0]) {
      // (the shared spectrum of psi may still be in the making on the side stream: v == 0)
      if (use_side && v == 0) side_.join_into(stream_.get());
      dim0_conv(s, 0, (const cfloat*)psi_spec_.get(), pn(), (cfloat*)work_, wn(), prof);
      if (use_side) side_.fork_from(stream_.get());
    } else {
      if (use_side) side_.fork_from(stream_.get());
      P.axis0(MVN_ST_FWD_MUL_INV, (cfloat*)work_, wn(), (const cfloat*)s.spec[0].get(), s.nyq[0].get(), stream_.get(), prof, sn,
              (const cfloat*)psi_spec_.get(), pn(), spec_tiled_);
    }
    P.axis1(MVN_ST_INV, (cfloat*)work_, wn(), stream_.get(), prof, sn);
    if (use_side) side_.join_into(stream_.get());
    arm(e1);
    if (fuse) {
      P.rows_c2r_r2c((cfloat*)work_, wn(), e1, stream_.get(), prof);
    } else {
      P.rows_c2r((const cfloat*)work_, wn(), work_, e1, stream_.get(), prof);
      P.rows_r2c(work_, (cfloat*)work_, wn(), stream_.get(), prof);
    }
    middle(s, 1, prof, use_side ? &side_ : nullptr);
    arm(e2);
    if (v + 1 < V) {
      P.rows_c2r((const cfloat*)work_, wn(), psi_.get(), e2, stream_.get(), prof);
    } else {  // the last view's final pass is launched chunk by chunk (compute_delta_chunk)
      tail_epi_ = e2;
      tail_prof_ = prof;
      tail_pending_ = true;
    }
  }
}

void Engine::compute_delta_chunk(int c, int n) {
  be::set_device(device_);
  int z0 = 0, nz = 0;
  chunk_planes(c, n, &z0, &nz);
  const Layout& L = plan_->L;
  if (views_.empty()) {
    size_t off = 0, cnt = 0;
    delta_chunk_range(c, n, &off, &cnt);
    be::dzero(delta_ptr() + off, cnt * sizeof(float), stream_.get());
    return;
  }
  if (!tail_pending_) throw std::logic_error("mvn: compute_delta_chunk without compute_delta_head");
  plan_->rows_c2r((const cfloat*)work_, lines_ ? nullptr : wn(), psi_.get(), tail_epi_, stream_.get(), c == 0 ? tail_prof_ : nullptr,
                  (long)z0 * L.d1, (long)nz * L.d1, lines_);
  if (c == n - 1) tail_pending_ = false;
}

void Engine::apply_delta_chunk(int c, int n, bool feed_next) {
  be::set_device(device_);
  int z0 = 0, nz = 0;
  chunk_planes(c, n, &z0, &nz);
  size_t off = 0, cnt = 0;
  delta_chunk_range(c, n, &off, &cnt);
  const Plan3D& P = *plan_;
  work_has_psi_spectrum_ = false;
  psi_spec_valid_ = false;
  if (fed_n_ != n) {  // a new round of chunks (any order within a round)
    fed_n_ = n;
    fed_ = 0;
  }
  be::launch_axpy1(psi_.get() + off, delta_ptr() + off, cnt, stream_.get());
  if (feed_next && !views_.empty()) {
    if (!psi_spec_.get()) {
      psi_spec_ = be::DeviceBuffer<float>(P.main_bytes());
      if (P.nyq_bytes()) psi_spec_nyq_ = be::DeviceBuffer<cfloat>(P.nyq_bytes());
    }
    if (lines_) {  // (the layout of the step this correction belongs to; the next head checks it against its own)
      P.rows_r2c(psi_.get(), (cfloat*)psi_spec_.get(), nullptr, stream_.get(), nullptr, (long)z0 * P.L.d1, (long)nz * P.L.d1, true);
    } else {
      P.rows_r2c(psi_.get(), (cfloat*)psi_spec_.get(), pn(), stream_.get(), nullptr, (long)z0 * P.L.d1,
                 (long)nz * P.L.d1);
      P.axis1(MVN_ST_FWD, (cfloat*)psi_spec_.get(), pn(), stream_.get(), nullptr, stream_.get(), z0, nz);
    }
    psi_spec_lines_ = lines_;
    if (++fed_ == n) {  // every plane of the spectrum belongs to the new psi
      psi_spec_valid_ = true;
      fed_ = 0;
    }
  } else {
    fed_ = 0;
  }
}

void Engine::apply_delta() {
  be::set_device(device_);
  psi_spec_valid_ = false;
  be::launch_axpy1(psi_.get(), delta_ptr(), plan_->L.real_floats(), stream_.get());
}

void Engine::sync() {
  be::set_device(device_);
  be::stream_sync(stream_.get());
  prof_.collect();
}

// ---------------------------------------------------------------------------------------------
// SlabEngine
// ---------------------------------------------------------------------------------------------
SlabEngine::SlabEngine(int device, const shape_t& dims, int nranks, int rank, int num_views)
    : device_(device), P_(nranks), rank_(rank), dims_(dims) {
  if (num_views < 1) throw std::invalid_argument("mvn: num_views must be >= 1");
  if (nranks < 1 || rank < 0 || rank >= nranks) throw std::invalid_argument("mvn: bad rank / nranks");
  if (dims[0] % nranks || dims[1] % nranks || dims[0] / nranks < 2 || dims[1] / nranks < 2)
    throw std::invalid_argument("mvn: slab mode needs d0 and d1 divisible by the rank count, "
                                "with at least two planes / rows per rank");
  be::set_device(device_);
  shape_t a = {{dims[0] / nranks, dims[1], dims[2]}};
  shape_t b = {{dims[0], dims[1] / nranks, dims[2]}};
  planA_ = PlanStore::get().add(device_, a);
  planB_ = PlanStore::get().add(device_, b);
  stream_ = be::Stream::create();
  const size_t mb = planA_->main_bytes(), nb = planA_->nyq_bytes();
  psi_ = be::DeviceBuffer<float>(mb);
  work_ = be::DeviceBuffer<float>(mb);
  own_a_ = be::DeviceBuffer<float>(mb);
  own_b_ = be::DeviceBuffer<float>(mb);
  be::dzero(psi_.get(), mb, stream_.get());
  be::dzero(work_.get(), mb, stream_.get());
  if (nb) {
    work_nyq_ = be::DeviceBuffer<cfloat>(nb);
    own_an_ = be::DeviceBuffer<cfloat>(nb);
    own_bn_ = be::DeviceBuffer<cfloat>(nb);
  }
  a_main_ = own_a_.get();
  b_main_ = own_b_.get();
  a_nyq_ = own_an_.get();
  b_nyq_ = own_bn_.get();
  views_.resize((size_t)num_views);
  be::stream_sync(stream_.get());
}

SlabEngine::~SlabEngine() {
  try {
    be::set_device(device_);
    if (stream_.get()) be::stream_sync(stream_.get());
  } catch (...) {
  }
}

void SlabEngine::sync() {
  be::set_device(device_);
  be::stream_sync(stream_.get());
}

void SlabEngine::bind_buffers(float* a_main, float* b_main, float* a_nyq, float* b_nyq) {
  sync();
  const bool need_nyq = planA_->nyq_bytes() != 0;
  const bool any = a_main || b_main || a_nyq || b_nyq;
  const bool all = a_main && b_main && (!need_nyq || (a_nyq && b_nyq));
  if (any && !all)
    throw std::invalid_argument("mvn: bind all exchange buffers (main and, for even d2, Nyquist) or none");
  if (all) {
    a_main_ = a_main;
    b_main_ = b_main;
    a_nyq_ = (cfloat*)a_nyq;
    b_nyq_ = (cfloat*)b_nyq;
  } else {
    a_main_ = own_a_.get();
    b_main_ = own_b_.get();
    a_nyq_ = own_an_.get();
    b_nyq_ = own_bn_.get();
  }
}

void SlabEngine::upload_slab(float* dst, const float* host) {
  const Layout& L = planA_->L;
  if (L.RP == L.d2)
    be::h2d(dst, host, L.logical() * sizeof(float), stream_.get());
  else
    be::h2d_2d(dst, (size_t)L.RP * sizeof(float), host, (size_t)L.d2 * sizeof(float),
               (size_t)L.d2 * sizeof(float), L.rows, stream_.get());
}

void SlabEngine::set_psi(const float* host) {
  be::set_device(device_);
  if (planA_->L.RP != planA_->L.d2) be::dzero(psi_.get(), planA_->main_bytes(), stream_.get());
  upload_slab(psi_.get(), host);
  be::stream_sync(stream_.get());
  work_has_psi_spectrum_ = false;
}

void SlabEngine::get_psi(float* host) {
  be::set_device(device_);
  const Layout& L = planA_->L;
  be::d2h_2d(host, (size_t)L.d2 * 4, psi_.get(), (size_t)L.RP * 4, (size_t)L.d2 * 4, L.rows, stream_.get());
  be::stream_sync(stream_.get());
}

void SlabEngine::set_view(int v, const float* image, const float* weights, const float* kernel1,
                          const int* k1dims, const float* kernel2, const int* k2dims) {
  if (v < 0 || v >= (int)views_.size()) throw std::out_of_range("mvn: view index");
  be::set_device(device_);
  SlabView& s = views_[(size_t)v];
  const size_t mb = planA_->main_bytes();
  const size_t nbT = planB_->nyq_bytes();
  if (!s.image.get()) {
    s.image = be::DeviceBuffer<float>(mb);
    s.weights = be::DeviceBuffer<float>(mb);
    for (int i = 0; i < 2; ++i) {
      s.spec[i] = be::DeviceBuffer<float>(planB_->main_bytes());
      if (nbT) s.nyq[i] = be::DeviceBuffer<cfloat>(nbT);
    }
    if (planA_->L.RP != planA_->L.d2) {
      be::dzero(s.image.get(), mb, stream_.get());
      be::dzero(s.weights.get(), mb, stream_.get());
    }
  }
  upload_slab(s.image.get(), image);
  upload_slab(s.weights.get(), weights);
  // PSF spectra: the whole 3-D spectrum is formed locally (three passes on a temporary full
  // volume) and this rank's dim1 block cut out of it -- position order along dim1 is the same in
  // the full and in the decomposed transform, so the block is what a decomposed forward
  // transform of the PSF would leave here.
  std::shared_ptr<Plan3D> full = PlanStore::get().add(device_, dims_);
  const Layout& F = full->L;
  const float scale = (float)(1.0 / (double)F.logical());
  be::DeviceBuffer<float> fspec(full->main_bytes()), dk;
  be::DeviceBuffer<cfloat> fnyq;
  try {
    if (full->nyq_bytes()) fnyq = be::DeviceBuffer<cfloat>(full->nyq_bytes());
    const float* ks[2] = {kernel1, kernel2};
    const int* kd[2] = {k1dims, k2dims};
    const size_t yb = (size_t)(F.d1 / P_);
    for (int i = 0; i < 2; ++i) {
      const size_t kb = sizeof(float) * (size_t)kd[i][0] * (size_t)kd[i][1] * (size_t)kd[i][2];
      dk = be::DeviceBuffer<float>(kb);
      be::h2d(dk.get(), ks[i], kb, stream_.get());
      full->psf_spectrum(dk.get(), kd[i], scale, fspec.get(), fnyq.get(), stream_.get());
      const size_t wrow = yb * (size_t)F.C * sizeof(cfloat);
      be::d2d_2d(s.spec[i].get(), wrow, (const cfloat*)fspec.get() + (size_t)rank_ * yb * F.C,
                 (size_t)F.d1 * F.C * sizeof(cfloat), wrow, (size_t)F.d0, stream_.get());
      if (fnyq.get())
        be::d2d_2d(s.nyq[i].get(), yb * sizeof(cfloat), fnyq.get() + (size_t)rank_ * yb,
                   (size_t)F.d1 * sizeof(cfloat), yb * sizeof(cfloat), (size_t)F.d0, stream_.get());
      be::stream_sync(stream_.get());
      dk.reset();
    }
  } catch (...) {
    be::drain_quietly(stream_.get());  // the engine's stream outlives the three temporaries
    throw;
  }
  s.set = true;
}

void SlabEngine::begin_sweeps() { work_has_psi_spectrum_ = false; }

// conv 0 starts from psi (its last-axis transform may already sit in the work buffer, left there
// by the previous view's fused update pass); conv 1 starts from the quotient's last-axis
// transform, left there by step_unpack(conv 0)
void SlabEngine::step_pack(int v, int conv) {
  be::set_device(device_);
  if (!views_.at((size_t)v).set) throw std::runtime_error("mvn: view " + std::to_string(v) + " was never set");
  const Plan3D& A = *planA_;
  const Layout& L = A.L;
  cfloat* W = (cfloat*)work_.get();
  if (conv == 0) {
    if (!work_has_psi_spectrum_) A.rows_r2c(psi_.get(), W, work_nyq_.get(), stream_.get());
    work_has_psi_spectrum_ = false;
  }
  A.axis1(MVN_ST_FWD, W, work_nyq_.get(), stream_.get());
  const size_t yb = (size_t)(L.d1 / P_);
  const size_t wrow = yb * (size_t)L.C * sizeof(cfloat);
  const size_t blk = (size_t)L.d0 * yb * L.C;  // cfloats per destination rank
  for (int j = 0; j < P_; ++j) {
    be::d2d_2d((cfloat*)a_main_ + (size_t)j * blk, wrow, W + (size_t)j * yb * L.C,
               (size_t)L.d1 * L.C * sizeof(cfloat), wrow, (size_t)L.d0, stream_.get());
    if (work_nyq_.get())
      be::d2d_2d(a_nyq_ + (size_t)j * L.d0 * yb, yb * sizeof(cfloat), work_nyq_.get() + (size_t)j * yb,
                 (size_t)L.d1 * sizeof(cfloat), yb * sizeof(cfloat), (size_t)L.d0, stream_.get());
  }
}

void SlabEngine::step_mid(int v, int conv) {
  be::set_device(device_);
  const SlabView& s = views_.at((size_t)v);
  planB_->axis0(MVN_ST_FWD_MUL_INV, (cfloat*)b_main_, b_nyq_, (const cfloat*)s.spec[conv].get(),
                s.nyq[conv].get(), stream_.get());
}

void SlabEngine::step_unpack(int v, int conv, double lambda, float min_value, bool feed_next) {
  be::set_device(device_);
  const SlabView& s = views_.at((size_t)v);
  const Plan3D& A = *planA_;
  const Layout& L = A.L;
  cfloat* W = (cfloat*)work_.get();
  const size_t yb = (size_t)(L.d1 / P_);
  const size_t wrow = yb * (size_t)L.C * sizeof(cfloat);
  const size_t blk = (size_t)L.d0 * yb * L.C;
  for (int j = 0; j < P_; ++j) {
    be::d2d_2d(W + (size_t)j * yb * L.C, (size_t)L.d1 * L.C * sizeof(cfloat),
               (const cfloat*)a_main_ + (size_t)j * blk, wrow, wrow, (size_t)L.d0, stream_.get());
    if (work_nyq_.get())
      be::d2d_2d(work_nyq_.get() + (size_t)j * yb, (size_t)L.d1 * sizeof(cfloat),
                 a_nyq_ + (size_t)j * L.d0 * yb, yb * sizeof(cfloat), yb * sizeof(cfloat),
                 (size_t)L.d0, stream_.get());
  }
  A.axis1(MVN_ST_INV, W, work_nyq_.get(), stream_.get());
  EpilogueParams e;
  std::memset(&e, 0, sizeof(e));
  e.scale = 1.f;  // 1/N lives in the PSF spectra
  if (conv == 0) {
    e.mode = MVN_EPI_DIVIDE;
    e.view = s.image.get();
    if (A.can_fuse_rows()) {
      A.rows_c2r_r2c(W, work_nyq_.get(), e, stream_.get());
    } else {
      A.rows_c2r(W, work_nyq_.get(), work_.get(), e, stream_.get());
      A.rows_r2c(work_.get(), W, work_nyq_.get(), stream_.get());
    }
  } else {
    e.mode = MVN_EPI_UPDATE;
    e.psi = psi_.get();
    e.weights = s.weights.get();
    e.lambda = lambda;
    e.lambda_inv = lambda > 0 ? (float)(1.f / lambda) : 0.f;
    e.min_value = min_value;
    if (A.can_fuse_rows() && feed_next) {
      A.rows_c2r_r2c(W, work_nyq_.get(), e, stream_.get());
      work_has_psi_spectrum_ = true;
    } else {
      A.rows_c2r(W, work_nyq_.get(), psi_.get(), e, stream_.get());
    }
  }
}

}  // namespace mvn
