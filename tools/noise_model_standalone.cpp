// Stand-alone check of the noise-model divide epilogues of the host emulation (MVN_EPI_DIVIDE_NM,
// MVN_EPI_DIVIDE_NM_U16; csrc/mvn_pass_bodies.hpp, mvn_wave_rows.hpp) and of the reduce that follows them: the
// last-axis pass bodies, plain and fused, float32 and uint16 views, with and without a background and the quotient
// guard, on (3, 5, 2), (10, 14, 45) with a window strictly inside the volume, and (6, 8, 512) - the run-time-radix
// bodies of an even and an odd extent and the wave-row body - against a plain triple loop.  The bodies are run the
// way mvn_backend_emu.cpp runs them, on tables built here from mvn_plan.hpp.  Built with
// -fsanitize=address,undefined by tests/test_noise_model_standalone.py; exits non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc> \
//       noise_model_standalone.cpp -o noise_model_standalone
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "mvn_plan.hpp"
#include "mvn_wave_rows.hpp"

using namespace mvn;

// the last-axis passes of one shape: the tables a plan holds and the launches of the emulation, one workgroup after
// the other.  d2 = 512 runs the wave-row bodies (whole row pairs per half-wave), every other extent the
// run-time-radix bodies on tiles of 4 rows.
struct HostRows {
  Layout L;
  bool wave;
  AxisPlanHost host;
  std::vector<cfloat> roots;
  unsigned zero = 0;
  static constexpr int T = 4;
  HostRows(int d0, int d1, int d2) : L(d0, d1, d2), wave(d2 == 512 && L.rows % 2 == 0), host(L.h, wave) {
    roots.resize((size_t)L.h / 2 + 1);
    for (size_t k = 0; k < roots.size(); ++k) {
      const double a = -2.0 * M_PI * (double)k / (double)d2;
      roots[k] = cmake((float)std::cos(a), (float)std::sin(a));
    }
  }
  long lds_cfloats() const {
    const long n = host.nfft, TP = T | 1;
    return wave ? (long)WrCfg::lds_cfloats : n * TP * (host.generic ? 2 : 1) + n + 8;
  }
  RowsParams params(const EpilogueParams& e, const MvnStatsParams* st) const {
    RowsParams p;
    std::memset(&p, 0, sizeof(p));
    p.ax = host.view(host.tw.data(), host.rev.data(), host.inv.data(), host.tws.data());
    p.twr = roots.data();
    p.d2 = L.d2, p.h = L.h, p.C = L.C, p.RP = L.RP;
    p.rows = (long)L.rows;
    p.T = T, p.TP = T | 1;
    p.lds_alt = host.generic ? (long)host.nfft * p.TP : 0;
    p.lds_tw = (long)host.nfft * p.TP * (host.generic ? 2 : 1);
    p.hmul = mvn_fastdiv_mul((unsigned)L.h);
    p.Cmul = mvn_fastdiv_mul((unsigned)L.C);
    p.fixed = wave ? 1 : 0;
    p.epi = e;
    p.epi.poison = &zero, p.epi.poison_epoch = 0xffffffffu;  // (no direct dim0 leg came before)
    if (st) p.st = *st;
    return p;
  }
  template <int MODE, int EPI>
  void wave_run(const RowsParams& p) const {
    typedef FxCtx<WrRegs, WrCfg::NT> Ctx;
    const long pairs = (p.rows + 1) / 2;
    const long full = (pairs + WrCfg::WAVES - 1) / WrCfg::WAVES;
    const long grid = full > 2 ? (full + 2) / 3 : full;  // (fewer workgroups than row groups: the sweep loop runs)
    std::vector<cfloat> lds((size_t)lds_cfloats());  // exactly sized: the statistics scratch must fit
    std::unique_ptr<Ctx> ctx(new Ctx());
    for (long b = 0; b < grid; ++b) wr_rows_body<MODE, EPI>(p, b, grid, lds.data(), *ctx);
  }
  void rows_r2c(const float* in, cfloat* out, cfloat* out_nyq) const {
    RowsParams p = params(EpilogueParams(), nullptr);
    p.in_real = in, p.out_cplx = out, p.out_nyq = out_nyq;
    if (wave) return wave_run<MVN_WR_R2C, MVN_EPI_STORE>(p);
    std::vector<cfloat> lds((size_t)lds_cfloats());
    for (long t = 0; t < (p.rows + T - 1) / T; ++t) {
      if (L.even)
        rows_r2c_even_body<T>(p, t, 0, 1, lds.data());
      else
        rows_r2c_odd_body<T>(p, t, 0, 1, lds.data());
    }
  }
  // KEEP: the fused pass, in place on (data, nyq); else the real rows go to out_real
  template <bool U16, bool NM, bool KEEP>
  void rows_c2r(cfloat* data, cfloat* nyq, float* out_real, const EpilogueParams& e, const MvnStatsParams* st) const {
    RowsParams p = params(e, st);
    p.in_cplx = data, p.in_nyq = nyq, p.out_real = out_real;
    if (KEEP) p.out_cplx = data, p.out_nyq = nyq;
    constexpr int EPI = NM ? (U16 ? MVN_EPI_DIVIDE_NM_U16 : MVN_EPI_DIVIDE_NM) : MVN_EPI_STORE;
    if (wave) return wave_run<KEEP ? MVN_WR_C2R_R2C : MVN_WR_C2R, EPI>(p);
    constexpr int FORM = NM ? EPI : U16 ? (int)MVN_EPI_DIVIDE_U16 : (int)MVN_EPI_STORE;  // (of the run-time-radix bodies)
    std::vector<cfloat> lds((size_t)lds_cfloats());
    for (long t = 0; t < (p.rows + T - 1) / T; ++t) {
      if (L.even)
        rows_c2r_even_body<T, KEEP, FORM>(p, t, 0, 1, lds.data());
      else
        rows_c2r_odd_body<T, FORM>(p, t, 0, 1, lds.data());
    }
  }
};

static bool close_enough(double got, double want) {
  // (the lanes and workgroups sum in another order than the loop: doubles, a few thousand terms)
  return std::fabs(got - want) <= 1e-12 * std::fabs(want) || (got != got && want != want);
}

static int check(int d0, int d1, int d2, const int* off, const int* ext, float background, int guard) {
  HostRows P(d0, d1, d2);
  const Layout& L = P.L;
  const long rows = (long)L.rows, RP = L.RP, n = rows * RP;
  std::mt19937 rng(5u + (unsigned)d2);
  std::uniform_real_distribution<float> dist(20.f, 200.f);
  // exactly-sized allocations: the sanitizer sees every access past a volume
  std::vector<float> x(n, 0.f), xs(n, -77.f), q(n, -77.f), view(n, 0.f);
  std::vector<uint16_t> view16(n, 0);
  for (long r = 0; r < rows; ++r)
    for (int c = 0; c < d2; ++c) {
      x[r * RP + c] = dist(rng);
      const uint16_t y = (uint16_t)((r * 7 + c) % 5 == 0 ? 0 : (int)dist(rng));  // (zeros: the guard, and term = m - y)
      view16[r * RP + c] = y;
      view[r * RP + c] = (float)y;
    }
  std::vector<cfloat> spec(rows * L.C), nyq(L.nyq_cplx());
  cfloat* nq = L.even ? nyq.data() : nullptr;
  P.rows_r2c(x.data(), spec.data(), nq);
  const float scale = 1.f / (float)d2;
  EpilogueParams e;
  std::memset(&e, 0, sizeof(e));
  e.mode = MVN_EPI_STORE, e.scale = scale;
  P.rows_c2r<false, false, false>(spec.data(), nq, xs.data(), e, nullptr);  // x * scale as every epilogue sees it, bit for bit
  // the plain triple loop
  std::vector<float> want_q(n, -77.f);
  double D = 0., Y = 0., M = 0.;
  for (int z = 0; z < d0; ++z)
    for (int y = 0; y < d1; ++y)
      for (int c = 0; c < d2; ++c) {
        const long i = ((long)z * d1 + y) * RP + c;
        const float v = view[i];
        const float m = background != 0.f ? xs[i] + background : xs[i];
        const float t = 1.0f / m;
        const float qq = (guard && v == 0.f) ? 0.f : v * t;
        want_q[i] = qq;
        const float term = v > 0.f ? (v * logf(qq) - v) + m : m - v;
        if (z >= off[0] && z < off[0] + ext[0] && y >= off[1] && y < off[1] + ext[1] && c >= off[2] && c < off[2] + ext[2])
          D += (double)term, Y += (double)v, M += (double)m;
      }
  int bad = 0;
  const long cap = rows;
  std::vector<double> rec(3 * cap, -1.), out(3, -1.);
  unsigned count = 0;
  MvnStatsParams st;
  std::memset(&st, 0, sizeof(st));
  st.d1 = d1;
  st.o0 = off[0], st.o1 = off[1], st.o2 = off[2];
  st.n0 = (unsigned)ext[0], st.n1 = (unsigned)ext[1], st.n2 = (unsigned)ext[2];
  st.rec = rec.data(), st.count = &count, st.cap = cap;
  for (int u16 = 0; u16 < 2; ++u16)
    for (int fused = 0; fused < (L.even ? 2 : 1); ++fused) {
      e.mode = u16 ? MVN_EPI_DIVIDE_NM_U16 : MVN_EPI_DIVIDE_NM;
      if (u16)
        e.view16 = view16.data();
      else
        e.view = view.data();
      e.background = background;
      e.guard_zero_view = guard;
      std::fill(q.begin(), q.end(), -77.f);
      std::fill(rec.begin(), rec.end(), -1.);
      count = 0;
      if (fused) {
        std::vector<cfloat> s2 = spec, n2 = nyq;
        if (u16)
          P.rows_c2r<true, true, true>(s2.data(), n2.data(), nullptr, e, &st);
        else
          P.rows_c2r<false, true, true>(s2.data(), n2.data(), nullptr, e, &st);
      } else {
        if (u16)
          P.rows_c2r<true, true, false>(spec.data(), nq, q.data(), e, &st);
        else
          P.rows_c2r<false, true, false>(spec.data(), nq, q.data(), e, &st);
        for (long r = 0; r < rows; ++r) {
          for (int c = 0; c < d2; ++c)
            if (std::memcmp(&q[r * RP + c], &want_q[r * RP + c], sizeof(float)) != 0) ++bad;
          for (long c = d2; c < RP; ++c)
            if (q[r * RP + c] != -77.f) ++bad;  // the row padding is not written
        }
      }
      if (count < 1 || (long)count > cap) ++bad;
      double lds3[3];
      mvn_nm_reduce_body(rec.data(), &count, cap, out.data(), lds3, 0, 1);
      if (!close_enough(out[0], D) || out[1] != Y || !close_enough(out[2], M)) {
        ++bad;
        std::printf("  u16 %d fused %d: {%.17g, %.17g, %.17g} want {%.17g, %.17g, %.17g}\n", u16, fused, out[0], out[1],
                    out[2], D, Y, M);
      }
    }
  std::printf("(%d, %d, %d) window (%d, %d, %d) + (%d, %d, %d), b %g, guard %d: wave rows %d, %d mismatches\n", d0,
              d1, d2, off[0], off[1], off[2], ext[0], ext[1], ext[2], (double)background, guard, (int)P.wave, bad);
  return bad;
}

int main() {
  int bad = 0;
  {
    const int off[3] = {0, 0, 0}, ext[3] = {3, 5, 2};
    bad += check(3, 5, 2, off, ext, 100.f, 0);
    bad += check(3, 5, 2, off, ext, 0.f, 1);
  }
  {
    const int off[3] = {2, 2, 3}, ext[3] = {6, 10, 39};  // strictly inside
    bad += check(10, 14, 45, off, ext, 100.f, 1);
    bad += check(10, 14, 45, off, ext, 37.5f, 0);
  }
  {
    const int off[3] = {0, 0, 0}, ext[3] = {6, 8, 512};
    const int off2[3] = {1, 2, 5}, ext2[3] = {4, 5, 500};
    bad += check(6, 8, 512, off, ext, 100.f, 0);
    bad += check(6, 8, 512, off2, ext2, 100.f, 1);
  }
  std::printf(bad ? "MISMATCH\n" : "ok\n");
  return bad ? 1 : 0;
}
