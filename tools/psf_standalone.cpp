// Stand-alone check of the passes behind mvn_derive_kernels on the host emulation (csrc/mvn_psf.hpp, the launches
// mvn_backend_emu.cpp makes): the correlation, the two steps of the normalisation and the pointwise pass on small
// kernels - (1, 3, 5), and (33, 7, 11) with its autocorrelation of (65, 13, 21), whose rows cross a wave - against a
// plain loop over the definition in include/mvn_engine_api.h.  Every buffer is allocated at exactly its size: the
// sanitizer sees an access past it.  Built with -fsanitize=address,undefined by tests/test_psf_standalone.py; exits
// non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc> \
//       psf_standalone.cpp -o psf_standalone
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mvn_psf.hpp"

typedef std::vector<float> Arr;

static long count(const int* e) { return (long)e[0] * e[1] * e[2]; }

static Arr random_kernel(const int* e, unsigned seed, bool zeros) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> dist(0.f, 1.f);
  Arr a((size_t)count(e));
  for (float& x : a) {
    const float u = dist(rng);
    x = (u * u) * (u * u) * (u * u);
    if (zeros && dist(rng) < 0.3f) x = 0.f;
  }
  return a;
}

// value of an array of extents e at offset d from its centre; outside: not a term
static bool at(const Arr& a, const int* e, int d0, int d1, int d2, float* v) {
  const int i0 = d0 + e[0] / 2, i1 = d1 + e[1] / 2, i2 = d2 + e[2] / 2;
  if (i0 < 0 || i0 >= e[0] || i1 < 0 || i1 >= e[1] || i2 < 0 || i2 >= e[2]) return false;
  *v = a[((size_t)i0 * e[1] + i1) * e[2] + i2];
  return true;
}

// corr(a, b)(d) = sum over t of a(-t) b(d - t), t in raster order, in double from +0.0
static Arr corr_plain(const Arr& a, const int* ea, const Arr& b, const int* eb, const int* eo) {
  Arr out((size_t)count(eo));
  size_t i = 0;
  for (int d0 = -(eo[0] / 2); d0 <= eo[0] / 2; ++d0)
    for (int d1 = -(eo[1] / 2); d1 <= eo[1] / 2; ++d1)
      for (int d2 = -(eo[2] / 2); d2 <= eo[2] / 2; ++d2) {
        double s = 0.0;
        for (int t0 = -(ea[0] / 2); t0 <= ea[0] / 2; ++t0)
          for (int t1 = -(ea[1] / 2); t1 <= ea[1] / 2; ++t1)
            for (int t2 = -(ea[2] / 2); t2 <= ea[2] / 2; ++t2) {
              float av = 0.f, bv = 0.f;
              at(a, ea, -t0, -t1, -t2, &av);
              if (!at(b, eb, d0 - t0, d1 - t1, d2 - t2, &bv)) continue;
              s = s + (double)av * (double)bv;
            }
        out[i++] = (float)s;
      }
  return out;
}

static int differing(const Arr& got, const Arr& want) {
  int bad = 0;
  for (size_t i = 0; i < want.size(); ++i) bad += std::memcmp(&got[i], &want[i], sizeof(float)) != 0;
  return bad;
}

// one stage of correlations through the launch's own loop
static void run_correlate(const std::vector<PsfJob>& jobs) {
  for (const PsfJob& j : jobs) mvn_psf_job_check(j);
  PsfCorrParams p;
  p.jobs = jobs.data(), p.njobs = (int)jobs.size();
  p.blocks_per_job = (int)mvn_psf_blocks(count(jobs[0].eo));
  mvn_psf_corr_check(p);
  const long nblocks = (long)p.njobs * p.blocks_per_job;
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_correlate_item(p, blk, t);
}

static PsfJob job(const Arr& a, const int* ea, const Arr& b, const int* eb, Arr& out, const int* eo) {
  PsfJob j;
  std::memset(&j, 0, sizeof(j));
  j.a = a.data(), j.b = b.data(), j.out = out.data();
  for (int k = 0; k < 3; ++k) j.ea[k] = ea[k], j.eb[k] = eb[k], j.eo[k] = eo[k];
  return j;
}

static int check(const int* K, int V, bool zeros) {
  const int K2[3] = {2 * K[0] - 1, 2 * K[1] - 1, 2 * K[2] - 1};
  const long n = count(K), nA = count(K2);
  int bad = 0;
  // normalisation: V arrays one behind the other, in place
  Arr P((size_t)(V * n));
  for (int v = 0; v < V; ++v) {
    const Arr r = random_kernel(K, 11u + (unsigned)v + (unsigned)n, zeros);
    std::copy(r.begin(), r.end(), P.begin() + v * n);
  }
  const Arr q = P;
  std::vector<double> partial((size_t)V * MVN_PSF_WG), sums((size_t)V);
  PsfNormParams nm;
  nm.src = P.data(), nm.dst = P.data(), nm.partial = partial.data(), nm.sums = sums.data(), nm.n = n, nm.count = V;
  mvn_psf_norm_check(nm);
  for (long blk = 0; blk < V; ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_sum_item(nm, blk, t);
  for (long blk = 0; blk < V * mvn_psf_blocks(n); ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_scale_item(nm, blk, t);
  for (int v = 0; v < V; ++v) {
    double S = 0.0;
    for (long i = 0; i < n; ++i) S += (double)q[(size_t)(v * n + i)];
    if (std::fabs(sums[(size_t)v] - S) > 1e-11 * S) ++bad;
    for (long i = 0; i < n; ++i) {  // (the sum's order is free: a quotient may sit on the other side of a tie)
      const float want = (float)((double)q[(size_t)(v * n + i)] / S), got = P[(size_t)(v * n + i)];
      if (got != want && got != std::nextafterf(want, 0.f) && got != std::nextafterf(want, 2.f)) ++bad;
    }
  }
  // pointwise: the flipped kernels, bit for bit
  Arr T((size_t)(V * n));
  PsfPointParams pt;
  pt.P = P.data(), pt.C = nullptr, pt.T = T.data(), pt.n = n, pt.V = V, pt.type = PSF_INDEPENDENT;
  mvn_psf_point_check(pt);
  for (long blk = 0; blk < V * mvn_psf_blocks(n); ++blk)
    for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_pointwise_item(pt, blk, t);
  for (int v = 0; v < V; ++v)
    for (long i = 0; i < n; ++i) bad += T[(size_t)(v * n + i)] != P[(size_t)(v * n + n - 1 - i)];
  // the two stages of the efficient Bayesian type, and the plain products behind them
  std::vector<Arr> Pv, Fv, A((size_t)V, Arr((size_t)nA)), C;
  for (int v = 0; v < V; ++v) {
    Pv.emplace_back(P.begin() + v * n, P.begin() + (v + 1) * n);
    Fv.emplace_back(T.begin() + v * n, T.begin() + (v + 1) * n);
  }
  std::vector<PsfJob> ja, jc;
  for (int w = 0; w < V; ++w) ja.push_back(job(Fv[(size_t)w], K, Fv[(size_t)w], K, A[(size_t)w], K2));
  run_correlate(ja);
  for (int w = 0; w < V; ++w) bad += differing(A[(size_t)w], corr_plain(Fv[(size_t)w], K, Fv[(size_t)w], K, K2));
  Arr Call((size_t)(V * (V - 1) * n));
  if (V > 1) {
    C.assign((size_t)(V * (V - 1)), Arr((size_t)n));
    for (int v = 0; v < V; ++v)
      for (int w = 0; w < V; ++w)
        if (w != v) jc.push_back(job(Pv[(size_t)v], K, A[(size_t)w], K2, C[(size_t)(v * (V - 1) + (w < v ? w : w - 1))], K));
    run_correlate(jc);
    for (int v = 0; v < V; ++v)
      for (int w = 0; w < V; ++w)
        if (w != v) {
          const size_t at_ = (size_t)(v * (V - 1) + (w < v ? w : w - 1));
          bad += differing(C[at_], corr_plain(Pv[(size_t)v], K, A[(size_t)w], K2, K));
          std::copy(C[at_].begin(), C[at_].end(), Call.begin() + (long)at_ * n);
        }
  }
  for (int type = PSF_EFFICIENT_BAYESIAN; type <= PSF_OPTIMIZATION_II; ++type) {
    pt.C = V > 1 ? Call.data() : nullptr, pt.type = type;
    mvn_psf_point_check(pt);
    for (long blk = 0; blk < V * mvn_psf_blocks(n); ++blk)
      for (int t = 0; t < MVN_PSF_WG; ++t) mvn_psf_pointwise_item(pt, blk, t);
    for (int v = 0; v < V; ++v)
      for (long i = 0; i < n; ++i) {
        float want = Fv[(size_t)v][(size_t)i];
        if (type == PSF_OPTIMIZATION_II)
          for (int k = 1; k < V; ++k) want = want * Fv[(size_t)v][(size_t)i];
        else
          for (int w = 0; w < V - 1; ++w) want = want * Call[(size_t)((v * (V - 1) + w) * n + i)];
        bad += std::memcmp(&want, &T[(size_t)(v * n + i)], sizeof(float)) != 0;
      }
  }
  std::printf("(%d, %d, %d) x %d views%s: autocorrelation (%d, %d, %d), %d mismatches\n", K[0], K[1], K[2], V,
              zeros ? " with zeros" : "", K2[0], K2[1], K2[2], bad);
  return bad;
}

int main() {
  const int small[3] = {1, 3, 5}, group[3] = {33, 7, 11}, cube[3] = {3, 3, 3};
  int bad = 0;
  bad += check(small, 3, false);
  bad += check(group, 2, false);
  bad += check(group, 2, true);
  bad += check(cube, 1, false);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
