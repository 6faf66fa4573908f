// Stand-alone check of the passes behind mvn_extract_psf on the host emulation (csrc/mvn_beads.hpp, run the way
// mvn_backend_emu.cpp launches them): the gather with the sum over the groups, the minimum, and the scores, against a
// plain loop over the definition in include/mvn_engine_api.h - beads in the corners of the stack, at integers and a hair
// below them, 33 and 70 of them, windows of (3, 5, 7), (5, 3, 67) and, wider than the stack along two axes,
// (7, 9, 11) in (6, 7, 40), uint16 and float32.  Every buffer is allocated at exactly its size - the raw stack at its
// element count, so a mirror index one off the end is an access the sanitizer sees.  Built with
// -fsanitize=address,undefined by tests/test_beads_standalone.py; exits non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc> \
//       beads_standalone.cpp -o beads_standalone
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "mvn_beads.hpp"

static int mirror(long i, int n) {  // by walking: the definition, not the remainder
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2L * (n - 1) - i;
  return (int)i;
}

template <typename T>
static float sample_plain(const T* raw, const int* m, const int* B, const float* f, const int* d) {
  int lo[3], hi[3];
  for (int k = 0; k < 3; ++k) lo[k] = mirror((long)B[k] + d[k], m[k]), hi[k] = mirror((long)B[k] + d[k] + 1, m[k]);
  auto S = [&](int a, int b, int c) { return (float)raw[((size_t)a * m[1] + b) * m[2] + c]; };
  auto lerp = [](float p, float q, float t) {
    const float dd = q - p;
    const float u = t * dd;
    return p + u;
  };
  float b2[2];
  for (int a0 = 0; a0 < 2; ++a0) {
    float a2[2];
    for (int a1 = 0; a1 < 2; ++a1) {
      const int z = a0 ? hi[0] : lo[0], y = a1 ? hi[1] : lo[1];
      a2[a1] = lerp(S(z, y, lo[2]), S(z, y, hi[2]), f[2]);
    }
    b2[a0] = lerp(a2[0], a2[1], f[1]);
  }
  return lerp(b2[0], b2[1], f[0]);
}

template <typename T>
static long run_case(const char* type, const int* m, const int* r, int nbeads, unsigned seed) {
  std::mt19937 rng(seed);
  const size_t count = (size_t)m[0] * m[1] * m[2], n = (size_t)r[0] * r[1] * r[2];
  std::unique_ptr<T[]> raw(new T[count]);
  for (size_t i = 0; i < count; ++i) raw[i] = (T)(100 + rng() % 3900);
  // positions: the corner, the far corner exactly, an integer, a hair below an integer, then anywhere
  std::vector<double> pos(3 * (size_t)nbeads);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int b = 0; b < nbeads; ++b)
    for (int k = 0; k < 3; ++k) {
      double p = u(rng) * (m[k] - 1);
      if (b == 0) p = 0.0;
      if (b == 1) p = (double)(m[k] - 1);
      if (b == 2) p = (double)(m[k] / 2);
      if (b == 3) p = std::nextafter((double)(m[k] / 2), 0.0);
      pos[3 * (size_t)b + k] = p;
    }
  std::unique_ptr<BeadRec[]> recs(new BeadRec[(size_t)nbeads]);
  for (int b = 0; b < nbeads; ++b) {
    BeadRec& rec = recs[(size_t)b];
    std::memset(&rec, 0, sizeof(rec));
    rec.interior = 1;
    for (int k = 0; k < 3; ++k) {
      const double p = pos[3 * (size_t)b + k];
      const int h = (r[k] - 1) / 2;
      rec.B[k] = (int)p, rec.f[k] = (float)(p - (double)rec.B[k]);
      if (rec.B[k] - h < 0 || rec.B[k] + h + 1 > m[k] - 1) rec.interior = 0;
    }
  }
  const int G = mvn_beads_groups(nbeads);
  std::unique_ptr<double[]> partial(new double[(size_t)G * n]);
  std::unique_ptr<float[]> psf(new float[n]), minima(new float[MVN_BEADS_WG]);
  std::unique_ptr<unsigned[]> flag(new unsigned[1]);
  std::unique_ptr<double[]> records(new double[(size_t)nbeads * MVN_BEADS_WG * MVN_BEADS_SUMS]);
  std::unique_ptr<double[]> scores(new double[(size_t)nbeads]);
  flag[0] = 0u;
  BeadsParams p;
  std::memset(&p, 0, sizeof(p));
  p.src = raw.get(), p.s0 = (long long)m[1] * m[2], p.s1 = m[2], p.s2 = 1;
  for (int k = 0; k < 3; ++k) p.m[k] = m[k], p.r[k] = r[k];
  p.beads = recs.get(), p.nbeads = nbeads;
  p.partial = partial.get(), p.psf = psf.get(), p.minima = minima.get(), p.flag = flag.get();
  p.records = records.get(), p.scores = scores.get();
  mvn_beads_check(p);
  const long tiles = mvn_beads_tiles(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < G * tiles; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_gather_item<T>(p, blk, t);
  for (long blk = 0; blk < tiles; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_reduce_item(p, blk, t);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < (long)nbeads; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_score_item<T>(p, blk, t);
  for (long blk = 0; blk < (nbeads + MVN_BEADS_WG - 1) / MVN_BEADS_WG; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_score_fold_item(p, blk, t);

  // the definition, one voxel and one bead at a time
  long bad = 0;
  std::vector<float> want(n);
  std::vector<std::vector<float>> win((size_t)nbeads, std::vector<float>(n));
  const int h[3] = {(r[0] - 1) / 2, (r[1] - 1) / 2, (r[2] - 1) / 2};
  for (size_t j = 0; j < n; ++j) {
    const int d[3] = {(int)(j / ((size_t)r[1] * r[2])) - h[0], (int)(j / r[2] % r[1]) - h[1], (int)(j % r[2]) - h[2]};
    double T_ = 0.0;
    for (int g = 0; g < G; ++g) {
      double P = 0.0;
      for (int b = g * MVN_BEADS_PER_GROUP; b < nbeads && b < (g + 1) * MVN_BEADS_PER_GROUP; ++b) {
        const float s = sample_plain<T>(raw.get(), m, recs[(size_t)b].B, recs[(size_t)b].f, d);
        win[(size_t)b][j] = s;
        P = P + (double)s;
      }
      T_ = g == 0 ? P : T_ + P;
    }
    want[j] = (float)(T_ / (double)nbeads);
    if (std::memcmp(&want[j], &psf[j], sizeof(float)) != 0) ++bad;
  }
  if (flag[0]) ++bad;
  double worst = 0.0;
  for (int b = 0; b < nbeads; ++b) {
    double ss = 0, ss2 = 0, sp = 0, sp2 = 0, ssp = 0;
    for (size_t j = 0; j < n; ++j) {
      const double s = win[(size_t)b][j], P = want[j];
      ss += s, ss2 += s * s, sp += P, sp2 += P * P, ssp += s * P;
    }
    const double den = std::sqrt((ss2 - ss * ss / (double)n) * (sp2 - sp * sp / (double)n));
    const double sc = den > 0 && std::isfinite(den) ? (ssp - ss * sp / (double)n) / den : 0.0;
    worst = std::fmax(worst, std::fabs(sc - scores[(size_t)b]));
  }
  if (!(worst <= 1e-6)) ++bad;
  // the minimum, behind the scores as in a call
  for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_min_item(p, t);
  for (long blk = 0; blk < tiles; ++blk)
    for (int t = 0; t < MVN_BEADS_WG; ++t) mvn_beads_sub_item(p, blk, t);
  float mn = want[0];
  for (size_t j = 1; j < n; ++j) mn = want[j] < mn ? want[j] : mn;
  bool zero = false;
  for (size_t j = 0; j < n; ++j) {
    const float v = want[j] - mn;
    if (std::memcmp(&v, &psf[j], sizeof(float)) != 0) ++bad;
    zero = zero || psf[j] == 0.f;
  }
  if (!zero) ++bad;
  std::printf("%s, stack (%d, %d, %d), window (%d, %d, %d), %d beads: %ld mismatches, scores within %.3g\n", type, m[0],
              m[1], m[2], r[0], r[1], r[2], nbeads, bad, worst);
  return bad;
}

int main() {
  const int stacks[2][3] = {{9, 11, 70}, {6, 7, 40}};
  const int windows[3][3] = {{3, 5, 7}, {5, 3, 67}, {7, 9, 11}};
  long bad = 0;
  unsigned seed = 1;
  for (const int* m : {stacks[0], stacks[1]})
    for (const int* r : {windows[0], windows[1], windows[2]})
      for (int nbeads : {4, 33, 70}) {
        bad += run_case<uint16_t>("uint16", m, r, nbeads, seed++);
        bad += run_case<float>("float32", m, r, nbeads, seed++);
      }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
