// Stand-alone check of the passes behind mvn_detect_beads on the host emulation (csrc/mvn_detect.hpp, run the way
// mvn_backend_emu.cpp launches them): the row, column and plane blurs, the extremum pass and the fit, against a plain
// loop over the definition in include/mvn_engine_api.h - stacks of (5, 6, 40) (narrower than the radius: several
// reflections), (9, 11, 70) and (34, 37, 70), three sigma sets, uint16 and float32, maxima and minima, with blobs
// planted one voxel from the faces so that candidates lie next to them.  Every buffer is allocated at exactly its
// size - the raw stack at its element count, each volume at m0 m1 m2 floats, the list and the results at the number of
// candidates - so an index one off the end is an access the sanitizer sees.  Built with -fsanitize=address,undefined
// by tests/test_detect_standalone.py; exits non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc>
//       detect_standalone.cpp -o detect_standalone
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "mvn_detect.hpp"

static int mirror(long i, int n) {  // by walking: the definition, not the remainder
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2L * (n - 1) - i;
  return (int)i;
}

// v blurred along axis k, one voxel and one tap at a time
static std::vector<float> blur_plain(const std::vector<float>& u, const int* m, int k, const float* w, int R) {
  std::vector<float> v(u.size());
  const size_t stride[3] = {(size_t)m[1] * m[2], (size_t)m[2], 1};
  for (int c0 = 0; c0 < m[0]; ++c0)
    for (int c1 = 0; c1 < m[1]; ++c1)
      for (int c2 = 0; c2 < m[2]; ++c2) {
        const int c[3] = {c0, c1, c2};
        const size_t at = c0 * stride[0] + c1 * stride[1] + c2;
        const size_t line = at - (size_t)c[k] * stride[k];
        float acc = 0.f;
        for (int j = 0; j <= 2 * R; ++j) {
          const float prod = w[j] * u[line + (size_t)mirror((long)c[k] - R + j, m[k]) * stride[k]];
          acc = j == 0 ? prod : acc + prod;
        }
        v[at] = acc;
      }
  return v;
}

static void fit_plain(const double E[3][3][3], double o[3]) {
  const double c = E[1][1][1];
  double g[3], H[3][3];
  auto at = [&](int a, int b, int d) { return E[1 + a][1 + b][1 + d]; };
  auto step = [](int k, int s, int* d) { d[0] = d[1] = d[2] = 0, d[k] = s; };
  for (int k = 0; k < 3; ++k) {
    int p[3], q[3];
    step(k, 1, p), step(k, -1, q);
    const double P = at(p[0], p[1], p[2]), M = at(q[0], q[1], q[2]);
    g[k] = (P - M) / 2.0;
    H[k][k] = (P + M) - 2.0 * c;
    for (int l = k + 1; l < 3; ++l) {
      int pp[3], pm[3], mp[3], mm[3];
      step(k, 1, pp), pp[l] = 1, step(k, 1, pm), pm[l] = -1, step(k, -1, mp), mp[l] = 1, step(k, -1, mm), mm[l] = -1;
      H[k][l] = H[l][k] = ((at(pp[0], pp[1], pp[2]) - at(pm[0], pm[1], pm[2])) -
                           (at(mp[0], mp[1], mp[2]) - at(mm[0], mm[1], mm[2]))) / 4.0;
    }
  }
  const double C00 = H[1][1] * H[2][2] - H[1][2] * H[1][2], C01 = H[0][2] * H[1][2] - H[0][1] * H[2][2];
  const double C02 = H[0][1] * H[1][2] - H[0][2] * H[1][1], C11 = H[0][0] * H[2][2] - H[0][2] * H[0][2];
  const double C12 = H[0][1] * H[0][2] - H[0][0] * H[1][2], C22 = H[0][0] * H[1][1] - H[0][1] * H[0][1];
  const double det = (H[0][0] * C00 + H[0][1] * C01) + H[0][2] * C02;
  const double n[3] = {(C00 * g[0] + C01 * g[1]) + C02 * g[2], (C01 * g[0] + C11 * g[1]) + C12 * g[2],
                       (C02 * g[0] + C12 * g[1]) + C22 * g[2]};
  o[0] = o[1] = o[2] = 0.0;
  if (det == 0.0 || !std::isfinite(det)) return;
  double t[3];
  for (int k = 0; k < 3; ++k) {
    t[k] = -n[k] / det;
    if (!std::isfinite(t[k]) || std::fabs(t[k]) > 1.0) return;
  }
  o[0] = t[0], o[1] = t[1], o[2] = t[2];
}

static long g_faces[2] = {0, 0};  // candidates next to a face: uint16, float32

template <typename T>
static long run_case(const char* type, const int* m, const double* s1, const double* s2, int minima, unsigned seed) {
  std::mt19937 rng(seed);
  const size_t n = (size_t)m[0] * m[1] * m[2];
  std::unique_ptr<T[]> raw(new T[n]);
  {  // random values plus blobs, the first ones a voxel from the faces
    std::vector<double> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = 100.0 + (double)(rng() % 900);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const int blobs = 6 + (int)(n / 3000);
    for (int b = 0; b < blobs; ++b) {
      double p[3];
      for (int k = 0; k < 3; ++k) p[k] = u(rng) * (m[k] - 1);
      if (b < 6) p[b % 3] = b < 3 ? 1.0 : (double)(m[b % 3] - 2);
      for (int c0 = 0; c0 < m[0]; ++c0)
        for (int c1 = 0; c1 < m[1]; ++c1)
          for (int c2 = 0; c2 < m[2]; ++c2) {
            const double d = (c0 - p[0]) * (c0 - p[0]) + (c1 - p[1]) * (c1 - p[1]) + (c2 - p[2]) * (c2 - p[2]);
            v[((size_t)c0 * m[1] + c1) * m[2] + c2] += (minima ? -3000.0 : 3000.0) * std::exp(-d / 4.5);
          }
    }
    for (size_t i = 0; i < n; ++i) raw[i] = (T)std::fmax(0.0, std::rint(v[i] + 4000.0));
  }
  const float threshold = 5.f;

  std::unique_ptr<float[]> table(new float[MVN_DETECT_TABLE]);
  std::unique_ptr<float[]> a0(new float[n]), a1(new float[n]), b0(new float[n]), b1(new float[n]);
  std::unique_ptr<unsigned long long[]> count(new unsigned long long[1]);
  DetectParams p;
  std::memset(&p, 0, sizeof(p));
  std::memset(table.get(), 0, MVN_DETECT_TABLE * sizeof(float));
  p.src = raw.get(), p.s0 = (long long)m[1] * m[2], p.s1 = m[2], p.s2 = 1;
  for (int k = 0; k < 3; ++k) {
    p.m[k] = m[k];
    p.R[0][k] = mvn_detect_make_taps(s1[k], table.get() + (0 * 3 + k) * MVN_DETECT_TAPS);
    p.R[1][k] = mvn_detect_make_taps(s2[k], table.get() + (1 * 3 + k) * MVN_DETECT_TAPS);
  }
  p.taps = table.get();
  p.a[0] = a0.get(), p.a[1] = a1.get(), p.b[0] = b0.get(), p.b[1] = b1.get();
  p.threshold = threshold, p.minima = minima;
  mvn_detect_check_blur(p);
  mvn_detect_rows_host<T>(p);
  mvn_detect_lines_host<1>(p);
  mvn_detect_lines_host<0>(p);

  // the definition: both blurs, one axis at a time, and their difference
  long bad = 0;
  std::vector<float> D(n);
  {
    std::vector<float> L[2];
    for (int a = 0; a < 2; ++a) {
      L[a].resize(n);
      for (size_t i = 0; i < n; ++i) L[a][i] = (float)raw[i];
      for (int k = 2; k >= 0; --k)
        L[a] = blur_plain(L[a], m, k, table.get() + (a * 3 + k) * MVN_DETECT_TAPS, p.R[a][k]);
    }
    for (size_t i = 0; i < n; ++i) {
      D[i] = L[0][i] - L[1][i];
      if (std::memcmp(&D[i], &a0[i], sizeof(float)) != 0) ++bad;
    }
  }
  // the candidates in raster order
  auto E = [&](int c0, int c1, int c2) {
    const float v = D[((size_t)c0 * m[1] + c1) * m[2] + c2];
    return minima ? -v : v;
  };
  std::vector<long long> want;
  for (int c0 = 1; c0 <= m[0] - 2; ++c0)
    for (int c1 = 1; c1 <= m[1] - 2; ++c1)
      for (int c2 = 1; c2 <= m[2] - 2; ++c2) {
        const float e = E(c0, c1, c2);
        bool top = e > threshold;
        for (int d0 = -1; d0 <= 1 && top; ++d0)
          for (int d1 = -1; d1 <= 1; ++d1)
            for (int d2 = -1; d2 <= 1; ++d2)
              if ((d0 || d1 || d2) && !(e > E(c0 + d0, c1 + d1, c2 + d2))) top = false;
        if (top) want.push_back(((long long)c0 * m[1] + c1) * m[2] + c2);
      }
  long faces = 0;  // candidates next to a face
  for (long long at : want) {
    const int c[3] = {(int)(at / ((long long)m[1] * m[2])), (int)(at / m[2] % m[1]), (int)(at % m[2])};
    for (int k = 0; k < 3; ++k)
      if (c[k] == 1 || c[k] == m[k] - 2) {
        ++faces;
        break;
      }
  }
  const size_t found = want.size();
  g_faces[sizeof(T) == 2 ? 0 : 1] += faces;
  // the extremum pass into a list of exactly `found` entries, then into one that is one entry short
  count[0] = 0;
  std::unique_ptr<long long[]> list(new long long[found ? found : 1]);
  p.count = count.get(), p.list = list.get(), p.list_cap = (long long)(found ? found : 1);
  mvn_detect_check_list(p);
  mvn_detect_extrema_host(p);
  if (count[0] != found) ++bad;
  if (count[0] == found && found > 0) {
    std::sort(list.get(), list.get() + found);
    for (size_t i = 0; i < found; ++i)
      if (list[i] != want[i]) ++bad;
    if (found > 1) {
      std::unique_ptr<long long[]> shorter(new long long[found - 1]);
      DetectParams s = p;
      count[0] = 0;
      s.list = shorter.get(), s.list_cap = (long long)found - 1;
      mvn_detect_extrema_host(s);
      if (count[0] != found) ++bad;  // counted, not stored
    }
    // the fit
    std::unique_ptr<double[]> pos(new double[3 * found]);
    std::unique_ptr<float[]> val(new float[found]);
    std::unique_ptr<int[]> vox(new int[3 * found]);
    p.nfound = (long long)found, p.pos = pos.get(), p.val = val.get(), p.vox = vox.get();
    mvn_detect_refine_host(p);
    for (size_t i = 0; i < found; ++i) {
      const long long at = want[i];
      const int c[3] = {(int)(at / ((long long)m[1] * m[2])), (int)(at / m[2] % m[1]), (int)(at % m[2])};
      double N[3][3][3], o[3];
      for (int d0 = 0; d0 < 3; ++d0)
        for (int d1 = 0; d1 < 3; ++d1)
          for (int d2 = 0; d2 < 3; ++d2) N[d0][d1][d2] = (double)E(c[0] + d0 - 1, c[1] + d1 - 1, c[2] + d2 - 1);
      fit_plain(N, o);
      const float e = E(c[0], c[1], c[2]);
      if (std::memcmp(&e, &val[i], sizeof(float)) != 0) ++bad;
      for (int k = 0; k < 3; ++k) {
        const double pk = (double)c[k] + o[k];
        if (std::memcmp(&pk, &pos[3 * i + k], sizeof(double)) != 0 || vox[3 * i + k] != c[k]) ++bad;
      }
    }
  }
  std::printf("%s, stack (%d, %d, %d), sigma (%g, %g, %g) / (%g, %g, %g), %s: %zu candidates, %ld next to a face, "
              "%ld mismatches\n", type, m[0], m[1], m[2], s1[0], s1[1], s1[2], s2[0], s2[1], s2[2],
              minima ? "minima" : "maxima", found, faces, bad);
  return bad;
}

int main() {
  const int stacks[3][3] = {{5, 6, 40}, {9, 11, 70}, {34, 37, 70}};
  const double sig[3][2][3] = {{{1.5, 1.5, 1.5}, {1.7838, 1.7838, 1.7838}}, {{0, 1.5, 1.5}, {0, 1.8, 1.8}},
                               {{2.5, 2.5, 2.5}, {3, 3, 3}}};
  long bad = 0;
  unsigned seed = 1;
  for (const int* m : {stacks[0], stacks[1], stacks[2]})
    for (int q = 0; q < 3; ++q) {
      for (int minima = 0; minima < 2; ++minima) {
        bad += run_case<uint16_t>("uint16", m, sig[q][0], sig[q][1], minima, seed++);
        bad += run_case<float>("float32", m, sig[q][0], sig[q][1], minima, seed++);
      }
    }
  if (g_faces[0] < 100 || g_faces[1] < 100) ++bad;  // both element types with candidates next to the faces
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
