// register_standalone.cpp -- the four pass bodies behind mvn_register_beads (csrc/mvn_register.hpp) of the host emulation
// on exactly sized heap blocks, against a plain loop over the definition.  Built with -DMVN_HOST_EMU under
// AddressSanitizer + UBSan by tests/test_register_standalone.py, with its own main: nothing is loaded into Python.
// Cases: sets of 5, 65 and 257 beads (one tile, a tile and one bead, a partial second tile), B cut into chunks whose
// last one is partial, 1 and 257 hypotheses, and exactly four candidates.  Exits non-zero on a mismatch.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "mvn_register.hpp"

static unsigned g_x = 2463534242u;
static double rnd() {
  g_x = g_x * 1664525u + 1013904223u;
  return (double)(g_x >> 8) * (1.0 / 16777216.0);
}

// n points of a box of (60, 200, 200), each in a heap block of its own size
static std::vector<double> points(int n) {
  std::vector<double> p(3 * (size_t)n);
  for (int i = 0; i < n; ++i) p[3 * i] = 60.0 * rnd(), p[3 * i + 1] = 200.0 * rnd(), p[3 * i + 2] = 200.0 * rnd();
  return p;
}

static std::vector<double> moved(const std::vector<double>& a, int n, double noise) {
  std::vector<double> b(3 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const double* q = &a[3 * (size_t)i];
    b[3 * i] = 1.01 * q[0] + 0.03 * q[1] + 1.5 + noise * (rnd() - 0.5);
    b[3 * i + 1] = 0.99 * q[1] - 0.03 * q[0] - 2.0 + noise * (rnd() - 0.5);
    b[3 * i + 2] = 1.005 * q[2] + 3.0 + noise * (rnd() - 0.5);
  }
  return b;
}

static int neighbours_case(int n, std::vector<int>* nn_out, std::vector<float>* desc_out, const std::vector<double>& p) {
  std::vector<int> nn(4 * (size_t)n, -1);
  std::vector<float> desc(MVN_REG_DESC * (size_t)n, -1.f);
  RegParams q;
  std::memset(&q, 0, sizeof(q));
  q.pts = p.data(), q.n = n, q.nn = nn.data(), q.desc = desc.data();
  mvn_reg_check_neighbours(q);
  mvn_reg_neighbours_host(q);
  int bad = 0;
  const int triple[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
  for (int i = 0; i < n; ++i) {
    std::vector<std::pair<double, int>> order;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double dz = p[3 * j] - p[3 * i], dy = p[3 * j + 1] - p[3 * i + 1], dx = p[3 * j + 2] - p[3 * i + 2];
      order.push_back(std::make_pair((dz * dz + dy * dy) + dx * dx, j));
    }
    std::sort(order.begin(), order.end());
    for (int k = 0; k < 4; ++k) bad += nn[4 * i + k] != order[k].second;
    for (int d = 0; d < 4; ++d)
      for (int m = 0; m < 3; ++m)
        for (int c = 0; c < 3; ++c) {
          const float want = (float)(p[3 * (size_t)order[triple[d][m]].second + c] - p[3 * (size_t)i + c]);
          bad += std::memcmp(&want, &desc[MVN_REG_DESC * (size_t)i + 9 * d + 3 * m + c], sizeof(float)) != 0;
        }
  }
  std::printf("neighbours and descriptors, %d beads: %d mismatches\n", n, bad);
  *nn_out = nn, *desc_out = desc;
  return bad;
}

static int match_case(int na, int nb, int chunk, const std::vector<float>& da, const std::vector<float>& db) {
  const int chunks = mvn_reg_chunks(nb, chunk);
  std::vector<float> pd1((size_t)na * chunks), pd2((size_t)na * chunks), d1(na), d2(na);
  std::vector<int> pj1((size_t)na * chunks), j1(na);
  RegParams q;
  std::memset(&q, 0, sizeof(q));
  q.da = da.data(), q.db = db.data(), q.na = na, q.nb = nb, q.chunk = chunk;
  q.pd1 = pd1.data(), q.pj1 = pj1.data(), q.pd2 = pd2.data(), q.d1 = d1.data(), q.j1 = j1.data(), q.d2 = d2.data();
  mvn_reg_check_match(q);
  mvn_reg_match_host(q);
  int bad = 0;
  for (int i = 0; i < na; ++i) {
    std::vector<float> d(nb);
    for (int j = 0; j < nb; ++j) {
      float best = INFINITY;
      for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {
          float s = 0.f;
          for (int k = 0; k < 9; ++k) {
            const float e = da[MVN_REG_DESC * (size_t)i + 9 * x + k] - db[MVN_REG_DESC * (size_t)j + 9 * y + k];
            s = k == 0 ? e * e : s + e * e;
          }
          best = s < best ? s : best;
        }
      d[j] = best;
    }
    int w1 = 0;
    for (int j = 1; j < nb; ++j)
      if (d[j] < d[w1]) w1 = j;
    float w2 = INFINITY;
    for (int j = 0; j < nb; ++j)
      if (j != w1 && d[j] < w2) w2 = d[j];
    bad += j1[i] != w1 || d1[i] != d[w1] || d2[i] != w2;
  }
  std::printf("match, %d x %d beads in %d chunks of %d: %d mismatches\n", na, nb, chunks, chunk, bad);
  return bad;
}

static void plain_sample(unsigned long long seed, unsigned h, int n, int out[4]) {
  std::vector<int> picks;
  for (int q = 0; q < 4; ++q) {
    const unsigned long long u = mvn_reg_mix(seed + 0x9E3779B97F4A7C15ull * (16ull * h + (unsigned long long)q + 1ull));
    int r = (int)(((u >> 32) * (unsigned long long)(n - q)) >> 32);
    std::vector<int> sorted = picks;
    std::sort(sorted.begin(), sorted.end());
    for (int s : sorted)
      if (s <= r) ++r;
    picks.push_back(r), out[q] = r;
  }
}

static int ransac_case(int nc, int hyps, double noise) {
  const std::vector<double> a = points(nc), b = moved(a, nc, noise);
  std::vector<double> rec(6 * (size_t)nc);
  for (int m = 0; m < nc; ++m)
    for (int k = 0; k < 3; ++k) rec[6 * (size_t)m + k] = a[3 * (size_t)m + k], rec[6 * (size_t)m + 3 + k] = b[3 * (size_t)m + k];
  std::vector<unsigned long long> best(1, 0ull);
  RegParams q;
  std::memset(&q, 0, sizeof(q));
  q.cand = rec.data(), q.nc = nc, q.hyps = hyps, q.seed = 42ull, q.maxerr2 = 0.25 * 0.25, q.best = best.data();
  mvn_reg_check_ransac(q);
  mvn_reg_ransac_host(q);
  int wscore = 0;
  unsigned wh = 0;
  int bad = 0;
  for (int h = 0; h < hyps; ++h) {
    int s[4], t[4];
    plain_sample(q.seed, (unsigned)h, nc, s);
    mvn_reg_sample(q.seed, (unsigned)h, nc, t);
    for (int k = 0; k < 4; ++k) bad += s[k] != t[k] || s[k] < 0 || s[k] >= nc;
    for (int k = 0; k < 4; ++k)
      for (int l = 0; l < k; ++l) bad += s[k] == s[l];
    double sa[12], sb[12], L[9], tr[3];
    for (int m = 0; m < 4; ++m)
      for (int k = 0; k < 3; ++k) sa[3 * m + k] = a[3 * (size_t)s[m] + k], sb[3 * m + k] = b[3 * (size_t)s[m] + k];
    int score = 0;
    if (mvn_reg_fit4(sa, sb, L, tr))
      for (int m = 0; m < nc; ++m) score += mvn_reg_residual2(L, tr, &a[3 * (size_t)m], &b[3 * (size_t)m]) <= q.maxerr2;
    if (score > wscore) wscore = score, wh = (unsigned)h;
  }
  bad += mvn_reg_key_score(best[0]) != wscore || mvn_reg_key_h(best[0]) != wh;
  std::printf("ransac, %d candidates, %d hypotheses: best score %d at h = %u, %d mismatches\n", nc, hyps, wscore, wh, bad);
  return bad;
}

int main() {
  int bad = 0;
  const int sizes[3] = {5, 65, 257};
  std::vector<std::vector<float>> desc(3);
  std::vector<std::vector<float>> desc_b(3);
  for (int k = 0; k < 3; ++k) {
    const std::vector<double> a = points(sizes[k]), b = moved(a, sizes[k], 0.1);
    std::vector<int> nn;
    bad += neighbours_case(sizes[k], &nn, &desc[k], a);
    bad += neighbours_case(sizes[k], &nn, &desc_b[k], b);
  }
  for (int ka = 0; ka < 3; ++ka)
    for (int kb = 0; kb < 3; ++kb) {
      bad += match_case(sizes[ka], sizes[kb], mvn_reg_chunk(sizes[ka], sizes[kb]), desc[ka], desc_b[kb]);
      bad += match_case(sizes[ka], sizes[kb], 2 * MVN_REG_MTILE, desc[ka], desc_b[kb]);  // 257: two chunks and one bead
    }
  const int hyps[2] = {1, 257};
  for (int h = 0; h < 2; ++h) {
    bad += ransac_case(4, hyps[h], 0.0);
    bad += ransac_case(65, hyps[h], 0.4);
    bad += ransac_case(257, hyps[h], 0.8);
  }
  std::printf(bad ? "FAILED: %d mismatches\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
