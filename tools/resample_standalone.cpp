// Stand-alone check of the resample pass and of the weights normalisation of the host emulation
// (csrc/mvn_resample.hpp, the launches mvn_backend_emu.cpp makes): the pass bodies on small blocks - an odd last extent
// with its row padding, a row pitch that is a multiple of 4, a block with tile seams on all three axes, a raw stack of
// one plane, voxels outside the raw stack, a window inside a larger volume - against a plain triple loop over the
// definition in include/mvn_engine_api.h.  Every buffer is allocated at exactly its size: the sanitizer sees an access
// past it.  Built with -fsanitize=address,undefined by tests/test_resample_standalone.py; exits non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc> \
//       resample_standalone.cpp -o resample_standalone
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mvn_resample.hpp"

struct Case {
  int n[3];     // block
  int ext[3];   // the volume around it
  int off[3];   // the block's offset in it
  int m[3];     // raw stack
  double M[12];
  float border[3], range[3];
};

static float ramp(float dk, float border, float range) {
  if (dk < border) return 0.f;
  if (range == 0.f || dk >= border + range) return 1.f;
  const float u = (dk - border) / range;
  return 0.5f * (1.0f - cosf(3.14159265358979323846f * u));
}

static float lerp(float p, float q, float f) { return p + f * (q - p); }

template <typename T>
static int check(const Case& c, const char* tname) {
  const long RP = c.ext[2] % 2 ? c.ext[2] + 1 : c.ext[2];
  const long vol = (long)c.ext[0] * c.ext[1] * RP, raw_n = (long)c.m[0] * c.m[1] * c.m[2];
  std::mt19937 rng(5u + (unsigned)raw_n);
  std::uniform_int_distribution<int> dist(100, 4000);
  std::vector<T> raw((size_t)raw_n);
  for (T& x : raw) x = (T)dist(rng);
  const float pad = -77.f;
  const int V = 2;
  std::vector<std::vector<float>> image((size_t)V), weights((size_t)V);
  ResampleParams p;
  std::memset(&p, 0, sizeof(p));
  p.RP = RP, p.D0 = c.ext[0], p.D1 = c.ext[1];
  p.n0 = c.n[0], p.n1 = c.n[1], p.n2 = c.n[2];
  p.o0 = c.off[0], p.o1 = c.off[1], p.o2 = c.off[2];
  p.src = raw.data(), p.s0 = (long long)c.m[1] * c.m[2], p.s1 = c.m[2], p.s2 = 1;
  for (int k = 0; k < 3; ++k) p.g.m[k] = c.m[k], p.g.border[k] = c.border[k], p.g.range[k] = c.range[k];
  int bad = 0;
  for (int v = 0; v < V; ++v) {
    image[(size_t)v].assign((size_t)vol, pad);
    weights[(size_t)v].assign((size_t)vol, pad);
    p.image = image[(size_t)v].data(), p.weights = weights[(size_t)v].data();
    for (int i = 0; i < 12; ++i) p.g.M[i] = c.M[i];
    p.g.M[3] += 0.375 * v;  // the second view: shifted along raw axis 0
    const long nblocks = mvn_resample_blocks(p);
#pragma omp parallel for schedule(static)
    for (long blk = 0; blk < nblocks; ++blk)
      for (int t = 0; t < MVN_RS_WG; ++t) mvn_resample_tile<T>(p, blk, t);
    // the plain triple loop over the whole volume: zeros wherever the definition gives no value
    for (int z = 0; z < c.ext[0]; ++z)
      for (int y = 0; y < c.ext[1]; ++y)
        for (long x = 0; x < RP; ++x) {
          float wi = 0.f, ww = 0.f;
          const int zi = z - c.off[0], yi = y - c.off[1];
          const long xi = x - c.off[2];
          if (zi >= 0 && zi < c.n[0] && yi >= 0 && yi < c.n[1] && xi >= 0 && xi < c.n[2]) {
            double cc[3];
            bool in = true;
            for (int k = 0; k < 3; ++k) {
              const double* r = p.g.M + 4 * k;
              cc[k] = ((r[0] * (double)zi + r[1] * (double)yi) + r[2] * (double)xi) + r[3];
              in = in && cc[k] >= 0. && cc[k] <= (double)(c.m[k] - 1);
            }
            if (in) {
              long i[3], j[3];
              float f[3];
              ww = 1.f;
              float rk[3];
              for (int k = 0; k < 3; ++k) {
                i[k] = (long)std::floor(cc[k]);
                j[k] = i[k] + 1 < c.m[k] ? i[k] + 1 : c.m[k] - 1;
                f[k] = (float)(cc[k] - (double)i[k]);
                const double d = std::fmin(cc[k], (double)(c.m[k] - 1) - cc[k]);
                rk[k] = ramp((float)d, c.border[k], c.range[k]);
              }
              ww = (rk[0] * rk[1]) * rk[2];
              auto S = [&](long a, long b, long cx) { return (float)raw[(size_t)((a * c.m[1] + b) * c.m[2] + cx)]; };
              float bb[2];
              for (int a0 = 0; a0 < 2; ++a0) {
                const long pz = a0 ? j[0] : i[0];
                const float a_lo = lerp(S(pz, i[1], i[2]), S(pz, i[1], j[2]), f[2]);
                const float a_hi = lerp(S(pz, j[1], i[2]), S(pz, j[1], j[2]), f[2]);
                bb[a0] = lerp(a_lo, a_hi, f[1]);
              }
              wi = lerp(bb[0], bb[1], f[0]);
            }
          }
          const size_t at = (size_t)(((long)z * c.ext[1] + y) * RP + x);
          if (image[(size_t)v][at] != wi) ++bad;
          if (weights[(size_t)v][at] != ww) ++bad;
        }
  }
  // the normalisation over the two views, on the window only
  std::vector<std::vector<float>> before = weights;
  std::vector<float*> tab = {weights[0].data(), weights[1].data()};
  NormalizeParams q;
  std::memset(&q, 0, sizeof(q));
  q.vols = tab.data(), q.V = V, q.RP = RP, q.D1 = c.ext[1];
  q.n0 = c.n[0], q.n1 = c.n[1], q.n2 = c.n[2];
  q.o0 = c.off[0], q.o1 = c.off[1], q.o2 = c.off[2];
  const long nb = mvn_normalize_blocks(q);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nb; ++blk)
    for (int t = 0; t < MVN_INGEST_WG; ++t) mvn_normalize_rows(q, blk, t);
  long positive = 0;
  for (int z = 0; z < c.ext[0]; ++z)
    for (int y = 0; y < c.ext[1]; ++y)
      for (long x = 0; x < RP; ++x) {
        const size_t at = (size_t)(((long)z * c.ext[1] + y) * RP + x);
        const int zi = z - c.off[0], yi = y - c.off[1];
        const long xi = x - c.off[2];
        const bool win = zi >= 0 && zi < c.n[0] && yi >= 0 && yi < c.n[1] && xi >= 0 && xi < c.n[2];
        const float W = before[0][at] + before[1][at];
        for (int v = 0; v < V; ++v) {
          const float want = !win ? before[(size_t)v][at] : W > 0.f ? before[(size_t)v][at] / W : 0.f;
          if (weights[(size_t)v][at] != want) ++bad;
        }
        if (win && W > 0.f) ++positive;
      }
  if (positive == 0) ++bad;  // (a case whose weights all vanish checks nothing)
  std::printf("(%d, %d, %d) in (%d, %d, %d) from %s (%d, %d, %d): %ld workgroups, %d mismatches\n", c.n[0], c.n[1], c.n[2],
              c.ext[0], c.ext[1], c.ext[2], tname, c.m[0], c.m[1], c.m[2], mvn_resample_blocks(p), bad);
  return bad;
}

int main() {
  const double c30 = std::cos(std::acos(-1.0) / 6), s30 = 0.5;
  const Case cases[] = {
      // identity, odd last extent: RP = 2 mod 4, c_2 reaches m_2 - 1
      {{3, 5, 7}, {3, 5, 7}, {0, 0, 0}, {5, 6, 7}, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {0, 1, 0.5f}, {1, 2, 1.5f}},
      // an integer shift inside a padded volume: plane z = 0 of the block lies outside the raw stack
      {{4, 6, 10}, {6, 9, 15}, {1, 2, 3}, {3, 9, 11}, {1, 0, 0, -1, 0, 1, 0, 2, 0, 0, 1, 1}, {0, 0, 1}, {1, 3, 0}},
      // a fractional shift, RP a multiple of 4
      {{2, 3, 20}, {2, 3, 20}, {0, 0, 0}, {3, 9, 11}, {1, 0, 0, 0.25, 0, 1, 0, 1.5, 0, 0, 1, -2.6}, {0, 0.5f, 0}, {0.75f, 2, 3}},
      // a raw z-step of 3 block voxels; tile seams on all three axes, in a volume with margins
      {{MVN_RS_TZ + 2, MVN_RS_TY + 6, MVN_RS_TX + 6}, {MVN_RS_TZ + 5, MVN_RS_TY + 9, MVN_RS_TX + 11}, {2, 1, 3}, {5, 6, 7},
       {1. / 3, 0, 0, 0, 0, 0.35, 0, 0, 0, 0, 0.08, 0}, {0.5f, 0, 0.25f}, {1, 1.5f, 2}},
      // 30 degrees about axis 1
      {{3, 5, 7}, {5, 8, 9}, {1, 1, 1}, {5, 6, 7},
       {c30, 0, s30, 2 - c30 - 3 * s30, 0, 1, 0, 0.5, -s30, 0, c30, 3 + s30 - 3 * c30}, {0, 0.25f, 0}, {1, 1, 1.5f}},
      // one raw plane
      {{2, 3, 20}, {2, 3, 20}, {0, 0, 0}, {1, 6, 7}, {0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0.3, 0}, {0, 0, 0.5f}, {0, 1, 1}},
  };
  int bad = 0;
  for (const Case& c : cases) {
    bad += check<uint16_t>(c, "uint16");
    bad += check<float>(c, "float32");
  }
  std::printf(bad ? "MISMATCH\n" : "ok\n");
  return bad ? 1 : 0;
}
