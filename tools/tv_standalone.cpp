// Stand-alone check of the total-variation pass of the host emulation (csrc/mvn_tv.hpp, the launch mvn_backend_emu.cpp
// makes): the pass body on small volumes - x+1 and x-1 the same voxel, an extent of 1, an odd last extent with its row
// padding, more planes than one workgroup walks - against a plain triple loop.  Built with
// -fsanitize=address,undefined by tests/test_tv_standalone.py; exits non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc> \
//       tv_standalone.cpp -o tv_standalone
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mvn_tv.hpp"

static int check(int d0, int d1, int d2) {
  const int RP = d2 % 2 ? d2 + 1 : d2;
  const long rows = (long)d0 * d1, n = rows * RP;
  std::mt19937 rng(11u + (unsigned)d2);
  std::uniform_real_distribution<float> dist(0.5f, 2.f);
  const float pad = -77.f, lambda = 0.005f, eps = 0.01f, e2 = eps * eps;
  // exactly-sized allocations: the sanitizer sees every access past the volume
  std::vector<float> u(n, pad), t(n, pad);
  for (long r = 0; r < rows; ++r)
    for (int c = 0; c < d2; ++c) u[r * RP + c] = dist(rng);
  TvParams p;
  std::memset(&p, 0, sizeof(p));
  p.psi = u.data(), p.t = t.data();
  p.d0 = d0, p.d1 = d1, p.d2 = d2, p.RP = RP;
  p.lambda = lambda, p.e2 = e2;
  mvn_tv_geometry(p);
  mvn_tv_host(p);
  // the plain triple loop
  auto at = [&](int z, int y, int x) {
    return u[(((long)((z + d0) % d0) * d1) + (y + d1) % d1) * RP + (x + d2) % d2];
  };
  auto pvec = [&](int z, int y, int x, float* out) {
    const float c = at(z, y, x);
    const float gz = at(z + 1, y, x) - c, gy = at(z, y + 1, x) - c, gx = at(z, y, x + 1) - c;
    const float m = std::sqrt(((gx * gx + gy * gy) + gz * gz) + e2);
    const float r = 1.0f / m;
    out[0] = gx * r, out[1] = gy * r, out[2] = gz * r;
  };
  int bad = 0;
  for (int z = 0; z < d0; ++z)
    for (int y = 0; y < d1; ++y)
      for (int x = 0; x < d2; ++x) {
        float c[3], mx[3], my[3], mz[3];
        pvec(z, y, x, c), pvec(z, y, x - 1, mx), pvec(z, y - 1, x, my), pvec(z - 1, y, x, mz);
        const float dv = ((c[0] - mx[0]) + (c[1] - my[1])) + (c[2] - mz[2]);
        const float want = 1.0f / (1.0f - lambda * dv);
        if (t[((long)z * d1 + y) * RP + x] != want) ++bad;
      }
  if (RP != d2)  // the row padding is neither read nor written
    for (long r = 0; r < rows; ++r)
      if (t[r * RP + d2] != pad) ++bad;
  std::printf("(%d, %d, %d): %ld workgroups, %d mismatches\n", d0, d1, d2, mvn_tv_blocks(p), bad);
  return bad;
}

int main() {
  int bad = 0;
  bad += check(3, 5, 2);
  bad += check(1, 3, 5);
  bad += check(10, 14, 45);
  bad += check(MVN_TV_SEG + 3, MVN_TV_TY + 1, MVN_TV_TX + 3);  // tile and segment seams on every axis
  std::printf(bad ? "MISMATCH\n" : "ok\n");
  return bad ? 1 : 0;
}
