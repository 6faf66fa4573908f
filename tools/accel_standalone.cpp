// Stand-alone check of the extrapolation passes of the host emulation (csrc/mvn_extrapolate.hpp, the launches
// mvn_backend_emu.cpp makes): pass A, the reduction and pass B on small volumes - an odd last extent with its row padding,
// less than one workgroup, an even extent that is no multiple of 4 - against a plain loop.  Built with
// -fsanitize=address,undefined by tests/test_accel_standalone.py; exits non-zero on a mismatch.
//   g++ -std=c++17 -DMVN_HOST_EMU -fopenmp -ffp-contract=off -fsanitize=address,undefined -I<csrc> \
//       accel_standalone.cpp -o accel_standalone
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mvn_extrapolate.hpp"

static int check(int d0, int d1, int d2) {
  const int RP = d2 % 2 ? d2 + 1 : d2;
  const long rows = (long)d0 * d1, n = rows * RP;
  const long nrec = mvn_accel_blocks(n, RP == d2 ? 4 : 2);
  std::mt19937 rng(7u + (unsigned)d2);
  std::uniform_real_distribution<float> u(0.f, 2.f);
  const float pad = -77.f, min_value = 0.9f;  // (a clamp that does fire)
  // exactly-sized allocations: the sanitizer sees every access past the volume
  std::vector<float> psi(n, pad), ysave(n, pad), g(n, pad), xprev(n, pad);
  std::vector<double> rec(2 * nrec);
  float alpha = -1.f;
  int bad = 0;
  for (int k = 1; k <= 3; ++k) {
    for (long r = 0; r < rows; ++r)
      for (int c = 0; c < d2; ++c) {
        psi[r * RP + c] = u(rng);
        if (k == 1) ysave[r * RP + c] = u(rng);
      }
    const std::vector<float> x = psi, y0 = ysave, g0 = g, xp0 = xprev;
    AccelParams p;
    std::memset(&p, 0, sizeof(p));
    p.psi = psi.data(), p.ysave = ysave.data(), p.g = g.data(), p.xprev = xprev.data();
    p.n = n, p.RP = RP, p.d2 = d2, p.first = k == 1, p.rec = rec.data(), p.alpha = &alpha, p.min_value = min_value;
    mvn_accel_host_a(p);
    mvn_accel_host_reduce(rec.data(), nrec, &alpha);
    mvn_accel_host_b(p);
    // the plain loop
    double num = 0., den = 0.;
    for (long r = 0; r < rows; ++r)
      for (int c = 0; c < d2; ++c) {
        const long i = r * RP + c;
        const float gi = x[i] - y0[i];
        if (k > 1) num += (double)gi * (double)g0[i], den += (double)g0[i] * (double)g0[i];
        if (g[i] != gi) ++bad;
        float yi = x[i];
        if (k > 1) {
          const float d = x[i] - xp0[i];
          const float t = x[i] + alpha * d;
          yi = t > min_value ? t : min_value;
        }
        if (psi[i] != yi || ysave[i] != yi || xprev[i] != x[i]) ++bad;
      }
    double want = den == 0. ? 0. : num / den;
    want = want < 0. ? 0. : (want > 1. ? 1. : want);
    if (std::fabs((double)alpha - want) > 1e-6) ++bad;  // (another order of summation, one rounding to float32)
    if (k == 1 && alpha != 0.f) ++bad;
    if (RP != d2)  // the row padding is neither read into a sum nor written
      for (long r = 0; r < rows; ++r)
        if (psi[r * RP + d2] != pad || ysave[r * RP + d2] != pad || g[r * RP + d2] != pad || xprev[r * RP + d2] != pad) ++bad;
    std::printf("(%d, %d, %d) sweep %d: alpha %.7f (plain loop %.7f), %d mismatches so far\n", d0, d1, d2, k,
                (double)alpha, want, bad);
  }
  return bad;
}

int main() {
  int bad = 0;
  bad += check(10, 14, 45);
  bad += check(3, 5, 2);
  bad += check(5, 4, 46);
  bad += check(9, 16, 64);  // more than one workgroup, full 16-byte trips
  std::printf(bad ? "MISMATCH\n" : "ok\n");
  return bad ? 1 : 0;
}
