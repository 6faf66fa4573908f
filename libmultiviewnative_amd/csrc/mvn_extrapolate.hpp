// mvn_extrapolate.hpp -- vector extrapolation between Richardson-Lucy sweeps (Biggs & Andrews 1997, first order).
//
// The sequential sweep stays as it is; between two sweeps the engine moves the estimate along the direction of the
// last change (Engine::iterate_sweeps, acceleration on):
//
//   x_k = Sweep(y_{k-1})            g_k = x_k - y_{k-1}                                (float32)
//   a_k = clamp(sum g_k g_{k-1} / sum g_{k-1} g_{k-1}, 0, 1)                           (double, then float32)
//   t   = x_k + a_k (x_k - x_{k-1})      y_k = t > minValue ? t : minValue             (float32, no contraction)
//
// with a_1 = 0 and y_1 = x_1.  Three launches per sweep boundary:
//
//   k_accel_a<W>     pass A.  Reads psi (x_k), the saved y_{k-1} and g_{k-1}; writes g_k over g_{k-1}; every lane sums
//                    the two dot products in double, the workgroup reduces its 256 lanes in a fixed order through the
//                    LDS and stores ONE record {num, den} with plain stores.
//   k_accel_reduce   one workgroup sums the records in a fixed order and leaves a_k, clamped and rounded to float32,
//                    in a device word.  The host never waits for it.
//   k_accel_b<W>     pass B.  Reads psi, x_{k-1} and that word; writes y_k into psi and into the saved copy, x_k into
//                    the x_prev volume.
//
// Both passes are one-shot 256-lane workgroups in address order (the fastest way to launch a
// streaming skeleton); a workgroup owns MVN_ACCEL_CHUNK * W consecutive floats, a lane W of them per trip.  W = 4
// (16-byte accesses) for an even last extent, whose volume is contiguous; W = 2 for an odd one, whose rows carry one
// float of padding that is neither summed nor written: a pair never straddles a row because the pitch is even.  The
// grid - and with it the order of every sum - depends on the extents only.  No atomics and no cross-lane
// instructions: the host emulation runs the same bodies, lane after lane, and sums in the same order.
#pragma once

#include "mvn_pass_bodies.hpp"

#define MVN_ACCEL_WG 256     // lanes of a workgroup
#define MVN_ACCEL_TRIPS 4    // accesses of a lane
#define MVN_ACCEL_CHUNK (MVN_ACCEL_WG * MVN_ACCEL_TRIPS)  // accesses of a workgroup

struct AccelParams {
  float* psi;          // in: x_k; pass B leaves y_k
  float* ysave;        // y_{k-1}; pass B leaves y_k
  float* g;            // g_{k-1}; pass A leaves g_k
  float* xprev;        // x_{k-1}; pass B leaves x_k
  long n;              // floats of a volume, row padding included
  int RP, d2;          // row pitch and last extent (RP == d2, or d2 + 1 for an odd d2)
  int first;           // sweep 1: there is no g_0 and no x_0 - both sums are 0, and y_1 = x_1
  double* rec;         // pass A: 2 doubles per workgroup
  const float* alpha;  // pass B: a_k
  float min_value;
};

typedef float mvn_accel_v4 __attribute__((vector_size(16)));
typedef float mvn_accel_v2 __attribute__((vector_size(8)));
template <int W>
struct AccelVec;
template <>
struct AccelVec<4> {
  typedef mvn_accel_v4 type;
};
template <>
struct AccelVec<2> {
  typedef mvn_accel_v2 type;
};

// workgroups of a pass over n floats, W per access
MVN_HD long mvn_accel_blocks(long n, int W) {
  const long per = (long)MVN_ACCEL_CHUNK * W;
  return (n + per - 1) / per;
}

// how many of the W floats at i a lane owns: the tail of the volume (W = 4), the padding of an odd row (W = 2)
template <int W>
MVN_HD int mvn_accel_width(const AccelParams& p, long i) {
  if (W == 4) return p.n - i >= 4 ? 4 : (int)(p.n - i);
  return (int)(i % p.RP) + 1 < p.d2 ? 2 : 1;
}

MVN_HD float mvn_accel_step(float x, float xp, float a, float min_value) {
  MVN_FP_EXACT
  const float d = x - xp;
  const float t = x + a * d;
  return t > min_value ? t : min_value;  // (a NaN becomes minValue, as in the update's own clamp)
}

// lanes tid, tid + nthreads, ... of workgroup `block`; lds: 2 * MVN_ACCEL_WG doubles
template <int W>
MVN_HD void mvn_accel_a_body(const AccelParams& p, long block, double* lds, int tid, int nthreads) {
  typedef typename AccelVec<W>::type V;
  for (int t = tid; t < MVN_ACCEL_WG; t += nthreads) {
    double num = 0., den = 0.;
#pragma unroll
    for (int u = 0; u < MVN_ACCEL_TRIPS; ++u) {
      const long i = ((block * MVN_ACCEL_TRIPS + u) * MVN_ACCEL_WG + t) * W;
      if (i >= p.n) continue;
      const int w = mvn_accel_width<W>(p, i);
      if (w == W) {
        const V x = *reinterpret_cast<const V*>(p.psi + i);
        const V y = *reinterpret_cast<const V*>(p.ysave + i);
        V gp = {};
        if (!p.first) gp = *reinterpret_cast<const V*>(p.g + i);
        V g;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          g[j] = x[j] - y[j];
          num += (double)g[j] * (double)gp[j];
          den += (double)gp[j] * (double)gp[j];
        }
        *reinterpret_cast<V*>(p.g + i) = g;
      } else {
        for (int j = 0; j < w; ++j) {
          const float g = p.psi[i + j] - p.ysave[i + j];
          const float gp = p.first ? 0.f : p.g[i + j];
          num += (double)g * (double)gp;
          den += (double)gp * (double)gp;
          p.g[i + j] = g;
        }
      }
    }
    lds[t] = num;
    lds[MVN_ACCEL_WG + t] = den;
  }
  MVN_SYNC();
  for (int h = MVN_ACCEL_WG >> 1; h > 0; h >>= 1) {
    for (int t = tid; t < h; t += nthreads) {
      lds[t] += lds[t + h];
      lds[MVN_ACCEL_WG + t] += lds[MVN_ACCEL_WG + t + h];
    }
    MVN_SYNC();
  }
  if (tid == 0) {
    p.rec[2 * block] = lds[0];
    p.rec[2 * block + 1] = lds[MVN_ACCEL_WG];
  }
}

// the clamp of a_k: 0 for an empty or non-finite ratio
MVN_HD float mvn_accel_alpha(double num, double den) {
  double r = den == 0. ? 0. : num / den;
  if (!((r - r) == 0.)) r = 0.;  // NaN or infinite
  r = r < 0. ? 0. : (r > 1. ? 1. : r);
  return (float)r;
}

// k_accel_reduce: lane t sums records t, t + 256, ..., then the lanes are reduced as above.  lds: 2 * 256 doubles
MVN_HD void mvn_accel_reduce_body(const double* rec, long nrec, float* alpha, double* lds, int tid, int nthreads) {
  for (int t = tid; t < MVN_ACCEL_WG; t += nthreads) {
    double num = 0., den = 0.;
    for (long i = t; i < nrec; i += MVN_ACCEL_WG) {
      num += rec[2 * i];
      den += rec[2 * i + 1];
    }
    lds[t] = num;
    lds[MVN_ACCEL_WG + t] = den;
  }
  MVN_SYNC();
  for (int h = MVN_ACCEL_WG >> 1; h > 0; h >>= 1) {
    for (int t = tid; t < h; t += nthreads) {
      lds[t] += lds[t + h];
      lds[MVN_ACCEL_WG + t] += lds[MVN_ACCEL_WG + t + h];
    }
    MVN_SYNC();
  }
  if (tid == 0) *alpha = mvn_accel_alpha(lds[0], lds[MVN_ACCEL_WG]);
}

template <int W>
MVN_HD void mvn_accel_b_body(const AccelParams& p, long block, int tid, int nthreads) {
  typedef typename AccelVec<W>::type V;
  const float a = p.first ? 0.f : *p.alpha;
  for (int t = tid; t < MVN_ACCEL_WG; t += nthreads) {
#pragma unroll
    for (int u = 0; u < MVN_ACCEL_TRIPS; ++u) {
      const long i = ((block * MVN_ACCEL_TRIPS + u) * MVN_ACCEL_WG + t) * W;
      if (i >= p.n) continue;
      const int w = mvn_accel_width<W>(p, i);
      if (w == W) {
        const V x = *reinterpret_cast<const V*>(p.psi + i);
        V y = x;
        if (!p.first) {
          const V xp = *reinterpret_cast<const V*>(p.xprev + i);
#pragma unroll
          for (int j = 0; j < W; ++j) y[j] = mvn_accel_step(x[j], xp[j], a, p.min_value);
          *reinterpret_cast<V*>(p.psi + i) = y;
        }
        *reinterpret_cast<V*>(p.ysave + i) = y;
        *reinterpret_cast<V*>(p.xprev + i) = x;
      } else {
        for (int j = 0; j < w; ++j) {
          const float x = p.psi[i + j];
          float y = x;
          if (!p.first) {
            y = mvn_accel_step(x, p.xprev[i + j], a, p.min_value);
            p.psi[i + j] = y;
          }
          p.ysave[i + j] = y;
          p.xprev[i + j] = x;
        }
      }
    }
  }
}

#ifdef MVN_HOST_EMU
// The launches of the host emulation (mvn_backend_emu.cpp; tools/accel_standalone.cpp runs them under sanitizers):
// one "lane" runs the 256 logical lanes of a workgroup in order, so the sums come out in the device's order.
inline void mvn_accel_host_a(const AccelParams& p) {
  const int W = p.RP == p.d2 ? 4 : 2;
  const long nblocks = mvn_accel_blocks(p.n, W);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    double lds[2 * MVN_ACCEL_WG];
    if (W == 4)
      mvn_accel_a_body<4>(p, blk, lds, 0, 1);
    else
      mvn_accel_a_body<2>(p, blk, lds, 0, 1);
  }
}

inline void mvn_accel_host_reduce(const double* rec, long nrec, float* alpha) {
  double lds[2 * MVN_ACCEL_WG];
  mvn_accel_reduce_body(rec, nrec, alpha, lds, 0, 1);
}

inline void mvn_accel_host_b(const AccelParams& p) {
  const int W = p.RP == p.d2 ? 4 : 2;
  const long nblocks = mvn_accel_blocks(p.n, W);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    if (W == 4)
      mvn_accel_b_body<4>(p, blk, 0, 1);
    else
      mvn_accel_b_body<2>(p, blk, 0, 1);
  }
}
#endif
