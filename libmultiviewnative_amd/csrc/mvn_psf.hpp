// mvn_psf.hpp -- a view's two kernels from its raw PSF: the passes behind mvn_derive_kernels.
//
// include/mvn_engine_api.h states the arithmetic (mvn_derive_kernels).  Every array here is DENSE float32 of odd extents
// E with centre c = (E - 1) / 2, indexed by the offset d from the centre; a value outside an array is 0, and
// flip(P)(d) = P(-d) is the array read backwards: flip(P)[i] = P[n - 1 - i].
//
//   k_psf_sum / k_psf_scale   normalisation, for `count` arrays of n elements that lie one behind the other.  The sum
//                      S is formed in double in two steps that need no barrier and no atomics: MVN_PSF_WG partial sums
//                      per array (work item t adds elements t, t + MVN_PSF_WG, ...), which every work item of the scale
//                      pass adds up again in the same order - a wave-uniform read of MVN_PSF_WG doubles from the cache -
//                      before it writes (float)((double)q[i] / S).  S itself is left in p.sums for the host, which
//                      refuses S <= 0 and a non-finite S.
//   k_psf_pointwise    T_v = flip(P_v), times the V - 1 cropped correlations C_vw (w != v, view order) or V - 1 more
//                      factors flip(P_v): float32 multiplies, each rounded once.
//   k_psf_correlate    corr(a, b)(d) = sum over t of (double)a(-t) * (double)b(d - t), t over a's offsets in raster
//                      order (t_0 outermost, ascending), terms whose d - t lies outside b skipped, the sum held in
//                      double from +0.0 and rounded to float32 once.  One launch takes all the jobs of a stage: the
//                      records (a, b, out and their extents) lie in a device table read through the constant address
//                      space, and every job of a launch has the same output extents, so a workgroup finds its job by
//                      one division.  A work item owns ONE output voxel, consecutive along the last axis across the
//                      lanes, and walks the taps itself: no atomics, no cross-lane sum, the order is the definition's.
//                      a(-t) has the same address in every lane - a scalar load and one conversion per tap and wave -
//                      and b(d - t) is contiguous across the lanes of a row.  The loops over t_0 and t_1 run over the
//                      taps that ANY lane of the wave can use (the wave's 64 outputs span at most two planes; inside
//                      one plane the rows they span are known): bounds formed from the workgroup's number and the
//                      wave's alone, so they stay in scalar registers.  A lane whose d - t is outside b loads b's
//                      element from a clamped (valid) address and adds a (+/-)0 product instead, which leaves a sum
//                      that started from +0.0 as it is - the kernels are finite (the host checks the raw PSFs and S).
//                      b is NOT staged through the LDS: the halo of a tile is as wide as the PSF itself (a tile of 64
//                      outputs along a row of 31 needs 2 x 30 further elements on each of the three axes), b is at most
//                      (2K - 1)^3 floats - under 1 MiB at K = (33, 31, 31) - and is read by every workgroup of the job,
//                      so it lives in the L2 and, per row, in the vector L1; an LDS copy would add a barrier per tile
//                      of taps and take the occupancy that hides the load latency here.
//
// The bodies are plain C++ shared with the host emulation (mvn_backend_emu.cpp), like every other pass.
#pragma once

#include <stdint.h>

#include <stdexcept>

#include "mvn_resample.hpp"

#define MVN_PSF_WG 256    // work items of a workgroup, in all four passes
#define MVN_PSF_WAVE 64
#define MVN_PSF_MAX 257   // largest extent of a derived kernel (an autocorrelation then has 513)

// the kernel types of mvn_derive_kernels (include/mvn_engine_api.h)
enum { PSF_INDEPENDENT = 0, PSF_EFFICIENT_BAYESIAN = 1, PSF_OPTIMIZATION_I = 2, PSF_OPTIMIZATION_II = 3 };

// one correlation: 64 bytes
struct PsfJob {
  const float* a;  // the taps
  const float* b;  // the array they slide over
  float* out;
  int ea[3], eb[3], eo[3];  // extents, all odd
  int reserved;
};
static_assert(sizeof(PsfJob) == 64, "the table of a stage is njobs records of 64 bytes");

struct PsfCorrParams {
  const PsfJob* jobs;  // device table
  int njobs;
  int blocks_per_job;  // ceil(prod eo / MVN_PSF_WG): the same for every job of a launch
};

struct PsfNormParams {
  const float* src;  // count arrays of n floats, one behind the other
  float* dst;        // likewise (may be src)
  double* partial;   // count * MVN_PSF_WG doubles
  double* sums;      // count doubles: S of every array
  long n;
  int count;
};

struct PsfPointParams {
  const float* P;  // V kernels of n floats (kernel1)
  const float* C;  // V * (V - 1) cropped correlations of n floats, C_vw at v * (V - 1) + (w < v ? w : w - 1)
  float* T;        // V products of n floats
  long n;
  int V;
  int type;
};

#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
// read-only for the whole launch and the same address in every lane: scalar loads
typedef const __attribute__((address_space(4))) PsfJob* mvn_psf_table_t;
typedef const __attribute__((address_space(4))) float* mvn_psf_taps_t;
#define MVN_PSF_TABLE(p) ((mvn_psf_table_t)(p))
#define MVN_PSF_TAPS(p) ((mvn_psf_taps_t)(p))
#define MVN_PSF_UNIFORM(v) mvn_uniform(v)
#else
typedef const PsfJob* mvn_psf_table_t;
typedef const float* mvn_psf_taps_t;
#define MVN_PSF_TABLE(p) (p)
#define MVN_PSF_TAPS(p) (p)
#define MVN_PSF_UNIFORM(v) (v)
#endif

inline void mvn_psf_job_check(const PsfJob& j) {
  if (!j.a || !j.b || !j.out) throw std::invalid_argument("mvn: psf: null pointer");
  for (int k = 0; k < 3; ++k) {
    const int e[3] = {j.ea[k], j.eb[k], j.eo[k]};
    for (int i = 0; i < 3; ++i)
      if (e[i] < 1 || !(e[i] & 1) || e[i] > 2 * MVN_PSF_MAX - 1)
        throw std::invalid_argument("mvn: psf: extents must be odd and at most 513");
  }
}

MVN_HD long mvn_psf_blocks(long n) { return (n + MVN_PSF_WG - 1) / MVN_PSF_WG; }

inline void mvn_psf_norm_check(const PsfNormParams& p) {
  if (!p.src || !p.dst || !p.partial || !p.sums) throw std::invalid_argument("mvn: psf: null pointer");
  if (p.n < 1 || p.count < 1) throw std::invalid_argument("mvn: psf: nothing to normalise");
}
inline void mvn_psf_point_check(const PsfPointParams& p) {
  if (!p.P || !p.T || p.n < 1 || p.V < 1) throw std::invalid_argument("mvn: psf: nothing to multiply");
  if (p.type < PSF_INDEPENDENT || p.type > PSF_OPTIMIZATION_II) throw std::invalid_argument("mvn: psf: unknown kernel type");
  if ((p.type == PSF_EFFICIENT_BAYESIAN || p.type == PSF_OPTIMIZATION_I) && p.V > 1 && !p.C)
    throw std::invalid_argument("mvn: psf: null pointer");
}
// (the records themselves are checked on the host before they are uploaded: mvn_psf_job_check)
inline void mvn_psf_corr_check(const PsfCorrParams& p) {
  if (!p.jobs || p.njobs < 1 || p.blocks_per_job < 1) throw std::invalid_argument("mvn: psf: no correlations");
}

// ---- normalisation ---------------------------------------------------------------------------------------------------
// block: the array
MVN_HD void mvn_psf_sum_item(const PsfNormParams& p, long block, int tid) {
  const float* s = p.src + block * p.n;
  double acc = 0.0;
  for (long i = tid; i < p.n; i += MVN_PSF_WG) acc = acc + (double)s[i];
  p.partial[block * MVN_PSF_WG + tid] = acc;
}

MVN_HD void mvn_psf_scale_item(const PsfNormParams& p, long block, int tid) {
  const long bpa = mvn_psf_blocks(p.n);
  const long arr = block / bpa, blk = block - arr * bpa;
  const double* part = p.partial + arr * MVN_PSF_WG;
  double S = 0.0;
  for (int k = 0; k < MVN_PSF_WG; ++k) S = S + part[k];
  if (blk == 0 && tid == 0) p.sums[arr] = S;
  const long i = blk * MVN_PSF_WG + tid;
  if (i < p.n) p.dst[arr * p.n + i] = (float)((double)p.src[arr * p.n + i] / S);
}

// ---- flip and running product ----------------------------------------------------------------------------------------
MVN_HD void mvn_psf_pointwise_item(const PsfPointParams& p, long block, int tid) {
  const long bpa = mvn_psf_blocks(p.n);
  const long v = block / bpa, i = (block - v * bpa) * MVN_PSF_WG + tid;
  if (i >= p.n) return;
  float t = p.P[v * p.n + (p.n - 1 - i)];
  if ((p.type == PSF_EFFICIENT_BAYESIAN || p.type == PSF_OPTIMIZATION_I) && p.V > 1) {
    const float* c = p.C + v * (p.V - 1) * p.n + i;
    for (int w = 0; w < p.V - 1; ++w) t = t * c[w * p.n];
  } else if (p.type == PSF_OPTIMIZATION_II) {
    const float f = t;
    for (int w = 1; w < p.V; ++w) t = t * f;
  }
  p.T[v * p.n + i] = t;
}

// ---- correlation -----------------------------------------------------------------------------------------------------
MVN_HD int mvn_psf_max(int a, int b) { return a > b ? a : b; }
MVN_HD int mvn_psf_min(int a, int b) { return a < b ? a : b; }

// U consecutive taps t2, t2 + 1, ... of one row of a: a(-t) walks DOWN from `a`, b's last index down from b2
template <int U>
MVN_HD double mvn_psf_taps(double acc, mvn_psf_taps_t a, const float* brow, int b2, int eb2, bool ok1) {
  float av[U], bv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = b2 - u;
    bv[u] = brow[mvn_psf_min(mvn_psf_max(i, 0), eb2 - 1)];
    av[u] = a[-u];
  }
  // a lane outside b keeps +0 of what it loaded: masked as bits, so that no load waits behind a branch
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = b2 - u;
    const unsigned keep = 0u - (unsigned)((int)ok1 & (int)(i >= 0) & (int)(i < eb2));
    unsigned bits;
    __builtin_memcpy(&bits, &bv[u], sizeof(bits));
    bits &= keep;
    __builtin_memcpy(&bv[u], &bits, sizeof(bits));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) acc = acc + (double)av[u] * (double)bv[u];
  return acc;
}

MVN_HD void mvn_psf_correlate_item(const PsfCorrParams& p, long block, int tid) {
  const int job = (int)(block / p.blocks_per_job), blk = (int)(block - (long)job * p.blocks_per_job);
  const mvn_psf_table_t J = MVN_PSF_TABLE(p.jobs) + job;
  const int ea0 = J->ea[0], ea1 = J->ea[1], ea2 = J->ea[2];
  const int eb0 = J->eb[0], eb1 = J->eb[1], eb2 = J->eb[2];
  const int eo0 = J->eo[0], eo1 = J->eo[1], eo2 = J->eo[2];
  const int ca0 = ea0 / 2, ca1 = ea1 / 2, ca2 = ea2 / 2;
  const int cb0 = eb0 / 2, cb1 = eb1 / 2, cb2 = eb2 / 2;
  const int co0 = eo0 / 2, co1 = eo1 / 2, co2 = eo2 / 2;
  const int plane = eo1 * eo2, nout = eo0 * plane;
  // the wave's outputs [first, last]: everything up to `o` is the same in every lane
  const int wave = MVN_PSF_UNIFORM(tid / MVN_PSF_WAVE), lane = tid % MVN_PSF_WAVE;
  const int first = blk * MVN_PSF_WG + wave * MVN_PSF_WAVE;
  if (first >= nout) return;
  const int last = mvn_psf_min(first + MVN_PSF_WAVE - 1, nout - 1);
  const int zf = first / plane, zl = last / plane;
  int t0lo = mvn_psf_max(-ca0, (zf - co0) - cb0), t0hi = mvn_psf_min(ca0, (zl - co0) + cb0);
  int t1lo = -ca1, t1hi = ca1;
  if (zf == zl) {  // one plane: the rows between the first and the last output
    const int yf = (first - zf * plane) / eo2, yl = (last - zf * plane) / eo2;
    t1lo = mvn_psf_max(t1lo, (yf - co1) - cb1), t1hi = mvn_psf_min(t1hi, (yl - co1) + cb1);
  }
  // this lane's output (a lane past the end repeats the last one and stores nothing)
  const int o = mvn_psf_min(first + lane, last);
  const int z = o / plane, rem = o - z * plane;
  const int y = rem / eo2, x = rem - y * eo2;
  const int d0 = z - co0, d1 = y - co1, d2 = x - co2;
  const mvn_psf_taps_t a = MVN_PSF_TAPS(J->a);
  const float* b = J->b;
  const int x2 = d2 + cb2;  // b's last index is x2 - t2
  double acc = 0.0;
  for (int t0 = t0lo; t0 <= t0hi; ++t0) {
    const int b0 = d0 - t0 + cb0;
    const bool ok0 = b0 >= 0 && b0 < eb0;
    for (int t1 = t1lo; t1 <= t1hi; ++t1) {
      const int b1 = d1 - t1 + cb1;
      const bool ok1 = ok0 && b1 >= 0 && b1 < eb1;
      const float* brow = b + ((long)(ok1 ? b0 : 0) * eb1 + (ok1 ? b1 : 0)) * eb2;
      const int arow = ((ca0 - t0) * ea1 + (ca1 - t1)) * ea2 + ca2;  // a(-t) is a[arow - t2]
      // groups of 8, then 4, then single taps: the loads of a group are issued together, its terms added in order
      int t2 = -ca2;
      for (; t2 + 7 <= ca2; t2 += 8) acc = mvn_psf_taps<8>(acc, a + (arow - t2), brow, x2 - t2, eb2, ok1);
      if (t2 + 3 <= ca2) acc = mvn_psf_taps<4>(acc, a + (arow - t2), brow, x2 - t2, eb2, ok1), t2 += 4;
      for (; t2 <= ca2; ++t2) acc = mvn_psf_taps<1>(acc, a + (arow - t2), brow, x2 - t2, eb2, ok1);
    }
  }
  if (first + lane <= last) J->out[o] = (float)acc;
}
