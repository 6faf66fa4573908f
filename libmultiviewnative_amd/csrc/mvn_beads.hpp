// mvn_beads.hpp -- a view's PSF from its beads: the passes behind mvn_extract_psf.
//
// include/mvn_engine_api.h states the arithmetic (mvn_extract_psf).  The raw stack (uint16 or float32, element strides)
// of extents m is read where it lies; the PSF is DENSE float32 of odd extents r with h = (r - 1) / 2, n = prod r voxels.
// A bead is a record of 32 bytes made on the host: B_k = floor(p_k), f_k = (float)(p_k - B_k), and one bit that says
// that the whole window plus one lies inside the stack (B_k - h_k >= 0 and B_k + h_k + 1 <= m_k - 1 for every k).
//
//   k_beads_gather<T>   the work: per PSF voxel j and bead b the trilinear sample s_b(j) of the cell whose low corner is
//                       B + (j - h), mirrored into the stack ("reflect": no repeated edge sample, any number of
//                       reflections).  The grid is (groups of MVN_BEADS_GROUP beads) x (tiles of MVN_BEADS_WG voxels);
//                       a work item owns ONE voxel, consecutive along the last axis across the lanes, so the two
//                       x-neighbours of a row are coalesced reads that adjacent lanes share.  The records are read
//                       through the constant address space with an index formed from the workgroup's number and the
//                       loop counter: scalar loads, and B, f and the bead's base address stay in scalar registers.  The
//                       window is a pure translation, so a lane's offset into it, (j - h) . strides, is formed once in
//                       front of the bead loop; per bead an INTERIOR bead costs one 64-bit add and eight loads, and
//                       only a bead near a face (a wave-uniform branch) takes the mirror's two remainders per axis.
//                       The sum over the group's beads is held in a double register, in bead order from +0.0, and
//                       written to partial[g][j]: no atomics, no barrier, the order is the definition's.  The groups
//                       are what fills the device - n is 7 k to 30 k voxels, 27 to 117 workgroups - which is why the
//                       group size is part of the arithmetic and no tuning knob.
//   k_beads_reduce      T(j) = ((P_0 + P_1) + ...) + P_{G-1} in group order, psf(j) = (float)(T / num_beads), and a flag
//                       word that any work item with a non-finite result sets.
//   k_beads_min / k_beads_sub   MVN_BEADS_REMOVE_MIN, k_psf_sum / k_psf_scale's scheme: MVN_BEADS_WG partial minima (work
//                       item t takes elements t, t + MVN_BEADS_WG, ...) that every work item of the subtract pass folds
//                       itself - no order matters for a minimum - before it writes psf(j) - mn.
//   k_beads_score / k_beads_score_fold   Pearson's correlation of each bead's window with the mean.  One workgroup per
//                       bead; work item t adds the five double sums over the voxels t, t + MVN_BEADS_WG, ... - the
//                       samples recomputed from the raw stack by the gather's own device function - into a record of
//                       its own, and the second pass, one work item per bead, folds the bead's MVN_BEADS_WG records in
//                       index order and forms the score.  No barrier and no atomics here either.
//
// The bodies are plain C++ shared with the host emulation (mvn_backend_emu.cpp), like every other pass; they switch
// contraction off as mvn_resample.hpp does.
#pragma once

#include <math.h>
#include <stdint.h>

#include <stdexcept>

#include "mvn_resample.hpp"

#define MVN_BEADS_WG 256     // work items of a workgroup, in every pass
#define MVN_BEADS_PER_GROUP 32  // beads per partial sum (MVN_BEADS_GROUP of the header: part of the arithmetic)
#define MVN_BEADS_MAX 129    // largest extent of an extracted PSF
#define MVN_BEADS_SUMS 5     // sum s, sum s^2, sum P, sum P^2, sum sP

// one bead: 32 bytes
struct BeadRec {
  int B[3];    // floor of the position
  float f[3];  // its fraction
  int interior;  // the window plus one lies inside the stack: no mirror
  int reserved;
};
static_assert(sizeof(BeadRec) == 32, "the table of a view is num_beads records of 32 bytes");

struct BeadsParams {
  const void* src;       // element (0, 0, 0) of the raw stack
  long long s0, s1, s2;  // its element strides (>= 0)
  int m[3];              // its extents
  int r[3];              // extents of the PSF, odd
  const BeadRec* beads;  // device table
  int nbeads;
  double* partial;       // [groups][n]
  float* psf;            // n
  float* minima;         // MVN_BEADS_WG partial minima (REMOVE_MIN)
  unsigned* flag;        // set to 1 by a non-finite result
  double* records;       // [nbeads][MVN_BEADS_WG][MVN_BEADS_SUMS] (scores)
  double* scores;        // nbeads (scores)
};

#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
// read-only for the whole launch and the same address in every lane: scalar loads
typedef const __attribute__((address_space(4))) BeadRec* mvn_beads_table_t;
#define MVN_BEADS_TABLE(p) ((mvn_beads_table_t)(p))
#else
typedef const BeadRec* mvn_beads_table_t;
#define MVN_BEADS_TABLE(p) (p)
#endif

MVN_HD long mvn_beads_voxels(const BeadsParams& p) { return (long)p.r[0] * p.r[1] * p.r[2]; }
MVN_HD long mvn_beads_tiles(const BeadsParams& p) { return (mvn_beads_voxels(p) + MVN_BEADS_WG - 1) / MVN_BEADS_WG; }
MVN_HD int mvn_beads_groups(int nbeads) { return (nbeads + MVN_BEADS_PER_GROUP - 1) / MVN_BEADS_PER_GROUP; }

inline void mvn_beads_check(const BeadsParams& p) {
  if (!p.src || !p.beads || !p.partial || !p.psf || !p.flag) throw std::invalid_argument("mvn: beads: null pointer");
  if (p.nbeads < 1) throw std::invalid_argument("mvn: beads: no beads");
  if (p.s0 < 0 || p.s1 < 0 || p.s2 < 0) throw std::invalid_argument("mvn: beads: negative stride");
  for (int k = 0; k < 3; ++k) {
    if (p.m[k] < 1 || p.m[k] > 0x3fffffff) throw std::invalid_argument("mvn: beads: raw extents must be in 1..2^30 - 1");
    if (p.r[k] < 1 || !(p.r[k] & 1) || p.r[k] > MVN_BEADS_MAX)
      throw std::invalid_argument("mvn: beads: PSF extents must be odd and at most 129");
  }
}

// the mirror without repeating the edge sample (numpy.pad's "reflect"), for any i
MVN_HD int mvn_beads_mir(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  int q = i % period;
  if (q < 0) q += period;
  return q < n ? q : period - q;
}

// mvn_view_geometry's trilinear rule on the eight samples at q + {lo0, hi0} + {lo1, hi1} + {lo2, hi2}
template <typename T>
MVN_HD float mvn_beads_trilerp(const T* q, long long lo0, long long hi0, long long lo1, long long hi1, long long lo2,
                               long long hi2, float f0, float f1, float f2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const T* q0 = q + lo0;
  const T* q1 = q + hi0;
  const float v000 = (float)q0[lo1 + lo2], v001 = (float)q0[lo1 + hi2];
  const float v010 = (float)q0[hi1 + lo2], v011 = (float)q0[hi1 + hi2];
  const float v100 = (float)q1[lo1 + lo2], v101 = (float)q1[lo1 + hi2];
  const float v110 = (float)q1[hi1 + lo2], v111 = (float)q1[hi1 + hi2];
  const float a00 = mvn_resample_lerp(v000, v001, f2), a01 = mvn_resample_lerp(v010, v011, f2);
  const float a10 = mvn_resample_lerp(v100, v101, f2), a11 = mvn_resample_lerp(v110, v111, f2);
  const float b0 = mvn_resample_lerp(a00, a01, f1), b1 = mvn_resample_lerp(a10, a11, f1);
  return mvn_resample_lerp(b0, b1, f0);
}

// s_b(j) of bead `b` for the PSF voxel at offset d = j - h from the centre; off = d . strides
template <typename T>
MVN_HD float mvn_beads_sample(const BeadsParams& p, mvn_beads_table_t b, int d0, int d1, int d2, long long off) {
  const int B0 = b->B[0], B1 = b->B[1], B2 = b->B[2];
  const float f0 = b->f[0], f1 = b->f[1], f2 = b->f[2];
  const T* s = (const T*)p.src;
  if (b->interior) {  // (the same in every lane)
    const long long base = ((long long)B0 * p.s0 + (long long)B1 * p.s1) + (long long)B2 * p.s2;
    return mvn_beads_trilerp<T>(s + (base + off), 0, p.s0, 0, p.s1, 0, p.s2, f0, f1, f2);
  }
  const int i0 = B0 + d0, i1 = B1 + d1, i2 = B2 + d2;
  return mvn_beads_trilerp<T>(s, mvn_beads_mir(i0, p.m[0]) * p.s0, mvn_beads_mir(i0 + 1, p.m[0]) * p.s0,
                              mvn_beads_mir(i1, p.m[1]) * p.s1, mvn_beads_mir(i1 + 1, p.m[1]) * p.s1,
                              mvn_beads_mir(i2, p.m[2]) * p.s2, mvn_beads_mir(i2 + 1, p.m[2]) * p.s2, f0, f1, f2);
}

// voxel j of the PSF as its offset from the centre, and that offset in elements of the raw stack
MVN_HD long long mvn_beads_offset(const BeadsParams& p, int j, int* d0, int* d1, int* d2) {
  const int plane = p.r[1] * p.r[2];
  const int j0 = j / plane, rem = j - j0 * plane;
  const int j1 = rem / p.r[2], j2 = rem - j1 * p.r[2];
  *d0 = j0 - p.r[0] / 2, *d1 = j1 - p.r[1] / 2, *d2 = j2 - p.r[2] / 2;
  return ((long long)*d0 * p.s0 + (long long)*d1 * p.s1) + (long long)*d2 * p.s2;
}

// ---- the gather ------------------------------------------------------------------------------------------------------
// block: group * tiles + tile
template <typename T>
MVN_HD void mvn_beads_gather_item(const BeadsParams& p, long block, int tid) {
  const int n = (int)mvn_beads_voxels(p);
  const long tiles = mvn_beads_tiles(p);
  const int g = (int)(block / tiles), tile = (int)(block - (long)g * tiles);
  const int j = tile * MVN_BEADS_WG + tid;
  // (a lane past the end repeats the last voxel and stores nothing)
  int d0, d1, d2;
  const long long off = mvn_beads_offset(p, j < n ? j : n - 1, &d0, &d1, &d2);
  const int first = g * MVN_BEADS_PER_GROUP;
  const int last = first + MVN_BEADS_PER_GROUP < p.nbeads ? first + MVN_BEADS_PER_GROUP : p.nbeads;
  const mvn_beads_table_t table = MVN_BEADS_TABLE(p.beads);
  double acc = 0.0;
  for (int b = first; b < last; ++b) acc = acc + (double)mvn_beads_sample<T>(p, table + b, d0, d1, d2, off);
  if (j < n) p.partial[(long)g * n + j] = acc;
}

// ---- the sum over the groups, the mean ----------------------------------------------------------------------------------
MVN_HD bool mvn_beads_finite(float v) {
  unsigned bits;
  __builtin_memcpy(&bits, &v, sizeof(bits));
  return (bits & 0x7f800000u) != 0x7f800000u;
}

MVN_HD void mvn_beads_reduce_item(const BeadsParams& p, long block, int tid) {
  const long n = mvn_beads_voxels(p);
  const long j = block * MVN_BEADS_WG + tid;
  if (j >= n) return;
  const int G = mvn_beads_groups(p.nbeads);
  double t = p.partial[j];
  for (int g = 1; g < G; ++g) t = t + p.partial[(long)g * n + j];
  const float v = (float)(t / (double)p.nbeads);
  p.psf[j] = v;
  if (!mvn_beads_finite(v)) *p.flag = 1u;
}

// ---- MVN_BEADS_REMOVE_MIN --------------------------------------------------------------------------------------------
// one workgroup
MVN_HD void mvn_beads_min_item(const BeadsParams& p, int tid) {
  const long n = mvn_beads_voxels(p);
  float mn = INFINITY;
  for (long i = tid; i < n; i += MVN_BEADS_WG) {
    const float v = p.psf[i];
    mn = v < mn ? v : mn;
  }
  p.minima[tid] = mn;
}

MVN_HD void mvn_beads_sub_item(const BeadsParams& p, long block, int tid) {
  const long n = mvn_beads_voxels(p);
  float mn = p.minima[0];
  for (int k = 1; k < MVN_BEADS_WG; ++k) mn = p.minima[k] < mn ? p.minima[k] : mn;
  const long j = block * MVN_BEADS_WG + tid;
  if (j < n) p.psf[j] = p.psf[j] - mn;
}

// ---- scores ----------------------------------------------------------------------------------------------------------
// block: the bead
template <typename T>
MVN_HD void mvn_beads_score_item(const BeadsParams& p, long block, int tid) {
  const int n = (int)mvn_beads_voxels(p);
  const mvn_beads_table_t b = MVN_BEADS_TABLE(p.beads) + block;
  double ss = 0.0, ss2 = 0.0, sp = 0.0, sp2 = 0.0, ssp = 0.0;
  for (int j = tid; j < n; j += MVN_BEADS_WG) {
    int d0, d1, d2;
    const long long off = mvn_beads_offset(p, j, &d0, &d1, &d2);
    const double s = (double)mvn_beads_sample<T>(p, b, d0, d1, d2, off);
    const double P = (double)p.psf[j];
    ss = ss + s, ss2 = ss2 + s * s, sp = sp + P, sp2 = sp2 + P * P, ssp = ssp + s * P;
  }
  double* rec = p.records + ((long)block * MVN_BEADS_WG + tid) * MVN_BEADS_SUMS;
  rec[0] = ss, rec[1] = ss2, rec[2] = sp, rec[3] = sp2, rec[4] = ssp;
}

// one work item per bead
MVN_HD void mvn_beads_score_fold_item(const BeadsParams& p, long block, int tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long bead = block * MVN_BEADS_WG + tid;
  if (bead >= p.nbeads) return;
  const double* rec = p.records + bead * MVN_BEADS_WG * MVN_BEADS_SUMS;
  double a[MVN_BEADS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t < MVN_BEADS_WG; ++t)
    for (int q = 0; q < MVN_BEADS_SUMS; ++q) a[q] = a[q] + rec[t * MVN_BEADS_SUMS + q];
  const double n = (double)mvn_beads_voxels(p);
  const double cov = a[4] - a[0] * a[2] / n;
  const double vs = a[1] - a[0] * a[0] / n, vp = a[3] - a[2] * a[2] / n;
  const double den = sqrt(vs * vp);
  p.scores[bead] = (den > 0.0 && den <= 1.7976931348623157e308) ? cov / den : 0.0;  // (a NaN fails both)
}
