// mvn_detect.hpp -- a view's beads from its raw stack: the passes behind mvn_detect_beads.
//
// include/mvn_engine_api.h states the arithmetic (mvn_detect_beads): the difference of two separable Gaussian blurs of
// the raw stack, D = L_1 - L_2, its strict 26-neighbour extrema above a threshold in raster order, and a quadratic fit
// around each.  The raw stack (uint16 or float32, element strides) of extents m is read where it lies, ONCE; every
// other volume is DENSE float32 of extents m.  At most four such volumes exist: a[0], a[1] (the blurs along axis 2),
// b[0], b[1] (then along axis 1); the axis-0 pass writes D over a[0] and stores neither L.
//
//   k_detect_rows<T>    axis 2.  A workgroup takes MVN_DETECT_NR consecutive rows x one segment of MVN_DETECT_SEG
//                       voxels: it stages the segment plus a halo of R = max(R_1, R_2) on either side into the LDS -
//                       widened to float32, the mirror applied while staging, for any number of reflections - and a
//                       lane forms BOTH blurs of its voxel from that one copy (consecutive lanes read consecutive LDS
//                       words: no bank conflict) and writes a[0] and a[1].
//   k_detect_lines<AXIS>  axis 1, then axis 0: one body.  A workgroup owns a tile of MVN_DETECT_TX voxels along the
//                       last axis x MVN_DETECT_TL along the walked one (AXIS), at one index of the third.  Consecutive
//                       lanes run along the last axis in the global reads, the LDS accesses and the writes, so every
//                       access is a whole 256-byte run.  Per blur: the tile plus R_a lines on either side goes into
//                       the LDS (mirrored along AXIS), then a lane walks its MVN_DETECT_LK outputs down the column,
//                       taps in ascending order.  The results stay in registers until both blurs are done; AXIS == 1
//                       writes b[0] and b[1], AXIS == 0 writes D = L_1 - L_2 alone.
//   k_detect_extrema    walks planes of D like k_tv_factor: a tile of MVN_DETECT_EX x MVN_DETECT_EY voxels plus a
//                       one-voxel rim, three planes of it in an LDS ring, MVN_DETECT_ESEG planes per workgroup.  A
//                       voxel is compared with the threshold first - candidates are thousands in 10^9 voxels - and
//                       only then with its 26 neighbours.  A candidate's raster index is appended to a list through
//                       one atomic counter; the ORDER of that list is undefined and never reaches a result: the host
//                       sorts the indices (mvn_abi.cpp) before the fit, so the output is in raster order whatever the
//                       schedule.  Entries past the list's capacity are counted and dropped; the call then fails.
//   k_detect_refine     one work item per sorted candidate: the 27 values of E widened to double, the gradient, the
//                       Hessian, the cofactors and the determinant exactly as the header writes them out.
//
// The taps are made on the host (mvn_detect_make_taps, what mvn_detect_taps returns), uploaded as a table of
// 2 x 3 vectors of MVN_DETECT_TAPS floats and read through the constant address space with a workgroup-uniform index:
// scalar loads, as mvn_beads.hpp reads its records.
//
// No cross-lane instructions; the host emulation runs the same bodies with one "thread" that owns all the lanes of a
// workgroup (mvn_tv.hpp's form).  Every float32 and double operation is rounded once: contraction is off.
#pragma once

#include <math.h>
#include <stdint.h>

#include <stdexcept>

#include "mvn_beads.hpp"

#define MVN_DETECT_WG 256       // work items of a workgroup, in every pass
#define MVN_DETECT_RMAX 30      // largest radius: ceil(3 * 10) (MVN_DETECT_MAX_RADIUS of the header)
#define MVN_DETECT_TAPS 64      // floats of one tap vector in the table (>= 2 * MVN_DETECT_RMAX + 1)
#define MVN_DETECT_TABLE (2 * 3 * MVN_DETECT_TAPS)  // floats of the table: [blur a][axis k][tap]
#define MVN_DETECT_SEG 256      // row pass: voxels of a segment ...
#define MVN_DETECT_NR 4         // ... and rows of a workgroup
#define MVN_DETECT_RPITCH (MVN_DETECT_SEG + 2 * MVN_DETECT_RMAX)
#define MVN_DETECT_ROWS_LDS (MVN_DETECT_NR * MVN_DETECT_RPITCH)
#define MVN_DETECT_TX 64        // line passes: columns of a tile ...
#define MVN_DETECT_TL 64        // ... and its outputs along the walked axis
#define MVN_DETECT_LR (MVN_DETECT_WG / MVN_DETECT_TX)     // lines a workgroup covers at once
#define MVN_DETECT_LK (MVN_DETECT_TL / MVN_DETECT_LR)     // outputs of a lane
#define MVN_DETECT_LINES_LDS ((MVN_DETECT_TL + 2 * MVN_DETECT_RMAX) * MVN_DETECT_TX)
#define MVN_DETECT_EX 64        // extremum pass: columns ...
#define MVN_DETECT_EY 16        // ... and rows of a tile,
#define MVN_DETECT_ESEG 32      // planes a workgroup walks
#define MVN_DETECT_EK (MVN_DETECT_EX * MVN_DETECT_EY / MVN_DETECT_WG)  // voxels of a lane per plane
#define MVN_DETECT_ESX (MVN_DETECT_EX + 2)
#define MVN_DETECT_ESY (MVN_DETECT_EY + 2)
#define MVN_DETECT_EPLANE (MVN_DETECT_ESX * MVN_DETECT_ESY)
#define MVN_DETECT_EXTREMA_LDS (3 * MVN_DETECT_EPLANE)

struct DetectParams {
  const void* src;       // element (0, 0, 0) of the raw stack
  long long s0, s1, s2;  // its element strides (>= 0)
  int m[3];              // its extents
  int R[2][3];           // radius of blur a along axis k
  const float* taps;     // device table, MVN_DETECT_TABLE floats
  float* a[2];           // the blurs along axis 2; a[0] receives D
  float* b[2];           // ... then along axis 1
  float threshold;
  int minima;            // E = -D
  unsigned long long* count;  // candidates found
  long long* list;       // their raster indices: any order behind the extremum pass, ascending for the fit
  long long list_cap;    // entries of the list
  long long nfound;      // the fit: candidates in the list
  double* pos;           // nfound x 3
  float* val;            // nfound
  int* vox;              // nfound x 3
};

#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
// read-only for the whole launch and the same address in every lane: scalar loads
typedef const __attribute__((address_space(4))) float* mvn_detect_taps_t;
#define MVN_DETECT_TAPS_AT(p) ((mvn_detect_taps_t)(p))
#define MVN_DETECT_APPEND(p) atomicAdd((p), 1ull)
#else
typedef const float* mvn_detect_taps_t;
#define MVN_DETECT_TAPS_AT(p) (p)
#define MVN_DETECT_APPEND(p) __atomic_fetch_add((p), 1ull, __ATOMIC_RELAXED)
#endif

MVN_HD long mvn_detect_ceil(long n, long d) { return (n + d - 1) / d; }
MVN_HD long long mvn_detect_voxels(const DetectParams& p) { return (long long)p.m[0] * p.m[1] * p.m[2]; }
MVN_HD long mvn_detect_rows_blocks(const DetectParams& p) {
  return mvn_detect_ceil((long)p.m[0] * p.m[1], MVN_DETECT_NR) * mvn_detect_ceil(p.m[2], MVN_DETECT_SEG);
}
// AXIS: the walked axis; the third axis is 1 - AXIS
MVN_HD long mvn_detect_lines_blocks(const DetectParams& p, int axis) {
  return mvn_detect_ceil(p.m[2], MVN_DETECT_TX) * mvn_detect_ceil(p.m[axis], MVN_DETECT_TL) * p.m[1 - axis];
}
MVN_HD long mvn_detect_extrema_blocks(const DetectParams& p) {
  return mvn_detect_ceil(p.m[2], MVN_DETECT_EX) * mvn_detect_ceil(p.m[1], MVN_DETECT_EY) *
         mvn_detect_ceil(p.m[0], MVN_DETECT_ESEG);
}

inline void mvn_detect_check_blur(const DetectParams& p) {
  if (!p.src || !p.taps || !p.a[0] || !p.a[1] || !p.b[0] || !p.b[1])
    throw std::invalid_argument("mvn: detect: null pointer");
  if (p.s0 < 0 || p.s1 < 0 || p.s2 < 0) throw std::invalid_argument("mvn: detect: negative stride");
  for (int k = 0; k < 3; ++k) {
    if (p.m[k] < 1 || p.m[k] > 0x3fffffff) throw std::invalid_argument("mvn: detect: raw extents must be in 1..2^30 - 1");
    for (int a = 0; a < 2; ++a)
      if (p.R[a][k] < 0 || p.R[a][k] > MVN_DETECT_RMAX) throw std::invalid_argument("mvn: detect: radius out of range");
  }
}

inline void mvn_detect_check_list(const DetectParams& p) {
  if (!p.a[0] || !p.count || !p.list || p.list_cap < 1) throw std::invalid_argument("mvn: detect: null pointer");
  for (int k = 0; k < 3; ++k)
    if (p.m[k] < 1 || p.m[k] > 0x3fffffff) throw std::invalid_argument("mvn: detect: raw extents must be in 1..2^30 - 1");
}

// the taps of one sigma, in double on the host (the header states them): R = ceil(3 s), g_i = exp(-(i i) / (2 s s)),
// S = the sum of the g_i in ascending i from g_{-R}, w_i = (float)(g_i / S); s == 0: R = 0, w = {1}.  `taps` holds at
// least 2 * MVN_DETECT_RMAX + 1 floats; returns R
inline int mvn_detect_make_taps(double sigma, float* taps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(sigma >= 0.0 && sigma <= 10.0)) throw std::invalid_argument("sigma must be finite and in 0..10");
  const int R = (int)ceil(3.0 * sigma);
  if (R == 0) {
    taps[0] = 1.0f;
    return 0;
  }
  double g[2 * MVN_DETECT_RMAX + 1];
  const double den = (2.0 * sigma) * sigma;
  for (int i = -R; i <= R; ++i) g[i + R] = exp(-(double)(i * i) / den);
  double S = g[0];
  for (int i = 1; i <= 2 * R; ++i) S = S + g[i];
  for (int i = 0; i <= 2 * R; ++i) taps[i] = (float)(g[i] / S);
  return R;
}

// ---- axis 2: the raw stack, read once, into both blurs ----------------------------------------------------------------
// block: row group * segments + segment; lds: MVN_DETECT_ROWS_LDS floats; lanes tid, tid + nthreads, ...
template <typename T>
MVN_HD void mvn_detect_rows_body(const DetectParams& p, long block, float* lds, int tid, int nthreads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int WG = MVN_DETECT_WG, SEG = MVN_DETECT_SEG, NR = MVN_DETECT_NR, PITCH = MVN_DETECT_RPITCH;
  const int m1 = p.m[1], m2 = p.m[2];
  const long nseg = mvn_detect_ceil(m2, SEG);
  const long rows = (long)p.m[0] * m1;
  const long rg = block / nseg;
  const int x0 = (int)(block - rg * nseg) * SEG;
  const int R1 = p.R[0][2], R2 = p.R[1][2];
  const int R = R1 > R2 ? R1 : R2;
  const int width = SEG + 2 * R;
  const T* src = (const T*)p.src;
  for (int q = 0; q < NR; ++q) {
    const long row = rg * NR + q;
    if (row >= rows) break;  // (the same in every lane)
    const long c0 = row / m1, c1 = row - c0 * m1;
    const T* line = src + (c0 * p.s0 + c1 * p.s1);
    for (int i = tid; i < width; i += nthreads)
      lds[q * PITCH + i] = (float)line[(long long)mvn_beads_mir(x0 - R + i, m2) * p.s2];
  }
  MVN_SYNC();
  const mvn_detect_taps_t w1 = MVN_DETECT_TAPS_AT(p.taps) + (0 * 3 + 2) * MVN_DETECT_TAPS;
  const mvn_detect_taps_t w2 = MVN_DETECT_TAPS_AT(p.taps) + (1 * 3 + 2) * MVN_DETECT_TAPS;
  for (int t = tid; t < WG; t += nthreads) {
    const int x = x0 + t;
    if (x >= m2) continue;
    for (int q = 0; q < NR; ++q) {
      const long row = rg * NR + q;
      if (row >= rows) break;
      const float* u1 = lds + q * PITCH + t + (R - R1);
      const float* u2 = lds + q * PITCH + t + (R - R2);
      float v1 = w1[0] * u1[0];
      for (int j = 1; j <= 2 * R1; ++j) v1 = v1 + w1[j] * u1[j];
      float v2 = w2[0] * u2[0];
      for (int j = 1; j <= 2 * R2; ++j) v2 = v2 + w2[j] * u2[j];
      p.a[0][row * m2 + x] = v1;
      p.a[1][row * m2 + x] = v2;
    }
  }
}

// ---- axis 1 and axis 0 ---------------------------------------------------------------------------------------------------
// block: (index along the third axis * tiles along AXIS + tile along AXIS) * tiles along axis 2 + tile along axis 2;
// lds: MVN_DETECT_LINES_LDS floats; NL lanes per thread
template <int AXIS, int NL>
MVN_HD void mvn_detect_lines_body(const DetectParams& p, long block, float* lds, int tid, int nthreads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int WG = MVN_DETECT_WG, TX = MVN_DETECT_TX, TL = MVN_DETECT_TL, LR = MVN_DETECT_LR, LK = MVN_DETECT_LK;
  static_assert(NL == 1 || NL == WG, "a thread owns one lane, or all of them");
  const int m2 = p.m[2], mL = p.m[AXIS];
  const long plane = (long)p.m[1] * m2;
  const long lstride = AXIS == 1 ? (long)m2 : plane;  // along the walked axis
  const long ostride = AXIS == 1 ? plane : (long)m2;  // along the third one
  const long ntx = mvn_detect_ceil(m2, TX), ntl = mvn_detect_ceil(mL, TL);
  const int x0 = (int)(block % ntx) * TX;
  const int l0 = (int)((block / ntx) % ntl) * TL;
  const long base = (block / (ntx * ntl)) * ostride;
  const int nl = l0 + TL < mL ? TL : mL - l0;  // lines of this tile
  float acc[NL][2][LK];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const float* in = (AXIS == 1 ? p.a[a] : p.b[a]) + base;
    const int R = p.R[a][AXIS];
    const mvn_detect_taps_t w = MVN_DETECT_TAPS_AT(p.taps) + (a * 3 + AXIS) * MVN_DETECT_TAPS;
    if (a == 1) MVN_SYNC();  // (blur 0 has read its tile)
    const int staged = (nl + 2 * R) * TX;
    for (int idx = tid; idx < staged; idx += nthreads) {
      const int i = idx / TX, x = x0 + (idx - i * TX);
      lds[idx] = in[(long)mvn_beads_mir(l0 - R + i, mL) * lstride + (x < m2 ? x : m2 - 1)];
    }
    MVN_SYNC();
    for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
      const int tx = t % TX, tr = t / TX;
#pragma unroll
      for (int k = 0; k < LK; ++k) {
        const int ty = tr + k * LR;
        float v = 0.f;
        if (ty < nl) {
          const float* u = lds + ty * TX + tx;
          v = w[0] * u[0];
          for (int j = 1; j <= 2 * R; ++j) v = v + w[j] * u[j * TX];
        }
        acc[l][a][k] = v;
      }
    }
  }
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const int tx = t % TX, tr = t / TX;
    if (x0 + tx >= m2) continue;
#pragma unroll
    for (int k = 0; k < LK; ++k) {
      const int ty = tr + k * LR;
      if (ty >= nl) continue;
      const long at = base + (long)(l0 + ty) * lstride + x0 + tx;
      if (AXIS == 1) {
        p.b[0][at] = acc[l][0][k];
        p.b[1][at] = acc[l][1][k];
      } else {
        p.a[0][at] = acc[l][0][k] - acc[l][1][k];
      }
    }
  }
}

// ---- the extrema ---------------------------------------------------------------------------------------------------------
// block: (segment * tiles along axis 1 + tile along axis 1) * tiles along axis 2 + tile along axis 2;
// lds: MVN_DETECT_EXTREMA_LDS floats
MVN_HD void mvn_detect_extrema_body(const DetectParams& p, long block, float* lds, int tid, int nthreads) {
  constexpr int WG = MVN_DETECT_WG, EX = MVN_DETECT_EX, EY = MVN_DETECT_EY, EK = MVN_DETECT_EK, SX = MVN_DETECT_ESX,
                PL = MVN_DETECT_EPLANE, ROWS = WG / EX;
  const int m0 = p.m[0], m1 = p.m[1], m2 = p.m[2];
  const long ntx = mvn_detect_ceil(m2, EX), nty = mvn_detect_ceil(m1, EY);
  const int x0 = (int)(block % ntx) * EX, y0 = (int)((block / ntx) % nty) * EY;
  const int zs = (int)(block / (ntx * nty)) * MVN_DETECT_ESEG;
  const int ze = zs + MVN_DETECT_ESEG < m0 ? zs + MVN_DETECT_ESEG : m0;
  const int za = zs > 1 ? zs : 1, zb = ze < m0 - 1 ? ze : m0 - 1;  // the planes that can hold a candidate
  if (za >= zb) return;  // (the same in every lane)
  const long plane = (long)m1 * m2;
  const float* D = p.a[0];
  // plane z of E, the tile plus its rim, into slot z % 3 (a cell outside the stack repeats the edge: no candidate
  // looks at it)
  for (int z = za - 1; z <= zb; ++z) {
    float* U = lds + (z % 3) * PL;
    const float* src = D + (long)z * plane;
    for (int idx = tid; idx < PL; idx += nthreads) {
      const int ey = idx / SX, ex = idx - ey * SX;
      int y = y0 - 1 + ey, x = x0 - 1 + ex;
      y = y < 0 ? 0 : (y < m1 ? y : m1 - 1);
      x = x < 0 ? 0 : (x < m2 ? x : m2 - 1);
      const float v = src[(long)y * m2 + x];
      U[idx] = p.minima ? -v : v;
    }
    if (z < za + 1) continue;  // (planes za - 1 and za are only staged)
    MVN_SYNC();
    const int zc = z - 1;  // the plane under test: zc - 1, zc, zc + 1 are staged
    const float* Um = lds + ((zc + 2) % 3) * PL;
    const float* Uc = lds + (zc % 3) * PL;
    const float* Up = lds + ((zc + 1) % 3) * PL;
    for (int t = tid; t < WG; t += nthreads) {
      const int tx = t % EX, tr = t / EX;
#pragma unroll
      for (int k = 0; k < EK; ++k) {
        const int ty = tr + k * ROWS;
        const int y = y0 + ty, x = x0 + tx;
        if (y < 1 || y > m1 - 2 || x < 1 || x > m2 - 2) continue;
        const int s = (ty + 1) * SX + tx + 1;
        const float e = Uc[s];
        if (!(e > p.threshold)) continue;
        bool top = true;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int n = s + dy * SX + dx;
            top = top && e > Um[n] && e > Up[n] && (n == s || e > Uc[n]);
          }
        if (!top) continue;
        const unsigned long long slot = MVN_DETECT_APPEND(p.count);
        if (slot < (unsigned long long)p.list_cap) p.list[slot] = ((long long)zc * m1 + y) * m2 + x;
      }
    }
    MVN_SYNC();  // (the next plane goes into the slot of plane zc - 1)
  }
}

// ---- the fit --------------------------------------------------------------------------------------------------------------
// o = -(adj(H) g) / det H by cofactors, every operation written out; 0 where the fit is not to be trusted
MVN_HD void mvn_detect_fit(const double E[3][3][3], double o[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c = E[1][1][1];
  const double g0 = (E[2][1][1] - E[0][1][1]) / 2.0;
  const double g1 = (E[1][2][1] - E[1][0][1]) / 2.0;
  const double g2 = (E[1][1][2] - E[1][1][0]) / 2.0;
  const double h00 = (E[2][1][1] + E[0][1][1]) - 2.0 * c;
  const double h11 = (E[1][2][1] + E[1][0][1]) - 2.0 * c;
  const double h22 = (E[1][1][2] + E[1][1][0]) - 2.0 * c;
  const double h01 = ((E[2][2][1] - E[2][0][1]) - (E[0][2][1] - E[0][0][1])) / 4.0;
  const double h02 = ((E[2][1][2] - E[2][1][0]) - (E[0][1][2] - E[0][1][0])) / 4.0;
  const double h12 = ((E[1][2][2] - E[1][2][0]) - (E[1][0][2] - E[1][0][0])) / 4.0;
  const double c00 = h11 * h22 - h12 * h12;
  const double c01 = h02 * h12 - h01 * h22;
  const double c02 = h01 * h12 - h02 * h11;
  const double c11 = h00 * h22 - h02 * h02;
  const double c12 = h01 * h02 - h00 * h12;
  const double c22 = h00 * h11 - h01 * h01;
  const double det = (h00 * c00 + h01 * c01) + h02 * c02;
  const double n0 = (c00 * g0 + c01 * g1) + c02 * g2;
  const double n1 = (c01 * g0 + c11 * g1) + c12 * g2;
  const double n2 = (c02 * g0 + c12 * g1) + c22 * g2;
  const double big = 1.7976931348623157e308;
  o[0] = o[1] = o[2] = 0.0;
  if (det == 0.0 || !(det >= -big && det <= big)) return;
  const double o0 = -n0 / det, o1 = -n1 / det, o2 = -n2 / det;
  // (a NaN fails the comparison: |o| <= 1 also says finite)
  if (!(o0 >= -1.0 && o0 <= 1.0 && o1 >= -1.0 && o1 <= 1.0 && o2 >= -1.0 && o2 <= 1.0)) return;
  o[0] = o0, o[1] = o1, o[2] = o2;
}

// one work item per candidate of the sorted list
MVN_HD void mvn_detect_refine_item(const DetectParams& p, long block, int tid) {
  const long long i = (long long)block * MVN_DETECT_WG + tid;
  if (i >= p.nfound) return;
  const int m1 = p.m[1], m2 = p.m[2];
  const long long at = p.list[i];
  const int c2 = (int)(at % m2), c1 = (int)((at / m2) % m1), c0 = (int)(at / ((long long)m1 * m2));
  double E[3][3][3];
  for (int d0 = 0; d0 < 3; ++d0)
    for (int d1 = 0; d1 < 3; ++d1)
      for (int d2 = 0; d2 < 3; ++d2) {
        const float v = p.a[0][((long long)(c0 + d0 - 1) * m1 + (c1 + d1 - 1)) * m2 + (c2 + d2 - 1)];
        E[d0][d1][d2] = (double)(p.minima ? -v : v);
      }
  double o[3];
  mvn_detect_fit(E, o);
  p.pos[3 * i + 0] = (double)c0 + o[0];
  p.pos[3 * i + 1] = (double)c1 + o[1];
  p.pos[3 * i + 2] = (double)c2 + o[2];
  p.val[i] = (float)E[1][1][1];
  p.vox[3 * i + 0] = c0, p.vox[3 * i + 1] = c1, p.vox[3 * i + 2] = c2;
}

#ifdef MVN_HOST_EMU
// the launches of the host emulation (mvn_backend_emu.cpp; tools/detect_standalone.cpp runs them under sanitizers):
// one thread owns all the lanes of a workgroup
template <typename T>
inline void mvn_detect_rows_host(const DetectParams& p) {
  const long nblocks = mvn_detect_rows_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    float lds[MVN_DETECT_ROWS_LDS];
    mvn_detect_rows_body<T>(p, blk, lds, 0, 1);
  }
}

template <int AXIS>
inline void mvn_detect_lines_host(const DetectParams& p) {
  const long nblocks = mvn_detect_lines_blocks(p, AXIS);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    float lds[MVN_DETECT_LINES_LDS];
    mvn_detect_lines_body<AXIS, MVN_DETECT_WG>(p, blk, lds, 0, 1);
  }
}

inline void mvn_detect_extrema_host(const DetectParams& p) {
  const long nblocks = mvn_detect_extrema_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    float lds[MVN_DETECT_EXTREMA_LDS];
    mvn_detect_extrema_body(p, blk, lds, 0, 1);
  }
}

inline void mvn_detect_refine_host(const DetectParams& p) {
  const long nblocks = (long)mvn_detect_ceil((long)p.nfound, MVN_DETECT_WG);
  for (long blk = 0; blk < nblocks; ++blk)
    for (int t = 0; t < MVN_DETECT_WG; ++t) mvn_detect_refine_item(p, blk, t);
}
#endif
