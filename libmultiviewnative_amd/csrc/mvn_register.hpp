// mvn_register.hpp -- two views' beads into the affine matrix between them: the passes behind mvn_register_beads.
//
// include/mvn_engine_api.h states the arithmetic (mvn_register_beads): each bead's 4 nearest neighbours within its own
// set, four translation-invariant descriptors of 9 floats from them, the best and second best match of every bead of A
// among the beads of B, RANSAC over affine models of four candidate pairs, and a least-squares refit on the host.  The
// work is all-pairs and all-hypotheses, so every pass is a brute-force scan in which a work item keeps ITS element in
// registers and the scanned set comes through the LDS in tiles: all lanes of a wave read the same tile word at the same
// time, which the LDS serves as one broadcast read without bank conflicts.
//
//   k_reg_neighbours    one work item per bead of a set of n points (doubles, z y x).  The set goes through the LDS in
//                       tiles of MVN_REG_NTILE points; a work item keeps the 4 nearest (distance, index) in registers,
//                       sorted, and inserts with selects only (no indexed registers).  It ends by gathering its 4
//                       neighbours and writing their indices and the bead's 36 descriptor floats.
//   k_reg_match         grid = (tiles of MVN_REG_WG beads of A) x (chunks of B): n_A / 256 workgroups alone leave most
//                       of the 256 CUs idle at a few thousand beads, so B is cut into chunks of p.chunk beads (a
//                       multiple of the tile, mvn_reg_chunk).  A work item holds its bead's 36 floats in registers; B's
//                       descriptors come through the LDS in tiles of MVN_REG_MTILE beads.  Per pair the 16 descriptor
//                       distances and their minimum; per chunk the work item writes (d1, j1, d2).
//   k_reg_match_fold    one work item per bead of A merges its chunks in ascending order.  Minima are exact in any
//                       order and a tie keeps the lower j, so the result does not depend on the split.
//   k_reg_ransac        one work item per hypothesis: it draws its four candidates (mvn_reg_sample), fits
//                       (mvn_reg_solve), then scores against all candidates, which come through the LDS in tiles of
//                       MVN_REG_RTILE records (a, b: 6 doubles).  key = score << 32 | (2^32 - 1 - h); a workgroup
//                       takes the maximum of its keys through the LDS and one 64-bit atomic maximum folds it into
//                       *p.best: the highest score, the lowest h on a tie, whatever the schedule.
//
// The uniqueness filter and the refit are host code over short lists (mvn_abi.cpp) on the functions of this header.
// No cross-lane instructions; the host emulation runs the same bodies with one "thread" that owns all the lanes of a
// workgroup (mvn_detect.hpp's form: NL lanes per thread).  Every float32 and double operation is rounded once:
// contraction is off.
#pragma once

#include <math.h>
#include <stdint.h>

#include <stdexcept>

#include "mvn_fft_core.hpp"

#define MVN_REG_WG 256       // work items of a workgroup, in every pass
#define MVN_REG_NN 4         // neighbours of a bead (MVN_REGISTER_NEIGHBOURS of the header)
#define MVN_REG_DESC 36      // floats of a bead's descriptors: 4 triples x 3 neighbours x (z, y, x)
#define MVN_REG_NTILE 512    // neighbour pass: points of an LDS tile (12 KiB of doubles)
#define MVN_REG_MTILE 64     // match pass: beads of B in an LDS tile (9 KiB of floats)
#define MVN_REG_RTILE 256    // RANSAC pass: candidate records of an LDS tile (12 KiB of doubles)
#define MVN_REG_TARGET 1024  // workgroups the match pass aims at: 4 per CU
#define MVN_REG_MAX_BEADS 65536
#define MVN_REG_MAX_HYPOTHESES (1 << 24)

struct RegParams {
  // the neighbour pass: one set
  const double* pts;  // n x 3
  int n;
  int* nn;      // n x 4: the neighbours, nearest first
  float* desc;  // n x MVN_REG_DESC
  // the match pass and its fold
  const float* da;  // na x MVN_REG_DESC
  const float* db;  // nb x MVN_REG_DESC
  int na, nb;
  int chunk;    // beads of B in a chunk: a positive multiple of MVN_REG_MTILE
  float* pd1;   // [chunk][na]: the least distance within the chunk,
  int* pj1;     //   its j (the lower on a tie; -1: the chunk has no distance below +inf),
  float* pd2;   //   and the least distance over the chunk's other j
  float* d1;    // na: the same over all of B
  int* j1;
  float* d2;
  // the RANSAC pass
  const double* cand;  // nc x 6: a (z, y, x), b (z, y, x)
  int nc;
  int hyps;
  unsigned long long seed;
  double maxerr2;            // max_error * max_error
  unsigned long long* best;  // the maximum of the keys (cleared by the caller)
};

#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
#define MVN_REG_MAX(p, v) atomicMax((p), (v))
#else
inline void mvn_reg_host_max(unsigned long long* p, unsigned long long v) {
  unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
}
#define MVN_REG_MAX(p, v) mvn_reg_host_max((p), (v))
#endif

MVN_HD long mvn_reg_ceil(long n, long d) { return (n + d - 1) / d; }
// the beads of B in a chunk of the match pass: whole tiles, as few as give MVN_REG_TARGET workgroups
MVN_HD int mvn_reg_chunk(int na, int nb) {
  const long tiles = mvn_reg_ceil(nb, MVN_REG_MTILE);
  long chunks = mvn_reg_ceil(MVN_REG_TARGET, mvn_reg_ceil(na, MVN_REG_WG));
  if (chunks > tiles) chunks = tiles;
  return (int)(mvn_reg_ceil(tiles, chunks) * MVN_REG_MTILE);
}
MVN_HD int mvn_reg_chunks(int nb, int chunk) { return (int)mvn_reg_ceil(nb, chunk); }
MVN_HD long mvn_reg_neighbours_blocks(const RegParams& p) { return mvn_reg_ceil(p.n, MVN_REG_WG); }
MVN_HD long mvn_reg_match_blocks(const RegParams& p) {
  return mvn_reg_ceil(p.na, MVN_REG_WG) * mvn_reg_chunks(p.nb, p.chunk);
}
MVN_HD long mvn_reg_fold_blocks(const RegParams& p) { return mvn_reg_ceil(p.na, MVN_REG_WG); }
MVN_HD long mvn_reg_ransac_blocks(const RegParams& p) { return mvn_reg_ceil(p.hyps, MVN_REG_WG); }

inline void mvn_reg_check_neighbours(const RegParams& p) {
  if (!p.pts || !p.nn || !p.desc) throw std::invalid_argument("mvn: register: null pointer");
  if (p.n < MVN_REG_NN + 1 || p.n > MVN_REG_MAX_BEADS) throw std::invalid_argument("mvn: register: bead count out of range");
}
inline void mvn_reg_check_match(const RegParams& p) {
  if (!p.da || !p.db || !p.pd1 || !p.pj1 || !p.pd2 || !p.d1 || !p.j1 || !p.d2)
    throw std::invalid_argument("mvn: register: null pointer");
  if (p.na < 1 || p.na > MVN_REG_MAX_BEADS || p.nb < 1 || p.nb > MVN_REG_MAX_BEADS)
    throw std::invalid_argument("mvn: register: bead count out of range");
  if (p.chunk < MVN_REG_MTILE || p.chunk % MVN_REG_MTILE) throw std::invalid_argument("mvn: register: chunk is no multiple of the tile");
}
inline void mvn_reg_check_ransac(const RegParams& p) {
  if (!p.cand || !p.best) throw std::invalid_argument("mvn: register: null pointer");
  if (p.nc < 4 || p.nc > MVN_REG_MAX_BEADS) throw std::invalid_argument("mvn: register: candidate count out of range");
  if (p.hyps < 1 || p.hyps > MVN_REG_MAX_HYPOTHESES) throw std::invalid_argument("mvn: register: hypotheses out of range");
}

MVN_HD bool mvn_reg_finite(double x) {
  const double big = 1.7976931348623157e308;
  return x >= -big && x <= big;  // (a NaN fails the comparison)
}

// ---- the sample of a hypothesis ------------------------------------------------------------------------------------------
MVN_HD unsigned long long mvn_reg_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// four distinct indices below n (n >= 4): draw q over n - q, stepped over the earlier picks in ascending order
MVN_HD void mvn_reg_sample(unsigned long long seed, unsigned h, int n, int out[4]) {
  int s0 = 0x7fffffff, s1 = 0x7fffffff, s2 = 0x7fffffff;  // the earlier picks, ascending
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned long long u = mvn_reg_mix(seed + 0x9E3779B97F4A7C15ull * (16ull * h + (unsigned long long)q + 1ull));
    int r = (int)(((u >> 32) * (unsigned long long)(n - q)) >> 32);
    if (s0 <= r) ++r;
    if (s1 <= r) ++r;
    if (s2 <= r) ++r;
    out[q] = r;
    if (r < s0)
      s2 = s1, s1 = s0, s0 = r;
    else if (r < s1)
      s2 = s1, s1 = r;
    else if (r < s2)
      s2 = r;
  }
}

// ---- the model -------------------------------------------------------------------------------------------------------------
// L = (F adj E) / det E, row-major 3 x 3 each, by cofactors, every operation written out; false where det is zero or
// not finite or an entry of L is not finite
MVN_HD bool mvn_reg_solve(const double E[9], const double F[9], double L[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c00 = E[4] * E[8] - E[5] * E[7];
  const double c01 = E[5] * E[6] - E[3] * E[8];
  const double c02 = E[3] * E[7] - E[4] * E[6];
  const double c10 = E[2] * E[7] - E[1] * E[8];
  const double c11 = E[0] * E[8] - E[2] * E[6];
  const double c12 = E[1] * E[6] - E[0] * E[7];
  const double c20 = E[1] * E[5] - E[2] * E[4];
  const double c21 = E[2] * E[3] - E[0] * E[5];
  const double c22 = E[0] * E[4] - E[1] * E[3];
  const double det = (E[0] * c00 + E[1] * c01) + E[2] * c02;
  if (det == 0.0 || !mvn_reg_finite(det)) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f0 = F[3 * k], f1 = F[3 * k + 1], f2 = F[3 * k + 2];
    L[3 * k + 0] = ((f0 * c00 + f1 * c01) + f2 * c02) / det;
    L[3 * k + 1] = ((f0 * c10 + f1 * c11) + f2 * c12) / det;
    L[3 * k + 2] = ((f0 * c20 + f1 * c21) + f2 * c22) / det;
    ok = ok && mvn_reg_finite(L[3 * k]) && mvn_reg_finite(L[3 * k + 1]) && mvn_reg_finite(L[3 * k + 2]);
  }
  return ok;
}

// t = c_b - L c_a; false where an entry is not finite
MVN_HD bool mvn_reg_offset(const double L[9], const double* ca, const double* cb, double t[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t[k] = cb[k] - ((L[3 * k] * ca[0] + L[3 * k + 1] * ca[1]) + L[3 * k + 2] * ca[2]);
    ok = ok && mvn_reg_finite(t[k]);
  }
  return ok;
}

// the model through four pairs: a and b are 4 x 3
MVN_HD bool mvn_reg_fit4(const double* a, const double* b, double L[9], double t[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double E[9], F[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      E[3 * k + c] = a[3 * (c + 1) + k] - a[k];
      F[3 * k + c] = b[3 * (c + 1) + k] - b[k];
    }
  if (!mvn_reg_solve(E, F, L)) return false;
  return mvn_reg_offset(L, a, b, t);
}

// the squared residual of one pair under a model
MVN_HD double mvn_reg_residual2(const double L[9], const double t[3], const double* a, const double* b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double r0 = (((L[0] * a[0] + L[1] * a[1]) + L[2] * a[2]) + t[0]) - b[0];
  const double r1 = (((L[3] * a[0] + L[4] * a[1]) + L[5] * a[2]) + t[1]) - b[1];
  const double r2 = (((L[6] * a[0] + L[7] * a[1]) + L[8] * a[2]) + t[2]) - b[2];
  return (r0 * r0 + r1 * r1) + r2 * r2;
}

// ---- the neighbours and the descriptors -------------------------------------------------------------------------------
// (d, j) before (bd, bi): by distance, then by index
MVN_HD bool mvn_reg_before(double d, int j, double bd, int bi) { return d < bd || (d == bd && j < bi); }

// block: tile of MVN_REG_WG beads; lds: 3 * MVN_REG_NTILE doubles; NL lanes per thread
template <int NL>
MVN_HD void mvn_reg_neighbours_body(const RegParams& p, long block, double* lds, int tid, int nthreads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int WG = MVN_REG_WG, TILE = MVN_REG_NTILE;
  static_assert(NL == 1 || NL == WG, "a thread owns one lane, or all of them");
  const int n = p.n;
  double pi[NL][3], bd[NL][4];
  int bi[NL][4], self[NL];
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const long i = block * WG + t;
    self[l] = i < n ? (int)i : n - 1;  // (a lane past the set scans for the last bead and writes nothing)
#pragma unroll
    for (int k = 0; k < 3; ++k) pi[l][k] = p.pts[3 * (long)self[l] + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) bd[l][k] = (double)INFINITY, bi[l][k] = 0x7fffffff;
  }
  for (int j0 = 0; j0 < n; j0 += TILE) {
    const int cnt = j0 + TILE < n ? TILE : n - j0;
    if (j0 > 0) MVN_SYNC();  // (the tile before has been scanned)
    for (int idx = tid; idx < 3 * cnt; idx += nthreads) lds[idx] = p.pts[3 * (long)j0 + idx];
    MVN_SYNC();
    for (int l = 0; l < NL; ++l) {
      for (int jj = 0; jj < cnt; ++jj) {
        const int j = j0 + jj;
        if (j == self[l]) continue;
        const double dz = lds[3 * jj] - pi[l][0], dy = lds[3 * jj + 1] - pi[l][1], dx = lds[3 * jj + 2] - pi[l][2];
        const double d = (dz * dz + dy * dy) + dx * dx;
        if (!mvn_reg_before(d, j, bd[l][3], bi[l][3])) continue;
#pragma unroll
        for (int k = 3; k >= 0; --k) {  // (downwards: entry k - 1 is still the old one)
          const bool here = mvn_reg_before(d, j, bd[l][k], bi[l][k]);
          const bool above = k > 0 && mvn_reg_before(d, j, bd[l][k > 0 ? k - 1 : 0], bi[l][k > 0 ? k - 1 : 0]);
          const double od = bd[l][k > 0 ? k - 1 : 0];
          const int oi = bi[l][k > 0 ? k - 1 : 0];
          bd[l][k] = above ? od : (here ? d : bd[l][k]);
          bi[l][k] = above ? oi : (here ? j : bi[l][k]);
        }
      }
    }
  }
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const long i = block * WG + t;
    if (i >= n) continue;
    float q[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p.nn[4 * i + k] = bi[l][k];
#pragma unroll
      for (int c = 0; c < 3; ++c) q[k][c] = (float)(p.pts[3 * (long)bi[l][k] + c] - pi[l][c]);
    }
    float* out = p.desc + MVN_REG_DESC * i;
    const int triple[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[9 * d + 3 * m + c] = q[triple[d][m]][c];
  }
}

// ---- the match -------------------------------------------------------------------------------------------------------------
// block: chunk * tiles of A + tile of A; lds: MVN_REG_MTILE * MVN_REG_DESC floats
template <int NL>
MVN_HD void mvn_reg_match_body(const RegParams& p, long block, float* lds, int tid, int nthreads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int WG = MVN_REG_WG, TILE = MVN_REG_MTILE, DESC = MVN_REG_DESC;
  static_assert(NL == 1 || NL == WG, "a thread owns one lane, or all of them");
  const int na = p.na, nb = p.nb;
  const long nta = mvn_reg_ceil(na, WG);
  const long ta = block % nta, ch = block / nta;
  const int jb = (int)ch * p.chunk;
  const int je = jb + p.chunk < nb ? jb + p.chunk : nb;
  float u[NL][DESC], d1[NL], d2[NL];
  int j1[NL];
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const long i = ta * WG + t;
    const float* src = p.da + DESC * (i < na ? i : (long)na - 1);
#pragma unroll
    for (int k = 0; k < DESC; ++k) u[l][k] = src[k];
    d1[l] = d2[l] = INFINITY, j1[l] = -1;
  }
  for (int j0 = jb; j0 < je; j0 += TILE) {
    const int cnt = j0 + TILE < je ? TILE : je - j0;
    if (j0 > jb) MVN_SYNC();
    for (int idx = tid; idx < DESC * cnt; idx += nthreads) lds[idx] = p.db[DESC * (long)j0 + idx];
    MVN_SYNC();
    for (int l = 0; l < NL; ++l) {
      for (int jj = 0; jj < cnt; ++jj) {
        const float* v = lds + DESC * jj;  // (the same word in every lane: a broadcast)
        float w[DESC];
#pragma unroll
        for (int k = 0; k < DESC; ++k) w[k] = v[k];
        float d = INFINITY;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            const float e0 = u[l][9 * x] - w[9 * y];
            float s = e0 * e0;
#pragma unroll
            for (int k = 1; k < 9; ++k) {
              const float e = u[l][9 * x + k] - w[9 * y + k];
              s = s + e * e;
            }
            d = s < d ? s : d;  // (a NaN is never a minimum)
          }
        if (d < d1[l]) {
          d2[l] = d1[l], d1[l] = d, j1[l] = j0 + jj;
        } else if (d < d2[l]) {
          d2[l] = d;
        }
      }
    }
  }
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const long i = ta * WG + t;
    if (i >= na) continue;
    const long at = ch * na + i;
    p.pd1[at] = d1[l], p.pj1[at] = j1[l], p.pd2[at] = d2[l];
  }
}

// one work item per bead of A: its chunks in ascending order
MVN_HD void mvn_reg_fold_item(const RegParams& p, long block, int tid) {
  const long i = block * MVN_REG_WG + tid;
  if (i >= p.na) return;
  const int chunks = mvn_reg_chunks(p.nb, p.chunk);
  float d1 = INFINITY, d2 = INFINITY;
  int j1 = -1;
  for (int c = 0; c < chunks; ++c) {
    const long at = (long)c * p.na + i;
    const float c1 = p.pd1[at], c2 = p.pd2[at];
    if (c1 < d1) {  // (strict: a tie keeps the earlier chunk's lower j)
      d2 = d1 < c2 ? d1 : c2;
      d1 = c1, j1 = p.pj1[at];
    } else {
      d2 = c1 < d2 ? c1 : d2;
    }
  }
  p.d1[i] = d1, p.j1[i] = j1, p.d2[i] = d2;
}

// ---- RANSAC ----------------------------------------------------------------------------------------------------------------
MVN_HD unsigned long long mvn_reg_key(int score, unsigned h) {
  return ((unsigned long long)(unsigned)score << 32) | (unsigned long long)(0xffffffffu - h);
}
MVN_HD int mvn_reg_key_score(unsigned long long key) { return (int)(key >> 32); }
MVN_HD unsigned mvn_reg_key_h(unsigned long long key) { return 0xffffffffu - (unsigned)(key & 0xffffffffull); }

// the model of hypothesis h from the candidate records; false: it scores 0
MVN_HD bool mvn_reg_hypothesis(const double* cand, int nc, unsigned long long seed, unsigned h, double L[9], double t[3]) {
  int s[4];
  mvn_reg_sample(seed, h, nc, s);
  double a[12], b[12];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[3 * m + k] = cand[6 * (long)s[m] + k], b[3 * m + k] = cand[6 * (long)s[m] + 3 + k];
  return mvn_reg_fit4(a, b, L, t);
}

// block: tile of MVN_REG_WG hypotheses; lds: 6 * MVN_REG_RTILE doubles; keys: MVN_REG_WG words
template <int NL>
MVN_HD void mvn_reg_ransac_body(const RegParams& p, long block, double* lds, unsigned long long* keys, int tid,
                                int nthreads) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int WG = MVN_REG_WG, TILE = MVN_REG_RTILE;
  static_assert(NL == 1 || NL == WG, "a thread owns one lane, or all of them");
  const int nc = p.nc;
  double L[NL][9], tr[NL][3];
  bool ok[NL];
  int score[NL];
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const long h = block * WG + t;
    ok[l] = mvn_reg_hypothesis(p.cand, nc, p.seed, h < p.hyps ? (unsigned)h : 0u, L[l], tr[l]) && h < p.hyps;
    score[l] = 0;
  }
  for (int c0 = 0; c0 < nc; c0 += TILE) {
    const int cnt = c0 + TILE < nc ? TILE : nc - c0;
    if (c0 > 0) MVN_SYNC();
    for (int idx = tid; idx < 6 * cnt; idx += nthreads) lds[idx] = p.cand[6 * (long)c0 + idx];
    MVN_SYNC();
    for (int l = 0; l < NL; ++l) {
      if (!ok[l]) continue;
      int s = 0;
      for (int cc = 0; cc < cnt; ++cc)
        s += mvn_reg_residual2(L[l], tr[l], lds + 6 * cc, lds + 6 * cc + 3) <= p.maxerr2 ? 1 : 0;
      score[l] += s;
    }
  }
  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
    const long h = block * WG + t;
    keys[t] = h < p.hyps ? mvn_reg_key(ok[l] ? score[l] : 0, (unsigned)h) : 0ull;
  }
  MVN_SYNC();
  if (tid == 0) {
    unsigned long long m = keys[0];
    for (int t = 1; t < WG; ++t) m = keys[t] > m ? keys[t] : m;
    MVN_REG_MAX(p.best, m);
  }
}

#ifdef MVN_HOST_EMU
// the launches of the host emulation (mvn_backend_emu.cpp; tools/register_standalone.cpp runs them under sanitizers):
// one thread owns all the lanes of a workgroup
inline void mvn_reg_neighbours_host(const RegParams& p) {
  const long nblocks = mvn_reg_neighbours_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    double lds[3 * MVN_REG_NTILE];
    mvn_reg_neighbours_body<MVN_REG_WG>(p, blk, lds, 0, 1);
  }
}

inline void mvn_reg_match_host(const RegParams& p) {
  const long nblocks = mvn_reg_match_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    float lds[MVN_REG_MTILE * MVN_REG_DESC];
    mvn_reg_match_body<MVN_REG_WG>(p, blk, lds, 0, 1);
  }
  const long folds = mvn_reg_fold_blocks(p);
  for (long blk = 0; blk < folds; ++blk)
    for (int t = 0; t < MVN_REG_WG; ++t) mvn_reg_fold_item(p, blk, t);
}

inline void mvn_reg_ransac_host(const RegParams& p) {
  const long nblocks = mvn_reg_ransac_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    double lds[6 * MVN_REG_RTILE];
    unsigned long long keys[MVN_REG_WG];
    mvn_reg_ransac_body<MVN_REG_WG>(p, blk, lds, keys, 0, 1);
  }
}
#endif
