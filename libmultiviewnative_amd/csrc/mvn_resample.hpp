// mvn_resample.hpp -- a RAW view into the engine's volumes: affine transform, trilinear samples and blend weights.
//
// The other placement routes (mvn_ingest.hpp) take stacks that the caller has already resampled into the block's
// frame.  This one takes what a caller has: the raw stack (uint16 or float32, element strides) and a 3 x 4 matrix that
// maps block voxel (z, y, x) to a raw index.  include/mvn_engine_api.h states the arithmetic (mvn_view_geometry); in
// short, per block voxel of the embedding window:
//
//     c_k = ((M[k][0] z + M[k][1] y) + M[k][2] x) + M[k][3]            in double, every operation rounded once
//     inside iff 0 <= c_k <= m_k - 1 for k = 0, 1, 2                   else image 0 and weight 0
//     i_k = floor(c_k), f_k = (float)(c_k - i_k), j_k = min(i_k + 1, m_k - 1)
//     image  = lerp along raw axis 2, then 1, then 0 in float32, lerp(p, q, f) = p + f * (q - p)
//     weight = (r_0 r_1) r_2, r_k the cosine ramp of the distance to the nearer face of raw axis k
//
// No operation may be contracted into a fused multiply-add: the bodies switch contraction off themselves (clang), the
// emulation is built with -ffp-contract=off.
//
//   k_resample3d<T>       T the raw element type.  Writes the image volume and - in the same pass, from the same
//                         coordinates - the UNNORMALISED weights volume (p.weights may be null: the caller brings
//                         weights).  A workgroup owns a compact tile of the volume, MVN_RS_TZ planes x MVN_RS_TY rows x
//                         MVN_RS_TX columns, a work item 4 consecutive columns of a row of it: under a rotation a row
//                         of the block walks a strided line through the raw stack, a compact tile maps to a compact box
//                         of it, so the 8-neighbour reads of a tile meet in the cache.  Like k_ingest3d it writes EVERY
//                         element of the rows it owns - values inside the window, zeros in the margins and in the row
//                         padding - and depends on no earlier clear.  Stores are 16 bytes where RP is a multiple of 4,
//                         4 bytes otherwise (odd last extents).  The raw samples are plain (cached) loads.
//   k_weights_normalize   w_v <- W > 0 ? w_v / W : 0 with W = ((w_0 + w_1) + ...) + w_{V-1}, over the window rows of the
//                         V weights volumes of a device table of pointers, mvn_ingest.hpp's shape (a wave owns whole
//                         rows), 16-byte accesses on the same terms; elements outside the window keep what they hold.
//
// The bodies are plain C++ shared with the host emulation (mvn_backend_emu.cpp), like every other pass.
#pragma once

#include <math.h>
#include <stdint.h>

#include <stdexcept>
#include <string>

#include "mvn_ingest.hpp"

#define MVN_RS_WG 256  // work items of a workgroup
#define MVN_RS_TZ 8    // planes,
#define MVN_RS_TY 8    // rows
#define MVN_RS_TX 64   // and columns of its tile: 16 work items of 4 columns along a row, 8 rows, 2 planes at a time
#define MVN_RS_PI_F 3.14159265358979323846f

// mvn_view_geometry of include/mvn_engine_api.h, member for member
struct ResampleGeom {
  int m[3];         // extents of the raw stack
  double M[12];     // row-major 3 x 4
  float border[3];  // weight 0 within this distance of a face, per raw axis
  float range[3];   // width of the cosine ramp behind it
};

struct ResampleParams {
  float* image;          // the engine's image volume (float32)
  float* weights;        // its weights volume, or null: not written
  long RP;               // row pitch of both in floats
  int D0, D1;            // planes, rows of a plane
  const void* src;       // element (0, 0, 0) of the raw stack
  long long s0, s1, s2;  // its element strides (>= 0)
  int n0, n1, n2;        // extents of the block = of the embedding window
  int o0, o1, o2;        // the window's offset inside the volume
  ResampleGeom g;
};

struct NormalizeParams {
  float* const* vols;  // device table of V weights volumes
  int V;
  long RP;
  int D1;
  int n0, n1, n2;
  int o0, o1, o2;
};

// the window [o, o + n) of a launch inside a volume of D0 x D1 rows of RP elements
inline void mvn_window_check(const char* what, long RP, int D0, int D1, const int n[3], const int o[3]) {
  const long D[3] = {D0, D1, RP};
  for (int d = 0; d < 3; ++d)
    if (n[d] < 1 || o[d] < 0 || (long)o[d] + n[d] > D[d])
      throw std::invalid_argument(std::string("mvn: ") + what + ": the window does not fit the volume");
  if (RP < 2 || (RP & 1)) throw std::invalid_argument(std::string("mvn: ") + what + ": bad volume");
}
inline void mvn_resample_check(const ResampleParams& p) {
  const int n[3] = {p.n0, p.n1, p.n2}, o[3] = {p.o0, p.o1, p.o2};
  mvn_window_check("resample", p.RP, p.D0, p.D1, n, o);
  if (!p.image || !p.src) throw std::invalid_argument("mvn: resample: null pointer");
  if (p.s0 < 0 || p.s1 < 0 || p.s2 < 0) throw std::invalid_argument("mvn: resample: negative stride");
  for (int k = 0; k < 3; ++k)
    if (p.g.m[k] < 1) throw std::invalid_argument("mvn: resample: raw extents must be >= 1");
}
inline void mvn_normalize_check(const NormalizeParams& p) {
  const int n[3] = {p.n0, p.n1, p.n2}, o[3] = {p.o0, p.o1, p.o2};
  // (the last plane's rows are all the launch needs of D0)
  mvn_window_check("normalise", p.RP, p.o0 + p.n0, p.D1, n, o);
  if (!p.vols || p.V < 1) throw std::invalid_argument("mvn: normalise: no volumes");
}

MVN_HD long mvn_resample_blocks(const ResampleParams& p) {
  const long bz = (p.D0 + MVN_RS_TZ - 1) / MVN_RS_TZ, by = (p.D1 + MVN_RS_TY - 1) / MVN_RS_TY,
             bx = (p.RP + MVN_RS_TX - 1) / MVN_RS_TX;
  return bz * by * bx;
}

MVN_HD float mvn_resample_lerp(float a, float b, float f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = b - a;
  const float t = f * d;
  return a + t;
}

// the cosine ramp of one raw axis: dk the distance to the nearer face
MVN_HD float mvn_resample_ramp(float dk, float border, float range) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (dk < border) return 0.f;
  if (range == 0.f || dk >= border + range) return 1.f;
  const float u = (dk - border) / range;
  const float a = MVN_RS_PI_F * u;
  return 0.5f * (1.0f - cosf(a));
}

// image and unnormalised weight of the block voxel whose raw coordinate is c; false: outside the raw stack
template <typename T>
MVN_HD bool mvn_resample_voxel(const ResampleParams& p, const double c[3], float* image, float* weight) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  long long lo[3], hi[3];
  float f[3], r[3];
  const long long st[3] = {p.s0, p.s1, p.s2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double top = (double)(p.g.m[k] - 1);
    if (!(c[k] >= 0. && c[k] <= top)) return false;  // (a NaN is outside)
    const int i = (int)c[k];                         // floor: c >= 0
    const int j = i + 1 < p.g.m[k] ? i + 1 : p.g.m[k] - 1;
    f[k] = (float)(c[k] - (double)i);
    lo[k] = (long long)i * st[k], hi[k] = (long long)j * st[k];
    const double far = top - c[k];
    const double d = c[k] < far ? c[k] : far;
    r[k] = mvn_resample_ramp((float)d, p.g.border[k], p.g.range[k]);
  }
  const T* s = (const T*)p.src;
  float b[2];
#pragma unroll
  for (int a0 = 0; a0 < 2; ++a0) {
    const T* s0 = s + (a0 ? hi[0] : lo[0]);
    float a[2];
#pragma unroll
    for (int a1 = 0; a1 < 2; ++a1) {
      const T* s1 = s0 + (a1 ? hi[1] : lo[1]);
      a[a1] = mvn_resample_lerp((float)s1[lo[2]], (float)s1[hi[2]], f[2]);
    }
    b[a0] = mvn_resample_lerp(a[0], a[1], f[1]);
  }
  *image = mvn_resample_lerp(b[0], b[1], f[0]);
  *weight = (r[0] * r[1]) * r[2];
  return true;
}

template <typename T>
MVN_HD void mvn_resample_tile(const ResampleParams& p, long block, int tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long by = (p.D1 + MVN_RS_TY - 1) / MVN_RS_TY, bx = (p.RP + MVN_RS_TX - 1) / MVN_RS_TX;
  const long tz = block / (by * bx), rem = block - tz * (by * bx);
  const long ty = rem / bx, tx = rem - ty * bx;
  const int cg = tid % (MVN_RS_TX / 4), ry = (tid / (MVN_RS_TX / 4)) % MVN_RS_TY;
  const int rz = tid / ((MVN_RS_TX / 4) * MVN_RS_TY);
  constexpr int ZSTEP = MVN_RS_WG / ((MVN_RS_TX / 4) * MVN_RS_TY);
  const long x0 = tx * MVN_RS_TX + cg * 4;
  const long y = ty * MVN_RS_TY + ry;
  if (y >= p.D1 || x0 >= p.RP) return;
  const bool wide_stores = (p.RP & 3) == 0;
  const int yi = (int)y - p.o1;
  const double* M = p.g.M;
  for (int kz = rz; kz < MVN_RS_TZ; kz += ZSTEP) {
    const long z = tz * MVN_RS_TZ + kz;
    if (z >= p.D0) break;
    const int zi = (int)z - p.o0;
    const bool row_in = zi >= 0 && zi < p.n0 && yi >= 0 && yi < p.n1;
    // the part of the coordinate that every voxel of the row (z, y) shares
    double u[3] = {0., 0., 0.};
    if (row_in) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double a = M[4 * k] * (double)zi;
        const double b = M[4 * k + 1] * (double)yi;
        u[k] = a + b;
      }
    }
    float vi[4], vw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vi[j] = 0.f, vw[j] = 0.f;
      const long xi = x0 + j - p.o2;
      if (!row_in || xi < 0 || xi >= p.n2) continue;
      double c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double t = M[4 * k + 2] * (double)xi;  // (formed from x itself: no running sum along the row)
        const double w = u[k] + t;
        c[k] = w + M[4 * k + 3];
      }
      float im, wt;
      if (mvn_resample_voxel<T>(p, c, &im, &wt)) vi[j] = im, vw[j] = wt;
    }
    const long at = (z * p.D1 + y) * p.RP + x0;
    if (wide_stores) {  // (x0 + 4 <= RP)
      const mvn_v4f oi = {vi[0], vi[1], vi[2], vi[3]};
      *(mvn_v4f*)(p.image + at) = oi;
      if (p.weights) {
        const mvn_v4f ow = {vw[0], vw[1], vw[2], vw[3]};
        *(mvn_v4f*)(p.weights + at) = ow;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < p.RP) {
          p.image[at + j] = vi[j];
          if (p.weights) p.weights[at + j] = vw[j];
        }
    }
  }
}

MVN_HD long mvn_normalize_blocks(const NormalizeParams& p) { return mvn_ingest_blocks((long)p.n0 * p.n1); }

MVN_HD void mvn_normalize_rows(const NormalizeParams& p, long block, int tid) {
  const int wave = mvn_uniform(tid / MVN_INGEST_WAVE), lane = tid % MVN_INGEST_WAVE;
  const long rows = (long)p.n0 * p.n1;
  const long r_end = block * MVN_INGEST_ROWS + MVN_INGEST_ROWS < rows ? block * MVN_INGEST_ROWS + MVN_INGEST_ROWS : rows;
  for (long r = block * MVN_INGEST_ROWS + wave; r < r_end; r += MVN_INGEST_WG / MVN_INGEST_WAVE) {
    const long zi = r / p.n1;
    const int yi = (int)(r - zi * p.n1);
    const long row = mvn_uniform(((zi + p.o0) * p.D1 + yi + p.o1) * p.RP);
    if ((p.RP & 3) == 0) {  // aligned groups of 4 that meet the window (every group ends inside the row)
      const int g0 = p.o2 / 4, g1 = (p.o2 + p.n2 + 3) / 4;
      for (int q = g0 + lane; q < g1; q += MVN_INGEST_WAVE) {
        const long at = row + 4L * q;
        mvn_v4f W = *(const mvn_v4f*)(p.vols[0] + at);
        for (int v = 1; v < p.V; ++v) {
          const mvn_v4f w = *(const mvn_v4f*)(p.vols[v] + at);
#pragma unroll
          for (int j = 0; j < 4; ++j) W[j] = W[j] + w[j];
        }
        for (int v = 0; v < p.V; ++v) {
          mvn_v4f w = *(const mvn_v4f*)(p.vols[v] + at);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int xi = 4 * q + j - p.o2;
            if (xi >= 0 && xi < p.n2) w[j] = W[j] > 0.f ? w[j] / W[j] : 0.f;
          }
          *(mvn_v4f*)(p.vols[v] + at) = w;
        }
      }
    } else {
      for (int xi = lane; xi < p.n2; xi += MVN_INGEST_WAVE) {
        const long at = row + p.o2 + xi;
        float W = p.vols[0][at];
        for (int v = 1; v < p.V; ++v) W = W + p.vols[v][at];
        for (int v = 0; v < p.V; ++v) p.vols[v][at] = W > 0.f ? p.vols[v][at] / W : 0.f;
      }
    }
  }
}
