// mvn_fuse.hpp -- fusion: the weighted average of the registered views, sum_v w_v I_v / sum_v w_v.
//
// include/mvn_engine_api.h states the arithmetic (mvn_fuse_resampled); per output voxel, views in view order, float32,
// every operation rounded once, nothing contracted:
//
//     t_v = w_v * s_v
//     N   = ((t_0 + t_1) + ...) + t_{V-1}          (starts from t_0 itself)
//     W   = ((w_0 + w_1) + ...) + w_{V-1}
//     F   = W > 0 ? N / W : fill
//
// (s_v, w_v) are the trilinear sample and the unnormalised blend weight of mvn_resample.hpp, both 0 where the voxel is
// not inside view v.  A uint16 output stores F >= 65535 ? 65535 : F > 0 ? rintf(F) : 0 (ties to even, a NaN gives 0).
//
//   k_fuse_resampled   from the V RAW stacks: mvn_resample_voxel<T> of every view per output voxel, so a view's sample and
//                      weight are the bits the resample pass gives, and ONE volume written - no image and no weights
//                      volumes in between.  The compact tile of k_resample3d (MVN_RS_TZ x MVN_RS_TY x MVN_RS_TX, a work
//                      item owns 4 consecutive columns) for the same cache reason.  The per-view record (source, strides,
//                      element type, geometry) lives in a table in device memory - V is unbounded - and is read once per
//                      view and row through the constant address space, i.e. into scalar registers; the element type
//                      is a wave-uniform branch, so the views of a call may mix uint16 and float32.  The loop over the
//                      views is OUTSIDE the 4 columns, so the row part of the coordinate is formed once per view and
//                      row; the column term comes from x itself.  The output is float32 or uint16 with element strides:
//                      one store of 4 elements (16 or 8 bytes) where rows are contiguous and pitches and base keep
//                      groups of 4 aligned, element stores otherwise.  Only the output's own elements are written.
//   k_fuse_volumes     the same formula on an engine's resident volumes: s_v and w_v read from the V image and V weights
//                      volumes behind a device table of pointers, over the window rows of the psi volume, in the shape
//                      of mvn_normalize_rows (a wave owns whole rows, 16-byte accesses on the same terms); elements
//                      outside the window keep what they hold.
//
// The bodies are plain C++ shared with the host emulation (mvn_backend_emu.cpp), like every other pass.
#pragma once

#include "mvn_resample.hpp"

// one view of k_fuse_resampled: 176 bytes (mvn_fuse_memory_resampled counts them)
struct FuseView {
  const void* src;       // element (0, 0, 0) of the raw stack (device memory)
  long long s0, s1, s2;  // its element strides (>= 0)
  int u16;               // its elements: uint16, else float32
  int reserved;
  ResampleGeom g;
};
static_assert(sizeof(FuseView) == 176, "mvn_fuse_memory_resampled documents the size of a view's record");

struct FuseParams {
  void* out;             // element (0, 0, 0) of the output (device memory)
  int out_u16;           // its elements: uint16, else float32
  long long q0, q1, q2;  // its element strides (> 0 wherever the extent is > 1)
  int n0, n1, n2;        // extents of the block
  const FuseView* views; // device table of V records
  int V;
  float fill;            // where no view contributes
};

struct FuseVolumesParams {
  float* psi;                // the volume written
  const float* const* vols;  // device table: V image volumes, then V weights volumes
  int V;
  long RP;
  int D1;
  int n0, n1, n2;
  int o0, o1, o2;
  float fill;
};

typedef unsigned short mvn_v4u16 __attribute__((vector_size(8)));

#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
// read-only for the whole launch and the same address in every lane: scalar loads
typedef const __attribute__((address_space(4))) FuseView* mvn_fuse_table_t;
#define MVN_FUSE_TABLE(p) ((mvn_fuse_table_t)(p))
#else
typedef const FuseView* mvn_fuse_table_t;
#define MVN_FUSE_TABLE(p) (p)
#endif

inline void mvn_fuse_check(const FuseParams& p) {
  if (!p.out || !p.views) throw std::invalid_argument("mvn: fuse: null pointer");
  if (p.V < 1) throw std::invalid_argument("mvn: fuse: no views");
  if (p.n0 < 1 || p.n1 < 1 || p.n2 < 1) throw std::invalid_argument("mvn: fuse: extents must be >= 1");
  const long long q[3] = {p.q0, p.q1, p.q2};
  const int n[3] = {p.n0, p.n1, p.n2};
  for (int d = 0; d < 3; ++d)
    if (q[d] < 0 || (n[d] > 1 && q[d] == 0)) throw std::invalid_argument("mvn: fuse: the output needs positive strides");
}
inline void mvn_fuse_volumes_check(const FuseVolumesParams& p) {
  const int n[3] = {p.n0, p.n1, p.n2}, o[3] = {p.o0, p.o1, p.o2};
  mvn_window_check("fuse", p.RP, p.o0 + p.n0, p.D1, n, o);
  if (!p.psi || !p.vols || p.V < 1) throw std::invalid_argument("mvn: fuse: no volumes");
}

MVN_HD long mvn_fuse_blocks(const FuseParams& p) {
  const long bz = (p.n0 + MVN_RS_TZ - 1) / MVN_RS_TZ, by = (p.n1 + MVN_RS_TY - 1) / MVN_RS_TY,
             bx = (p.n2 + MVN_RS_TX - 1) / MVN_RS_TX;
  return bz * by * bx;
}

MVN_HD unsigned short mvn_fuse_u16(float F) { return F >= 65535.f ? (unsigned short)65535 : F > 0.f ? (unsigned short)rintf(F) : (unsigned short)0; }

// sample and weight of one view at the 4 columns of a work item, added to the running sums (first: the sums start here)
template <typename T>
MVN_HD void mvn_fuse_view(const ResampleParams& rp, const double u[3], long x0, int n2, bool first, float N[4],
                          float W[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double* M = rp.g.M;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float im = 0.f, wt = 0.f;
    const long xi = x0 + j;
    if (xi < n2) {
      double c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double t = M[4 * k + 2] * (double)xi;  // (formed from x itself: no running sum along the row)
        const double w = u[k] + t;
        c[k] = w + M[4 * k + 3];
      }
      float s, r;
      if (mvn_resample_voxel<T>(rp, c, &s, &r)) im = s, wt = r;
    }
    const float t = wt * im;
    N[j] = first ? t : N[j] + t;
    W[j] = first ? wt : W[j] + wt;
  }
}

MVN_HD void mvn_fuse_tile(const FuseParams& p, long block, int tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long by = (p.n1 + MVN_RS_TY - 1) / MVN_RS_TY, bx = (p.n2 + MVN_RS_TX - 1) / MVN_RS_TX;
  const long tz = block / (by * bx), rem = block - tz * (by * bx);
  const long ty = rem / bx, tx = rem - ty * bx;
  const int cg = tid % (MVN_RS_TX / 4), ry = (tid / (MVN_RS_TX / 4)) % MVN_RS_TY;
  const int rz = tid / ((MVN_RS_TX / 4) * MVN_RS_TY);
  constexpr int ZSTEP = MVN_RS_WG / ((MVN_RS_TX / 4) * MVN_RS_TY);
  const long x0 = tx * MVN_RS_TX + cg * 4;
  const long y = ty * MVN_RS_TY + ry;
  if (y >= p.n1 || x0 >= p.n2) return;
  const size_t esz = p.out_u16 ? sizeof(uint16_t) : sizeof(float);
  // groups of 4 columns start on multiples of 4 elements: one store where rows are contiguous and every row starts aligned
  const bool wide = p.q2 == 1 && (p.q0 & 3) == 0 && (p.q1 & 3) == 0 && ((uintptr_t)p.out & (4 * esz - 1)) == 0 &&
                    x0 + 4 <= p.n2;
  const mvn_fuse_table_t views = MVN_FUSE_TABLE(p.views);
  for (int kz = rz; kz < MVN_RS_TZ; kz += ZSTEP) {
    const long z = tz * MVN_RS_TZ + kz;
    if (z >= p.n0) break;
    float N[4], W[4];
    for (int v = 0; v < p.V; ++v) {
      ResampleParams rp = {};
      rp.src = views[v].src, rp.s0 = views[v].s0, rp.s1 = views[v].s1, rp.s2 = views[v].s2;
#pragma unroll
      for (int k = 0; k < 3; ++k) rp.g.m[k] = views[v].g.m[k], rp.g.border[k] = views[v].g.border[k], rp.g.range[k] = views[v].g.range[k];
#pragma unroll
      for (int i = 0; i < 12; ++i) rp.g.M[i] = views[v].g.M[i];
      // the part of the coordinate that every voxel of the row (z, y) shares
      double u[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double a = rp.g.M[4 * k] * (double)z;
        const double b = rp.g.M[4 * k + 1] * (double)y;
        u[k] = a + b;
      }
      if (views[v].u16)
        mvn_fuse_view<uint16_t>(rp, u, x0, p.n2, v == 0, N, W);
      else
        mvn_fuse_view<float>(rp, u, x0, p.n2, v == 0, N, W);
    }
    float F[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) F[j] = W[j] > 0.f ? N[j] / W[j] : p.fill;
    const long long at = z * p.q0 + y * p.q1 + x0 * p.q2;
    if (p.out_u16) {
      uint16_t* o = (uint16_t*)p.out + at;
      if (wide) {
        const mvn_v4u16 ov = {mvn_fuse_u16(F[0]), mvn_fuse_u16(F[1]), mvn_fuse_u16(F[2]), mvn_fuse_u16(F[3])};
        *(mvn_v4u16*)o = ov;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < p.n2) o[j * p.q2] = mvn_fuse_u16(F[j]);
      }
    } else {
      float* o = (float*)p.out + at;
      if (wide) {
        const mvn_v4f ov = {F[0], F[1], F[2], F[3]};
        *(mvn_v4f*)o = ov;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < p.n2) o[j * p.q2] = F[j];
      }
    }
  }
}

MVN_HD long mvn_fuse_volumes_blocks(const FuseVolumesParams& p) { return mvn_ingest_blocks((long)p.n0 * p.n1); }

MVN_HD void mvn_fuse_rows(const FuseVolumesParams& p, long block, int tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
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
        mvn_v4f N, W;
        for (int v = 0; v < p.V; ++v) {
          const mvn_v4f s = *(const mvn_v4f*)(p.vols[v] + at);
          const mvn_v4f w = *(const mvn_v4f*)(p.vols[p.V + v] + at);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float t = w[j] * s[j];
            N[j] = v == 0 ? t : N[j] + t;
            W[j] = v == 0 ? w[j] : W[j] + w[j];
          }
        }
        mvn_v4f o = *(const mvn_v4f*)(p.psi + at);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int xi = 4 * q + j - p.o2;
          if (xi >= 0 && xi < p.n2) o[j] = W[j] > 0.f ? N[j] / W[j] : p.fill;
        }
        *(mvn_v4f*)(p.psi + at) = o;
      }
    } else {
      for (int xi = lane; xi < p.n2; xi += MVN_INGEST_WAVE) {
        const long at = row + p.o2 + xi;
        float N = 0.f, W = 0.f;
        for (int v = 0; v < p.V; ++v) {
          const float s = p.vols[v][at], w = p.vols[p.V + v][at];
          const float t = w * s;
          N = v == 0 ? t : N + t;
          W = v == 0 ? w : W + w;
        }
        p.psi[at] = W > 0.f ? N / W : p.fill;
      }
    }
  }
}
