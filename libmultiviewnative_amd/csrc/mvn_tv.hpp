// mvn_tv.hpp -- the total-variation factor of the Richardson-Lucy update (Dey et al. 2006), one pass over psi.
//
// With regularisation kind MVN_REG_TV the update of a view multiplies its integral by
//
//   t = 1 / (1 - lambda * div(grad psi / |grad psi|_eps))
//
// (include/mvn_engine_api.h states the arithmetic operation by operation; mvn_tv_p and mvn_tv_t below are that
// statement).  k_tv_factor reads psi and writes t in psi's own layout - same index, same row pitch - once per view
// update, before the update pass that consumes it (Engine::conv_pair).
//
// Shape of a workgroup: MVN_TV_WG lanes own a tile of MVN_TV_TY x MVN_TV_TX voxels of a plane, MVN_TV_K voxels a
// lane (rows ty, ty + 4, ...: a wave reads and writes whole 256-byte runs), and walk MVN_TV_SEG planes along dim0.
// Per plane z:
//
//   stage    plane z + 1 of u, tile plus a one-voxel rim, into the LDS (plane z is there from the step before)
//   phase P  every lane forms (px, py, pz) of its voxels from the two staged planes, keeps them in registers and
//            leaves px, py in the LDS; lanes 0 .. TX + TY - 1 do the same for the rim: py of the row below the
//            tile, px of the column left of it
//   phase T  dv from the own registers, px[x-1] and py[y-1] out of the LDS and the pz of the plane behind, which
//            never left its register; t is stored
//
// A segment starts one plane early (that step forms pz only), so a volume is read once, plus 1 / MVN_TV_SEG of it
// and the rims - neighbouring workgroups' tiles, which the L2 holds - and t is written once.  Every axis is cyclic
// at the extent of the volume: staged rows, columns and planes are wrapped one by one, so an extent of 1 makes
// the neighbour the voxel itself and an extent of 2 makes x+1 and x-1 the same voxel with no special case.  The row
// padding of an odd last extent is never staged and never written.
//
// No cross-lane instructions and no atomics: the host emulation runs the same body with one "thread" that owns all
// MVN_TV_WG lanes (NL of them per thread; the per-lane registers are then an array).  The grid depends on the
// extents alone.
#pragma once

#include "mvn_pass_bodies.hpp"

#define MVN_TV_WG 256   // lanes of a workgroup
#define MVN_TV_TX 64    // tile: columns ...
#define MVN_TV_TY 16    // ... and rows of a plane
#define MVN_TV_SEG 32   // planes a workgroup walks
#define MVN_TV_K (MVN_TV_TX * MVN_TV_TY / MVN_TV_WG)                    // voxels of a lane per plane
#define MVN_TV_SX (MVN_TV_TX + 2)                                       // staged tile: columns x0 - 1 .. x0 + TX
#define MVN_TV_SY (MVN_TV_TY + 2)                                       // rows y0 - 1 .. y0 + TY
#define MVN_TV_NS ((MVN_TV_SX * MVN_TV_SY + MVN_TV_WG - 1) / MVN_TV_WG)  // staged floats of a lane per plane
#define MVN_TV_PP (MVN_TV_TX + 1)                                       // pitch of the px / py tiles (rim included)
#define MVN_TV_LDS_FLOATS (2 * MVN_TV_SX * MVN_TV_SY + 2 * (MVN_TV_TY + 1) * MVN_TV_PP)

struct TvParams {
  const float* psi;  // u
  float* t;          // the factor volume, psi's layout
  int d0, d1, d2;    // extents of the engine's volume
  int RP;            // row pitch (d2, or d2 + 1 for an odd d2)
  int ntx, nty, nseg;  // tiles along dim2 and dim1, segments along dim0
  float lambda;      // (float)lambda
  float e2;          // (float)epsilon * (float)epsilon
};

MVN_HD int mvn_tv_ceil(int n, int d) { return (n + d - 1) / d; }

// the geometry of a launch: a function of the extents only
MVN_HD void mvn_tv_geometry(TvParams& p) {
  p.ntx = mvn_tv_ceil(p.d2, MVN_TV_TX);
  p.nty = mvn_tv_ceil(p.d1, MVN_TV_TY);
  p.nseg = mvn_tv_ceil(p.d0, MVN_TV_SEG);
}
MVN_HD long mvn_tv_blocks(const TvParams& p) { return (long)p.ntx * p.nty * p.nseg; }

// v mod d for v >= -1
MVN_HD int mvn_tv_wrap(int v, int d) {
  v %= d;
  return v < 0 ? v + d : v;
}

// p = grad u / |grad u|_eps at one voxel: u and its neighbours at x+1, y+1, z+1
MVN_HD void mvn_tv_p(float u, float ux, float uy, float uz, float e2, float& px, float& py, float& pz) {
  MVN_FP_EXACT
  const float gz = uz - u, gy = uy - u, gx = ux - u;
  const float m = sqrtf(((gx * gx + gy * gy) + gz * gz) + e2);
  const float r = 1.0f / m;
  px = gx * r;
  py = gy * r;
  pz = gz * r;
}

MVN_HD float mvn_tv_t(float px, float pxm, float py, float pym, float pz, float pzm, float lambda) {
  MVN_FP_EXACT
  const float dv = ((px - pxm) + (py - pym)) + (pz - pzm);
  return 1.0f / (1.0f - lambda * dv);
}

// what a lane keeps across the phases of a plane and from plane to plane
struct TvLane {
  int soff[MVN_TV_NS];  // offsets inside a plane of the floats it stages (-1: none)
  float px[MVN_TV_K], py[MVN_TV_K], pz[MVN_TV_K];
  float pzm[MVN_TV_K];  // pz of the plane behind
};

// lanes tid, tid + nthreads, ... (NL of them) of workgroup `block`; lds: MVN_TV_LDS_FLOATS floats
template <int NL>
MVN_HD void mvn_tv_body(const TvParams& p, long block, float* lds, int tid, int nthreads) {
  constexpr int WG = MVN_TV_WG, TX = MVN_TV_TX, TY = MVN_TV_TY, K = MVN_TV_K, SX = MVN_TV_SX, SY = MVN_TV_SY,
                NS = MVN_TV_NS, PP = MVN_TV_PP, ROWS = WG / TX;
  TvLane st[NL];
  float* U = lds;
  float* PX = lds + 2 * SX * SY;
  float* PY = PX + (TY + 1) * PP;
  const int bx = (int)(block % p.ntx), by = (int)((block / p.ntx) % p.nty), seg = (int)(block / ((long)p.ntx * p.nty));
  const int x0 = bx * TX, y0 = by * TY, zs = seg * MVN_TV_SEG;
  const int ze = zs + MVN_TV_SEG < p.d0 ? zs + MVN_TV_SEG : p.d0;
  const long plane = (long)p.d1 * p.RP;

  for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int idx = t + j * WG;
      int off = -1;
      if (idx < SX * SY) {
        const int ey = idx / SX, ex = idx - ey * SX;
        off = mvn_tv_wrap(y0 - 1 + ey, p.d1) * p.RP + mvn_tv_wrap(x0 - 1 + ex, p.d2);
      }
      st[l].soff[j] = off;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) st[l].pzm[k] = 0.f;
  }
  // plane zs - 1 (it only yields the pz behind plane zs)
  {
    const float* src = p.psi + (long)mvn_tv_wrap(zs - 1, p.d0) * plane;
    for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
#pragma unroll
      for (int j = 0; j < NS; ++j)
        if (st[l].soff[j] >= 0) U[t + j * WG] = src[st[l].soff[j]];
    }
  }
  for (int z = zs - 1, cur = 0; z < ze; ++z, cur ^= 1) {
    float* Uc = U + cur * SX * SY;
    float* Un = U + (cur ^ 1) * SX * SY;
    {
      const float* src = p.psi + (long)mvn_tv_wrap(z + 1, p.d0) * plane;
      for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
        float v[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) v[j] = st[l].soff[j] >= 0 ? src[st[l].soff[j]] : 0.f;
#pragma unroll
        for (int j = 0; j < NS; ++j)
          if (st[l].soff[j] >= 0) Un[t + j * WG] = v[j];
      }
    }
    MVN_SYNC();
    // phase P
    for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
      const int tx = t % TX, tr = t / TX;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int ty = tr + k * ROWS;
        const int s = (ty + 1) * SX + tx + 1;
        mvn_tv_p(Uc[s], Uc[s + 1], Uc[s + SX], Un[s], p.e2, st[l].px[k], st[l].py[k], st[l].pz[k]);
        PX[(ty + 1) * PP + tx + 1] = st[l].px[k];
        PY[(ty + 1) * PP + tx + 1] = st[l].py[k];
      }
      if (t < TX + TY) {  // the rim: row y0 - 1 (py) and column x0 - 1 (px)
        const bool row = t < TX;
        const int ey = row ? 0 : t - TX + 1, ex = row ? t + 1 : 0;
        const int s = ey * SX + ex;
        float px, py, pz;
        mvn_tv_p(Uc[s], Uc[s + 1], Uc[s + SX], Un[s], p.e2, px, py, pz);
        if (row)
          PY[ey * PP + ex] = py;
        else
          PX[ey * PP + ex] = px;
      }
    }
    MVN_SYNC();
    // phase T
    for (int l = 0, t = tid; l < NL; ++l, t += nthreads) {
      const int tx = t % TX, tr = t / TX;
      if (z >= zs) {
        float* dst = p.t + (long)z * plane;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int ty = tr + k * ROWS;
          if (y0 + ty < p.d1 && x0 + tx < p.d2)
            dst[(long)(y0 + ty) * p.RP + x0 + tx] =
                mvn_tv_t(st[l].px[k], PX[(ty + 1) * PP + tx], st[l].py[k], PY[ty * PP + tx + 1], st[l].pz[k],
                         st[l].pzm[k], p.lambda);
        }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) st[l].pzm[k] = st[l].pz[k];
    }
    // (the next step's staging overwrites Uc, which nobody reads after the barrier above; its phase P writes PX and
    // PY behind the barrier that follows the staging)
  }
}

#ifdef MVN_HOST_EMU
// the launch of the host emulation (mvn_backend_emu.cpp; tools/tv_standalone.cpp runs it under sanitizers)
inline void mvn_tv_host(const TvParams& p) {
  const long nblocks = mvn_tv_blocks(p);
#pragma omp parallel for schedule(static)
  for (long blk = 0; blk < nblocks; ++blk) {
    float lds[MVN_TV_LDS_FLOATS];
    mvn_tv_body<MVN_TV_WG>(p, blk, lds, 0, 1);
  }
}
#endif
