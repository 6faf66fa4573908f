// mvn_reflect.hpp -- the margins of an embedded stack as its mirror image (padding policy "reflect").
//
// Under "zero" the volume around a stack's window holds zeros.  Under "reflect" volume voxel (z, y, x) holds the
// stack's voxel (f(z - o0, n0), f(y - o1, n1), f(x - o2, n2)) with
//
//     f(i, n):  m = i mod 2n (non-negative);  f = m < n ? m : 2n - 1 - m
//
// whole-sample symmetric extension, periodic with period 2n (numpy.pad's "symmetric"): margins wider than the stack
// and extents of 1 are no special case.  The row padding of an odd last extent keeps its zeros.
//
// The fill runs IN PLACE, behind whatever placed the stack in its window (Engine::ingest_stack: the copies and the
// ingest pass of mvn_ingest.hpp), and only copies.  The extension is separable, so three launches of one kernel do it:
//
//   axis 2   rows inside the window: the columns outside the window, from the row itself (element accesses: the
//            mirror reverses the order of the columns)
//   axis 1   planes inside the window: the margin rows, each the whole row (all RP elements, the columns axis 2 has
//            filled and the row padding included) o1 + f(y - o1, n1) of its plane
//   axis 0   the margin planes, each row from the same row of plane o0 + f(z - o0, n0)
//
// Every launch reads inside the window of its axis and writes outside it, so no launch reads what it writes; each
// reads what the one before has written, so they run in this order on one stream.  A launch along an axis without a
// margin is skipped (mvn_reflect_rows_of() == 0).  Together they write the margins and nothing else: 25.4 % of a
// 512^3 stack's 542 x 576 x 576 volume.
//
//   k_reflect3d<T>  one workgroup per run of MVN_INGEST_ROWS destination rows, a wave owns whole rows, source and
//                   destination row addresses are wave-uniform, a lane adds its column (mvn_ingest.hpp's shape).  Row
//                   copies take 16-byte accesses where a row is a whole number of them (float32: RP a multiple of 4;
//                   uint16: of 8 - every row of the volume then starts 16-byte aligned), 4-byte accesses otherwise
//                   (RP is even).  T is the element type of the volume: float32, or uint16 in image storage mode 1
//                   (the float32 volume's element grid at 2 bytes).
//
// The bodies are plain C++ shared with the host emulation (mvn_backend_emu.cpp), like every other pass.
#pragma once

#include <stdint.h>

#include <stdexcept>

#include "mvn_ingest.hpp"

struct ReflectParams {
  void* vol;       // the engine volume: float32 or uint16
  long RP;         // its row pitch in elements (even)
  int D0, D1, D2;  // its extents
  int n0, n1, n2;  // extents of the stack = of the embedding window
  int o0, o1, o2;  // the window's offset inside the volume
  int axis;        // which of the three launches
};

inline void mvn_reflect_check(const ReflectParams& p) {
  const int D[3] = {p.D0, p.D1, p.D2}, n[3] = {p.n0, p.n1, p.n2}, o[3] = {p.o0, p.o1, p.o2};
  for (int d = 0; d < 3; ++d)
    if (n[d] < 1 || o[d] < 0 || (long)o[d] + n[d] > D[d] || n[d] > 0x3fffffff)
      throw std::invalid_argument("mvn: reflect fill: the window does not fit the volume");
  if (!p.vol || p.RP < p.D2 || (p.RP & 1)) throw std::invalid_argument("mvn: reflect fill: bad volume");
}

// index of the stack's element that volume index o + i mirrors
MVN_HD int mvn_reflect_index(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// destination rows of the launch along p.axis (0: nothing to fill, no launch)
MVN_HD long mvn_reflect_rows_of(const ReflectParams& p) {
  if (p.axis == 2) return p.D2 > p.n2 ? (long)p.n0 * p.n1 : 0;
  if (p.axis == 1) return (long)p.n0 * (p.D1 - p.n1);
  return (long)(p.D0 - p.n0) * p.D1;
}

// the k-th index outside the window [o, o + n)
MVN_HD int mvn_reflect_outside(int k, int o, int n) { return k < o ? k : k + n; }

// the q-th aligned unit V of row s into row d
template <typename V>
MVN_HD void mvn_reflect_copy(char* d, const char* s, int q) {
  V v;
  __builtin_memcpy(&v, __builtin_assume_aligned(s + (long)q * (long)sizeof(V), sizeof(V)), sizeof(V));
  __builtin_memcpy(__builtin_assume_aligned(d + (long)q * (long)sizeof(V), sizeof(V)), &v, sizeof(V));
}

template <typename T>
MVN_HD void mvn_reflect_rows(const ReflectParams& p, long block, int tid) {
  const int wave = mvn_uniform(tid / MVN_INGEST_WAVE), lane = tid % MVN_INGEST_WAVE;
  const long rows = mvn_reflect_rows_of(p);
  const long r_end = block * MVN_INGEST_ROWS + MVN_INGEST_ROWS < rows ? block * MVN_INGEST_ROWS + MVN_INGEST_ROWS : rows;
  const long row_bytes = p.RP * (long)sizeof(T);
  for (long r = block * MVN_INGEST_ROWS + wave; r < r_end; r += MVN_INGEST_WG / MVN_INGEST_WAVE) {
    // (everything up to the column loops is the same in every lane of the wave)
    if (p.axis == 2) {
      const long zi = r / p.n1;
      const int yi = (int)(r - zi * p.n1);
      T* d = mvn_uniform((T*)p.vol + ((zi + p.o0) * p.D1 + yi + p.o1) * p.RP);
      const T* s = d + p.o2;
      const int margin = p.D2 - p.n2;
      for (int k = lane; k < margin; k += MVN_INGEST_WAVE) {
        const int x = mvn_reflect_outside(k, p.o2, p.n2);
        d[x] = s[mvn_reflect_index(x - p.o2, p.n2)];
      }
      continue;
    }
    long zd, zs;
    int yd, ys;
    if (p.axis == 1) {
      const int m1 = p.D1 - p.n1;
      const long zi = r / m1;
      zd = zs = zi + p.o0;
      yd = mvn_reflect_outside((int)(r - zi * m1), p.o1, p.n1);
      ys = p.o1 + mvn_reflect_index(yd - p.o1, p.n1);
    } else {
      const long k = r / p.D1;
      yd = ys = (int)(r - k * p.D1);
      zd = mvn_reflect_outside((int)k, p.o0, p.n0);
      zs = p.o0 + mvn_reflect_index((int)zd - p.o0, p.n0);
    }
    char* d = mvn_uniform((char*)p.vol + (zd * p.D1 + yd) * row_bytes);
    const char* s = mvn_uniform((const char*)p.vol + (zs * p.D1 + ys) * row_bytes);
    if ((row_bytes & 15) == 0) {
      const int items = (int)(row_bytes / 16);
      for (int q = lane; q < items; q += MVN_INGEST_WAVE) mvn_reflect_copy<mvn_v4u32>(d, s, q);
    } else {
      const int items = (int)(row_bytes / 4);
      for (int q = lane; q < items; q += MVN_INGEST_WAVE) mvn_reflect_copy<unsigned>(d, s, q);
    }
  }
}
