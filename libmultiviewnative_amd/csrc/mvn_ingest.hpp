// mvn_ingest.hpp -- a caller's stack into the engine's volume in ONE pass, and psi back out.
//
// Every stack enters the engine as a StackRef (mvn_engine.hpp) through Engine::ingest_stack: float32 or uint16, in host
// or device memory, with element strides (the described entry points, mvn_deconvolve_described and
// mvn_engine_*_described in include/mvn_engine_api.h, take stacks as the caller has them; the plain ones describe theirs
// as dense float32 in host memory).  A float32 stack in host memory with contiguous rows is placed with a copy of its
// window (H2D, or H2D into the embedding scratch and a strided device copy), which relies on margins cleared when the
// volume was allocated; every other stack - uint16, in device memory, or one value for every voxel - takes the ingest
// pass, which converts, follows strides, reads the caller's device memory and depends on no earlier clear.  (In image
// storage mode 1 a uint16 image keeps its element type: a host stack with contiguous rows into a volume of its own
// extents is then placed by the copy as well, with 2-byte pitches, and the pass has a uint16 -> uint16 form.)
// (An image that is a RAW view with a geometry is not copied but resampled into the window: mvn_resample.hpp.)
//
//   k_ingest3d<T>   one workgroup per run of MVN_INGEST_ROWS rows of the engine volume (row pitch RP floats, plane
//                   pitch D1 * RP).  It writes EVERY float of its rows - the converted source inside the embedding
//                   window, zeros in the margins and in the row padding - so no separate clear is needed.  A wave
//                   owns whole rows: the row's source and destination addresses are wave-uniform (scalar registers,
//                   as mvn_dim0_direct.hpp keeps its planes), a lane adds its column.
//                   Fast form (stride[2] == 1): a work item converts 16 source bytes (4 floats / 8 uint16) of the
//                   destination-aligned column group it owns - one 16-byte load where that group lies inside the
//                   window and its source address is 16-byte aligned (decided per row: the groups of a row are 16
//                   bytes apart), scalar loads for the head / tail groups and for unaligned rows - and stores 16
//                   bytes at a time (the engine side is aligned whenever RP is a multiple of 4; rows of an odd last
//                   extent with RP = 2 mod 4 take 4-byte stores).  The source is read once: the loads carry the
//                   non-temporal hint, the stores are plain (the first pass of the loop reads them back).
//                   General form (any positive stride[2], and the broadcast {0, 0, 0}): scalar loads, same stores.
//                   uint16 destination (k_ingest3d_u16, image storage mode 1, mvn_engine_api.h): the
//                   same pass without the conversion - the volume is the float32 volume's element grid (row pitch RP
//                   elements) at 2 bytes per voxel.  A work item owns 8 columns: 16 source bytes as above, ONE 16-byte
//                   store where RP is a multiple of 8 (every row then starts 16-byte aligned and ends with a whole
//                   group); other row pitches (RP is even: odd last extents, and even ones such as 20) take 4-byte
//                   stores of column pairs, the last pair of a row included.
//   k_extract3d     the window of psi out of the engine volume into a strided float32 destination.
//
// The bodies are plain C++ shared with the host emulation (mvn_backend_emu.cpp), like every other pass.
#pragma once

#include <stdint.h>

#include "mvn_dim0_direct.hpp"  // mvn_uniform

#define MVN_INGEST_WG 256    // work items of a workgroup: 4 waves
#define MVN_INGEST_WAVE 64
#define MVN_INGEST_ROWS 16   // rows of a workgroup: 4 per wave, 32 KB of output at 512 floats per row

struct IngestParams {
  void* dst;             // the engine volume: float32, or uint16 for the uint16 -> uint16 form
  long RP;               // its row pitch in elements (even)
  int D1;                // rows of a plane
  long rows;             // D0 * D1
  const void* src;       // element (0, 0, 0) of the stack; unused with use_value
  long long s0, s1, s2;  // element strides of the stack ({0, 0, 0}: one value for every voxel)
  int n0, n1, n2;        // extents of the stack = of the embedding window
  int o0, o1, o2;        // the window's offset inside the volume
  int use_value;         // 1: every voxel of the window is `value` (a broadcast stack in host memory)
  float value;
};

struct ExtractParams {
  const float* src;      // the engine volume
  long RP;
  int D1;
  float* dst;            // element (0, 0, 0) of the destination
  long long s0, s1, s2;  // its element strides (positive)
  int n0, n1, n2;
  int o0, o1, o2;
};

typedef float mvn_v4f __attribute__((vector_size(16)));
typedef unsigned short mvn_v8u16 __attribute__((vector_size(16)));

template <typename T>
struct IngestVec;
template <>
struct IngestVec<float> {
  typedef mvn_v4f type;
};
template <>
struct IngestVec<uint16_t> {
  typedef mvn_v8u16 type;
};

// 16 aligned bytes of a stack that is read exactly once
template <typename V>
MVN_HD V mvn_ingest_load16(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
  return __builtin_nontemporal_load((const V*)p);
#else
  V v;
  __builtin_memcpy(&v, p, sizeof(V));
  return v;
#endif
}

template <typename T>
MVN_HD T mvn_ingest_load1(const T* p) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

MVN_HD long mvn_ingest_blocks(long rows) { return (rows + MVN_INGEST_ROWS - 1) / MVN_INGEST_ROWS; }

typedef unsigned int mvn_v4u32 __attribute__((vector_size(16)));

// 8 uint16 values of a work item into the uint16 row d at column x0
MVN_HD void mvn_ingest_store_u16(uint16_t* d, int x0, long RP, const uint16_t* v) {
  unsigned w[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) w[g] = (unsigned)v[2 * g] | ((unsigned)v[2 * g + 1] << 16);
  if ((RP & 7) == 0) {  // (x0 + 8 <= RP for every work item of the row)
    mvn_v4u32 o = {w[0], w[1], w[2], w[3]};
    *(mvn_v4u32*)(void*)(d + x0) = o;
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (x0 + 2 * g < RP) __builtin_memcpy(__builtin_assume_aligned(d + x0 + 2 * g, 4), &w[g], 4);
  }
}

template <typename T, typename D = float>
MVN_HD void mvn_ingest_rows(const IngestParams& p, long block, int tid) {
  constexpr int E = 16 / (int)sizeof(T);  // columns of a work item
  static_assert(sizeof(D) == 4 || (sizeof(D) == 2 && sizeof(T) == 2), "float32 volumes, or uint16 -> uint16");
  const int wave = mvn_uniform(tid / MVN_INGEST_WAVE), lane = tid % MVN_INGEST_WAVE;
  const long r_end = block * MVN_INGEST_ROWS + MVN_INGEST_ROWS < p.rows ? block * MVN_INGEST_ROWS + MVN_INGEST_ROWS : p.rows;
  const int items = (int)((p.RP + E - 1) / E);
  const bool wide_stores = (p.RP & 3) == 0;
  for (long r = block * MVN_INGEST_ROWS + wave; r < r_end; r += MVN_INGEST_WG / MVN_INGEST_WAVE) {
    // (everything up to the column loop is the same in every lane of the wave)
    const long z = r / p.D1;
    const int y = (int)(r - z * p.D1);
    const long zi = z - p.o0;
    const int yi = y - p.o1;
    const bool inside = zi >= 0 && zi < p.n0 && yi >= 0 && yi < p.n1;
    D* d = mvn_uniform((D*)p.dst + r * p.RP);
    const T* s = nullptr;
    if (inside && !p.use_value) s = mvn_uniform((const T*)p.src + zi * p.s0 + (long long)yi * p.s1);
    // the source of column group x0 is s + (x0 - o2): 16-byte aligned for every group of the row, or for none
    const bool vec = s && p.s2 == 1 && (((uintptr_t)s - (uintptr_t)p.o2 * sizeof(T)) & 15) == 0;
    for (int q = lane; q < items; q += MVN_INGEST_WAVE) {
      const int x0 = q * E, xi0 = x0 - p.o2;
      D v[E];
      if (vec && xi0 >= 0 && xi0 + E <= p.n2) {
        const typename IngestVec<T>::type t = mvn_ingest_load16<typename IngestVec<T>::type>(s + xi0);
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = (D)t[j];
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const int xi = xi0 + j;
          D f = 0;
          if (inside && xi >= 0 && xi < p.n2) f = p.use_value ? (D)p.value : (D)mvn_ingest_load1(s + (long long)xi * p.s2);
          v[j] = f;
        }
      }
      if constexpr (sizeof(D) == 2) {
        mvn_ingest_store_u16((uint16_t*)d, x0, p.RP, (const uint16_t*)v);
      } else if (wide_stores) {
#pragma unroll
        for (int g = 0; g < E; g += 4)
          if (x0 + g < p.RP) {
            mvn_v4f o = {v[g], v[g + 1], v[g + 2], v[g + 3]};
            *(mvn_v4f*)(d + x0 + g) = o;
          }
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j)
          if (x0 + j < p.RP) d[x0 + j] = v[j];
      }
    }
  }
}

MVN_HD long mvn_extract_blocks(const ExtractParams& p) {
  return ((long)p.n0 * p.n1 + MVN_INGEST_ROWS - 1) / MVN_INGEST_ROWS;
}

MVN_HD void mvn_extract_rows(const ExtractParams& p, long block, int tid) {
  const int wave = mvn_uniform(tid / MVN_INGEST_WAVE), lane = tid % MVN_INGEST_WAVE;
  const long rows = (long)p.n0 * p.n1;
  const long r_end = block * MVN_INGEST_ROWS + MVN_INGEST_ROWS < rows ? block * MVN_INGEST_ROWS + MVN_INGEST_ROWS : rows;
  for (long r = block * MVN_INGEST_ROWS + wave; r < r_end; r += MVN_INGEST_WG / MVN_INGEST_WAVE) {
    const long zi = r / p.n1;
    const int yi = (int)(r - zi * p.n1);
    const float* s = mvn_uniform(p.src + ((zi + p.o0) * p.D1 + yi + p.o1) * p.RP + p.o2);
    float* d = mvn_uniform(p.dst + zi * p.s0 + (long long)yi * p.s1);
    for (int x = lane; x < p.n2; x += MVN_INGEST_WAVE) d[(long long)x * p.s2] = s[x];
  }
}
