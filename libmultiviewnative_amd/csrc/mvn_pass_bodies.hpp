// mvn_pass_bodies.hpp -- workgroup bodies of the FFT pass kernels and the RL pointwise math.
//
// One body = what one workgroup does for one tile; `tid`/`nthreads` enumerate the work items
// of each phase, phases are separated by MVN_SYNC().  On the device the bodies are wrapped by
// __global__ kernels (mvn_kernels.hip); on a CPU-only box host_emu.cpp runs them with one
// "thread" per workgroup to validate the index math against numpy.
//
// Reference semantics restated here:
//   - un-normalised r2c / c2r over the last axis + c2c over the other two
//     (inc/cufft_utils.cuh:41-75, inc/fft_utils.h:55-104)
//   - spectrum multiply  F <- F*G  (inc/cuda_kernels.cuh:213-242; the 1/N scale is folded into G)
//   - quotient           I <- view * float(1.0/I)          (inc/cpu_kernels.h:19-26)
//   - update             psi <- w*(next-psi)+psi, next from the clamp/Tikhonov chain
//                                                           (inc/cpu_kernels.h:28-90)
#pragma once

#include <math.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "mvn_fft_core.hpp"

// The RL pointwise math mirrors the reference's rounding step by step: no FMA contraction there
// (the FFT butterflies may contract freely).  gcc has no per-function switch; the emulation
// build passes -ffp-contract=off globally instead.
#if defined(__clang__)
#define MVN_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define MVN_FP_EXACT
#endif

enum MvnEpilogue {
  MVN_EPI_STORE = 0,   // out = x * scale
  MVN_EPI_DIVIDE = 1,  // out = view * float(1.0 / (x*scale))
  MVN_EPI_UPDATE = 2,  // psi = w * (next(psi, x*scale) - psi) + psi
  MVN_EPI_DELTA = 3,   // delta (+)= w * (next(psi, x*scale) - psi)     (simultaneous mode)
  MVN_EPI_UPDATE_STATS = 4,  // UPDATE, plus the convergence statistics of the window (MvnStatsParams)
  MVN_EPI_DIVIDE_U16 = 5,    // DIVIDE with the view held as uint16 (EpilogueParams::view16): same quotient, bit for bit
  // total-variation regularisation (mvn_tv.hpp): the integral x*scale is multiplied by the factor tv[i] before `next`
  MVN_EPI_UPDATE_TV = 6,        // psi = w * (next(psi, (x*scale) * tv) - psi) + psi
  MVN_EPI_UPDATE_STATS_TV = 7,  // UPDATE_TV, plus the convergence statistics
  // noise model (camera background + per-sweep likelihood): the quotient against m = x*scale + background, plus the
  // statistics {D, Y, M} of the window (MvnStatsParams, MvnNmAcc)
  MVN_EPI_DIVIDE_NM = 8,      // view as float32
  MVN_EPI_DIVIDE_NM_U16 = 9,  // view as uint16 (EpilogueParams::view16)
  MVN_EPI_COUNT               // (not a mode: one past the last)
};
// A new mode is added HERE, in the predicates below (mvn_epi_allowed is the one table of which pass takes which
// mode) and in the bodies - nowhere else: both backends reach the bodies through mvn_epi_dispatch.

// the epilogues that read psi and the weights
constexpr bool mvn_epi_reads_psi(int epi) {
  return epi == MVN_EPI_UPDATE || epi == MVN_EPI_DELTA || epi == MVN_EPI_UPDATE_STATS || epi == MVN_EPI_UPDATE_TV ||
         epi == MVN_EPI_UPDATE_STATS_TV;
}
// the epilogues that multiply the integral by the total-variation factor, and the mode each of them extends
constexpr bool mvn_epi_tv(int epi) { return epi == MVN_EPI_UPDATE_TV || epi == MVN_EPI_UPDATE_STATS_TV; }
constexpr int mvn_epi_base(int epi) {
  return epi == MVN_EPI_UPDATE_TV ? (int)MVN_EPI_UPDATE : epi == MVN_EPI_UPDATE_STATS_TV ? (int)MVN_EPI_UPDATE_STATS : epi;
}
// the mode whose arithmetic an epilogue runs once its operands are floats
constexpr int mvn_epi_math(int epi) { return epi == MVN_EPI_DIVIDE_U16 ? (int)MVN_EPI_DIVIDE : mvn_epi_base(epi); }
// the noise-model divide epilogues, the epilogues on a uint16 view, and every epilogue that forms the quotient
constexpr bool mvn_epi_nm(int epi) { return epi == MVN_EPI_DIVIDE_NM || epi == MVN_EPI_DIVIDE_NM_U16; }
constexpr bool mvn_epi_u16(int epi) { return epi == MVN_EPI_DIVIDE_U16 || epi == MVN_EPI_DIVIDE_NM_U16; }
constexpr bool mvn_epi_divides(int epi) { return epi == MVN_EPI_DIVIDE || mvn_epi_u16(epi) || mvn_epi_nm(epi); }
// the epilogues that keep statistics of the window: the convergence statistics, the noise model's (above)
constexpr bool mvn_epi_stats(int epi) { return mvn_epi_base(epi) == MVN_EPI_UPDATE_STATS; }
// The run-time-radix bodies (rows_c2r_even_body / rows_c2r_odd_body) are one form for the four modes they tell apart
// at run time, by EpilogueParams::mode, and a form of its own for every other mode.
constexpr int mvn_epi_generic_form(int epi) {
  return (epi == MVN_EPI_DIVIDE || epi == MVN_EPI_UPDATE || epi == MVN_EPI_DELTA) ? (int)MVN_EPI_STORE : epi;
}

// the last-axis passes (the values of KIND in mvn_fixed.hpp and of MvnWaveRowsMode) and the modes each of them takes:
// r2c has no epilogue (its launches leave the mode at STORE), DELTA accumulates into a volume and is never fused
enum MvnPassKind { MVN_PASS_R2C = 0, MVN_PASS_C2R = 1, MVN_PASS_C2R_R2C = 2 };
constexpr bool mvn_epi_allowed(int kind, int epi) {
  return epi >= 0 && epi < MVN_EPI_COUNT &&
         (kind == MVN_PASS_R2C ? epi == MVN_EPI_STORE : kind == MVN_PASS_C2R ? true : kind == MVN_PASS_C2R_R2C && epi != MVN_EPI_DELTA);
}

// ---- launch side (host only): from the run-time mode of a launch to a compile-time constant -------------------------
// mvn_epi_dispatch<KIND>(mode, f) calls f(std::integral_constant<int, EPI>{}) for the mode of the launch - GENERIC:
// for its form in the run-time-radix bodies - and throws for a mode the pass does not take.  f is instantiated for the
// modes of KIND only, so a backend compiles exactly the kernels its passes can launch.
template <int KIND, bool GENERIC, int EPI, typename F>
inline void mvn_epi_dispatch_from(int mode, F& f) {
  if constexpr (EPI < MVN_EPI_COUNT) {
    if constexpr (mvn_epi_allowed(KIND, EPI)) {
      if (mode == EPI) return f(std::integral_constant<int, GENERIC ? mvn_epi_generic_form(EPI) : EPI>{});
    }
    mvn_epi_dispatch_from<KIND, GENERIC, EPI + 1>(mode, f);
  } else {
    static const char* const pass[] = {"r2c", "c2r", "fused c2r + r2c"};
    throw std::invalid_argument("mvn: epilogue mode " + std::to_string(mode) + " in a " + pass[KIND] + " last-axis pass");
  }
}
template <int KIND, bool GENERIC = false, typename F>
inline void mvn_epi_dispatch(int mode, F&& f) {
  static_assert(KIND >= MVN_PASS_R2C && KIND <= MVN_PASS_C2R_R2C, "a last-axis pass");
  mvn_epi_dispatch_from<KIND, GENERIC, 0>(mode, f);
}

// the tile width of the run-time-radix kernels
template <typename F>
inline void mvn_dispatch_tile_width(int T, F&& f) {
  switch (T) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 1: return f(std::integral_constant<int, 1>{});
    default: throw std::invalid_argument("mvn: unsupported tile width");
  }
}

// scratch of the lane reduction of the convergence statistics: n doubles (sum), n doubles (mass), n floats (max);
// of the noise model's: 3 n doubles
MVN_HD constexpr long mvn_stat_lds_bytes(int nthreads) { return 20L * nthreads; }
MVN_HD constexpr long mvn_nm_lds_bytes(int nthreads) { return 24L * nthreads; }
// the LDS a launch of the run-time-radix kernels needs for its mode's reduction (at least: the tile may be larger;
// the fixed and wave-row kernels reduce inside the LDS they have)
constexpr long mvn_epi_extra_lds_bytes(int epi, int nthreads) {
  return mvn_epi_stats(epi) ? mvn_stat_lds_bytes(nthreads) : mvn_epi_nm(epi) ? mvn_nm_lds_bytes(nthreads) : 0;
}
// wave-row launches (mvn_wave_rows.hpp): workgroups per resident slot - 32 where the fused pass also reads psi and
// the weights, 16 otherwise - and the bit of MVN_WAVE_ROWS_MASK that enables the launch
constexpr long mvn_wave_rows_per_slot(int kind, int epi) { return kind == MVN_PASS_C2R_R2C && mvn_epi_reads_psi(epi) ? 32 : 16; }
constexpr int mvn_wave_rows_kind_bit(int kind, int epi) {
  return kind == MVN_PASS_R2C ? 1 : kind == MVN_PASS_C2R ? (epi == MVN_EPI_DELTA ? 16 : 2) : (mvn_epi_divides(epi) ? 4 : 8);
}

struct EpilogueParams {
  int mode;
  float scale;          // applied to the raw inverse-transform output first
  union {
    const float* view;            // DIVIDE
    const unsigned short* view16; // DIVIDE_U16: the same element grid (row pitch RP elements) at 2 bytes per voxel
  };
  float* psi;           // UPDATE (in/out), DELTA (in)
  const float* weights; // UPDATE / DELTA
  float* delta;         // DELTA
  int accumulate;       // DELTA: 0 -> store, 1 -> add
  double lambda;        // > 0 selects the Tikhonov branch
  float lambda_inv;     // float(1.f / lambda)   (inc/cpu_kernels.h:71)
  float min_value;
  int guard_zero_view;  // DIVIDE: a view voxel that is exactly 0 gives quotient 0 even where the
                        // blurred estimate is 0 (0 * 1/0 = NaN otherwise); only set for the
                        // good-size zero-padding mode, whose extra zeros lie beyond the PSF's reach
  // The convolution this pass ends ran its dim0 leg as a direct convolution (mvn_dim0_direct.hpp), which stores
  // `poison_epoch` into *poison when its input held a non-finite value: the whole volume then has to come out
  // NaN, as it does through an FFT along dim0 (inc/cpu_convolve.h:256-268).  No such leg: a zero word and the
  // epoch 0xffffffff (Plan3D::no_poison) - the pointer is never null when a pass is launched.
  const unsigned* poison;
  unsigned poison_epoch;
  float background;     // DIVIDE_NM / DIVIDE_NM_U16: the view's camera offset b, m = x*scale + b (0: m = x*scale)
  const float* tv;      // UPDATE_TV / UPDATE_STATS_TV: the factor volume, psi's layout (mvn_tv.hpp)
};

// the total-variation factor of element i / of the pair (i, i + 1), loaded at its use
template <bool TV>
MVN_HD float mvn_tv_one(const EpilogueParams& e, long i) {
  if constexpr (TV)
    return e.tv[i];
  else
    return 1.f;
}
template <bool TV>
MVN_HD cfloat mvn_tv_pair(const EpilogueParams& e, long i) {
  if constexpr (TV)
    return *reinterpret_cast<const cfloat*>(e.tv + i);
  else
    return cmake(1.f, 1.f);
}

// Once per workgroup, before the first epilogue: a reported non-finite input turns the scale every raw output is
// multiplied with first into NaN - and with it every voxel (DIVIDE: view * 1 / NaN; UPDATE / DELTA: the clamp
// chain maps NaN to minValue) - at no cost per element.
MVN_HD void mvn_arm_poison(EpilogueParams& e) {
  // (no branch, and selected as an integer: the word, the epoch and the scale are the same for every lane, and an integer
  // select of scalars stays in a scalar register where a float select would move the scale into a vector one)
  unsigned bits;
  __builtin_memcpy(&bits, &e.scale, sizeof(bits));
  bits = *e.poison == e.poison_epoch ? 0x7fc00000u : bits;
  __builtin_memcpy(&e.scale, &bits, sizeof(bits));
}

// quotient with the optional guard above
MVN_HD float mvn_quotient_g(float view, float blurred, int guard);

// ---- uint16 views (MVN_EPI_DIVIDE_U16) -------------------------------------------------------------------------
// The pair (i, i + 1), i even, of a uint16 volume is ONE aligned 4-byte word (RP is even: rows start 4-byte
// aligned).  It is requested where the float32 form requests its 8-byte pair and waits in one register;
// mvn_u16_pair_widen turns it into the two floats at the use.  uint16 -> float is exact, so the quotient sees the
// float a converted volume would have held.
MVN_HD unsigned mvn_u16_pair_fetch(const unsigned short* p) {
  unsigned w;
  __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), sizeof(w));
  return w;
}
MVN_HD cfloat mvn_u16_pair_widen(unsigned w) { return cmake((float)(w & 0xffffu), (float)(w >> 16)); }

// inc/cpu_kernels.h:22-25: TransferT temp = 1. / out; out = in * temp, i.e. a DOUBLE divide
// rounded to float.  Double carries 53 >= 2*24+2 bits, so that double rounding is innocuous and
// float(1.0 / double(x)) is exactly the correctly rounded single-precision quotient 1.0f / x
// (checked on 1e8 random bit patterns in tests/test_oracle_kernels.py).  hipcc divides floats
// correctly rounded by default (-fhip-fp32-correctly-rounded-divide-sqrt), at a fraction of the
// cost of the f64 sequence.
MVN_HD float mvn_quotient(float view, float blurred) {
  MVN_FP_EXACT
  float t = 1.0f / blurred;
  return view * t;
}

MVN_HD float mvn_quotient_g(float view, float blurred, int guard) {
  return (guard && view == 0.f) ? 0.f : mvn_quotient(view, blurred);
}

// sqrt of a double >= 1 (the Tikhonov argument 1 + 2 lambda v with v > 0).  On the device this is
// the compiler's own correctly rounded f64 expansion (rsq seed, two coupled Goldschmidt steps,
// two residual corrections) minus its rescaling of tiny inputs and its zero / infinity fix-up,
// neither of which can trigger for arguments >= 1: same bits, a third fewer instructions in the
// VALU-bound update pass.  +inf comes out as NaN instead of +inf; the clamp that follows maps
// both to minValue (inc/cpu_kernels.h:82-83).
MVN_HD double mvn_sqrt_ge1(double x) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MVN_HOST_EMU)
  const double y = __builtin_amdgcn_rsq(x);
  const double h0 = y * 0.5, s0 = x * y;
  const double r0 = __builtin_fma(-h0, s0, 0.5);
  const double s1 = __builtin_fma(s0, r0, s0);
  const double h1 = __builtin_fma(h0, r0, h0);
  const double d0 = __builtin_fma(-s1, s1, x);
  const double s2 = __builtin_fma(d0, h1, s1);
  const double d1 = __builtin_fma(-s2, s2, x);
  return __builtin_fma(d1, h1, s2);
#else
  return sqrt(x);
#endif
}

// clamp / regularise chain of inc/cpu_kernels.h:40-49 (lambda == 0) and :75-86 (lambda > 0)
MVN_HD float mvn_next_value(float last, float integral, double lambda, float lambda_inv,
                            float min_value) {
  MVN_FP_EXACT
  float value = last * integral;
  // the regularised value is formed for every lane and selected afterwards: no divergent branch
  // around the f64 chain, so the chains of the 16 values a thread owns interleave (for
  // value <= 0 or NaN it is garbage that the select drops)
  float reg = value;
  if (lambda > 0.) reg = (float)((double)lambda_inv * (mvn_sqrt_ge1(1. + 2. * lambda * (double)value) - 1.));
  value = value > 0.f ? reg : min_value;
  float next;
  if (isnan(value) || isinf(value))
    next = min_value;
  else
    next = value > min_value ? value : min_value;
  return next;
}

// Legacy single-step update of iterate_fft_tikhonov (inc/cuda_kernels.cuh:162-193): lambda arrives
// as float, the regularised value is formed in double and divided (not multiplied by a
// reciprocal), there is no NaN/Inf test beyond the comparisons, and the weight blends against the
// NEW value: w * (max(min, t) - t) + t.
MVN_HD float mvn_legacy_tikhonov_value(float image, float integral, float weight, float lambda_f,
                                       float min_value) {
  MVN_FP_EXACT
  float t = image * integral;
  if (t > 0.f)
    t = (float)((sqrt(1.0 + 2.0 * (double)lambda_f * (double)t) - 1.) / (double)lambda_f);
  else
    t = min_value;
  float nv = (min_value > t) ? min_value : t;
  return weight * (nv - t) + t;
}

template <bool TV = false>
MVN_HD void mvn_epilogue(const EpilogueParams& e, float* out, long i, float x) {
  MVN_FP_EXACT
  x *= e.scale;
  if constexpr (TV) x *= mvn_tv_one<TV>(e, i);
  switch (e.mode) {
    case MVN_EPI_STORE: out[i] = x; break;
    case MVN_EPI_DIVIDE: out[i] = mvn_quotient_g(e.view[i], x, e.guard_zero_view); break;
    case MVN_EPI_UPDATE: {
      float last = e.psi[i];
      float next = mvn_next_value(last, x, e.lambda, e.lambda_inv, e.min_value);
      e.psi[i] = e.weights[i] * (next - last) + last;  // inc/cpu_kernels.h:51-52
    } break;
    case MVN_EPI_DELTA: {
      float last = e.psi[i];
      float next = mvn_next_value(last, x, e.lambda, e.lambda_inv, e.min_value);
      float d = e.weights[i] * (next - last);
      e.delta[i] = e.accumulate ? e.delta[i] + d : d;
    } break;
  }
}

// Pair form used by the even-d2 c2r pass: elements i, i+1 (i even, so 8-byte aligned) come out
// of one complex LDS word.  Operands are fetched separately from the arithmetic so that the
// fetch can be issued a whole transform ahead of its use; the (uniform) mode branch sits outside
// the unrolled loops so that every branch is straight-line code with all its loads in flight.
template <int U>
MVN_HD void mvn_epilogue_fetch_batch(const EpilogueParams& e, const long* idx, cfloat* a, cfloat* b) {
  if (e.mode == MVN_EPI_DIVIDE) {
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const cfloat*>(e.view + idx[u]);
  } else if (e.mode == MVN_EPI_UPDATE || e.mode == MVN_EPI_DELTA) {
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const cfloat*>(e.psi + idx[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) b[u] = *reinterpret_cast<const cfloat*>(e.weights + idx[u]);
  }
}

// the same for a view held as uint16 (MVN_EPI_DIVIDE_U16): one word per pair
template <int U>
MVN_HD void mvn_epilogue_fetch_batch_u16(const EpilogueParams& e, const long* idx, unsigned* a) {
#pragma unroll
  for (int u = 0; u < U; ++u) a[u] = mvn_u16_pair_fetch(e.view16 + idx[u]);
}

template <bool TV = false>
MVN_HD void mvn_epilogue_pair(const EpilogueParams& e, float* out, long i, cfloat z, cfloat a,
                              cfloat b) {
  MVN_FP_EXACT
  float x0 = z.x * e.scale, x1 = z.y * e.scale;
  if constexpr (TV) {
    const cfloat t = mvn_tv_pair<TV>(e, i);
    x0 *= t.x, x1 *= t.y;
  }
  switch (e.mode) {
    case MVN_EPI_STORE: *reinterpret_cast<cfloat*>(out + i) = cmake(x0, x1); break;
    case MVN_EPI_DIVIDE:
      *reinterpret_cast<cfloat*>(out + i) = cmake(mvn_quotient_g(a.x, x0, e.guard_zero_view),
                                                  mvn_quotient_g(a.y, x1, e.guard_zero_view));
      break;
    case MVN_EPI_UPDATE: {
      const float n0 = mvn_next_value(a.x, x0, e.lambda, e.lambda_inv, e.min_value);
      const float n1 = mvn_next_value(a.y, x1, e.lambda, e.lambda_inv, e.min_value);
      *reinterpret_cast<cfloat*>(e.psi + i) = cmake(b.x * (n0 - a.x) + a.x, b.y * (n1 - a.y) + a.y);
    } break;
    case MVN_EPI_DELTA: {
      const float n0 = mvn_next_value(a.x, x0, e.lambda, e.lambda_inv, e.min_value);
      const float n1 = mvn_next_value(a.y, x1, e.lambda, e.lambda_inv, e.min_value);
      cfloat d = cmake(b.x * (n0 - a.x), b.y * (n1 - a.y));
      if (e.accumulate) {
        const cfloat old = *reinterpret_cast<const cfloat*>(e.delta + i);
        d = cmake(old.x + d.x, old.y + d.y);
      }
      *reinterpret_cast<cfloat*>(e.delta + i) = d;
    } break;
  }
}

MVN_HD float mvn_blend(float w, float next, float last) {
  MVN_FP_EXACT
  return w * (next - last) + last;  // inc/cpu_kernels.h:51-52
}

// ---------------------------------------------------------------------------------------------
// convergence statistics (MVN_EPI_UPDATE_STATS).  Every lane sums |psi_after - psi_before| and psi_after, and
// takes the max of |psi_after - psi_before|, over the voxels of the window it updates; at the end the workgroup
// reduces its lanes in a fixed order through the LDS and writes ONE record {sum, max, mass} with plain stores.
// No atomics and no cross-lane instructions: the records, and the per-sweep sums of k_convergence_reduce, are
// the same bits for the same shape and grid.
// ---------------------------------------------------------------------------------------------
struct MvnStatsParams {
  long row0;              // volume row of the launch's row 0
  int d1;                 // rows per plane
  int o0, o1, o2;         // window: first plane, row, column ...
  unsigned n0, n1, n2;    // ... and extent
  double* rec;            // 3 doubles per workgroup: {sum |dpsi|, max |dpsi|, sum psi}
  unsigned* count;        // workgroups of the launch, written by workgroup 0
  long cap;               // records `rec` holds (a workgroup beyond writes none)
};

struct MvnStatAcc {
  double sum, mass;
  float max;
};

MVN_HD void mvn_stat_init(MvnStatAcc& a) {
  a.sum = 0.;
  a.mass = 0.;
  a.max = 0.f;
}

// the row's plane and row inside the window (one division per ROW; the column test is per element)
MVN_HD bool mvn_stat_row_in(const MvnStatsParams& s, long row) {
  const unsigned g = (unsigned)(s.row0 + row), d1 = (unsigned)s.d1;
  const unsigned z = g / d1, y = g - z * d1;
  return z - (unsigned)s.o0 < s.n0 && y - (unsigned)s.o1 < s.n1;
}

// a max that keeps a NaN once it has seen one
MVN_HD float mvn_stat_max(float m, float d) { return (d > m || d != d) ? d : m; }

// one voxel: psi `last` -> `y`, from the integral `x`.  (x - x) is +0 for a finite x and NaN otherwise: a
// non-finite integral (a poisoned call) makes the statistics NaN although the clamp chain keeps psi finite.
MVN_HD void mvn_stat_add(MvnStatAcc& a, bool in, float last, float y, float x) {
  MVN_FP_EXACT
  const float d = fabsf(y - last) + (x - x);
  a.sum += in ? (double)d : 0.;
  a.mass += in ? (double)y : 0.;
  a.max = in ? mvn_stat_max(a.max, d) : a.max;
}

// MVN_EPI_UPDATE of the pair (i, i + 1) in columns col, col + 1 of a row, with its statistics: psi (written
// and returned) is the UPDATE result bit for bit
template <bool TV = false>
MVN_HD cfloat mvn_update_pair_stats(const EpilogueParams& e, long i, cfloat z, cfloat a, cfloat b, MvnStatAcc& acc,
                                    const MvnStatsParams& s, bool row_in, int col) {
  MVN_FP_EXACT
  float x0 = z.x * e.scale, x1 = z.y * e.scale;
  if constexpr (TV) {
    const cfloat t = mvn_tv_pair<TV>(e, i);
    x0 *= t.x, x1 *= t.y;
  }
  const float n0 = mvn_next_value(a.x, x0, e.lambda, e.lambda_inv, e.min_value);
  const float n1 = mvn_next_value(a.y, x1, e.lambda, e.lambda_inv, e.min_value);
  const cfloat y = cmake(mvn_blend(b.x, n0, a.x), mvn_blend(b.y, n1, a.y));
  *reinterpret_cast<cfloat*>(e.psi + i) = y;
  const unsigned c = (unsigned)(col - s.o2);
  mvn_stat_add(acc, row_in && c < s.n2, a.x, y.x, x0);
  mvn_stat_add(acc, row_in && c + 1u < s.n2, a.y, y.y, x1);
  return y;
}

// the same for one element (odd d2)
template <bool TV = false>
MVN_HD void mvn_update_stats(const EpilogueParams& e, long i, float x, MvnStatAcc& acc, bool in) {
  MVN_FP_EXACT
  x *= e.scale;
  if constexpr (TV) x *= mvn_tv_one<TV>(e, i);
  const float last = e.psi[i];
  const float next = mvn_next_value(last, x, e.lambda, e.lambda_inv, e.min_value);
  const float y = e.weights[i] * (next - last) + last;  // inc/cpu_kernels.h:51-52
  e.psi[i] = y;
  mvn_stat_add(acc, in, last, y, x);
}

// lanes [tid] of the scratch after a barrier: a tree over the next power of two, pairs (t, t + h) in a fixed order
MVN_HD void mvn_stat_tree_step(char* lds, int n, int h, int tid) {
  double* ls = reinterpret_cast<double*>(lds);
  double* lm = ls + n;
  float* lx = reinterpret_cast<float*>(lm + n);
  if (tid < h && tid + h < n) {
    ls[tid] += ls[tid + h];
    lm[tid] += lm[tid + h];
    lx[tid] = mvn_stat_max(lx[tid], lx[tid + h]);
  }
}
MVN_HD void mvn_stat_put(char* lds, int n, int tid, const MvnStatAcc& a) {
  double* ls = reinterpret_cast<double*>(lds);
  ls[tid] = a.sum;
  ls[n + tid] = a.mass;
  reinterpret_cast<float*>(ls + 2 * n)[tid] = a.max;
}
MVN_HD void mvn_stat_record(const MvnStatsParams& s, const char* lds, int n, long block, long nblocks) {
  const double* ls = reinterpret_cast<const double*>(lds);
  if (block < s.cap) {
    s.rec[3 * block] = ls[0];
    s.rec[3 * block + 1] = (double)reinterpret_cast<const float*>(ls + 2 * n)[0];
    s.rec[3 * block + 2] = ls[n];
  }
  if (block == 0) *s.count = (unsigned)nblocks;
}
MVN_HD int mvn_pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// workgroup end of the run-time-radix bodies (tid / nthreads form): every lane calls it
MVN_HD void mvn_stat_flush(const MvnStatsParams& s, const MvnStatAcc& a, long block, long nblocks, cfloat* lds,
                           int tid, int nthreads) {
  char* l = reinterpret_cast<char*>(lds);
  MVN_SYNC();
  for (int t = tid; t < nthreads; t += nthreads) mvn_stat_put(l, nthreads, t, a);
  MVN_SYNC();
  for (int h = mvn_pow2_ceil(nthreads) >> 1; h > 0; h >>= 1) {
    for (int t = tid; t < h; t += nthreads) mvn_stat_tree_step(l, nthreads, h, t);
    MVN_SYNC();
  }
  if (tid == 0) mvn_stat_record(s, l, nthreads, block, nblocks);
}

// k_convergence_reduce: the records of one sweep's V view updates (view v at rec + 3 v cap, counts[v] of them)
// -> out = {S, M, P}.  Lane t sums records t, t + nthreads, ... view after view, then the lanes are reduced as
// above.  lds: 3 nthreads doubles.
MVN_HD void mvn_convergence_reduce_body(const double* rec, const unsigned* counts, int nviews, long cap,
                                        double* out, double* lds, int tid, int nthreads) {
  for (int t = tid; t < nthreads; t += nthreads) {
    double s = 0., m = 0., p = 0.;
    for (int v = 0; v < nviews; ++v) {
      const long n = (long)counts[v] < cap ? (long)counts[v] : cap;
      const double* r = rec + 3 * (long)v * cap;
      for (long i = t; i < n; i += nthreads) {
        s += r[3 * i];
        m = (r[3 * i + 1] > m || r[3 * i + 1] != r[3 * i + 1]) ? r[3 * i + 1] : m;
        p += r[3 * i + 2];
      }
    }
    lds[t] = s;
    lds[nthreads + t] = m;
    lds[2 * nthreads + t] = p;
  }
  MVN_SYNC();
  for (int h = mvn_pow2_ceil(nthreads) >> 1; h > 0; h >>= 1) {
    for (int t = tid; t < h; t += nthreads) {
      if (t + h < nthreads) {
        lds[t] += lds[t + h];
        const double a = lds[nthreads + t], b = lds[nthreads + t + h];
        lds[nthreads + t] = (b > a || b != b) ? b : a;
        lds[2 * nthreads + t] += lds[2 * nthreads + t + h];
      }
    }
    MVN_SYNC();
  }
  if (tid == 0) {
    out[0] = lds[0];
    out[1] = lds[nthreads];
    out[2] = lds[2 * nthreads];
  }
}

// ---------------------------------------------------------------------------------------------
// noise model (MVN_EPI_DIVIDE_NM, MVN_EPI_DIVIDE_NM_U16).  For a voxel with the inverse-transform output times
// scale x, the view's background b and the image voxel y widened to float32:
//   m = x + b        (float32, one correctly rounded add, never contracted with the multiply by scale;
//                     with b == 0 the add is NOT performed: m = x, -0 stays -0)
//   q = quotient_g(y, m, guard)                      (the existing quotient, unchanged)
//   term = y > 0 ? (y * logf(q) - y) + m : m - y     (float32, no contraction; q is the value written)
// Every lane sums term, y and m in double over the voxels of the window it divides; the workgroup reduces its lanes in
// a fixed order through the LDS and writes ONE record {D, Y, M} with plain stores, as the convergence statistics do.
// ---------------------------------------------------------------------------------------------
struct MvnNmAcc {
  double d, y, m;
};

MVN_HD void mvn_nm_init(MvnNmAcc& a) {
  a.d = 0.;
  a.y = 0.;
  a.m = 0.;
}

// one voxel: the quotient (returned) and the voxel's share of the statistics; x is already scaled
MVN_HD float mvn_nm_one(const EpilogueParams& e, float y, float x, MvnNmAcc& a, bool in) {
  MVN_FP_EXACT
  const float m = e.background != 0.f ? x + e.background : x;  // (the condition is the same for every lane)
  const float q = mvn_quotient_g(y, m, e.guard_zero_view);
  const float term = y > 0.f ? (y * logf(q) - y) + m : m - y;
  a.d += in ? (double)term : 0.;
  a.y += in ? (double)y : 0.;
  a.m += in ? (double)m : 0.;
  return q;
}

// the pair (i, i + 1) in columns col, col + 1 of a row: view pair a, raw transform output z
MVN_HD cfloat mvn_nm_pair(const EpilogueParams& e, cfloat z, cfloat a, MvnNmAcc& acc, const MvnStatsParams& s,
                          bool row_in, int col) {
  MVN_FP_EXACT
  const float x0 = z.x * e.scale, x1 = z.y * e.scale;
  const unsigned c = (unsigned)(col - s.o2);
  const float q0 = mvn_nm_one(e, a.x, x0, acc, row_in && c < s.n2);
  const float q1 = mvn_nm_one(e, a.y, x1, acc, row_in && c + 1u < s.n2);
  return cmake(q0, q1);
}

MVN_HD void mvn_nm_put(char* lds, int n, int tid, const MvnNmAcc& a) {
  double* l = reinterpret_cast<double*>(lds);
  l[tid] = a.d;
  l[n + tid] = a.y;
  l[2 * n + tid] = a.m;
}
// a tree over the next power of two, pairs (t, t + h) in a fixed order
MVN_HD void mvn_nm_tree_step(char* lds, int n, int h, int tid) {
  double* l = reinterpret_cast<double*>(lds);
  if (tid < h && tid + h < n) {
    l[tid] += l[tid + h];
    l[n + tid] += l[n + tid + h];
    l[2 * n + tid] += l[2 * n + tid + h];
  }
}
MVN_HD void mvn_nm_record(const MvnStatsParams& s, const char* lds, int n, long block, long nblocks) {
  const double* l = reinterpret_cast<const double*>(lds);
  if (block < s.cap) {
    s.rec[3 * block] = l[0];
    s.rec[3 * block + 1] = l[n];
    s.rec[3 * block + 2] = l[2 * n];
  }
  if (block == 0) *s.count = (unsigned)nblocks;
}

// workgroup end of the run-time-radix bodies (tid / nthreads form): every lane calls it
MVN_HD void mvn_nm_flush(const MvnStatsParams& s, const MvnNmAcc& a, long block, long nblocks, cfloat* lds, int tid,
                         int nthreads) {
  char* l = reinterpret_cast<char*>(lds);
  MVN_SYNC();
  for (int t = tid; t < nthreads; t += nthreads) mvn_nm_put(l, nthreads, t, a);
  MVN_SYNC();
  for (int h = mvn_pow2_ceil(nthreads) >> 1; h > 0; h >>= 1) {
    for (int t = tid; t < h; t += nthreads) mvn_nm_tree_step(l, nthreads, h, t);
    MVN_SYNC();
  }
  if (tid == 0) mvn_nm_record(s, l, nthreads, block, nblocks);
}

// k_nm_reduce: the records of ONE view's divide pass (rec, *count of them, at most cap) -> out = {D, Y, M}.  Lane t
// sums records t, t + nthreads, ..., then the lanes are reduced as above.  lds: 3 nthreads doubles.
MVN_HD void mvn_nm_reduce_body(const double* rec, const unsigned* count, long cap, double* out, double* lds, int tid,
                               int nthreads) {
  for (int t = tid; t < nthreads; t += nthreads) {
    double d = 0., y = 0., m = 0.;
    const long n = (long)*count < cap ? (long)*count : cap;
    for (long i = t; i < n; i += nthreads) {
      d += rec[3 * i];
      y += rec[3 * i + 1];
      m += rec[3 * i + 2];
    }
    lds[t] = d;
    lds[nthreads + t] = y;
    lds[2 * nthreads + t] = m;
  }
  MVN_SYNC();
  for (int h = mvn_pow2_ceil(nthreads) >> 1; h > 0; h >>= 1) {
    for (int t = tid; t < h; t += nthreads) mvn_nm_tree_step(reinterpret_cast<char*>(lds), nthreads, h, t);
    MVN_SYNC();
  }
  if (tid == 0) {
    out[0] = lds[0];
    out[1] = lds[nthreads];
    out[2] = lds[2 * nthreads];
  }
}

// Pair epilogue of the fused c2r + pointwise + r2c pass: hands the two results back as the packed
// input z[j] = (y[2j], y[2j+1]) of the next forward transform; UPDATE also writes psi.
template <bool TV = false>
MVN_HD cfloat mvn_epilogue_pair_value(int mode, const EpilogueParams& e, long i, cfloat z, cfloat a,
                                      cfloat b) {
  MVN_FP_EXACT
  float x0 = z.x * e.scale, x1 = z.y * e.scale;
  if constexpr (TV) {
    const cfloat t = mvn_tv_pair<TV>(e, i);
    x0 *= t.x, x1 *= t.y;
  }
  if (mode == MVN_EPI_DIVIDE)
    return cmake(mvn_quotient_g(a.x, x0, e.guard_zero_view), mvn_quotient_g(a.y, x1, e.guard_zero_view));
  if (mode == MVN_EPI_UPDATE) {
    const float n0 = mvn_next_value(a.x, x0, e.lambda, e.lambda_inv, e.min_value);
    const float n1 = mvn_next_value(a.y, x1, e.lambda, e.lambda_inv, e.min_value);
    const cfloat y = cmake(mvn_blend(b.x, n0, a.x), mvn_blend(b.y, n1, a.y));
    *reinterpret_cast<cfloat*>(e.psi + i) = y;
    return y;
  }
  return cmake(x0, x1);
}

// the same with the mode as a template constant (fixed-length kernels)
template <int EPI>
MVN_HD void mvn_epilogue_pair_t(const EpilogueParams& e, float* out, long i, cfloat z, cfloat a,
                                cfloat b) {
  EpilogueParams ee = e;
  ee.mode = mvn_epi_math(EPI);
  mvn_epilogue_pair<mvn_epi_tv(EPI)>(ee, out, i, z, a, b);
}

#define MVN_ROWS_U 8

// ---------------------------------------------------------------------------------------------
// last-axis passes (contiguous rows).  A tile is T rows; LDS holds them transposed,
// lds[pos * TP + row], TP odd to keep the transposing accesses conflict-free.
// ---------------------------------------------------------------------------------------------
struct RowsParams {
  AxisPlan ax;        // length h (= d2/2 for even d2, d2 for odd)
  const cfloat* twr;  // d2-th roots of unity (even d2: real<->half-complex post-processing)
  int d2, h, C, RP;   // see mvn::Layout
  long rows;          // d0*d1
  int T, TP;
  long lds_alt;       // offset (in cfloat) of the second LDS buffer, 0 if none
  long lds_tw;        // offset (in cfloat) of the LDS twiddle copy
  unsigned hmul, Cmul;  // mvn_fastdiv multipliers for h and C
  int fixed;            // 1: launch the compile-time specialised kernel for this h (mvn_fixed.hpp)
  // r2c: real rows in (pitch RP floats) -> complex rows out (pitch C) + Nyquist plane
  const float* in_real;
  cfloat* out_cplx;
  cfloat* out_nyq;
  // c2r: complex rows + Nyquist plane in -> real rows out through the epilogue
  const cfloat* in_cplx;
  const cfloat* in_nyq;
  float* out_real;
  EpilogueParams epi;
  // 1: the Nyquist bin of a row (real, like its DC bin) is carried in the IMAGINARY part of the DC bin and
  // there is no Nyquist plane (in_nyq / out_nyq unused): the dim1 passes then transform DC + i Nyquist as one
  // complex column and the direct dim0 leg separates the two by the k1 <-> -k1 symmetry (mvn_dim0_direct.hpp)
  int nyq_packed;
  // 1: the half-spectrum (in_cplx / out_cplx) is in the LINE layout of the fused middle pass (mvn_mid_fused.hpp),
  // [plane][position][row of the plane] with lines_d1 rows per plane; row r of the launch is row row_base + r of the
  // volume and in_cplx / out_cplx point at the volume's first element.  Fixed kernels only, nyq_packed only.
  int lines, lines_d1;
  long row_base;
  MvnStatsParams st;  // MVN_EPI_UPDATE_STATS (and _TV); MVN_EPI_DIVIDE_NM (and _U16): the window and the records
};

// the window bits of the T rows of a tile (run-time-radix bodies: the division stays per row)
template <int T>
MVN_HD unsigned mvn_stat_tile_rows(const RowsParams& P, long r0) {
  static_assert(T <= 32, "one bit per row");
  unsigned bits = 0;
  for (int rho = 0; rho < T; ++rho)
    if (r0 + rho < P.rows && mvn_stat_row_in(P.st, r0 + rho)) bits |= 1u << rho;
  return bits;
}

// forward stages + real<->complex step + store of a tile that already sits in LDS as the packed
// rows z[j] (shared by the plain r2c pass and the fused c2r + pointwise + r2c pass)
template <int T>
MVN_HD void rows_r2c_even_tail(const RowsParams& P, long r0, cfloat*& buf, cfloat*& alt,
                               const cfloat* tw, int tid, int nthreads) {
  const int h = P.h, TP = P.TP;
  lds_fft_dif<-1, T>(buf, alt, TP, P.ax, tw, tid, nthreads);
  const int npairs = h / 2 + 1;
  for (int w = tid; w < npairs * T; w += nthreads) {
    const int k = w / T, rho = w - k * T;
    const int m = (h - k) % h;
    const int pk = P.ax.inv[k], pm = P.ax.inv[m];
    const cfloat zk = buf[pk * TP + rho];
    if (k == 0) {
      if (P.nyq_packed) {
        buf[pk * TP + rho] = cmake(zk.x + zk.y, zk.x - zk.y);
      } else {
        buf[pk * TP + rho] = cmake(zk.x + zk.y, 0.f);
        if (r0 + rho < P.rows) P.out_nyq[r0 + rho] = cmake(zk.x - zk.y, 0.f);
      }
    } else {
      const cfloat zm = buf[pm * TP + rho];
      const cfloat E = cmake(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
      const cfloat D = cmake(0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y));
      const cfloat G = cmul(P.twr[k], D);
      buf[pk * TP + rho] = cadd(E, cmul_si<-1>(G));
      if (m != k) buf[pm * TP + rho] = cadd(cconj(E), cmul_si<-1>(cconj(G)));
    }
  }
  MVN_SYNC();
  for (int w = tid; w < T * h; w += nthreads) {
    // spectral rows are kept in position (digit-reversed) order: bin k sits at column inv[k]
    const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), p = w - rho * h;
    const long row = r0 + rho;
    if (row < P.rows) P.out_cplx[row * P.C + p] = buf[p * TP + rho];
  }
}

// real -> half-complex, even d2: z[j] = x[2j] + i x[2j+1], Z = FFT_h(z), then
// X[k] = E - i w^k D,  E = (Z[k] + conj Z[h-k])/2,  D = (Z[k] - conj Z[h-k])/2,  w = exp(-2 pi i/d2)
template <int T>
MVN_HD void rows_r2c_even_body(const RowsParams& P, long tile, int tid, int nthreads, cfloat* lds) {
  const int h = P.h, TP = P.TP;
  const long r0 = tile * T;
  cfloat* buf = lds;
  cfloat* alt = lds + P.lds_alt;
  const cfloat* tw = lds_stage_twiddles(lds + P.lds_tw, P.ax, tid, nthreads);
  constexpr int U = MVN_ROWS_U;
  const int total = T * h;
  const long last_row = P.rows - 1;
  for (int w0 = tid; w0 < total; w0 += U * nthreads) {
    cfloat v[U];
    // every load is unconditional (clamped address) so that all U are in flight together
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int w = w0 + u * nthreads;
      w = w < total ? w : total - 1;
      const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), j = w - rho * h;
      long row = r0 + rho;
      row = row < last_row ? row : last_row;
      v[u] = reinterpret_cast<const cfloat*>(P.in_real + row * P.RP)[j];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int w = w0 + u * nthreads;
      if (w < total) {
        const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), j = w - rho * h;
        buf[j * TP + rho] = (r0 + rho <= last_row) ? v[u] : cmake(0.f, 0.f);
      }
    }
  }
  MVN_SYNC();
  rows_r2c_even_tail<T>(P, r0, buf, alt, tw, tid, nthreads);
}

// half-complex -> real, even d2: Z[k] = E + i O, E = X[k] + conj X[h-k],
// O = (X[k] - conj X[h-k]) exp(+2 pi i k/d2); z = IFFT_h(Z); x[2j] = Re z[j], x[2j+1] = Im z[j]
// KEEP = true is the fused pass: the epilogue results stay in LDS and run straight through the
// forward half (rows_r2c_even_tail), writing the half-spectrum of the result over the input.
// EPI is the form of the launch's mode (mvn_epi_generic_form): MVN_EPI_STORE for the four modes told apart at run time
// by P.epi.mode, else P.epi.mode itself, from which follow
// STATS: the UPDATE epilogue with the convergence statistics;
// U16: the DIVIDE epilogue on a uint16 view;
// TV: the UPDATE epilogue (with STATS or without) on the integral times the total-variation factor, loaded at its use;
// NM: the noise-model divide (on a uint16 view with U16).
template <int T, bool KEEP = false, int EPI = MVN_EPI_STORE>
MVN_HD void rows_c2r_even_body(const RowsParams& P, long tile, int tid, int nthreads, cfloat* lds) {
  static_assert(mvn_epi_generic_form(EPI) == EPI, "a form of the run-time-radix bodies");
  constexpr bool STATS = mvn_epi_stats(EPI), U16 = mvn_epi_u16(EPI), TV = mvn_epi_tv(EPI), NM = mvn_epi_nm(EPI);
  // (a copy of the epilogue's few fields, not of P: the run-time radix tables in P are indexed dynamically and a
  // private copy of the whole struct would live in scratch memory)
  EpilogueParams epi = P.epi;
  mvn_arm_poison(epi);
  MvnStatAcc acc;
  unsigned rin = 0;
  if constexpr (STATS) {
    epi.mode = MVN_EPI_UPDATE;  // operands and psi as UPDATE
    mvn_stat_init(acc);
    rin = mvn_stat_tile_rows<T>(P, tile * T);
  }
  if constexpr (U16) epi.mode = MVN_EPI_DIVIDE;  // the arithmetic of DIVIDE, on operands widened at the use
  if constexpr (TV) epi.mode = MVN_EPI_UPDATE;   // operands and psi as UPDATE
  MvnNmAcc nacc;
  if constexpr (NM) {
    epi.mode = MVN_EPI_DIVIDE;  // operands as DIVIDE
    mvn_nm_init(nacc);
    rin = mvn_stat_tile_rows<T>(P, tile * T);
  }
  constexpr int U = MVN_ROWS_U;
  const int h = P.h, TP = P.TP;
  const long r0 = tile * T;
  const int total = T * h;
  const bool single = total <= U * nthreads;
  cfloat* buf = lds;
  cfloat* alt = lds + P.lds_alt;
  const cfloat* tw = lds_stage_twiddles(lds + P.lds_tw, P.ax, tid, nthreads);
  cfloat ea[U], eb[U];  // epilogue operands, fetched a whole transform ahead when `single`
  unsigned eu[U];       // (U16: the view's pairs, one word each)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    ea[u] = cmake(0.f, 0.f);
    eb[u] = cmake(0.f, 0.f);
    eu[u] = 0u;
  }
  const long last_row = P.rows - 1;
  for (int w0 = tid; w0 < total; w0 += U * nthreads) {
    cfloat v[U];
    long idx[U];
    // unconditional, clamped loads: all U (and, if `single`, the epilogue operands) in flight
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int w = w0 + u * nthreads;
      w = w < total ? w : total - 1;
      const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), k = w - rho * h;
      long row = r0 + rho;
      row = row < last_row ? row : last_row;
      v[u] = P.in_cplx[row * P.C + k];
      idx[u] = row * P.RP + 2 * k;
    }
    if (single) {
      if constexpr (U16)
        mvn_epilogue_fetch_batch_u16<U>(epi, idx, eu);
      else
        mvn_epilogue_fetch_batch<U>(epi, idx, ea, eb);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int w = w0 + u * nthreads;
      if (w < total) {
        const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), p = w - rho * h;
        buf[p * TP + rho] = (r0 + rho <= last_row) ? v[u] : cmake(0.f, 0.f);
      }
    }
  }
  MVN_SYNC();
  const int npairs = h / 2 + 1;
  for (int w = tid; w < npairs * T; w += nthreads) {
    const int k = w / T, rho = w - k * T;
    const int m = (h - k) % h;
    const int pk = P.ax.inv[k], pm = P.ax.inv[m];
    const cfloat xk = buf[pk * TP + rho];
    if (k == 0) {
      // imaginary parts of the DC and Nyquist bins are ignored, as FFTW's c2r does
      float xh = 0.f;
      if (P.nyq_packed)
        xh = xk.y;
      else if (r0 + rho < P.rows)
        xh = P.in_nyq[r0 + rho].x;
      buf[pk * TP + rho] = cmake(xk.x + xh, xk.x - xh);
    } else {
      const cfloat xm = buf[pm * TP + rho];
      const cfloat E = cmake(xk.x + xm.x, xk.y - xm.y);
      const cfloat Dk = cmake(xk.x - xm.x, xk.y + xm.y);
      const cfloat O = cmul(Dk, cconj(P.twr[k]));
      buf[pk * TP + rho] = cadd(E, cmul_si<+1>(O));
      if (m != k) buf[pm * TP + rho] = cadd(cconj(E), cmul_si<+1>(cconj(O)));
    }
  }
  MVN_SYNC();
  lds_fft_dit<+1, T>(buf, alt, TP, P.ax, tw, tid, nthreads);
  for (int w0 = tid; w0 < total; w0 += U * nthreads) {
    if (!single) {
      long idx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int w = w0 + u * nthreads;
        w = w < total ? w : total - 1;
        const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), j = w - rho * h;
        long row = r0 + rho;
        row = row < last_row ? row : last_row;
        idx[u] = row * P.RP + 2 * j;
      }
      if constexpr (U16)
        mvn_epilogue_fetch_batch_u16<U>(epi, idx, eu);
      else
        mvn_epilogue_fetch_batch<U>(epi, idx, ea, eb);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int w = w0 + u * nthreads;
      const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)h, P.hmul), j = w - rho * h;
      const long row = r0 + rho;
      if (w < total && row <= last_row) {
        if constexpr (U16) ea[u] = mvn_u16_pair_widen(eu[u]);
        if constexpr (NM) {
          const cfloat q = mvn_nm_pair(epi, buf[j * TP + rho], ea[u], nacc, P.st, (rin >> rho) & 1u, 2 * j);
          if (KEEP)
            buf[j * TP + rho] = q;
          else
            *reinterpret_cast<cfloat*>(P.out_real + row * P.RP + 2 * j) = q;
        } else if constexpr (STATS) {
          const cfloat y = mvn_update_pair_stats<TV>(epi, row * P.RP + 2 * j, buf[j * TP + rho], ea[u], eb[u], acc,
                                                     P.st, (rin >> rho) & 1u, 2 * j);
          if (KEEP) buf[j * TP + rho] = y;
        } else if (KEEP)
          buf[j * TP + rho] = mvn_epilogue_pair_value<TV>(epi.mode, epi, row * P.RP + 2 * j,
                                                          buf[j * TP + rho], ea[u], eb[u]);
        else
          mvn_epilogue_pair<TV>(epi, P.out_real, row * P.RP + 2 * j, buf[j * TP + rho], ea[u], eb[u]);
      }
    }
  }
  if (KEEP) {
    MVN_SYNC();
    rows_r2c_even_tail<T>(P, r0, buf, alt, tw, tid, nthreads);
  }
  if constexpr (STATS) mvn_stat_flush(P.st, acc, tile, (P.rows + T - 1) / T, lds, tid, nthreads);
  if constexpr (NM) mvn_nm_flush(P.st, nacc, tile, (P.rows + T - 1) / T, lds, tid, nthreads);
}

// odd d2: plain complex transform of the real row, first C = (d2+1)/2 bins kept
template <int T>
MVN_HD void rows_r2c_odd_body(const RowsParams& P, long tile, int tid, int nthreads, cfloat* lds) {
  const int n = P.h, TP = P.TP;
  const long r0 = tile * T;
  cfloat* buf = lds;
  cfloat* alt = lds + P.lds_alt;
  const cfloat* tw = lds_stage_twiddles(lds + P.lds_tw, P.ax, tid, nthreads);
  for (int w = tid; w < T * n; w += nthreads) {
    const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)n, P.hmul), j = w - rho * n;
    const long row = r0 + rho;
    float v = 0.f;
    if (row < P.rows) v = P.in_real[row * P.RP + j];
    buf[j * TP + rho] = cmake(v, 0.f);
  }
  MVN_SYNC();
  lds_fft_dif<-1, T>(buf, alt, TP, P.ax, tw, tid, nthreads);
  for (int w = tid; w < T * P.C; w += nthreads) {
    const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)P.C, P.Cmul), k = w - rho * P.C;
    const long row = r0 + rho;
    if (row < P.rows) P.out_cplx[row * P.C + k] = buf[P.ax.inv[k] * TP + rho];
  }
}

template <int T, int EPI = MVN_EPI_STORE>
MVN_HD void rows_c2r_odd_body(const RowsParams& P, long tile, int tid, int nthreads, cfloat* lds) {
  static_assert(mvn_epi_generic_form(EPI) == EPI, "a form of the run-time-radix bodies");
  constexpr bool STATS = mvn_epi_stats(EPI), U16 = mvn_epi_u16(EPI), TV = mvn_epi_tv(EPI), NM = mvn_epi_nm(EPI);
  // (a copy of the epilogue's few fields, not of P: the run-time radix tables in P are indexed dynamically and a
  // private copy of the whole struct would live in scratch memory)
  EpilogueParams epi = P.epi;
  mvn_arm_poison(epi);
  MvnStatAcc acc;
  unsigned rin = 0;
  if constexpr (STATS) {
    mvn_stat_init(acc);
    rin = mvn_stat_tile_rows<T>(P, tile * T);
  }
  if constexpr (TV) epi.mode = MVN_EPI_UPDATE;  // (MVN_EPI_UPDATE_TV: the arithmetic of UPDATE on the integral times tv)
  MvnNmAcc nacc;
  if constexpr (NM) {
    mvn_nm_init(nacc);
    rin = mvn_stat_tile_rows<T>(P, tile * T);
  }
  const int n = P.h, TP = P.TP;
  const long r0 = tile * T;
  cfloat* buf = lds;
  cfloat* alt = lds + P.lds_alt;
  const cfloat* tw = lds_stage_twiddles(lds + P.lds_tw, P.ax, tid, nthreads);
  for (int w = tid; w < T * n; w += nthreads) {
    const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)n, P.hmul), k = w - rho * n;
    const long row = r0 + rho;
    cfloat v = cmake(0.f, 0.f);
    if (row < P.rows) {
      if (k < P.C) {
        v = P.in_cplx[row * P.C + k];
        if (k == 0) v.y = 0.f;
      } else {
        v = cconj(P.in_cplx[row * P.C + (n - k)]);
      }
    }
    buf[P.ax.inv[k] * TP + rho] = v;
  }
  MVN_SYNC();
  lds_fft_dit<+1, T>(buf, alt, TP, P.ax, tw, tid, nthreads);
  for (int w = tid; w < T * n; w += nthreads) {
    const int rho = (int)mvn_fastdiv((unsigned)w, (unsigned)n, P.hmul), j = w - rho * n;
    const long row = r0 + rho;
    if constexpr (NM) {  // (one element at a time, the view as float32 or uint16)
      MVN_FP_EXACT
      if (row < P.rows) {
        const long i = row * P.RP + j;
        const float view = U16 ? (float)epi.view16[i] : epi.view[i];
        P.out_real[i] = mvn_nm_one(epi, view, buf[j * TP + rho].x * epi.scale, nacc,
                                   ((rin >> rho) & 1u) && (unsigned)(j - P.st.o2) < P.st.n2);
      }
    } else if constexpr (STATS) {
      if (row < P.rows)
        mvn_update_stats<TV>(epi, row * P.RP + j, buf[j * TP + rho].x, acc,
                         ((rin >> rho) & 1u) && (unsigned)(j - P.st.o2) < P.st.n2);
    } else if constexpr (U16) {  // (rows of an odd extent: one element at a time, as mvn_epilogue)
      MVN_FP_EXACT
      if (row < P.rows) {
        const long i = row * P.RP + j;
        const float view = (float)epi.view16[i];
        P.out_real[i] = mvn_quotient_g(view, buf[j * TP + rho].x * epi.scale, epi.guard_zero_view);
      }
    } else if (row < P.rows) {
      mvn_epilogue<TV>(epi, P.out_real, row * P.RP + j, buf[j * TP + rho].x);
    }
  }
  if constexpr (STATS) mvn_stat_flush(P.st, acc, tile, (P.rows + T - 1) / T, lds, tid, nthreads);
  if constexpr (NM) mvn_nm_flush(P.st, nacc, tile, (P.rows + T - 1) / T, lds, tid, nthreads);
}

// ---------------------------------------------------------------------------------------------
// strided-axis passes: lines run along an axis with element stride `estride`, a tile is T
// neighbouring lines (column stride `cstride`, 1 for the main array so a tile row is one
// contiguous T*8-byte segment).  lds[pos * TP + col].
// ---------------------------------------------------------------------------------------------
enum MvnStridedMode { MVN_ST_FWD = 0, MVN_ST_INV = 1, MVN_ST_FWD_MUL_INV = 2 };

struct StridedParams {
  AxisPlan ax;
  cfloat* data;        // destination (and source, unless `src` is set)
  const cfloat* src;   // optional separate source with the same addressing (out-of-place pass)
  const cfloat* spec;  // FWD_MUL_INV: pre-scaled PSF spectrum, same addressing as data ...
  int spec_tiled;      // ... or (fixed kernels only) tile-contiguous: [tile][row][T columns], so that a
                       // tile's operands are ONE contiguous stream of n * T * 8 bytes instead of n row
                       // segments n-1 pages apart
  long ostride;        // between outer slabs
  long estride;        // between elements of a line
  long cstride;        // between neighbouring lines of a tile
  int ncols;           // lines per outer slab
  int tiles_per_outer;
  int T, TP;
  long lds_alt;
  long lds_tw;  // offset (in cfloat) of the LDS twiddle copy
  int is_nyq;   // launch works on the Nyquist plane (profiling tag only)
  int fixed;    // 1: launch the compile-time specialised kernel for this length (mvn_fixed.hpp)
  long nblocks; // fixed kernels: tiles of the launch (a workgroup walks over several of them)
};

// The lines of the Nyquist plane may ride behind the walking workgroups of a plain fixed-length launch, one line per
// workgroup through the run-time-radix body (`rider`, null: none)
inline void mvn_strided_rider_check(int mode, const StridedParams& p, const StridedParams* rider, size_t rider_lds) {
  if (rider && (!p.fixed || mode == MVN_ST_FWD_MUL_INV || rider->T != 1 || rider->fixed || rider_lds > 160 * 1024))
    throw std::invalid_argument("mvn: Nyquist lines ride only in the plain fixed-length strided passes, one per workgroup");
}

// Loads are issued in batches of U per thread BEFORE any of them is consumed, so a tile's HBM
// latency is paid once, not once per element.  When the whole tile is a single batch
// (n*T <= U*nthreads, e.g. 512 x 16 on 512 threads) the fused mode also fetches its PSF-spectrum
// operands up front and keeps them in registers across the forward transform.
#define MVN_STRIDED_U 8

template <int MODE, int T, bool COMP = false>
MVN_HD void strided_body(const StridedParams& P, long block, int tid, int nthreads, cfloat* lds) {
  constexpr int U = MVN_STRIDED_U;
  const int n = P.ax.n, TP = P.TP;
  const long o = block / P.tiles_per_outer;
  const int t = (int)(block - o * P.tiles_per_outer);
  const int c0 = t * T;
  const int ncol = (P.ncols - c0) < T ? (P.ncols - c0) : T;
  const long base = o * P.ostride + (long)c0 * P.cstride;
  const int total = n * T;
  const bool single = total <= U * nthreads;
  const cfloat* in = P.src ? P.src : P.data;
  cfloat* buf = lds;
  cfloat* alt = lds + P.lds_alt;
  const cfloat* tw = lds_stage_twiddles(lds + P.lds_tw, P.ax, tid, nthreads);
  cfloat g[U];
  for (int w0 = tid; w0 < total; w0 += U * nthreads) {
    cfloat v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int w = w0 + u * nthreads;
      w = w < total ? w : total - 1;
      int j = w / T, c = w % T;
      c = c < ncol ? c : ncol - 1;  // clamped: the load itself is unconditional
      v[u] = in[base + (long)j * P.estride + (long)c * P.cstride];
    }
    if (MODE == MVN_ST_FWD_MUL_INV && single) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int w = w0 + u * nthreads;
        w = w < total ? w : total - 1;
        int p = w / T, c = w % T;
        c = c < ncol ? c : ncol - 1;
        g[u] = P.spec[base + (long)p * P.estride + (long)c * P.cstride];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int w = w0 + u * nthreads;
      if (w < total) {
        const int j = w / T, c = w % T;
        buf[j * TP + c] = (c < ncol) ? v[u] : cmake(0.f, 0.f);
      }
    }
  }
  MVN_SYNC();
  if (MODE == MVN_ST_INV) {
    lds_fft_dit<+1, T, COMP>(buf, alt, TP, P.ax, tw, tid, nthreads);
  } else {
    lds_fft_dif<-1, T, COMP>(buf, alt, TP, P.ax, tw, tid, nthreads);
    if (MODE == MVN_ST_FWD_MUL_INV) {
      if (single) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int w = tid + u * nthreads;
          if (w < total) {
            const int p = w / T, c = w % T;
            buf[p * TP + c] = cmul(buf[p * TP + c], g[u]);
          }
        }
      } else {
        for (int w0 = tid; w0 < total; w0 += U * nthreads) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            int w = w0 + u * nthreads;
            w = w < total ? w : total - 1;
            int p = w / T, c = w % T;
            c = c < ncol ? c : ncol - 1;
            g[u] = P.spec[base + (long)p * P.estride + (long)c * P.cstride];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int w = w0 + u * nthreads;
            if (w < total) {
              const int p = w / T, c = w % T;
              buf[p * TP + c] = cmul(buf[p * TP + c], g[u]);
            }
          }
        }
      }
      MVN_SYNC();
      lds_fft_dit<+1, T, COMP>(buf, alt, TP, P.ax, tw, tid, nthreads);
    }
  }
  for (int w = tid; w < total; w += nthreads) {
    const int p = w / T, c = w % T;
    if (c < ncol) P.data[base + (long)p * P.estride + (long)c * P.cstride] = buf[p * TP + c];
  }
}

// ---------------------------------------------------------------------------------------------
// PSF placement: kernel voxel (z,y,x) -> ((z-k0/2) mod D0, (y-k1/2) mod D1, (x-k2/2) mod D2),
// integer k/2, so the centre voxel lands on the origin (inc/padd_utils.h:11-40).
// ---------------------------------------------------------------------------------------------
MVN_HD void mvn_scatter_psf_item(const float* kernel, int k0, int k1, int k2, float* target,
                                 int D0, int D1, int D2, long pitch, float scale, long i) {
  const int x = (int)(i % k2);
  const int y = (int)((i / k2) % k1);
  const int z = (int)(i / ((long)k2 * k1));
  int ix = x - k2 / 2, iy = y - k1 / 2, iz = z - k0 / 2;
  if (ix < 0) ix += D2;
  if (iy < 0) iy += D1;
  if (iz < 0) iz += D0;
  target[((long)iz * D1 + iy) * pitch + ix] = kernel[i] * scale;
}
