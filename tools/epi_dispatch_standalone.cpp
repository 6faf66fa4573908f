// epi_dispatch_standalone.cpp -- the launch-side dispatch of csrc/mvn_pass_bodies.hpp and a shared launch check,
// headers only (g++ -DMVN_HOST_EMU -I csrc).  Exits non-zero on the first mismatch, prints "ok" otherwise.
//
//  * mvn_epi_dispatch<KIND, GENERIC>(mode, f), for every pass kind and every integer mode from -1 to one past the last
//    enumerator: f is called exactly once, with the constant equal to the mode (GENERIC: to its form in the
//    run-time-radix bodies), or std::invalid_argument is thrown - exactly for r2c with anything but STORE, the fused
//    pass with DELTA, and anything outside the enum;
//  * mvn_dispatch_tile_width, mvn_epi_extra_lds_bytes, mvn_wave_rows_per_slot, mvn_wave_rows_kind_bit against their
//    values written out;
//  * mvn_dim0_check (mvn_dim0_direct.hpp) on two launch geometries that the product's copy of the check refused and
//    the emulation's copy let through - no call of the C-ABI reaches them (the engine never builds them; the first
//    needs a plane of 2^28 bins).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mvn_dim0_direct.hpp"
#include "mvn_pass_bodies.hpp"

static int g_failures = 0;
#define EXPECT(cond, ...)                     \
  do {                                        \
    if (!(cond)) {                            \
      ++g_failures;                           \
      std::printf("FAIL %s: ", #cond);        \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

// what the table must say, written out
static bool expect_allowed(int kind, int mode) {
  if (mode < MVN_EPI_STORE || mode > MVN_EPI_DIVIDE_NM_U16) return false;
  if (kind == MVN_PASS_R2C) return mode == MVN_EPI_STORE;
  if (kind == MVN_PASS_C2R_R2C) return mode != MVN_EPI_DELTA;
  return true;
}
static int expect_form(int mode) {
  switch (mode) {
    case MVN_EPI_STORE:
    case MVN_EPI_DIVIDE:
    case MVN_EPI_UPDATE:
    case MVN_EPI_DELTA: return MVN_EPI_STORE;
    default: return mode;
  }
}

template <int KIND, bool GENERIC>
static void check_dispatch() {
  for (int mode = -1; mode <= MVN_EPI_DIVIDE_NM_U16 + 1; ++mode) {
    int calls = 0, got = -100;
    bool threw = false;
    try {
      mvn_epi_dispatch<KIND, GENERIC>(mode, [&](auto epi) {
        static_assert(mvn_epi_allowed(KIND, decltype(epi)::value) || GENERIC, "instantiated for a mode the pass does not take");
        ++calls;
        got = decltype(epi)::value;
      });
    } catch (const std::invalid_argument& e) {
      threw = true;
      static const char* const pass[] = {"r2c", "c2r", "fused c2r + r2c"};
      const std::string want = "mvn: epilogue mode " + std::to_string(mode) + " in a " + pass[KIND] + " last-axis pass";
      EXPECT(want == e.what(), "the message names the mode and the pass: %s", e.what());
    }
    const bool allowed = expect_allowed(KIND, mode);
    EXPECT(threw == !allowed, "kind %d generic %d mode %d: threw %d", KIND, (int)GENERIC, mode, (int)threw);
    EXPECT(calls == (allowed ? 1 : 0), "kind %d generic %d mode %d: %d calls", KIND, (int)GENERIC, mode, calls);
    if (allowed)
      EXPECT(got == (GENERIC ? expect_form(mode) : mode), "kind %d generic %d mode %d: constant %d", KIND, (int)GENERIC, mode, got);
  }
}

static void check_helpers() {
  for (int T : {16, 8, 4, 2, 1}) {
    int calls = 0, got = 0;
    mvn_dispatch_tile_width(T, [&](auto t) { ++calls, got = decltype(t)::value; });
    EXPECT(calls == 1 && got == T, "tile width %d: %d calls, constant %d", T, calls, got);
  }
  for (int T : {0, 3, 32, -1}) {
    bool threw = false;
    try {
      mvn_dispatch_tile_width(T, [&](auto) {});
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    EXPECT(threw, "tile width %d accepted", T);
  }
  const int nt = 512;
  for (int mode = 0; mode < MVN_EPI_COUNT; ++mode) {
    const bool stats = mode == MVN_EPI_UPDATE_STATS || mode == MVN_EPI_UPDATE_STATS_TV;
    const bool nm = mode == MVN_EPI_DIVIDE_NM || mode == MVN_EPI_DIVIDE_NM_U16;
    const bool psi = mode == MVN_EPI_UPDATE || mode == MVN_EPI_DELTA || stats || mode == MVN_EPI_UPDATE_TV;
    const bool divides = mode == MVN_EPI_DIVIDE || mode == MVN_EPI_DIVIDE_U16 || nm;
    EXPECT(mvn_epi_extra_lds_bytes(mode, nt) == (stats ? mvn_stat_lds_bytes(nt) : nm ? mvn_nm_lds_bytes(nt) : 0), "mode %d", mode);
    EXPECT(mvn_wave_rows_per_slot(MVN_PASS_R2C, mode) == 16 && mvn_wave_rows_per_slot(MVN_PASS_C2R, mode) == 16, "mode %d", mode);
    EXPECT(mvn_wave_rows_per_slot(MVN_PASS_C2R_R2C, mode) == (psi ? 32 : 16), "mode %d", mode);
    EXPECT(mvn_wave_rows_kind_bit(MVN_PASS_R2C, mode) == 1, "mode %d", mode);
    EXPECT(mvn_wave_rows_kind_bit(MVN_PASS_C2R, mode) == (mode == MVN_EPI_DELTA ? 16 : 2), "mode %d", mode);
    EXPECT(mvn_wave_rows_kind_bit(MVN_PASS_C2R_R2C, mode) == (divides ? 4 : 8), "mode %d", mode);
  }
  EXPECT(mvn_stat_lds_bytes(nt) == 20L * nt && mvn_nm_lds_bytes(nt) == 24L * nt, "scratch sizes");
}

static bool dim0_refused(const Dim0DirectParams& p) {
  try {
    mvn_dim0_check(p);
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static void check_dim0() {
  // (the check reads no memory: the pointers only have to differ)
  static cfloat a, b, c;
  static int inv;
  Dim0DirectParams p;
  std::memset(&p, 0, sizeof(p));
  p.in = &a, p.out = &b, p.taps = &c;
  p.d0 = 16, p.k = 5, p.kd = 6, p.h = 2, p.plane = 12;
  EXPECT(!dim0_refused(p), "a plain launch refused");
  Dim0DirectParams q = p;
  q.plane = 1L << 28;  // the plane-size limit, which only the product asked for
  EXPECT(dim0_refused(q), "a plane of 2^28 bins accepted");
  q.plane = (1L << 28) - 1;
  EXPECT(!dim0_refused(q), "a plane of 2^28 - 1 bins refused");
  q = p;
  q.packed = 1, q.inv1 = &inv, q.taps2 = &c, q.C = 4, q.d1 = 3;
  EXPECT(!dim0_refused(q), "a packed launch refused");
  q.C = -4, q.d1 = -3;  // C * d1 == plane all the same: only the product asked for C >= 1, d1 >= 1
  EXPECT(dim0_refused(q), "a packed launch with negative extents accepted");
}

int main() {
  check_dispatch<MVN_PASS_R2C, false>();
  check_dispatch<MVN_PASS_C2R, false>();
  check_dispatch<MVN_PASS_C2R_R2C, false>();
  check_dispatch<MVN_PASS_R2C, true>();
  check_dispatch<MVN_PASS_C2R, true>();
  check_dispatch<MVN_PASS_C2R_R2C, true>();
  check_helpers();
  check_dim0();
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
