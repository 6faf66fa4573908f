// mvn_engine.hpp -- plans, plan_store and the device-resident Richardson-Lucy engine.
//
// Replaces, MI355X-first, the reference's
//   gpu::plan_store<float>                         inc/plan_store.cuh:20-216
//   inplace_convolve_on_device                     inc/gpu_convolve.cuh:113-142
//   inplace_gpu_deconvolve_iteration_all_on_device src/gpu_deconvolve_methods.cuh:345-562
// Everything a call needs (views, weights, both PSF spectra per view, psi, one work volume)
// stays resident in HBM for the whole call; PSF spectra are computed once per call, not once
// per (view, iteration) as the reference GPU path does (inc/gpu_convolve.cuh:121-124).
#pragma once

#include <array>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "mvn_backend.hpp"
#include "mvn_plan.hpp"

namespace mvn {

enum KernelKind {
  KK_ROWS_R2C = 0,
  KK_ROWS_C2R,
  KK_ROWS_FUSED,      // c2r + divide + r2c
  KK_ROWS_FUSED_UPD,  // c2r + psi update + r2c
  KK_AXIS1_FWD,
  KK_AXIS1_INV,
  KK_AXIS0_FUSED,
  KK_AXIS0_FWD,
  KK_AXIS0_INV,
  KK_NYQ,
  KK_OTHER,
  KK_AXIS0_DIRECT,  // dim0 leg as a direct convolution with the PSF's planes (mvn_dim0_direct.hpp)
  KK_MID_FUSED,     // dim1 forward + direct dim0 leg + dim1 inverse in one pass (mvn_mid_fused.hpp)
  KK_TV,            // the total-variation factor of psi (mvn_tv.hpp)
  KK_COUNT
};
const char* kernel_kind_name(int k);

// Optional per-launch timing with events on the launch stream (bench.py's roofline leg).
class Profiler {
 public:
  bool enabled = false;
  int sample_every = 1;  // time every n-th (view, iteration) only: keeps the events' own cost low
  void begin(int kind, be::stream_t s);
  void end(be::stream_t s);
  // waits for the recorded events and folds them into the totals
  void collect();
  void reset();
  double total_ms[KK_COUNT] = {0};
  long count[KK_COUNT] = {0};
  ~Profiler();

 private:
  struct Rec {
    int kind;
    be::Event a, b;
  };
  std::vector<Rec> recs_;
  std::vector<be::Event> pool_;
  be::Event get_event();
};

struct DevAxis {
  AxisPlanHost host;
  be::DeviceBuffer<cfloat> tw, tws, chirp, bhat;  // (chirp, bhat: bluestein axes only)
  be::DeviceBuffer<int> rev, inv;
  AxisPlan view;  // the tables above, as the kernels take them
  explicit DevAxis(int n, bool composite = false);
};

struct PassGeom {
  int T = 1, TP = 1, threads = 256;
  size_t lds_bytes = 0;
  long lds_alt = 0;
  long lds_tw = 0;
};

typedef std::array<int, 3> shape_t;
typedef std::vector<std::array<int, 3>> kernel_list_t;  // the kernel extents of a call: kernel1, kernel2 of every view

// ---------------------------------------------------------------------------------------------
// The PSF form rule.  Every kernel is held in one form: the direct dim0 form (taps along dim0, no dim0 transform,
// mvn_dim0_direct.hpp) or the 3-D spectrum.  The forms of a call's kernels decide whether the sequential sweep takes
// the fused middle pass (mvn_mid_fused.hpp), whether the Nyquist bins are packed into the DC column, and under the
// zero padding policy whether dim0 keeps the exact extent image + kernel - 1 (mvn_abi.cpp).  The rule needs no
// device and no plan, so the ABI can apply it before an engine exists; an engine applies it to its own plan.
// ---------------------------------------------------------------------------------------------
struct FormSwitches {
  bool direct = true;                // MVN_DIM0_DIRECT (0: never the direct form)
  int direct_max = MVN_D0_MAX_TAPS;  // MVN_DIM0_DIRECT_MAX: most PSF planes of the direct form
  long min_plane = 131072;           // MVN_DIM0_DIRECT_MIN_PLANE: work items a launch of the leg should have
  long min_items = 0;                // MVN_DIM0_DIRECT_MIN_ITEMS: fewest work items for which the leg is used at all
  int mid_fused = 1;                 // MVN_MID_FUSED: 0 never, 1 where it is worth it, 2 whenever the shape has it
  bool fixed = true;                 // MVN_NO_FIXED unset or 0: plans use the fixed-length kernels where they can
  static FormSwitches from_env();    // read once per engine and once per ABI call (tests change them in between)
  bool operator==(const FormSwitches& o) const {
    return direct == o.direct && direct_max == o.direct_max && min_plane == o.min_plane && min_items == o.min_items &&
           mid_fused == o.mid_fused && fixed == o.fixed;
  }
};

// Which axes of a plan of layout L run the fixed-length kernels (mvn_fixed.hpp), `fixed` being the switch the plan
// is built with.  Known from the extents alone, and needed before the axis plans are built (the fixed kernels have
// their own radix schedule, see AxisPlanHost::factorize).
bool rows_fixed(const Layout& L, bool fixed);
bool ax1_fixed(const Layout& L, bool fixed);
bool ax0_fixed(const Layout& L, bool fixed);
// a plan of layout L has the line-layout forms of the last-axis kernels and the fused middle pass (d1 = d2 = 512)
bool lines_capable(const Layout& L, bool fixed);
// planes of the tap arrays of a PSF of k0 planes
inline int taps_depth(int k0) { return ((k0 + 1 + 15) / 16) * 16; }

// The rule for a volume of layout L whose plan was built with the fixed-length switch `plan_fixed` (a plan in the
// store keeps the switch of its construction; the tap arrays' plans take sw.fixed).
struct FormRule {
  Layout L;
  FormSwitches sw;
  bool plan_fixed;
  FormRule(const Layout& layout, const FormSwitches& s, bool pf) : L(layout), sw(s), plan_fixed(pf) {}
  // The direct dim0 form: the PSF has at most direct_max planes, the volume is deep enough for the kernel's window
  // and has enough work items, and the tap arrays' plan transforms dims 1 and 2 with the volume plan's kernel family
  // (same family => same position order of the spectra).
  bool direct(const int* kdims) const;
  // the direct form plus the taps of the fused middle pass: wherever the pass COULD run, worth it or not
  bool lines_taps(const int* kdims) const;
  // the fused middle pass is worth it for a PSF of k0 planes (or forced, MVN_MID_FUSED=2)
  bool lines_worth(int k0) const;
  // the kernel takes the fused middle pass
  bool lines(const int* kdims) const { return lines_taps(kdims) && lines_worth(kdims[0]); }
  // every kernel of a call is held in the direct form / takes the fused middle pass
  bool all_direct(const kernel_list_t& k) const;
  bool all_lines(const kernel_list_t& k) const;
};

// a second stream plus the two events used to fork it from / join it to the main stream
struct SideStream {
  be::Event fork, join;
  be::Stream s;
  void create();
  // side stream waits for everything enqueued on `main` so far / `main` waits for the side stream
  void fork_from(be::stream_t main);
  void join_into(be::stream_t main);
};

class Plan3D {
 public:
  const int device;
  const Layout L;
  const bool fixed;  // built with the fixed-length kernels allowed (FormSwitches::fixed)
  DevAxis ax2, ax1, ax0;
  be::DeviceBuffer<cfloat> twr;  // d2-th roots of unity (even d2)
  be::DeviceBuffer<unsigned> no_poison;  // a zero word: what EpilogueParams::poison points to after an FFT dim0 leg
  PassGeom g_rows, g_ax1, g_ax0, g_nyq1, g_nyq0, g_nyq1_line;
  // compile-time specialised kernels (mvn_fixed.hpp) are used where the shape allows
  bool fx_rows = false, fx_ax1 = false, fx_ax0 = false;
  // the Nyquist plane's dim1 transforms ride in the main array's launches where those are the fixed-length
  // walking kernels
  bool nyq_rides() const { return fx_ax1; }
  PassGeom gx_rows, gx_ax1, gx_ax0;

  Plan3D(int device, int d0, int d1, int d2, bool fixed);

  size_t main_bytes() const { return L.real_floats() * sizeof(float); }
  size_t nyq_bytes() const { return L.nyq_cplx() * sizeof(cfloat); }

  // last-axis passes
  // `row0` / `nrows` (default: all d0*d1 rows) restrict a pass to a range of rows: every array a
  // last-axis pass touches is indexed by row, so a range is the same launch on shifted pointers.
  // The view-sharded driver uses it to produce and consume the correction chunk by chunk under
  // the all-reduce (Engine::compute_delta_chunk / apply_delta_chunk).
  // `lines`: the half-spectrum is in the LINE layout of the fused middle pass ([plane][position][row], Nyquist bins
  // packed: the Nyquist pointer must be null); out-of-place for rows_r2c, in place tile by tile for rows_c2r_r2c
  void rows_r2c(const float* in_real, cfloat* out, cfloat* out_nyq, be::stream_t s,
                Profiler* prof = nullptr, long row0 = 0, long nrows = -1, bool lines = false) const;
  // (`st`: the window and records of an MVN_EPI_UPDATE_STATS epilogue)
  void rows_c2r(const cfloat* in, const cfloat* in_nyq, float* out_real,
                const EpilogueParams& epi, be::stream_t s, Profiler* prof = nullptr,
                long row0 = 0, long nrows = -1, bool lines = false, const MvnStatsParams* st = nullptr) const;
  bool lines_capable() const { return mvn::lines_capable(L, fixed); }
  // dim1 forward + K-tap direct convolution along dim0 + dim1 inverse, `in` -> `out` (both in the line layout);
  // taps: [kd][C][d1] as prepared by taps_to_lines()
  // zcount > 0: the output planes [zbeg, zbeg + zcount) only (slabs with halo planes); peers: further poison words
  void mid_fused(const cfloat* in, cfloat* out, const cfloat* taps, int k, int kd, unsigned* poison,
                 unsigned poison_epoch, be::stream_t s, Profiler* prof = nullptr, int zbeg = 0, int zcount = 0,
                 int n_peers = 0, unsigned* const* peers = nullptr) const;
  // PSF planes after the last-axis pass (line layout, this plan = the small plan of the tap arrays) -> transformed
  // along dim1 into the bin order mid_fused() filters in; in place
  void taps_to_lines(cfloat* taps, be::stream_t s) const;
  // rows per tile of the last-axis passes and whether a launch needs whole tiles
  int rows_tile() const { return fx_rows ? gx_rows.T : g_rows.T; }
  bool rows_need_full_tiles() const { return fx_rows; }
  // fused c2r + pointwise + r2c (even d2 only, see can_fuse_rows()); in place on
  // (data, nyq); epi.mode is DIVIDE, UPDATE or STORE
  bool can_fuse_rows() const { return L.even; }
  void rows_c2r_r2c(cfloat* data, cfloat* nyq, const EpilogueParams& epi, be::stream_t s,
                    Profiler* prof = nullptr, long row0 = 0, long nrows = -1, bool lines = false,
                    const MvnStatsParams* st = nullptr) const;
  // strided passes on the main array and its Nyquist plane; mode = MvnStridedMode
  // `s_nyq` (default: s) is the stream of the small Nyquist-plane launches; giving them their own
  // stream lets the 2 MB plane ride along with the full-volume passes (see SideStream)
  // `z0` / `nz` (default: all d0 planes) restrict the pass to a range of planes (lines along d1
  // never leave their plane)
  void axis1(int mode, cfloat* data, cfloat* nyq, be::stream_t s, Profiler* prof = nullptr,
             be::stream_t s_nyq = nullptr, int z0 = 0, int nz = -1) const;
  // `src` / `src_nyq` (optional) make the pass out of place: read there, write to data / nyq
  // `spec_tiled`: the main-array spectrum is in the tile-contiguous layout of retile_spectrum()
  void axis0(int mode, cfloat* data, cfloat* nyq, const cfloat* spec, const cfloat* spec_nyq,
             be::stream_t s, Profiler* prof = nullptr, be::stream_t s_nyq = nullptr,
             const cfloat* src = nullptr, const cfloat* src_nyq = nullptr, bool spec_tiled = false) const;
  // PSF spectra of a resident engine are kept TILE-CONTIGUOUS for the fused dim0 pass where that
  // pass runs the fixed-length kernels: [tile][row][T columns] instead of [row][d1 * C columns], so
  // that the operand fetch of a tile is one stream of d0 * T * 8 bytes (64 KB at 512^3) instead of d0
  // row segments of 128 bytes, each on another 1 MB-strided page.
  bool tiles_spectra() const { return fx_ax0; }
  void retile_spectrum(const cfloat* natural, cfloat* tiled, be::stream_t s) const;

  // whole transforms, un-normalised, in place on (vol, nyq)
  void forward(float* vol, cfloat* nyq, be::stream_t s, Profiler* prof = nullptr) const;
  void backward(float* vol, cfloat* nyq, float scale, be::stream_t s,
                Profiler* prof = nullptr) const;
  // cyclic convolution: out <- epilogue( IFFT( FFT(in) * spec ) ); `work` may alias `in`
  void convolve(const float* in_real, cfloat* work, cfloat* work_nyq, const cfloat* spec,
                const cfloat* spec_nyq, float* out_real, const EpilogueParams& epi,
                be::stream_t s, Profiler* prof = nullptr) const;
  // the three strided passes of a convolution (dim1 forward, dim0 forward*PSF*inverse, dim1
  // inverse); with `side` the Nyquist plane's three launches run on a second stream, forked
  // after and joined before the last-axis passes that produce / consume the plane
  void middle_passes(cfloat* work, cfloat* work_nyq, const cfloat* spec, const cfloat* spec_nyq,
                     be::stream_t s, Profiler* prof, struct SideStream* side, bool spec_tiled = false) const;
  // spectrum of a PSF: zero volume, centre->origin wrapped insert scaled by `scale`, forward FFT
  void psf_spectrum(const float* d_kernel, const int* kdims, float scale, float* spec_vol,
                    cfloat* spec_nyq, be::stream_t s) const;

 private:
  static PassGeom pick_geom(int n, bool generic, bool rows, int max_t);
};

// Process-wide plan cache keyed by (device, logical shape); the reference keys by logical shape
// only (inc/plan_store.cuh:31-33) because it knows a single device.  Thread-safe, unlike the
// reference's (SURVEY.md 8b "Threading").
class PlanStore {
 public:
  static PlanStore& get();
  std::shared_ptr<Plan3D> add(int device, const shape_t& shape);
  bool has_key(int device, const shape_t& shape);
  // throws std::runtime_error on a miss, like the reference (inc/plan_store.cuh:140-152)
  std::shared_ptr<Plan3D> lookup(int device, const shape_t& shape);
  std::shared_ptr<Plan3D> find(int device, const shape_t& shape);  // nullptr on a miss
  bool empty();
  size_t size();
  void clear();

 private:
  std::mutex mu_;
  std::map<std::array<int, 4>, std::shared_ptr<Plan3D>> plans_;
};

// The stacks a view update reads, not owned: a resident view's own volumes (ViewSlot::stacks), or the ring slot the
// pair of a streamed view has landed in (Engine::ring_acquire).
struct ViewStacks {
  float* image;  // image_u16: a uint16 volume (the same element grid at 2 bytes per voxel) behind this pointer
  bool image_u16;
  float* weights;
};

struct ViewSlot {
  // image and weights of a RESIDENT view; a streamed view never holds any (its stacks pass through the ring)
  be::DeviceBuffer<float> image;
  bool image_u16 = false;
  be::DeviceBuffer<float> weights;
  ViewStacks stacks() const { return ViewStacks{image.get(), image_u16, weights.get()}; }
  be::DeviceBuffer<float> spec[2];  // main array of the spectrum of kernel i (pre-scaled by 1/N)
  be::DeviceBuffer<cfloat> nyq[2];
  bool set = false;
  // host copies of the kernels whose spectra spec[0] / spec[1] currently hold: a later call that
  // brings the same PSF for this slot (Fiji's block-after-block calls do) skips the preparation
  std::vector<float> kcopy[2];
  int kdims[2][3] = {{0, 0, 0}, {0, 0, 0}};
  // direct dim0 form of kernel i (mvn_dim0_direct.hpp): its planes after the last-axis and dim1
  // transforms, [tap_kd][d1][C] (+ Nyquist [tap_kd][d1]), pre-scaled by 1 / (d1 d2).  tap_k = PSF planes
  // when this form is what the slot holds for kernel i, 0 when the 3-D spectrum (spec / nyq) is.
  be::DeviceBuffer<float> taps[2];
  be::DeviceBuffer<cfloat> taps_nyq[2];
  int tap_k[2] = {0, 0};
  int tap_kd[2] = {0, 0};
  // the same PSF planes for the fused middle pass (mvn_mid_fused.hpp): [tap_kd][C][d1], Nyquist bins packed, bins
  // along dim1 in that pass's own order.  taps_l_ok: valid for the kernel tap_k / tap_kd describe.
  be::DeviceBuffer<float> taps_l[2];
  bool taps_l_ok[2] = {false, false};
};

// ---------------------------------------------------------------------------------------------
// The opt-in switches of the Richardson-Lucy loop, as one value: what one call of the loop can be asked to do
// beyond the reference's sweeps (mvn_engine_api.h).  The ABI keeps one process-wide value and hands every call a
// copy; an engine holds one for its own API.  The only copy of each rule lives here.
// ---------------------------------------------------------------------------------------------
struct LoopOptions {
  double tolerance = -1.;  // >= 0: the update passes reduce {S, M, P} per sweep; > 0: the loop ends at S / P <= tolerance
  int accel = 0;           // 1: vector extrapolation between the sweeps (mvn_extrapolate.hpp)
  int reg_kind = 0;        // MVN_REG_TIKHONOV / MVN_REG_TV
  double epsilon = 0.;     // MVN_REG_TV only
  std::vector<float> background;  // camera background: empty none, one value every view, else one per view
  int likelihood = 0;      // 1: the divide pass sums {D, Y, M} per (sweep, view)

  // Who reports a broken rule, in the words each API has always used: the engine speaks of `lambda` under "mvn: ",
  // the reference-shaped entry points of the workspace's `lambda_`.
  struct Voice {
    const char* prefix;
    const char* lambda;
  };
  static constexpr Voice kEngine = {"mvn: ", "lambda"};
  static constexpr Voice kAbi = {"", "lambda_"};

  bool stats_on() const { return tolerance >= 0.; }
  bool accel_on() const { return accel == 1; }
  bool tv_on(double lambda) const { return reg_kind == 1 && lambda > 0.; }
  bool noise_model_on() const {
    if (likelihood) return true;
    for (float b : background)
      if (b != 0.f) return true;
    return false;
  }
  float background_of(int v) const {
    return background.empty() ? 0.f : background[background.size() == 1 ? 0 : (size_t)v];
  }
  static bool tv_epsilon_ok(double epsilon);
  // |div p| <= 6: below 1/12 the denominator 1 - lambda div p stays above 0.5 with no clamp in the kernel
  static void check_tv_lambda(double lambda, const Voice& who);
  // the ranges of the values themselves
  void validate(const Voice& who) const;
  // what can only be judged against a call: the TV weight, and the background count against the view count
  void check_call(int V, double lambda, const Voice& who) const;
  // The slab drivers (MVN_DEVICES) know none of the switches: the name of one that is on, or nullptr.
  const char* needs_single_device() const;
  // Halo mode (a slab of a multi-device group) and the simultaneous step run none of them either.  what == nullptr:
  // these options were asked of an engine in halo mode; else `what` ("no halo hook on an engine", ...) was asked of
  // an engine that holds them.  Throws when a switch is on.
  void refuse(const char* what = nullptr) const;
};

// What one call of the loop reports back.
struct LoopResult {
  int ran = 0;                 // sweeps run
  int views = 0;
  std::vector<double> rows;    // statistics on: {S, M, P} per sweep run
  std::vector<double> alphas;  // acceleration on: a_1 .. a_ran (the last one 0)
  std::vector<double> like;    // noise model on: {D, Y, M} per (sweep run k, view v) at 3 (k V + v)
};

// One set of records of the loop: every workgroup of a pass writes one record of 3 doubles for its view, and one
// reduce launch per sweep folds them into rows (convergence: the update passes; noise model: the divide passes).
struct RecordSet {
  double* rec = nullptr;      // per view: cap records
  unsigned* count = nullptr;  // per view: records of its last pass
  double* out = nullptr;      // the rows
  long cap = 0;
  bool on() const { return rec != nullptr; }
};

// The device state of the loop's switches.  bytes_of() is the one table of (buffer, bytes): Engine::memory_need
// prices a call by it and Engine::iterate allocates by it.  The buffers before kKept live for one iterate(); the TV
// factor volume stays with the engine while the calls keep asking for it.
struct LoopState {
  enum Buffer {
    STAT_REC, STAT_COUNT, STAT_OUT,          // convergence statistics
    NM_REC, NM_COUNT, NM_OUT,                // noise model
    X_PREV, G_PREV, Y_SAVE, ACCEL_REC, ALPHA,  // extrapolation: x_{k-1}, g_{k-1}, y_{k-1}, pass A's records, the a_k
    TV,                                      // the total-variation factor volume, psi's layout
    N_BUFFERS,
    kKept = TV
  };
  be::DeviceBuffer<> buf[N_BUFFERS];
  LoopOptions o;  // of the running iterate()
  static void bytes_of(const Layout& L, int V, int iterations, double lambda, const LoopOptions& o,
                       size_t bytes[N_BUFFERS]);
  // every workgroup of an update or divide pass writes one record; no launch has more workgroups than the volume has rows
  static long record_cap(const Layout& L) { return (long)L.rows; }
  // workgroups of the extrapolation's pass A (mvn_extrapolate.hpp): a function of the extents only
  static long accel_records(const Layout& L) { return mvn_accel_blocks((long)L.real_floats(), L.RP == L.d2 ? 4 : 2); }
  template <typename T>
  T* at(Buffer b) const { return (T*)buf[b].get(); }
  RecordSet records(Buffer first, const Layout& L) const {
    RecordSet r;
    r.rec = at<double>(first), r.count = at<unsigned>((Buffer)(first + 1)), r.out = at<double>((Buffer)(first + 2));
    r.cap = record_cap(L);
    return r;
  }
  void allocate(const size_t bytes[N_BUFFERS]);  // what the table asks for and is not held yet
  void release(int first, int last);             // buffers [first, last)
};

// the launch parameters of the pass of mvn_tv.hpp on a volume of layout L
inline TvParams tv_params(const Layout& L, const float* psi, float* t, double lambda, double epsilon) {
  TvParams p = {};
  p.psi = psi, p.t = t;
  p.d0 = L.d0, p.d1 = L.d1, p.d2 = L.d2, p.RP = L.RP;
  p.lambda = (float)lambda;
  p.e2 = (float)epsilon * (float)epsilon;
  return p;
}

// What one ABI call on a new engine allocates on the device (Engine::memory_need): the kernel extents of every
// view (kernel1 and kernel2), the host-shaped embedding scratch of the padded policies, the residency plan -
// how many views keep their image and weights in host memory and how many ring slots (pairs of volumes) they
// rotate through - and what the loop's switches add (LoopState::bytes_of).
struct MemoryQuery {
  shape_t ext = {{0, 0, 0}};
  kernel_list_t kernels;  // 2 per view: kernel1, kernel2
  size_t embed_floats = 0;
  int streamed = 0;
  int ring = 0;
  LoopOptions loop;  // the switches of the call,
  int iterations = 1;  // ... its sweeps
  double lambda = 0.;  // ... and its regularisation weight
  // per view: the call wants its image kept as uint16 (image storage mode 1 and a uint16 stack that is no broadcast);
  // empty: none.  What is then held as uint16: Engine::kept_u16.
  std::vector<char> image_u16;
};

// A stack as the engine takes it (the described entry points' mvn_stack_desc, include/mvn_engine_api.h; the plain ones
// hand over dense float32 host stacks, Engine::dense): where element (0, 0, 0) lives, what it is made of and how far
// apart its elements are.  Extents are the engine's embedding window.
struct StackRef {
  const void* ptr = nullptr;
  bool u16 = false;     // uint16 elements (images only), else float32
  bool device = false;  // device memory: the ingest / extract kernels work on it directly
  long long stride[3] = {0, 0, 0};  // in elements; all zero: one value for every voxel (inputs only)
  bool broadcast() const { return stride[0] == 0 && stride[1] == 0 && stride[2] == 0; }
  // an IMAGE only: the stack is a raw view of extents geom->m, strides over those, and is resampled into the window
  // through geom->M (mvn_resample.hpp) instead of being copied; the weights of such a view may have a null ptr: they
  // are then computed from the geometry, unnormalised (Engine::normalize_weights)
  const ResampleGeom* geom = nullptr;
  static StackRef dense_host(const float* p, const int* dims) {
    StackRef r;
    r.ptr = p;
    r.stride[0] = (long long)dims[1] * dims[2], r.stride[1] = dims[2], r.stride[2] = 1;
    return r;
  }
};

class Engine {
 public:
  Engine(int device, const shape_t& dims, int num_views);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  int device() const { return device_; }
  const Layout& layout() const { return plan_->L; }
  int num_views() const { return (int)views_.size(); }
  be::stream_t stream() const { return stream_.get(); }
  Profiler& profiler() { return prof_; }

  // Out-of-core calls: the views listed keep their image and weights stacks in host memory; every view update of
  // one of them reads the pair from a ring of `ring` device slots, filled by the uploader thread (stage_view in the
  // first sweep, stream_view after it) under the compute of the other views.  PSF forms, psi and the work volumes
  // stay resident.  Set once, before the views are allocated; an engine keeps its plan for life.
  void set_residency(const std::vector<int>& streamed, int ring);
  int streamed_count() const { return (int)streamed_order_.size(); }
  int ring_size() const { return (int)ring_.size(); }
  bool is_streamed(int v) const { return stream_pos_[(size_t)v] >= 0; }
  // uploader thread, sweeps 1 .. n-1: the next streamed view's stacks into their ring slot (views in sweep order)
  void stream_view(int v, const StackRef& image, const StackRef& weights);
  // main thread after an error: wake an uploader that waits for a ring slot
  void abort_streaming();
  // Bytes the ABI call described by q allocates on a new engine of extents q.ext, allocating nothing itself: the
  // PSF forms (direct taps, fused-pass taps, 3-D spectra) that `rule` gives for its kernels, the loop state of its
  // switches (LoopState::bytes_of), plus a small slack for plan tables and allocator rounding.  The single source of
  // truth of the memory planner (mvn_abi.cpp).
  static size_t memory_need(const MemoryQuery& q, const FormRule& rule);
  // The views s of V views stream: spread evenly over the sweep (view floor((j + 1/2) V / s) for j < s), so that
  // each upload runs under the resident view updates between two streamed ones.
  static std::vector<int> spread_views(int V, int s);
  // Image storage (mvn_set_image_storage, include/mvn_engine_api.h).  `want`: per view, keep the image as uint16.
  // A resident view is held as it is wanted.  The streamed views share the ring's slots, whose margins are cleared
  // once and never rewritten by a float32 upload: they are held as uint16 only when every streamed view is wanted so
  // (a ring slot is as wide as the widest streamed image).  Used by memory_need and by plan_image_types alike.
  static std::vector<char> kept_u16(const std::vector<char>& want, const std::vector<int>& streamed, int V);
  // ABI call, before reserve_views(): the call's wishes; slots (and the ring) that held the other element type are
  // re-allocated, their PSF forms stay
  void plan_image_types(const std::vector<char>& want);
  std::vector<char> image_types() const { return want_u16_; }
  // engine API (set_view): 1 = a uint16 image stack that is no broadcast is kept as uint16 unless a halo hook is set
  void set_image_storage(int mode) { image_storage_ = mode; }
  // The resample pass of mvn_resample.hpp on the raw stack `image` (image.geom set): p brings the destination volumes and
  // the window, the raw stack's side is filled in here.  A raw stack in host memory (contiguous rows, or one value)
  // crosses into a temporary device buffer first, which is freed once `s` has passed it (the host waits for that).
  // Returns the bytes that crossed PCIe.  The current device is the destination's.
  static long long resample_raw(ResampleParams p, const StackRef& image, be::stream_t s);
  // Its upload alone: a raw stack in HOST memory of extents m (contiguous rows, or one value) as it is into the
  // temporary `tmp`, allocated here and assigned before anything is enqueued on s; *there describes it in device
  // memory.  Returns the bytes that crossed.  check_raw_host: what it refuses, with nothing touched.
  static long long upload_raw(const StackRef& image, const int* m, be::DeviceBuffer<char>& tmp, StackRef* there,
                              be::stream_t s);
  static void check_raw_host(const StackRef& image, const int* m);
  // divide passes launched on a uint16 image, ingest passes that wrote a uint16 volume, since process start
  static void image_storage_counters(long long out[2]);
  // calls that streamed views, streamed view updates, bytes streamed (host -> device), since process start
  static void stream_counters(long long out[3]);
  static void count_streamed_call();

  // Staging (blocking).  A stack enters and leaves as a StackRef (mvn_ingest.hpp), whatever it is made of: a float32
  // stack in host memory (rows must be contiguous) is placed by the copy of its window - H2D, or H2D into the embedding
  // scratch and a strided device copy into margins that were cleared when the volume was allocated; a stack in device
  // memory is read by the ingest pass where it lies, and one value for every voxel (strides 0) is written by it; a
  // uint16 stack in host memory crosses PCIe as uint16 and is then converted and embedded by the same pass - or, where
  // the view's image is held as uint16 (plan_image_types / set_image_storage), placed or embedded unconverted.
  void set_view(int v, const StackRef& image, const StackRef& weights, const float* kernel1, const int* k1dims,
                const float* kernel2, const int* k2dims);
  void set_psi(const StackRef& psi);
  void get_psi(const StackRef& psi);
  // Computed weights (views set with a geometry and no weights stack) over their sum across ALL views, in view order,
  // on the window (mvn_resample.hpp); under "reflect" the fill of those weights volumes runs here, behind it.  Once,
  // after the last view has been placed.  Blocking.
  void normalize_weights();
  // psi <- the fusion of the views as they stand (mvn_fuse.hpp, k_fuse_volumes): over the window, from the V image and
  // the V weights volumes - unnormalised computed weights when it runs before normalize_weights -, `fill` where no
  // weight is positive; the margins then are what set_psi leaves (zeros, or the mirror image under "reflect").
  // Refused with a halo hook, streamed views or a uint16 image volume; psi is then left as it was.  Blocking.
  void fuse_psi(float fill);
  // the caller produced its device stacks on `caller_stream`: the engine's streams wait for what is enqueued there
  // now (an event, no host wait); nullptr: nothing to wait for
  void wait_for_caller(void* caller_stream);
  // ABI call, main thread, after reserve_views(): a view whose two stacks are both in device memory is ingested on
  // the compute stream (nothing to hide behind an upload); stage_view then only prepares its PSFs
  void ingest_device_view(int v, const StackRef& image, const StackRef& weights);

  // Pipelined staging for the blocking ABI call (what the reference's "interleaved" driver was
  // after, src/gpu_deconvolve_methods.cuh:82-326): a second host thread uploads view after view
  // on its own stream while the first RL iteration already runs on the views that have arrived.
  //   reserve_views(kernels)     main thread: allocate every view's buffers up front; from the call's kernel
  //                              extents, decide whether the loop starts on the packed Nyquist layout and the fused
  //                              middle pass before the last view has been staged
  //   stage_view(v, ...)         uploader thread: H2D + PSF spectra of view v on the upload stream
  //   staging_failed()           uploader thread: wake the main thread up after an error
  //   iterate(...)               main thread: waits for view v only before its first use
  void reserve_views(const kernel_list_t& kernels);
  void stage_view(int v, const StackRef& image, const StackRef& weights, const float* kernel1, const int* k1dims,
                  const float* kernel2, const int* k2dims);
  void staging_failed();
  void finish_staging();  // uploader thread, after the last view: drain and free scratch

  // `iterations` Gauss-Seidel sweeps over all views (the reference order,
  // src/gpu_deconvolve_methods.cuh:487-535) under the options o; asynchronous on stream() while every switch is
  // off.  Returns the sweeps run; *result (optional) takes what last_result() keeps.
  //   o.tolerance >= 0: the update passes also reduce the convergence statistics of every sweep k, {S_k, M_k, P_k}
  //     (mvn_engine_api.h); tolerance > 0 ends the loop after the first sweep with S_k / P_k <= tolerance (each
  //     sweep then waits for its statistics).
  //   o.accel == 1: vector extrapolation between the sweeps (mvn_extrapolate.hpp) - the next sweep starts from
  //     y_k = x_k + a_k (x_k - x_{k-1}) instead of x_k; no extrapolation follows the last sweep run, so psi is
  //     always a sweep's own result.
  //   o.reg_kind 0: `lambda` is the reference's Tikhonov weight.  1: total variation - lambda is the TV weight, the
  //     Tikhonov branch is off and every view update is preceded by the pass of mvn_tv.hpp, whose factor volume is
  //     allocated at first need and kept while the calls stay TV; lambda >= 1/12 is refused, lambda == 0 is the
  //     plain loop.
  //   o.background, o.likelihood: view v's camera background b_v enters the forward model, quotient = image /
  //     (H psi + b_v), and - with the likelihood or any b_v != 0 - the divide pass also sums {D, Y, M} per (sweep,
  //     view) over the stacks' window (MVN_EPI_DIVIDE_NM, mvn_pass_bodies.hpp).  Both off: the plain divide pass,
  //     launch for launch.  On: no captured sweep graph is used.
  // A switch that is on makes iterate() wait for the stream before it returns (its rows cross to the host and its
  // buffers go).  None is for an engine with a halo hook (a slab of a multi-device group).
  int iterate(int iterations, double lambda, float min_value, const LoopOptions& o, LoopResult* result = nullptr);
  // ... under the options the engine holds
  int iterate(int iterations, double lambda, float min_value) { return iterate(iterations, lambda, min_value, held_); }
  // The options the engine holds for its own API (mvn_engine_set_regularization, mvn_engine_set_noise_model): validated
  // here, refused on an engine with a halo hook; set_halo_hook and compute_delta* refuse an engine that holds TV or a
  // noise model.  Back at Tikhonov the factor volume goes.
  void set_options(const LoopOptions& o);
  const LoopOptions& options() const { return held_; }
  const LoopResult& last_result() const { return last_; }
  // simultaneous (Jacobi) mode for view sharding: delta <- sum over this engine's views of
  // w_v (next_v - psi), computed from the current psi without changing it
  void compute_delta(double lambda, float min_value);
  void apply_delta();
  // The same step in pieces, so that the caller's all-reduce can run under the compute
  // ("overlap ... by chunking along dim0").  The correction is produced by the LAST
  // pass of the last local view and consumed by passes that never leave a dim0 plane (psi += delta,
  // forward last-axis and dim1 passes of the next iteration), so both ends can go chunk by chunk:
  //   n = delta_chunks(wanted)
  //   compute_delta_head(lambda, min)            all passes but the last view's final one
  //   for c < n: compute_delta_chunk(c, n)       planes [c d0/n, (c+1) d0/n) of delta are final;
  //                                              the caller starts that chunk's all-reduce
  //   for c < n: [wait for chunk c's collective] apply_delta_chunk(c, n, feed_next)
  // feed_next != 0 additionally leaves the chunk's part of psi's dim1-transformed spectrum for the
  // next compute_delta_head (which then skips those two shared passes).
  int delta_chunks(int wanted) const;
  void delta_chunk_range(int c, int n, size_t* first_float, size_t* n_floats) const;
  void compute_delta_head(double lambda, float min_value);
  void compute_delta_chunk(int c, int n);
  void apply_delta_chunk(int c, int n, bool feed_next);
  float* delta_ptr();
  // use caller-owned device memory (volume_floats() floats) as the delta buffer, so that a
  // collective library can all-reduce it in place; nullptr returns to an engine-owned buffer
  void bind_delta(float* external);
  // Halo mode (dim0 slabs of one volume on several ranks, reference update order): the engine's volume is this
  // rank's planes with h halo planes either side; `fn` is called on the host right before every dim0 leg, with
  // the stream drained, and fills the halo planes of `spectrum` (the leg's input, [d0][d1][C] complex, packed
  // Nyquist layout) with the neighbours' planes (copy_planes moves planes between it and exchange buffers).
  // Needs every PSF in the direct form and the packed layout; throws at the first sweep otherwise.
  typedef void (*halo_fn_t)(void* user, void* spectrum, int view, int conv);
  // drain: wait for the stream before calling fn (fn works from the host); false: fn only enqueues work on stream()
  // post: fn is called a second time right AFTER the leg has been enqueued, with conv + 2 - where the ranks merge
  // their poison words (a non-finite input met by ONE slab's leg must turn EVERY slab's volume into NaN)
  void set_halo_hook(halo_fn_t fn, void* user, bool drain = true, bool post = false);
  bool has_halo_hook() const { return halo_fn_ != nullptr; }
  // Tells the engine how many planes at either end of its volume are halo planes (after set_halo_hook): no pass
  // computes them any more - the last-axis and dim1 passes and the leg run on the own planes only (where those
  // start and end on tile boundaries of the last-axis passes; otherwise everything is computed as before).
  // split: the leg runs in two parts, the own planes that do not depend on the halos first, and fn is called
  // once more in between, with conv + 4 - the halo planes need to be in place only behind THAT call, so that an
  // exchange started at the first call runs beside the first part.
  void set_halo_planes(int planes, bool split);
  // The hook also fills the halo planes of the Nyquist plane (leg_input_nyq(), [d0][d1] complex) when the engine
  // runs the split layout: the engine then need not pack the Nyquist bins into the DC column, which costs 6 % at
  // 512^3 (profiles/r04_layouts.md).  layout: -1 the engine's own rule (packed up to 256 MB per volume), 0 split,
  // 1 packed - slabs of one volume take the WHOLE volume's layout, so that they run its arithmetic.
  void set_halo_nyq_aware(int layout) {
    halo_nyq_aware_ = true;
    layout_override_ = layout;
    if (!plan_->nyq_rides()) layout_override_ = 1;  // (run-time-radix dim1 kernels carry no riders)
  }
  // input of the dim0 leg in flight: its Nyquist plane (nullptr in the packed layout); valid inside the hook
  void* leg_input_nyq() const { return (packed_ || lines_) ? nullptr : (void*)work_nyq_; }
  // The poison word (mvn_dim0_direct.hpp, EpilogueParams::poison): a direct dim0 leg that met a non-finite input
  // stores its epoch there.  poison_ptr(): the device word; bind_poison(): use caller-owned device memory (4 bytes,
  // zeroed) instead, e.g. a torch tensor a collective can MAX-reduce in place; poison_get() drains the stream and
  // reads it; poison_merge(v): word = max(word, v), enqueued on stream(); add_poison_peer(): a further word (another
  // slab's, reachable from this device) every report is also written to.
  unsigned* poison_ptr() { return poison_; }
  void bind_poison(unsigned* external);
  unsigned poison_get();
  void poison_merge(unsigned value);
  void add_poison_peer(unsigned* word);
  void clear_poison_peers() { poison_peers_.clear(); }  // (the device table is only read up to n_peers)
  // slabs of one volume on several engines count their direct legs together: same epoch for the same leg
  unsigned poison_epoch() const { return epoch_; }
  void set_poison_epoch(unsigned e) { epoch_ = e; }
  void copy_planes(void* spectrum, int plane0, int nplanes, void* buffer, bool to_buffer, bool host_buffer = false,
                   bool wait = true);
  float* psi_ptr() { return psi_.get(); }
  size_t volume_floats() const { return plan_->L.real_floats(); }
  // Host stacks of extents `dims` live at offset `off` inside the engine's (larger) volume, the
  // rest of which holds zeros: set_view / stage_view / set_psi embed, get_psi crops (the
  // reference's zero_padd policy, inc/padd_utils.h:121-190, without the host-side staging
  // copies).  dims == engine extents and off == 0 is the dense default.
  // scratch = false: no stack of the call passes through host-shaped device scratch (all of them are in device
  // memory or broadcast), so none is kept.
  void set_embedding(const int dims[3], const int off[3], bool scratch = true);
  // a dense float32 stack in host memory, of the extents of the current embedding window
  StackRef dense(const float* host) const { return StackRef::dense_host(host, host_dims_); }
  // quotient 0 wherever the view is exactly 0 (see EpilogueParams::guard_zero_view)
  void set_quotient_guard(bool on) { quotient_guard_ = on; }
  // Padding policy "reflect" (mvn_reflect.hpp): every stack placed from now on (set_view / stage_view / stream_view /
  // ingest_device_view / set_psi) has the margins around its window filled with its mirror image, on the stream that
  // placed it.  Called after set_embedding.  The copies that place a stack write its window only and rely on margins
  // that still hold zeros: an engine whose image and weights volumes may hold mirrored margins clears them all (ring
  // slots included) when it is switched back.
  void set_reflect(bool on);
  // the PSF form rule on this engine's plan, with the switches read when the engine was built
  FormRule form_rule() const { return FormRule(plan_->L, sw_, plan_->fixed); }
  // will a kernel of these extents be held in the direct dim0 form?
  bool would_be_direct(const int* kdims) const { return form_rule().direct(kdims); }
  // does a volume of this size keep its Nyquist bins packed in the DC column (when every PSF is in the direct form)?
  static bool packed_layout_for(size_t volume_bytes);
  // Halo mode (slabs of one volume): the slabs must all run the same middle - they exchange planes of its input -, so
  // whoever drives them decides for all of them (mvn_multi.cpp): on = the fused middle pass where this slab has it.
  // A hook set without this call keeps the three passes.
  void set_lines_in_halo_mode(bool on) { lines_override_ = on ? 1 : 0; }
  bool lines_in_use() const { return lines_; }
  // a cached engine starts every ABI call from a clean per-call state
  void begin_call() {
    pending_rows_ = nullptr;  // (a deferred pass of a call that failed half-way must never run on the next call's stacks)
    pipelined_ = false;
    quotient_guard_ = false;
    work_has_psi_spectrum_ = false;
    psi_spec_valid_ = false;
  }
  void sync();
  // PSF spectra re-used / prepared since process start (all engines)
  static long psf_cache_hits();
  static long psf_cache_misses();

 private:
  // true when slot spectrum i already belongs to this kernel; otherwise records the kernel
  bool psf_resident(ViewSlot& s, int i, const float* kernel, const int* kdims);
  void conv_pair(int v, const ViewStacks& in, double lambda, float min_value, int final_mode, int accumulate,
                 bool feed_next);
  // one stack into volume `dst` on stream s; `scratch`: where a host stack that needs converting or embedding
  // lands first; dst_dirty: dst has been used as such a scratch since its padding was cleared.  Returns the bytes
  // that crossed PCIe.
  // dst_u16: dst is a uint16 volume and st a uint16 stack, kept unconverted - placed by the copy itself where a
  // float32 stack would be, by the uint16 -> uint16 ingest pass otherwise
  long long ingest_stack(float* dst, const StackRef& st, float* scratch, bool dst_dirty, be::stream_t s,
                         bool dst_u16 = false);
  // the placement itself, of ingest_stack: the reflect fill goes behind it
  long long place_stack(float* dst, const StackRef& st, float* scratch, bool dst_dirty, be::stream_t s, bool dst_u16);
  // the reflect fill of ingest_stack, when the policy is on
  void mirror_margins(float* dst, bool dst_u16, be::stream_t s);
  // a raw view (image.geom) through the resample pass: a raw stack in host memory crosses into a temporary device
  // buffer that is freed once the stream has passed it; weights: the caller's, placed as ever, or (null ptr) computed
  long long resample_pair(float* image_dst, float* weights_dst, const StackRef& image, const StackRef& weights,
                          be::stream_t s);
  std::vector<float*> weights_tab_host_;  // what weights_tab_ was filled from
  be::DeviceBuffer<const float*> fuse_tab_;  // fuse_psi: V image volumes, then V weights volumes
  std::vector<const float*> fuse_tab_host_;
  bool reflect_ = false;           // set_reflect
  bool margins_mirrored_ = false;  // some image / weights volume or ring slot may hold mirrored margins
  // image and weights of one view; without an embedding scratch a uint16 image that is converted lands in the weights
  // volume first
  long long ingest_pair(float* image_dst, float* weights_dst, const StackRef& image, const StackRef& weights,
                        be::stream_t s, bool image_u16);
  std::vector<char> want_u16_;  // per view: its image is (to be) held as uint16
  int image_storage_ = 0;
  size_t image_bytes(bool u16) const { return u16 ? plan_->main_bytes() / 2 : plan_->main_bytes(); }
  void alloc_ring_images(bool u16);
  // the DIVIDE epilogue on the image of `in`: MVN_EPI_DIVIDE, or MVN_EPI_DIVIDE_U16 on a uint16 volume (counted)
  void divide_epilogue(EpilogueParams& e, const ViewStacks& in) const;
  int u16_views() const;
  // Both kernels of slot s on stream st, each unless the slot holds it already (psf_resident): device copy of the
  // kernel, then prepare_psf.  Blocking (set_view): the work volume is the scratch and each copy is freed once the
  // stream has drained.  Staging (stage_view): the staging scratch, and the copies are parked in stage_scratch_.
  void prepare_psfs(ViewSlot& s, const float* kernel1, const int* k1dims, const float* kernel2, const int* k2dims,
                    bool staging, be::stream_t st);
  std::vector<char> pre_ingested_;  // per view: ingest_device_view has taken its stacks
  bool embedded_ = false;
  int host_dims_[3] = {0, 0, 0}, host_off_[3] = {0, 0, 0};
  size_t host_floats() const { return (size_t)host_dims_[0] * host_dims_[1] * host_dims_[2]; }
 public:
  // floats of the embedding scratch this engine holds now (0: none) - what the memory planner prices it by
  size_t scratch_floats() const { return embed_scratch_.get() ? host_floats() : 0; }
 private:
  void alloc_view(ViewSlot& s);
  // PSF spectrum of slot array `spec` from a device-resident kernel: forward transform, then (where
  // the plan wants it) the tile-contiguous re-ordering through `scratch` (one volume)
  void make_spectrum(const float* d_kernel, const int* kdims, float scale, float* spec, cfloat* nyq,
                     float* scratch, be::stream_t s);
  // Kernel i of slot s from its device-resident copy: the direct dim0 form (taps) where the PSF is thin
  // enough along dim0 (FormRule::direct), the 3-D spectrum otherwise; buffers are allocated on first use.
  // `scratch` (one volume, or nullptr = allocate one with the staging scratch) serves the re-tiling of a
  // 3-D spectrum.
  void prepare_psf(ViewSlot& s, int i, const float* d_kernel, const int* kdims, float* scratch, bool staging,
                   be::stream_t st);
  Plan3D* taps_plan(int kd);
  size_t taps_scr_bytes_ = 0;  // of taps_scr_
  // dim1 forward -> dim0 leg (direct or fused FFT) -> dim1 inverse on the work volume, with kernel i of s
  // `produce` (optional): the last-axis pass that produces this convolution's input, as a function of a row range
  // (row0, nrows; nrows < 0 = all): launched by middle() - in one piece, or boundary planes first (halo mode)
  typedef std::function<void(long, long)> RowsProducer;
  void middle(const ViewSlot& s, int i, Profiler* prof, SideStream* side, const RowsProducer* produce = nullptr);
  RowsProducer pending_rows_;  // a fused update + forward pass deferred to the next convolution (boundary-first order)
  void flush_pending_rows();
  bool boundary_first() const;
  // zcount > 0: only the output planes [zbeg, zbeg + zcount); first = false: a further launch of the same leg
  void dim0_conv(const ViewSlot& s, int i, const cfloat* in, const cfloat* in_nyq, cfloat* out, cfloat* out_nyq,
                 Profiler* prof, int zbeg = 0, int zcount = 0, bool first = true);
  void ensure_work2();
  // Nyquist layout of the spectra between the last-axis passes of one call (mvn_dim0_direct.hpp, RowsParams::
  // nyq_packed): packed into the DC column when every kernel of every view is in the direct form, else the
  // separate plane.  Decided when a loop starts; a pipelined ABI call decides from the kernel extents up front.
  bool all_direct() const;
  void decide_layout();
  cfloat* wn() const { return packed_ ? nullptr : work_nyq_; }
  cfloat* pn() const { return packed_ ? nullptr : psi_spec_nyq_.get(); }
  bool packed_ = false, packed_hint_ = false, packed_allowed_ = true;
  bool packed_default_ = true;  // packed_allowed_ as the constructor decided it (a removed halo hook restores it)
  // the loops run their convolutions as last-axis pass -> fused middle pass -> last-axis pass on the line layout
  // (decided per iterate() call / per simultaneous step; halo and slab modes keep the three-pass middle)
  bool lines_ = false, lines_hint_ = false, lines_last_sweep_ = false;
  bool psi_spec_lines_ = false;  // the shared spectrum of psi (simultaneous steps) is in the line layout
  void decide_lines();
  void mid_fused_conv(const ViewSlot& s, int i, Profiler* prof, int zbeg = 0, int zcount = 0);
  int lines_override_ = -1;  // halo mode: -1 = three-pass middle (a hook of unknown kind), 0 / 1 = the slabs' common decision
  halo_fn_t halo_fn_ = nullptr;
  void* halo_user_ = nullptr;
  bool halo_drain_ = true, halo_post_ = false, halo_split_ = false, halo_nyq_aware_ = false;
  int layout_override_ = -1;
  int halo_planes_ = 0;
  bool halo_ranged() const;
  unsigned* poison_ = nullptr;  // the word in use: poison_own_'s first, or caller-owned memory (bind_poison)
  std::vector<unsigned*> poison_peers_;
  // The word a leg of `epoch` reports to (and the last-axis pass that ends its convolution reads), and the table of
  // the peers' words it reports to as well.  With peers (the slabs of one volume, mvn_multi.cpp) the words alternate
  // with the epoch's parity: another slab's NEXT leg may already report while this slab's last-axis pass still has
  // to read the current epoch (boundary-first order: the interior planes of that pass run after the exchange has
  // begun), so it must not overwrite that word; a leg two epochs on follows the peers' next leg, and with it their
  // last-axis pass (HaloGroup::behind_leg).
  unsigned* poison_word(unsigned epoch) const { return poison_peers_.empty() ? poison_ : poison_own_.get() + (epoch & 1u); }
  unsigned* const* poison_table(unsigned epoch) const { return (unsigned* const*)(poison_own_.get() + 16 + 16 * (epoch & 1u)); }
  size_t poison_bytes() const { return (poison_peers_.empty() ? 1 : 2) * sizeof(unsigned); }
  unsigned epoch_ = 0;        // direct dim0 legs enqueued so far = the epoch of the latest
  unsigned armed_epoch_ = 0;  // != 0: the convolution in flight ran a direct leg with this epoch
  // hands the report of the convolution's direct leg (if it had one) to the last-axis pass that ends it
  void arm(EpilogueParams& e);
  FormSwitches sw_;
  int d0_stagger_ = 0;
  bool spec_tiled_ = false;
  float* stage_spec_scratch_ = nullptr;  // owned by stage_scratch_
  void wait_staged(int v);
  // the public constructor delegates to this one, so that ~Engine runs - and drains - when a construction fails half-way
  explicit Engine(int device) : device_(device) {}
  int device_;
  // staging pipeline
  std::vector<int> staged_;  // per view: 0 pending, 1 enqueued on the upload stream, -1 failed
  bool pipelined_ = false;
  std::mutex stage_mu_;
  std::condition_variable stage_cv_;
  // out-of-core views (set_residency): per view its position in the sweep's streamed order, or -1 (resident)
  struct RingSlot {
    be::DeviceBuffer<float> image;
    bool image_u16 = false;  // the image is a uint16 volume (every streamed view of the call is held as uint16)
    be::DeviceBuffer<float> weights;
    be::Event filled;  // upload stream: the pair has landed
    be::Event freed;   // compute stream: the last pass that reads the pair has been enqueued before it
  };
  std::vector<int> stream_pos_;
  std::vector<int> streamed_order_;
  // uploads enqueued / streamed view updates enqueued in this call (under stage_mu_), upload order == use order
  long uploads_ = 0, consumed_ = 0;
  bool stream_abort_ = false;
  bool stream_done_ = false;  // the loop ended early: later uploads of streamed views are skipped
 public:
  // after an early stop (iterate() returned fewer sweeps than asked): releases an uploader thread that
  // would wait for ring slots no later view update frees
  void end_streaming();
 private:
  // the switches of the loop: the options the engine holds, the device state of the running iterate() (a buffer that
  // is held = its switch is on), and what the last one reported
  LoopOptions held_;
  LoopResult last_;
  RecordSet stat_records() const { return loop_.records(LoopState::STAT_REC, plan_->L); }
  RecordSet nm_records() const { return loop_.records(LoopState::NM_REC, plan_->L); }
  bool accel_running() const { return loop_.buf[LoopState::X_PREV].get() != nullptr; }
  float* tv_volume() const { return loop_.at<float>(LoopState::TV); }
  // the records of view v's pass and the window they cover: the stacks inside the padded volume, or all of it
  MvnStatsParams params_for(const RecordSet& r, int v) const;
  int iterate_sweeps(int iterations, double lambda, float min_value);
  void tv_free();
  void accel_extrapolate(int k, float min_value);  // after sweep k (1-based), before sweep k + 1
  void ring_upload(int v, const StackRef& image, const StackRef& weights);  // uploader thread
  ViewStacks ring_acquire();  // main thread, before the view update: the slot its pair has landed in
  void ring_release();        // main thread, after it
  bool work_has_psi_spectrum_ = false;  // work_ holds the last-axis transform of the current psi
  bool psi_spec_valid_ = false;         // psi_spec_ holds the last-axis + dim1 transform of the current psi
  // chunked simultaneous step: the last local view's final pass, parked by compute_delta_head
  EpilogueParams tail_epi_;
  bool tail_pending_ = false;
  int fed_n_ = 0, fed_ = 0;  // apply_delta_chunk(.., feed_next): chunks of the current round fed so far
  Profiler* tail_prof_ = nullptr;
  void chunk_planes(int c, int n, int* z0, int* nz) const;
  bool quotient_guard_ = false;
  long pair_counter_ = 0;
  // one steady-state sweep over all views captured as a graph (small, launch-bound volumes);
  // valid for the parameters it was captured with, buffers never move during an engine's life
  double graph_lambda_ = 0;
  int graph_reg_kind_ = 0;  // the regulariser the sweep was captured with
  double graph_reg_eps_ = 0;
  const float* graph_tv_ = nullptr;  // ... and the factor volume its launches address
  float graph_min_ = 0;
  bool graph_guard_ = false;
  // PSF preparations and layout changes so far / at capture: the graph bakes in the PSF buffers, their form
  // (taps or 3-D spectrum), depth and the Nyquist layout
  unsigned long graph_gen_ = 0, graph_captured_gen_ = 0;
  const float* graph_work_ = nullptr;  // which of the two work volumes was current when the sweep was captured
  // ---- the device state ---------------------------------------------------------------------------------------
  // The members below own what the engine holds on the device, and their ORDER carries the rule of mvn_backend.hpp:
  // buffers, events and the graph first, the streams last - side, upload, then compute -, so that destruction drains
  // and destroys the compute stream, the upload stream and the side stream, in that order, before the first buffer
  // goes.  A plain pointer beside an owner is a ROLE, not an allocation: it is never freed.
  std::shared_ptr<Plan3D> plan_;
  std::map<int, std::unique_ptr<Plan3D>> taps_plans_;  // (kd, d1, d2) plans of the tap arrays, private to the engine
  be::DeviceBuffer<float> psi_;
  // The two work volumes and their Nyquist planes.  The direct dim0 leg is out of place: work_ and work2_ (roles)
  // swap at every such leg; the second pair is allocated at first need (ensure_work2).
  be::DeviceBuffer<float> work_own_[2];
  be::DeviceBuffer<cfloat> work_nyq_own_[2];
  float *work_ = nullptr, *work2_ = nullptr;
  cfloat *work_nyq_ = nullptr, *work2_nyq_ = nullptr;
  // simultaneous mode: psi after the forward last-axis and dim1 passes, shared by all local views; the correction -
  // delta_ is the buffer in use (role): delta_own_, or caller-owned memory (bind_delta)
  be::DeviceBuffer<float> psi_spec_;
  be::DeviceBuffer<cfloat> psi_spec_nyq_;
  be::DeviceBuffer<float> delta_own_;
  float* delta_ = nullptr;
  be::DeviceBuffer<float> embed_scratch_;  // one dense host-shaped stack: H2D lands here, a strided device copy embeds it
  be::DeviceBuffer<float*> weights_tab_;   // device table of the views' weights volumes (normalize_weights)
  // scattered PSF planes the last-axis pass of the fused-pass taps reads (it cannot run in place into the line
  // layout): one buffer per engine, read only by prepare_psf's launches on the stream that prepares
  be::DeviceBuffer<float> taps_scr_;
  be::DeviceBuffer<unsigned> poison_own_;  // 256 bytes: [0] / [1] the engine's own words, bytes 64 / 128: tables of the peers'
  LoopState loop_;
  std::vector<ViewSlot> views_;
  std::vector<RingSlot> ring_;
  std::vector<be::DeviceBuffer<float>> stage_scratch_;
  std::vector<be::Event> staged_ev_;
  be::Event caller_ev_;
  be::GraphExec sweep_graph_;
  Profiler prof_;
  SideStream side_;
  be::Stream upload_stream_;
  be::Stream stream_;
};

// ---------------------------------------------------------------------------------------------
// Slab-decomposed engine: the reference's SEQUENTIAL sweep over views on several GPUs (SURVEY.md
// 8e row 3).  Rank r of P keeps planes [r d0/P, (r+1) d0/P) of psi and of every view and weight
// stack.  Last-axis and dim1 passes are local to a plane; the dim0 pass needs whole lines along
// d0, so each convolution exchanges the half-transformed slab twice:
//     W [d0/P][d1][C]  --pack-->  A [P][d0/P][d1/P][C]  ==all-to-all==>  B [d0][d1/P][C]
//     dim0 FWD * PSF * INV on B (PSF spectra kept in the same transposed layout)
//     B, seen as [P][d0/P][d1/P][C]  ==all-to-all==>  A  --unpack-->  W
// The exchanges themselves are the caller's (torch.distributed / RCCL on buffers it binds);
// everything between them is the single-GPU engine's kernels on two plans, (d0/P, d1, d2) for the
// plane-local passes and (d0, d1/P, d2) for the dim0 pass, so the arithmetic is the sequential
// sweep's, pass for pass.  Requires d0 % P == 0, d1 % P == 0, d0/P >= 2, d1/P >= 2.
// ---------------------------------------------------------------------------------------------
class SlabEngine {
 public:
  SlabEngine(int device, const shape_t& dims, int nranks, int rank, int num_views);
  ~SlabEngine();
  SlabEngine(const SlabEngine&) = delete;
  SlabEngine& operator=(const SlabEngine&) = delete;

  int device() const { return device_; }
  int nranks() const { return P_; }
  int rank() const { return rank_; }
  const Layout& slab_layout() const { return planA_->L; }  // (d0/P, d1, d2)
  size_t main_floats() const { return planA_->L.real_floats(); }    // per exchange buffer
  size_t nyq_floats() const { return 2 * planA_->L.nyq_cplx(); }

  // image / weights: this rank's planes, dense [d0/P][d1][d2]; kernels: whole
  void set_view(int v, const float* image_slab, const float* weights_slab, const float* kernel1,
                const int* k1dims, const float* kernel2, const int* k2dims);
  void set_psi(const float* psi_slab);
  void get_psi(float* psi_slab);
  // exchange buffers (device memory): A is packed / unpacked here, B is what the dim0 pass
  // works on.  nullptr arguments return to engine-owned buffers.
  void bind_buffers(float* a_main, float* b_main, float* a_nyq, float* b_nyq);
  float* a_main() { return a_main_; }
  float* b_main() { return b_main_; }
  float* a_nyq() { return (float*)a_nyq_; }
  float* b_nyq() { return (float*)b_nyq_; }

  // one view update = for conv in {0, 1}: pack, [A -> B all-to-all], mid, [B -> A all-to-all],
  // unpack.  All steps are asynchronous on stream(); sync() before handing a buffer to a
  // collective on another stream.
  void begin_sweeps();  // psi may have been replaced: forget the cached last-axis spectrum
  void step_pack(int v, int conv);
  void step_mid(int v, int conv);
  void step_unpack(int v, int conv, double lambda, float min_value, bool feed_next);
  void sync();
  be::stream_t stream() const { return stream_.get(); }

 private:
  void upload_slab(float* dst, const float* host);
  int device_, P_, rank_;
  shape_t dims_;
  bool work_has_psi_spectrum_ = false;
  struct SlabView {
    be::DeviceBuffer<float> image, weights;
    be::DeviceBuffer<float> spec[2];   // transposed slabs [d0][d1/P][C]
    be::DeviceBuffer<cfloat> nyq[2];   // [d0][d1/P]
    bool set = false;
  };
  // the device state, buffers before the stream (Engine); a_* / b_* are the exchange buffers in use (roles): own_*,
  // or caller-owned memory (bind_buffers)
  std::shared_ptr<Plan3D> planA_, planB_;
  be::DeviceBuffer<float> psi_, work_, own_a_, own_b_;
  be::DeviceBuffer<cfloat> work_nyq_, own_an_, own_bn_;
  float *a_main_ = nullptr, *b_main_ = nullptr;
  cfloat *a_nyq_ = nullptr, *b_nyq_ = nullptr;
  std::vector<SlabView> views_;
  be::Stream stream_;
};

}  // namespace mvn
