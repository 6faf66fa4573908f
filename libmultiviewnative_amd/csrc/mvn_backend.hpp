// mvn_backend.hpp -- the thin device interface the engine is written against.
//
// Product build (libmultiviewnative.so): implemented in mvn_kernels.hip on HIP streams and
// gfx950 kernels.  There is NO CPU implementation in the product.
// Test-only build (libmvn_emu.so, -DMVN_HOST_EMU): implemented in mvn_backend_emu.cpp, where
// "device memory" is host memory and a launch runs the same workgroup bodies one block at a
// time on the CPU.  It exists to validate plans, index math and the RL driver on a box without
// a GPU; it is never linked into, or loaded by, the product library.
#pragma once

#include <cstddef>
#include <utility>

#include "mvn_pass_bodies.hpp"
#include "mvn_dim0_direct.hpp"
#include "mvn_mid_fused.hpp"
#include "mvn_ingest.hpp"
#include "mvn_extrapolate.hpp"
#include "mvn_tv.hpp"
#include "mvn_reflect.hpp"
#include "mvn_resample.hpp"
#include "mvn_fuse.hpp"
#include "mvn_psf.hpp"
#include "mvn_beads.hpp"
#include "mvn_detect.hpp"
#include "mvn_register.hpp"

namespace mvn {
namespace be {

typedef void* stream_t;
typedef void* event_t;

const char* backend_name();

int device_count();
void set_device(int dev);
int get_device();
void device_name(int dev, char* name256);
long long device_total_mem(int dev);
void device_mem_info(size_t* free_b, size_t* total_b);
void device_arch(int dev, int* major, int* minor);

void* dmalloc(size_t bytes);
void dfree(void* p);
void h2d(void* d, const void* h, size_t bytes, stream_t s);
void d2h(void* h, const void* d, size_t bytes, stream_t s);
void d2d(void* dst, const void* src, size_t bytes, stream_t s);
void h2d_2d(void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t height,
            stream_t s);
void d2h_2d(void* h, size_t hpitch, const void* d, size_t dpitch, size_t width, size_t height,
            stream_t s);
void d2d_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
            stream_t s);
void dzero(void* d, size_t bytes, stream_t s);
// several devices in one process (slabs of one volume, mvn_multi.cpp): let kernels and copies running on `dev`
// reach memory of `peer` (once per pair; a no-op for dev == peer), and a device-to-device copy between two
// devices' memories enqueued on a stream of either
void enable_peer_access(int dev, int peer);
// Where the memory behind `p` lives, asked of the runtime's pointer attributes - `p` itself is never read: the
// ordinal of the device that owns it, POINTER_HOST for host memory (pinned, registered or unknown to the runtime),
// POINTER_ANY for memory either side may use (managed memory; every pointer of the host emulation).
enum { POINTER_HOST = -1, POINTER_ANY = -2 };
int pointer_device(const void* p);
void copy_peer(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, stream_t s);

stream_t stream_create();
// a stream of the device's highest priority: it gets hardware queues of its own, so that host->device
// copies never sit behind another engine's kernels in a SHARED hardware queue (ROCm multiplexes a
// process's normal-priority streams onto 4 queues: with two resident engines x (compute, Nyquist,
// upload) streams the upload stream of one aliased the compute stream of the other and block k+1's
// upload ran at 31 instead of 56 GB/s under block k's iterations -- profiles/r03_pipeline.md)
stream_t stream_create_upload();
void stream_destroy(stream_t s);
void stream_sync(stream_t s);

// make every later operation on `s` wait for event `e` (recorded on another stream)
void stream_wait_event(stream_t s, event_t e);
event_t event_create();
// an event that only orders streams (no timestamps: cheaper to record and to wait on)
event_t event_create_sync();
void event_destroy(event_t e);
void event_record(event_t e, stream_t s);
void event_sync(event_t e);
float event_elapsed_ms(event_t a, event_t b);

// stream capture into an executable graph (launch-bound small volumes replay a whole sweep with
// one submission); the host emulation has none
typedef void* graph_exec_t;
bool graphs_supported();
void capture_begin(stream_t s);
graph_exec_t capture_end(stream_t s);  // ends the capture and instantiates the graph
void graph_launch(graph_exec_t g, stream_t s);
void graph_destroy(graph_exec_t g);

// ---- kernel launches --------------------------------------------------------------------
void launch_rows_r2c(const RowsParams& p, bool even, long ntiles, int nthreads, size_t lds_bytes,
                     stream_t s);
void launch_rows_c2r(const RowsParams& p, bool even, long ntiles, int nthreads, size_t lds_bytes,
                     stream_t s);
// even d2 only: c2r + pointwise epilogue + r2c of the result in one pass (reads p.in_cplx /
// p.in_nyq, writes p.out_cplx / p.out_nyq, UPDATE also writes epi.psi); p.fixed selects the
// compile-time specialised kernel
void launch_rows_c2r_r2c(const RowsParams& p, long ntiles, int nthreads, size_t lds_bytes,
                         stream_t s);
// launches that went through the long-line (split-window, 16-column) kernels since process start
// statistics of one sweep: records of `nviews` view updates (view v at rec + 3 v cap) -> out[0..2] = {S, M, P}
void launch_convergence_reduce(const double* rec, const unsigned* counts, int nviews, long cap, double* out,
                               stream_t s);
// noise model: the records of `nviews` divide passes (view v at rec + 3 v cap) -> out[3 v ..] = {D, Y, M} of view v
void launch_nm_reduce(const double* rec, const unsigned* counts, int nviews, long cap, double* out, stream_t s);
long split_launch_count();
// vector extrapolation between sweeps (mvn_extrapolate.hpp): pass A with its records, the reduction of `nrec` records
// into the device word *alpha, pass B
void launch_accel_a(const AccelParams& p, stream_t s);
void launch_accel_reduce(const double* rec, long nrec, float* alpha, stream_t s);
void launch_accel_b(const AccelParams& p, stream_t s);
// the total-variation factor of p.psi into p.t (mvn_tv.hpp; the geometry fields of p are filled in here), and the
// launches of it since process start
void launch_tv(const TvParams& p, stream_t s);
long tv_launch_count();
// launches of the fused middle pass (mvn_mid_fused.hpp) since process start
long mid_fused_launch_count();
// `rider` (plain fixed-length passes only): a second pass of the same mode with tiles of ONE line (T = 1, run-time
// radix body) - the lines of the Nyquist plane, taken by rider->tiles_per_outer further workgroups of the same launch
void launch_strided(int mode, const StridedParams& p, long nblocks, int nthreads,
                    size_t lds_bytes, stream_t s, const StridedParams* rider = nullptr, size_t rider_lds = 0);

// the dim0 leg of a convolution as a direct cyclic convolution with the PSF's few planes
// (mvn_dim0_direct.hpp); p.k must satisfy mvn_dim0_direct_possible(p.k, p.d0)
void launch_dim0_direct(const Dim0DirectParams& p, stream_t s);

// dim1 forward + direct dim0 leg + dim1 inverse in ONE pass over a half-spectrum in the line layout, or (p.mode ==
// MF_TAPS) the forward transform of a PSF's planes into the bin order that pass filters in (mvn_mid_fused.hpp)
void launch_mid_fused(const MidFusedParams& p, stream_t s);

// target[(z-kz/2 mod D0, y-ky/2 mod D1, x-kx/2 mod D2)] = kernel[z][y][x] * scale
// (device-side wrapped_insert_at_point, inc/padd_utils.h:11-40; the reference's GPU twin is
// fftShiftKernel, src/multiviewnative.cu:154-192).  target has row pitch `pitch` floats.
void launch_scatter_psf(const float* kernel, int k0, int k1, int k2, float* target, int D0,
                        int D1, int D2, long pitch, float scale, stream_t s);

// strided 3-D copy of floats, dst[z][y][x] = src[z][y][x] for x < nx, y < ny, z < nz with row /
// plane pitches in floats: embeds a dense stack into a zero-padded volume and crops it back
// (insert_at_offsets / the crop on exit, inc/padd_utils.h:160-190, src/gpu_deconvolve_methods.cuh:
// 537-549, done by the reference on the host)
void launch_copy3d(float* dst, long drow, long dplane, const float* src, long srow, long splane,
                   int nx, int ny, int nz, stream_t s);

// a caller's stack (float32 or uint16, element strides) into the engine volume in one pass that writes every float of
// the volume, and the window of psi back out into a strided float32 destination (mvn_ingest.hpp); the stack is
// DEVICE memory here (host stacks cross PCIe first, Engine::ingest_stack)
// (dst_u16: a uint16 stack into a uint16 volume, unconverted)
void launch_ingest3d(const IngestParams& p, bool u16, stream_t s, bool dst_u16 = false);
void launch_extract3d(const ExtractParams& p, stream_t s);
// the margins around the window of an embedded stack as its mirror image, in place (mvn_reflect.hpp): one launch per
// axis that has a margin, in the order 2, 1, 0 (p.axis is set here); u16: a uint16 volume.  reflect_counters: launches
// and volumes filled since process start
void launch_reflect_fill(const ReflectParams& p, bool u16, stream_t s);
void reflect_counters(long long out[2]);
// a raw view into the image volume and (p.weights) the unnormalised weights volume (mvn_resample.hpp; the raw stack is
// DEVICE memory here, u16: its element type), and the weights of the V volumes behind the device table p.vols over
// their sum.  resample_counters: launches of the one and of the other since process start
void launch_resample(const ResampleParams& p, bool u16, stream_t s);
void launch_weights_normalize(const NormalizeParams& p, stream_t s);
void resample_counters(long long out[2]);
// fusion (mvn_fuse.hpp): the weighted average of the V raw views behind the device table p.views into p.out, and of an
// engine's V image and V weights volumes behind the device table p.vols into the window of p.psi.  fuse_counters:
// launches of the one and of the other since process start
void launch_fuse_resampled(const FuseParams& p, stream_t s);
void launch_fuse_volumes(const FuseVolumesParams& p, stream_t s);
void fuse_counters(long long out[2]);
// a view's kernels from its raw PSF (mvn_psf.hpp): p.count arrays over their sums (both steps), flip and running product
// of all V views, and ALL the correlations of a stage behind the device table p.jobs (the table is read on the host
// for its checks by the caller, mvn_psf_job_check, before it is uploaded).  psf_correlate_launches: launches of the
// last one since process start
void launch_psf_normalize(const PsfNormParams& p, stream_t s);
void launch_psf_pointwise(const PsfPointParams& p, stream_t s);
void launch_psf_correlate(const PsfCorrParams& p, stream_t s);
long long psf_correlate_launches();
// a view's PSF from its beads (mvn_beads.hpp; the raw stack is DEVICE memory here, u16: its element type): the gather
// into p.partial; the sum over the groups and the mean into p.psf (p.flag is cleared by the caller); the minimum taken
// off p.psf (both steps); and the scores of all beads against p.psf (both steps).  beads_counters: launches of the
// gather and of the score pass since process start
void launch_beads_gather(const BeadsParams& p, bool u16, stream_t s);
void launch_beads_reduce(const BeadsParams& p, stream_t s);
void launch_beads_remove_min(const BeadsParams& p, stream_t s);
void launch_beads_score(const BeadsParams& p, bool u16, stream_t s);
void beads_counters(long long out[2]);
// a view's beads from its raw stack (mvn_detect.hpp; the raw stack is DEVICE memory here, u16: its element type): the
// three blur passes - axis 2 from the raw stack into p.a, axis 1 into p.b, axis 0 into D = p.a[0] -; the extremum pass
// over D, which appends to p.list behind p.count (cleared by the caller); and the fit of the p.nfound candidates of
// the sorted list.  detect_counters: launches of the blur passes and of the extremum pass since process start
void launch_detect_blur(const DetectParams& p, bool u16, stream_t s);
void launch_detect_extrema(const DetectParams& p, stream_t s);
void launch_detect_refine(const DetectParams& p, stream_t s);
void detect_counters(long long out[2]);
// two views' beads into the matrix between them (mvn_register.hpp): the neighbours and the descriptors of the set p.pts;
// the match pass over (tiles of A) x (chunks of B) and its fold, one after the other; and the RANSAC pass, which folds
// its best key into *p.best (cleared by the caller).  register_counters: launches of the match pass and of the RANSAC
// pass since process start
void launch_register_neighbours(const RegParams& p, stream_t s);
void launch_register_match(const RegParams& p, stream_t s);
void launch_register_ransac(const RegParams& p, stream_t s);
void register_counters(long long out[2]);

// stand-alone pointwise ops on flat arrays (legacy ABI: compute_quotient / compute_final_values)
void launch_divide(const float* view, float* inout, size_t n, stream_t s);
void launch_update(float* psi, const float* integral, const float* weights, size_t n,
                   double lambda, float min_value, stream_t s);
// psi += delta  (applies the all-reduced correction in simultaneous mode)
// legacy iterate_fft_tikhonov final step (inc/cuda_kernels.cuh:162-193)
void launch_update_legacy_tikhonov(float* image, const float* integral, const float* weights,
                                   size_t n, float lambda_f, float min_value, stream_t s);
void launch_axpy1(float* psi, const float* delta, size_t n, stream_t s);

// ---- owning handles -----------------------------------------------------------------------
// A device buffer, a stream, an event and an instantiated graph that release themselves: move-only, written on the
// functions above alone, so the product and the emulation share them.  ONE rule of order: buffers are declared BEFORE
// their stream.  Locals and members are destroyed in reverse order, so every way out of the function, and an engine's
// destruction, drains the stream, destroys it and only then frees the buffers the stream's work used.  Work on the null stream needs buffer owners
// alone (freeing device memory synchronises); a buffer whose work runs on a stream somebody else owns is drained by
// hand (drain_quietly) before it goes out of scope on an error path.

// wait for `s` on a path that must not throw (destructors, error paths): a failure here has been or will be reported
// by the call that caused it
inline void drain_quietly(stream_t s) {
  try {
    stream_sync(s);
  } catch (...) {
  }
}

template <typename T = void>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t bytes) : p_(static_cast<T*>(dmalloc(bytes))) {}
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.release()) {}
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    reset(o.release());
    return *this;
  }
  ~DeviceBuffer() { dfree(p_); }
  T* get() const { return p_; }
  T* release() { return std::exchange(p_, nullptr); }
  void reset(T* p = nullptr) {
    dfree(p_);
    p_ = p;
  }

 private:
  T* p_ = nullptr;
};

class Stream {
 public:
  Stream() = default;  // empty: holds no stream (not the null stream)
  static Stream create() { return Stream(stream_create()); }
  static Stream create_upload() { return Stream(stream_create_upload()); }
  Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept {
    reset(std::exchange(o.s_, nullptr));
    return *this;
  }
  ~Stream() { reset(); }
  stream_t get() const { return s_; }
  void reset(stream_t s = nullptr) {
    if (s_) {
      drain_quietly(s_);
      stream_destroy(s_);
    }
    s_ = s;
  }

 private:
  explicit Stream(stream_t s) : s_(s) {}
  stream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  static Event timing() { return Event(event_create()); }
  static Event sync_only() { return Event(event_create_sync()); }
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    reset(std::exchange(o.e_, nullptr));
    return *this;
  }
  ~Event() { reset(); }
  event_t get() const { return e_; }
  void reset(event_t e = nullptr) {
    if (e_) event_destroy(e_);
    e_ = e;
  }

 private:
  explicit Event(event_t e) : e_(e) {}
  event_t e_ = nullptr;
};

// an instantiated graph (capture_end): whoever invalidates it resets it
class GraphExec {
 public:
  GraphExec() = default;
  explicit GraphExec(graph_exec_t g) : g_(g) {}
  GraphExec(GraphExec&& o) noexcept : g_(std::exchange(o.g_, nullptr)) {}
  GraphExec& operator=(GraphExec&& o) noexcept {
    reset(std::exchange(o.g_, nullptr));
    return *this;
  }
  ~GraphExec() { reset(); }
  graph_exec_t get() const { return g_; }
  void reset(graph_exec_t g = nullptr) {
    if (g_) graph_destroy(g_);
    g_ = g;
  }

 private:
  graph_exec_t g_ = nullptr;
};

}  // namespace be
}  // namespace mvn
