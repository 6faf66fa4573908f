// mvn_kernels.hip -- the product's device backend: gfx950 kernels + HIP runtime plumbing.
//
// Kernels (all HBM-bandwidth bound; no MFMA -- this path has no dense contraction):
//   k_rows_r2c / k_rows_c2r   last-axis real<->half-complex passes, LDS-staged, with the RL
//                             pointwise math fused into the c2r epilogue
//                             (replaces cufftExecR2C/C2R inc/cufft_utils.cuh:54-55,72-73 and
//                             device_divide / device_(regularized_)final_values,
//                             inc/cuda_kernels.cuh:14-112)
//   k_strided<MODE>           c2c passes along dim1 / dim0 on tiles of neighbouring columns;
//                             MODE FWD_MUL_INV fuses forward dim0, the PSF-spectrum multiply
//                             (multiply_scaled, inc/cuda_kernels.cuh:213-242) and inverse dim0
//   kx_rows_* / kx_strided    the same passes with every length, radix and tile shape a
//                             template constant (mvn_fixed.hpp); kx_rows_c2r_r2c additionally
//                             fuses c2r + pointwise step + r2c of the next convolution; the
//                             strided ones walk over several tiles per workgroup
//   k_scatter_psf             device-side wrapped insert (fftShiftKernel,
//                             src/multiviewnative.cu:154-192)
//   k_divide / k_update / k_update_legacy_tikhonov / k_axpy1   stand-alone pointwise ops for the
//                                   legacy entry points
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <stdexcept>
#include <string>

#include "mvn_backend.hpp"
#include "mvn_fixed_geom.hpp"
#include "mvn_wave_rows.hpp"

#define HIP_CHECK(expr)                                                                      \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      throw std::runtime_error(std::string("HIP error '") + hipGetErrorString(_e) + "' at " + \
                               __FILE__ + ":" + std::to_string(__LINE__) + " (" #expr ")");  \
  } while (0)

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
template <bool EVEN, int T>
__global__ void __launch_bounds__(512) k_rows_r2c(const RowsParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  if (EVEN)
    rows_r2c_even_body<T>(p, (long)blockIdx.x, (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
  else
    rows_r2c_odd_body<T>(p, (long)blockIdx.x, (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
}

// FORM: the form of the launch's mode in the run-time-radix bodies (mvn_epi_generic_form)
template <bool EVEN, int T, int FORM>
__global__ void __launch_bounds__(512) k_rows_c2r(const RowsParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  if (EVEN)
    rows_c2r_even_body<T, false, FORM>(p, (long)blockIdx.x, (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
  else
    rows_c2r_odd_body<T, FORM>(p, (long)blockIdx.x, (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
}
// run-time-radix form of the fused c2r + pointwise + r2c pass (any even d2)
template <int T, int FORM>
__global__ void __launch_bounds__(512) k_rows_c2r_r2c(const RowsParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  rows_c2r_even_body<T, true, FORM>(p, (long)blockIdx.x, (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
}

// once per sweep with the noise model on: workgroup v sums the records of view v's divide pass -> out + 3 v = {D, Y, M}
__global__ void __launch_bounds__(256) k_nm_reduce(const double* rec, const unsigned* counts, long cap, double* out) {
  __shared__ double lds[3 * 256];
  const long v = (long)blockIdx.x;
  mvn_nm_reduce_body(rec + 3 * v * cap, counts + v, cap, out + 3 * v, lds, (int)threadIdx.x, (int)blockDim.x);
}

// once per sweep with statistics on: the records of the sweep's view updates -> {S, M, P} (mvn_pass_bodies.hpp)
__global__ void __launch_bounds__(256) k_convergence_reduce(const double* rec, const unsigned* counts, int nviews,
                                                            long cap, double* out) {
  __shared__ double lds[3 * 256];
  mvn_convergence_reduce_body(rec, counts, nviews, cap, out, lds, (int)threadIdx.x, (int)blockDim.x);
}

// NYQ only tags the launches that work on the Nyquist plane, so that profilers list them apart
template <int MODE, int T, bool NYQ>
__global__ void __launch_bounds__(512) k_strided(const StridedParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  strided_body<MODE, T, NYQ>(p, (long)blockIdx.x, (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
}

// ---- compile-time specialised kernels for power-of-two lengths (mvn_fixed.hpp) ----------------
// (LINES: the half-spectrum side in the line layout of the fused middle pass, mvn_fixed.hpp fx_lines_base)
template <int H, bool LINES = false>
__global__ void __launch_bounds__(FxRowsCfg<H>::NT) kx_rows_r2c(const RowsParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  FxCtx<FxRowsRegsFor<H, MVN_EPI_STORE>, FxRowsCfg<H>::NT> ctx;
  ctx.tid = (int)threadIdx.x;
  fx_rows_workgroup<H, MVN_PASS_R2C, MVN_EPI_STORE, LINES>(p, (long)blockIdx.x, (long)gridDim.x, (cfloat*)mvn_smem, ctx);
}

template <int H, int EPI, bool LINES = false>
__global__ void __launch_bounds__(FxRowsCfg<H>::NT) kx_rows_c2r(const RowsParams p0) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  RowsParams p = p0;
  mvn_arm_poison(p.epi);
  FxCtx<FxRowsRegsFor<H, EPI>, FxRowsCfg<H>::NT> ctx;
  ctx.tid = (int)threadIdx.x;
  fx_rows_workgroup<H, MVN_PASS_C2R, EPI, LINES>(p, (long)blockIdx.x, (long)gridDim.x, (cfloat*)mvn_smem, ctx);
}

// (The divide form needs 93 VGPRs, just above the 84 that would let three 512-thread workgroups
// share a CU; forcing it there with a waves-per-SIMD bound spilled 56 bytes and gained nothing.)
template <int H, int EPI, bool LINES = false>
__global__ void __launch_bounds__(FxRowsCfg<H>::NT) kx_rows_c2r_r2c(const RowsParams p0) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  RowsParams p = p0;
  mvn_arm_poison(p.epi);
  FxCtx<FxRowsRegsFor<H, EPI>, FxRowsCfg<H>::NT> ctx;
  ctx.tid = (int)threadIdx.x;
  fx_rows_workgroup<H, MVN_PASS_C2R_R2C, EPI, LINES>(p, (long)blockIdx.x, (long)gridDim.x, (cfloat*)mvn_smem, ctx);
}

// the fused middle pass (mvn_mid_fused.hpp): one column (piece) per workgroup
template <int K>
__global__ void __launch_bounds__(MF_NT) kf_mid(const MidFusedParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  FxCtx<MfRegs<K>, MF_NT> ctx;
  ctx.tid = (int)threadIdx.x;
  mf_body<K>(p, (long)blockIdx.x, (cfloat*)mvn_smem, ctx);
}
__global__ void __launch_bounds__(MF_NT) kf_mid_taps(const MidFusedParams p) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  FxCtx<MfRegs<1>, MF_NT> ctx;
  ctx.tid = (int)threadIdx.x;
  mf_taps_body(p, (long)blockIdx.x, (cfloat*)mvn_smem, ctx);
}

// last-axis passes for d2 = 512 in which a row never leaves its half-wave (mvn_wave_rows.hpp): no
// workgroup barrier inside the loop over rows, 4 LDS exchanges per fused pass
template <int MODE, int EPI>
__global__ void __launch_bounds__(WrCfg::NT, 4) kw_rows(const RowsParams p0) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  RowsParams p = p0;
  if (MODE != MVN_WR_R2C) mvn_arm_poison(p.epi);
  FxCtx<WrRegs, WrCfg::NT> ctx;
  ctx.tid = (int)threadIdx.x;
  wr_rows_body<MODE, EPI>(p, (long)blockIdx.x, (long)gridDim.x, (cfloat*)mvn_smem, ctx);
}

// `main_grid` walking workgroups work on the main array; the workgroups behind them (plain dim1 passes only) take
// ONE line of the Nyquist plane each - 4 KB at 512 points, through the run-time-radix body - so that the plane
// needs no launch, stream and fork / join pair of its own: 512 two-microsecond workgroups that fill the slots
// the walkers leave at the end of the launch, instead of 32 workgroups of 16 lines that queued for a slot beside
// the next full-volume pass on a second hardware queue (round 3: 25 % of all GPU-busy time for 0.4 % of the bytes).
template <int N, int MODE>
__global__ void __launch_bounds__((FxStridedSel<N, MODE>::NT), (FxStridedSel<N, MODE>::WAVES))
    kx_strided(const StridedParams p, const StridedParams rider, unsigned main_grid) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  if constexpr (MODE != MVN_ST_FWD_MUL_INV) {
    if (blockIdx.x >= main_grid) {
      strided_body<MODE, 1, true>(rider, (long)(blockIdx.x - main_grid), (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
      return;
    }
  }
  typename FxStridedSel<N, MODE>::Ctx ctx;
  ctx.tid = (int)threadIdx.x;
  FxStridedSel<N, MODE>::run(p, (long)blockIdx.x, p.nblocks, (long)main_grid, (cfloat*)mvn_smem, ctx);
}

template <int N, int MODE>
__global__ void __launch_bounds__((FxSplitCfg<N>::NT)) kx_strided_split(const StridedParams p, const StridedParams rider,
                                                                       unsigned main_grid) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  if (blockIdx.x >= main_grid) {
    strided_body<MODE, 1, true>(rider, (long)(blockIdx.x - main_grid), (int)threadIdx.x, (int)blockDim.x, (cfloat*)mvn_smem);
    return;
  }
  FxCtx<FxSplitRegs<N>, FxSplitCfg<N>::NT> ctx;
  ctx.tid = (int)threadIdx.x;
  fx_strided_split_body<N, MODE>(p, (long)blockIdx.x, p.nblocks, (long)main_grid, (cfloat*)mvn_smem, ctx);
}

// direct dim0 convolution (mvn_dim0_direct.hpp): one bin per work item, all of dim0
// (K = 25 sits a register or two above the 128 that let four waves share a SIMD: bounded there)
template <int K, int PF = MVN_D0_PF>
__global__ void __launch_bounds__(MVN_D0_WG, (K == 25 ? 4 : 1)) kd_dim0(const Dim0DirectParams p, unsigned main_blocks) {
  extern __shared__ __attribute__((aligned(16))) char mvn_smem[];
  if (blockIdx.x >= main_blocks) {  // packed Nyquist: one (k1, -k1) pair of the DC column per workgroup
    const int pair = (int)(blockIdx.x - main_blocks);
    mvn_dim0_dc_load(p, pair, (cfloat*)mvn_smem, (int)threadIdx.x, MVN_D0_WG);
    __syncthreads();
    mvn_dim0_dc_compute(p, pair, (const cfloat*)mvn_smem, (int)threadIdx.x, MVN_D0_WG);
    return;
  }
  Dim0DirectParams q;
  long b;
  int zs, nout;
  // (zs, nout and the arrays in q depend on the workgroup only: scalar registers)
  if (mvn_dim0_job(p, (long)blockIdx.x, (int)threadIdx.x, q, b, zs, nout))
    mvn_dim0_direct_column<K, PF>(q, b, zs, nout);
}

__global__ void k_scatter_psf(const float* kernel, int k0, int k1, int k2, float* target, int D0,
                              int D1, int D2, long pitch, float scale) {
  const long total = (long)k0 * k1 * k2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    mvn_scatter_psf_item(kernel, k0, k1, k2, target, D0, D1, D2, pitch, scale, i);
}

// one workgroup row per (y, z): x runs over lanes, so both sides are read / written in contiguous
// runs whatever the offsets are
__global__ void k_copy3d(float* __restrict__ dst, long drow, long dplane, const float* __restrict__ src,
                         long srow, long splane, int nx, int ny, int nz) {
  const long rows = (long)ny * nz;
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const long z = r / ny, y = r - z * ny;
    const float* s = src + z * splane + y * srow;
    float* d = dst + z * dplane + y * drow;
    for (int x = threadIdx.x; x < nx; x += blockDim.x) d[x] = s[x];
  }
}

// a caller's stack into the engine volume / psi's window back out (mvn_ingest.hpp): pure streaming, a handful of
// registers, 4 waves per workgroup so that 8 workgroups fill a CU's wave slots
template <typename T>
__global__ __launch_bounds__(MVN_INGEST_WG) void k_ingest3d(const IngestParams p) {
  mvn_ingest_rows<T>(p, (long)blockIdx.x, (int)threadIdx.x);
}
// a uint16 stack into a uint16 volume, unconverted (image storage mode 1)
__global__ __launch_bounds__(MVN_INGEST_WG) void k_ingest3d_u16(const IngestParams p) {
  mvn_ingest_rows<uint16_t, uint16_t>(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_INGEST_WG) void k_extract3d(const ExtractParams p) {
  mvn_extract_rows(p, (long)blockIdx.x, (int)threadIdx.x);
}

// the margins of an embedded stack as its mirror image, one axis per launch (mvn_reflect.hpp)
template <typename T>
__global__ __launch_bounds__(MVN_INGEST_WG) void k_reflect3d(const ReflectParams p) {
  mvn_reflect_rows<T>(p, (long)blockIdx.x, (int)threadIdx.x);
}

// a raw view through its affine transform into the image and the unnormalised weights volume, and the weights of all
// views over their sum (mvn_resample.hpp)
template <typename T>
__global__ __launch_bounds__(MVN_RS_WG) void k_resample3d(const ResampleParams p) {
  mvn_resample_tile<T>(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_INGEST_WG) void k_weights_normalize(const NormalizeParams p) {
  mvn_normalize_rows(p, (long)blockIdx.x, (int)threadIdx.x);
}

// fusion (mvn_fuse.hpp): the weighted average of the views, from their raw stacks and from an engine's volumes
__global__ __launch_bounds__(MVN_RS_WG) void k_fuse_resampled(const FuseParams p) {
  mvn_fuse_tile(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_INGEST_WG) void k_fuse_volumes(const FuseVolumesParams p) {
  mvn_fuse_rows(p, (long)blockIdx.x, (int)threadIdx.x);
}

// a view's kernels from its raw PSF (mvn_psf.hpp): normalisation in two steps, flip and running product, and the
// correlations of a stage, all of its jobs in one launch
__global__ __launch_bounds__(MVN_PSF_WG) void k_psf_sum(const PsfNormParams p) {
  mvn_psf_sum_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_PSF_WG) void k_psf_scale(const PsfNormParams p) {
  mvn_psf_scale_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_PSF_WG) void k_psf_pointwise(const PsfPointParams p) {
  mvn_psf_pointwise_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_PSF_WG) void k_psf_correlate(const PsfCorrParams p) {
  mvn_psf_correlate_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

// a view's PSF from its beads (mvn_beads.hpp): the gather, the sum over the groups, the minimum in two steps, and the
// scores in two steps
template <typename T>
__global__ __launch_bounds__(MVN_BEADS_WG) void k_beads_gather(const BeadsParams p) {
  mvn_beads_gather_item<T>(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_BEADS_WG) void k_beads_reduce(const BeadsParams p) {
  mvn_beads_reduce_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_BEADS_WG) void k_beads_min(const BeadsParams p) {
  mvn_beads_min_item(p, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_BEADS_WG) void k_beads_sub(const BeadsParams p) {
  mvn_beads_sub_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

template <typename T>
__global__ __launch_bounds__(MVN_BEADS_WG) void k_beads_score(const BeadsParams p) {
  mvn_beads_score_item<T>(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_BEADS_WG) void k_beads_score_fold(const BeadsParams p) {
  mvn_beads_score_fold_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

// a view's beads from its raw stack (mvn_detect.hpp): the blur along axis 2 from the raw stack, along axis 1 and axis 0
// (which writes D), the extrema of D, and the fit of the sorted candidates
template <typename T>
__global__ __launch_bounds__(MVN_DETECT_WG) void k_detect_rows(const DetectParams p) {
  __shared__ float lds[MVN_DETECT_ROWS_LDS];
  mvn_detect_rows_body<T>(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_DETECT_WG);
}

template <int AXIS>
__global__ __launch_bounds__(MVN_DETECT_WG) void k_detect_lines(const DetectParams p) {
  __shared__ float lds[MVN_DETECT_LINES_LDS];
  mvn_detect_lines_body<AXIS, 1>(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_DETECT_WG);
}

__global__ __launch_bounds__(MVN_DETECT_WG) void k_detect_extrema(const DetectParams p) {
  __shared__ float lds[MVN_DETECT_EXTREMA_LDS];
  mvn_detect_extrema_body(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_DETECT_WG);
}

__global__ __launch_bounds__(MVN_DETECT_WG) void k_detect_refine(const DetectParams p) {
  mvn_detect_refine_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

// two views' beads into the matrix between them (mvn_register.hpp): brute-force scans, the scanned set broadcast from
// the LDS
__global__ __launch_bounds__(MVN_REG_WG) void k_reg_neighbours(const RegParams p) {
  __shared__ double lds[3 * MVN_REG_NTILE];
  mvn_reg_neighbours_body<1>(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_REG_WG);
}

__global__ __launch_bounds__(MVN_REG_WG) void k_reg_match(const RegParams p) {
  __shared__ float lds[MVN_REG_MTILE * MVN_REG_DESC];
  mvn_reg_match_body<1>(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_REG_WG);
}

__global__ __launch_bounds__(MVN_REG_WG) void k_reg_match_fold(const RegParams p) {
  mvn_reg_fold_item(p, (long)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(MVN_REG_WG) void k_reg_ransac(const RegParams p) {
  __shared__ double lds[6 * MVN_REG_RTILE];
  __shared__ unsigned long long keys[MVN_REG_WG];
  mvn_reg_ransac_body<1>(p, (long)blockIdx.x, lds, keys, (int)threadIdx.x, MVN_REG_WG);
}

// vector extrapolation between sweeps (mvn_extrapolate.hpp): two streaming passes and the reduction between them
template <int W>
__global__ __launch_bounds__(MVN_ACCEL_WG) void k_accel_a(const AccelParams p) {
  __shared__ double lds[2 * MVN_ACCEL_WG];
  mvn_accel_a_body<W>(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_ACCEL_WG);
}

__global__ __launch_bounds__(MVN_ACCEL_WG) void k_accel_reduce(const double* rec, long nrec, float* alpha) {
  __shared__ double lds[2 * MVN_ACCEL_WG];
  mvn_accel_reduce_body(rec, nrec, alpha, lds, (int)threadIdx.x, MVN_ACCEL_WG);
}

template <int W>
__global__ __launch_bounds__(MVN_ACCEL_WG) void k_accel_b(const AccelParams p) {
  mvn_accel_b_body<W>(p, (long)blockIdx.x, (int)threadIdx.x, MVN_ACCEL_WG);
}

// the total-variation factor of psi (mvn_tv.hpp): a tile of a plane per workgroup, walked along dim0
__global__ __launch_bounds__(MVN_TV_WG) void k_tv_factor(const TvParams p) {
  __shared__ float lds[MVN_TV_LDS_FLOATS];
  mvn_tv_body<1>(p, (long)blockIdx.x, lds, (int)threadIdx.x, MVN_TV_WG);
}

__global__ void k_divide(const float* __restrict__ view, float* __restrict__ inout, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    inout[i] = mvn_quotient(view[i], inout[i]);
}

__global__ void k_update(float* __restrict__ psi, const float* __restrict__ integral,
                         const float* __restrict__ weights, size_t n, double lambda,
                         float lambda_inv, float min_value) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    MVN_FP_EXACT
    const float last = psi[i];
    const float next = mvn_next_value(last, integral[i], lambda, lambda_inv, min_value);
    psi[i] = weights[i] * (next - last) + last;
  }
}

__global__ void k_update_legacy_tikhonov(float* __restrict__ image,
                                        const float* __restrict__ integral,
                                        const float* __restrict__ weights, size_t n,
                                        float lambda_f, float min_value) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    image[i] = mvn_legacy_tikhonov_value(image[i], integral[i], weights[i], lambda_f, min_value);
}

__global__ void k_axpy1(float* __restrict__ psi, const float* __restrict__ delta, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    psi[i] += delta[i];
}

// ---------------------------------------------------------------------------------------------
// runtime plumbing
// ---------------------------------------------------------------------------------------------
namespace mvn {
namespace be {

const char* backend_name() { return "hip-gfx950"; }

int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

void set_device(int dev) { HIP_CHECK(hipSetDevice(dev)); }

int get_device() {
  int d = 0;
  HIP_CHECK(hipGetDevice(&d));
  return d;
}

void device_name(int dev, char* name256) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  std::memset(name256, 0, 256);
  std::strncpy(name256, prop.name, 255);
  // some ROCm builds leave the marketing name empty: fall back to the gfx target
  if (!name256[0]) std::snprintf(name256, 256, "AMD GPU %s", prop.gcnArchName);
}

long long device_total_mem(int dev) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  return (long long)prop.totalGlobalMem;
}

void device_mem_info(size_t* free_b, size_t* total_b) { HIP_CHECK(hipMemGetInfo(free_b, total_b)); }

// "compute capability" of a gfx target: gfx950 -> (95, 0); gfx90a -> (90, 10)
void device_arch(int dev, int* major, int* minor) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  const char* a = prop.gcnArchName;
  *major = 0;
  *minor = 0;
  if (std::strncmp(a, "gfx", 3) != 0) return;
  a += 3;
  size_t len = 0;
  while (a[len] && a[len] != ':') ++len;
  if (len == 0) return;
  for (size_t i = 0; i + 1 < len; ++i)
    if (a[i] >= '0' && a[i] <= '9') *major = *major * 10 + (a[i] - '0');
  const char c = a[len - 1];
  *minor = (c >= '0' && c <= '9') ? c - '0' : ((c >= 'a' && c <= 'f') ? 10 + c - 'a' : 0);
}

void* dmalloc(size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1));
  return p;
}

void dfree(void* p) {
  if (p) (void)hipFree(p);
}

static hipStream_t hs(stream_t s) { return (hipStream_t)s; }

void h2d(void* d, const void* h, size_t bytes, stream_t s) {
  HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, hs(s)));
}
void d2h(void* h, const void* d, size_t bytes, stream_t s) {
  HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, hs(s)));
}
void d2d(void* dst, const void* src, size_t bytes, stream_t s) {
  HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, hs(s)));
}
void h2d_2d(void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t height,
            stream_t s) {
  if (dpitch == width && hpitch == width) return h2d(d, h, width * height, s);
  HIP_CHECK(hipMemcpy2DAsync(d, dpitch, h, hpitch, width, height, hipMemcpyHostToDevice, hs(s)));
}
void d2h_2d(void* h, size_t hpitch, const void* d, size_t dpitch, size_t width, size_t height,
            stream_t s) {
  if (dpitch == width && hpitch == width) return d2h(h, d, width * height, s);
  HIP_CHECK(hipMemcpy2DAsync(h, hpitch, d, dpitch, width, height, hipMemcpyDeviceToHost, hs(s)));
}
void d2d_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
            stream_t s) {
  if (dpitch == width && spitch == width) return d2d(dst, src, width * height, s);
  HIP_CHECK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, hs(s)));
}
void dzero(void* d, size_t bytes, stream_t s) { HIP_CHECK(hipMemsetAsync(d, 0, bytes, hs(s))); }

void enable_peer_access(int dev, int peer) {
  if (dev == peer) return;
  int can = 0;
  HIP_CHECK(hipDeviceCanAccessPeer(&can, dev, peer));
  if (!can) throw std::runtime_error("mvn: device " + std::to_string(dev) + " cannot access device " + std::to_string(peer));
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  HIP_CHECK(hipSetDevice(dev));
  const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
  (void)hipSetDevice(cur);
  if (e == hipErrorPeerAccessAlreadyEnabled) {
    (void)hipGetLastError();
    return;
  }
  HIP_CHECK(e);
}
void copy_peer(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, stream_t s) {
  if (dst_dev == src_dev)
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, hs(s)));
  else
    HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, hs(s)));
}

int pointer_device(const void* p) {
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {  // (memory the runtime has never seen: plain host memory)
    (void)hipGetLastError();
    return POINTER_HOST;
  }
  switch (attr.type) {
    case hipMemoryTypeDevice: return attr.device;
    case hipMemoryTypeManaged: return POINTER_ANY;
    default: return POINTER_HOST;
  }
}

stream_t stream_create() {
  hipStream_t s;
  HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return (stream_t)s;
}
stream_t stream_create_upload() {
  int least = 0, greatest = 0;
  HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  hipStream_t s;
  HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest));
  return (stream_t)s;
}
void stream_destroy(stream_t s) {
  if (s) (void)hipStreamDestroy(hs(s));
}
void stream_sync(stream_t s) { HIP_CHECK(hipStreamSynchronize(hs(s))); }

void stream_wait_event(stream_t s, event_t e) {
  HIP_CHECK(hipStreamWaitEvent(hs(s), (hipEvent_t)e, 0));
}

event_t event_create() {
  hipEvent_t e;
  HIP_CHECK(hipEventCreate(&e));
  return (event_t)e;
}
event_t event_create_sync() {
  hipEvent_t e;
  HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return (event_t)e;
}
void event_destroy(event_t e) {
  if (e) (void)hipEventDestroy((hipEvent_t)e);
}
void event_record(event_t e, stream_t s) { HIP_CHECK(hipEventRecord((hipEvent_t)e, hs(s))); }
void event_sync(event_t e) { HIP_CHECK(hipEventSynchronize((hipEvent_t)e)); }
float event_elapsed_ms(event_t a, event_t b) {
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b));
  return ms;
}

bool graphs_supported() { return true; }
void capture_begin(stream_t s) {
  // thread-local mode: the staging thread of the ABI call may allocate / free meanwhile
  HIP_CHECK(hipStreamBeginCapture(hs(s), hipStreamCaptureModeThreadLocal));
}
graph_exec_t capture_end(stream_t s) {
  hipGraph_t g = nullptr;
  HIP_CHECK(hipStreamEndCapture(hs(s), &g));
  hipGraphExec_t e = nullptr;
  hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  HIP_CHECK(err);
  return (graph_exec_t)e;
}
void graph_launch(graph_exec_t g, stream_t s) { HIP_CHECK(hipGraphLaunch((hipGraphExec_t)g, hs(s))); }
void graph_destroy(graph_exec_t g) {
  if (g) (void)hipGraphExecDestroy((hipGraphExec_t)g);
}

// a workgroup may ask for up to the CU's whole 160 KiB of LDS; above the 64 KiB default the
// kernel needs the attribute raised once
template <typename K>
static void ensure_lds(K kernel, size_t lds_bytes) {
  if (lds_bytes <= 64 * 1024) return;
  // once per (kernel, size): the attribute call costs a few microseconds per launch otherwise
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> done;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const void* fn = reinterpret_cast<const void*>(kernel);
  const auto key = std::make_pair(fn, dev);
  std::lock_guard<std::mutex> lk(mu);
  auto it = done.find(key);
  if (it != done.end() && it->second >= lds_bytes) return;
  HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  done[key] = lds_bytes;
}

static void check_launch(long nblocks, int nthreads, size_t lds_bytes) {
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  if (nthreads < 64 || nthreads > 1024 || nthreads % 64) throw std::invalid_argument("mvn: bad block size");
  if (lds_bytes > 160 * 1024) throw std::invalid_argument("mvn: LDS request exceeds 160 KiB");
}

template <typename K, typename P>
static void launch_pass(K kernel, const P& p, long nblocks, int nthreads, size_t lds_bytes, stream_t s) {
  ensure_lds(kernel, lds_bytes);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(nthreads), lds_bytes, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

// fixed last-axis kernels: one workgroup per tile, or (long rows, FxRowsCfg<H>::WALK) as many
// workgroups as the device holds at once, each walking over the tiles of the launch
template <bool WALK, typename K>
static void launch_rows_fixed(K kernel, const RowsParams& p, long nblocks, int nthreads, size_t lds_bytes,
                              stream_t s);

// Fixed strided kernels walk over several tiles per workgroup (the next tile's loads overlap the
// current tile's LDS stages): the grid is what the device holds at once, not one block per tile.
// The LDS-staged fused pass is launched one workgroup per tile: measured at 512^3, 0.333 ms against
// 0.380 ms walking (the walking workgroups of a CU stay in step, all loading or all computing at once).
static int current_device() {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  return dev;
}

// CUs of the current device (asked once per device)
static int device_cu_count() {
  static std::mutex mu;
  static std::map<int, int> cache;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
  cache[dev] = cus;
  return cus;
}

// resident workgroups per CU of a (device, kernel, block size, LDS) tuple: asked once, not per launch
static int resident_per_cu(const void* kernel, int nthreads, size_t lds_bytes) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, int, size_t>, int> cache;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(dev, kernel, nthreads, lds_bytes);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, nthreads, lds_bytes));
  if (per_cu < 1) per_cu = 1;
  cache[key] = per_cu;
  return per_cu;
}

template <typename K>
static void launch_walking(K kernel, StridedParams p, long nblocks, int nthreads, size_t lds_bytes,
                           stream_t s, bool walk, const StridedParams* rider = nullptr, size_t rider_lds = 0) {
  if (rider && rider_lds > lds_bytes) lds_bytes = rider_lds;
  ensure_lds(kernel, lds_bytes);
  long grid = nblocks;
  if (walk) {
    const long resident = (long)resident_per_cu(reinterpret_cast<const void*>(kernel), nthreads, lds_bytes) *
                          device_cu_count();
    if (grid > resident) grid = resident;
  }
  p.nblocks = nblocks;
  const long lines = rider ? rider->tiles_per_outer : 0;  // one line of the Nyquist plane per workgroup
  if (grid + lines > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  hipLaunchKernelGGL(kernel, dim3((unsigned)(grid + lines)), dim3(nthreads), lds_bytes, hs(s), p, rider ? *rider : p,
                     (unsigned)grid);
  HIP_CHECK(hipGetLastError());
}

// wave-row kernels (d2 = 512): workgroups sweep over the row pairs, the grid is what the device
// holds at once.  MVN_WAVE_ROWS_MASK selects the passes that use them (1 plain r2c, 2 plain c2r,
// 4 fused divide, 8 fused update / store, 16 c2r with the DELTA epilogue of the sharded step);
// default 28 (round 3: the DELTA form 0.498 vs 0.512 ms tiled, 16 workgroups per slot; 8 / 32 per
// slot 0.507 / 0.504 -- a pass with three read streams is bound by the read path,
// profiles/r03_mem_counters.md).  Bits 4 and 8: measured at 512^3 on MI355X (`tools/ab_env.sh`
// (removed; see git history before this change), same box) the fused divide gains 12 % over the
// tiled kernel (0.376 -> 0.330 ms) and, with the twiddle tables transposed in the LDS, the fused
// update 2 % (0.485 -> 0.475 ms); the plain r2c / c2r passes, which the tiled kernels already run
// at the streaming ceiling, lose 3-8 % and stay tiled.
static bool wave_rows_enabled(const RowsParams& p, int kind_bit) {
  static const int mask = wr_rows_mask(28);
  return wr_rows_enabled(p, mask, kind_bit);
}

// `mult` workgroups per resident slot: short-lived workgroups that the dispatcher keeps feeding in
// address order stream better than resident ones that walk (`tools/skeleton_probe.hip` (removed; see
// git history before this change): a bare 2-reads-1-write skeleton reaches 5.27 TB/s with resident
// walkers, 5.50 with 64 workgroups per slot, 5.84 one-shot); against that the tables are built once
// per workgroup.  Measured at 512^3 (`tools/ab_bench.sh` (removed; see git history before this
// change)): fused divide 0.336 -> 0.312 ms at 16 per slot, fused update 0.535 -> 0.498 ms at 32.
template <typename K>
static void launch_wave_rows(K kernel, const RowsParams& p, stream_t s, long mult) {
  const size_t lds = sizeof(cfloat) * (size_t)WrCfg::lds_cfloats;
  const long pairs = (p.rows + 1) / 2;
  long grid = (pairs + WrCfg::WAVES - 1) / WrCfg::WAVES;
  const long resident = (long)resident_per_cu(reinterpret_cast<const void*>(kernel), WrCfg::NT, lds) *
                        device_cu_count() * mult;
  if (grid > resident) grid = resident;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(WrCfg::NT), lds, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

template <bool WALK, typename K>
static void launch_rows_fixed(K kernel, const RowsParams& p, long nblocks, int nthreads, size_t lds_bytes,
                              stream_t s) {
  if (WALK) {
    ensure_lds(kernel, lds_bytes);
    // eight workgroups per resident slot (see launch_wave_rows): measured fused divide / update
    // -5 / -3 % at 576^3, -7 / -7 % at 320 x 1920 x 1920 against resident walkers
    const long resident = (long)resident_per_cu(reinterpret_cast<const void*>(kernel), nthreads, lds_bytes) *
                          device_cu_count() * 8;
    if (nblocks > resident) nblocks = resident;
  }
  launch_pass(kernel, p, nblocks, nthreads, lds_bytes, s);
}

static void check_aligned16(const void* p, const char* what) {
  if (((size_t)p) & 15) throw std::invalid_argument(std::string("mvn: fixed kernels need 16-byte aligned ") + what);
}

// the kernel of a last-axis pass (KIND: MvnPassKind) - of a fixed length, or of the run-time-radix bodies
typedef void (*rows_kernel_t)(const RowsParams);
template <int KIND, int H, int EPI, bool LINES>
static rows_kernel_t fixed_rows_kernel() {
  if constexpr (KIND == MVN_PASS_R2C)
    return kx_rows_r2c<H, LINES>;
  else if constexpr (KIND == MVN_PASS_C2R)
    return kx_rows_c2r<H, EPI, LINES>;
  else
    return kx_rows_c2r_r2c<H, EPI, LINES>;
}
template <int KIND, int T, int FORM>
static rows_kernel_t generic_rows_kernel(bool even) {
  if constexpr (KIND == MVN_PASS_R2C)
    return even ? k_rows_r2c<true, T> : k_rows_r2c<false, T>;
  else if constexpr (KIND == MVN_PASS_C2R)
    return even ? k_rows_c2r<true, T, FORM> : k_rows_c2r<false, T, FORM>;
  else
    return k_rows_c2r_r2c<T, FORM>;  // (even extents only: Plan3D::rows_c2r_r2c)
}

// The three last-axis passes: the families in their order - line layout, wave rows, fixed length, run-time radix -
// each behind the one dispatch of the launch's mode (mvn_pass_bodies.hpp), which refuses a mode the pass does not take.
template <int KIND>
static void launch_rows(const RowsParams& p, bool even, long nblocks, int nthreads, size_t lds_bytes, stream_t s) {
  check_launch(nblocks, nthreads, lds_bytes);
  const int mode = p.epi.mode;
  if (p.lines) {  // (H = 256: d2 = 512)
    fx_rows_lines_check(p, nblocks);
    return mvn_epi_dispatch<KIND>(mode, [&](auto epi) {
      launch_pass(fixed_rows_kernel<KIND, 256, decltype(epi)::value, true>(), p, nblocks, nthreads, lds_bytes, s);
    });
  }
  if (p.fixed) {
    check_aligned16(KIND == MVN_PASS_R2C ? (const void*)p.in_real : p.in_cplx, "input");
    check_aligned16(KIND == MVN_PASS_C2R ? (const void*)p.out_real : p.out_cplx, "output");
    if (wave_rows_enabled(p, mvn_wave_rows_kind_bit(KIND, mode)))
      return mvn_epi_dispatch<KIND>(mode, [&](auto epi) {
        launch_wave_rows(kw_rows<KIND, decltype(epi)::value>, p, s, mvn_wave_rows_per_slot(KIND, mode));
      });
    switch (p.h) {
#define X(H)                                                                                                     \
  case H:                                                                                                        \
    return mvn_epi_dispatch<KIND>(mode, [&](auto epi) {                                                          \
      launch_rows_fixed<FxRowsCfg<H>::WALK>(fixed_rows_kernel<KIND, H, decltype(epi)::value, false>(), p, nblocks, \
                                            nthreads, lds_bytes, s);                                             \
    });
      MVN_FIXED_ROWS_LENGTHS(X)
#undef X
      default: throw std::invalid_argument("mvn: no fixed rows kernel for this length");
    }
  }
  mvn_epi_dispatch<KIND, true>(mode, [&](auto form) {
    mvn_dispatch_tile_width(p.T, [&](auto t) {
      launch_pass(generic_rows_kernel<KIND, decltype(t)::value, decltype(form)::value>(even), p, nblocks, nthreads,
                  std::max(lds_bytes, (size_t)mvn_epi_extra_lds_bytes(mode, nthreads)), s);
    });
  });
}

void launch_rows_r2c(const RowsParams& p, bool even, long nblocks, int nthreads, size_t lds_bytes,
                     stream_t s) {
  launch_rows<MVN_PASS_R2C>(p, even, nblocks, nthreads, lds_bytes, s);
}
void launch_rows_c2r(const RowsParams& p, bool even, long nblocks, int nthreads, size_t lds_bytes,
                     stream_t s) {
  launch_rows<MVN_PASS_C2R>(p, even, nblocks, nthreads, lds_bytes, s);
}
void launch_rows_c2r_r2c(const RowsParams& p, long nblocks, int nthreads, size_t lds_bytes,
                         stream_t s) {
  launch_rows<MVN_PASS_C2R_R2C>(p, true, nblocks, nthreads, lds_bytes, s);
}

void launch_convergence_reduce(const double* rec, const unsigned* counts, int nviews, long cap, double* out,
                               stream_t s) {
  hipLaunchKernelGGL(k_convergence_reduce, dim3(1), dim3(256), 0, hs(s), rec, counts, nviews, cap, out);
  HIP_CHECK(hipGetLastError());
}

void launch_nm_reduce(const double* rec, const unsigned* counts, int nviews, long cap, double* out, stream_t s) {
  hipLaunchKernelGGL(k_nm_reduce, dim3((unsigned)nviews), dim3(256), 0, hs(s), rec, counts, cap, out);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long> g_split_launches{0};
long split_launch_count() { return g_split_launches.load(); }
static std::atomic<long> g_mid_fused_launches{0};
long mid_fused_launch_count() { return g_mid_fused_launches.load(); }

// long lines: 16-column tiles through the split-window body when the columns divide (fx_split_retile)
template <int N>
static bool try_launch_split(int mode, const StridedParams& p, long nblocks, stream_t s, const StridedParams* rider,
                             size_t rider_lds) {
  StridedParams q;
  if (!fx_split_retile<N>(mode, p, nblocks, q)) return false;
  if constexpr (FxSplitCfg<N>::USE) {
    typedef FxSplitCfg<N> C;
    const size_t lds = sizeof(cfloat) * (size_t)C::lds_cfloats;
    ++g_split_launches;
    if (mode == MVN_ST_FWD)
      launch_walking(kx_strided_split<N, MVN_ST_FWD>, q, q.nblocks, C::NT, lds, s, true, rider, rider_lds);
    else
      launch_walking(kx_strided_split<N, MVN_ST_INV>, q, q.nblocks, C::NT, lds, s, true, rider, rider_lds);
  }
  return true;
}

template <int T, bool NYQ>
static auto strided_kernel(int mode) -> void (*)(const StridedParams) {
  switch (mode) {
    case MVN_ST_FWD: return k_strided<MVN_ST_FWD, T, NYQ>;
    case MVN_ST_INV: return k_strided<MVN_ST_INV, T, NYQ>;
    case MVN_ST_FWD_MUL_INV: return k_strided<MVN_ST_FWD_MUL_INV, T, NYQ>;
    default: throw std::invalid_argument("mvn: unknown strided mode");
  }
}

void launch_strided(int mode, const StridedParams& p, long nblocks, int nthreads,
                    size_t lds_bytes, stream_t s, const StridedParams* rider, size_t rider_lds) {
  check_launch(nblocks, nthreads, lds_bytes);
  mvn_strided_rider_check(mode, p, rider, rider_lds);
  if (p.fixed) {
    check_aligned16(p.data, "data");
    if (mode == MVN_ST_FWD_MUL_INV) check_aligned16(p.spec, "spectrum");
    switch (p.ax.n) {
#define X(N)                                                                                       \
  case N:                                                                                          \
    if (try_launch_split<N>(mode, p, nblocks, s, rider, rider_lds)) return;                        \
    if (mode == MVN_ST_FWD) launch_walking(kx_strided<N, MVN_ST_FWD>, p, nblocks, FxStridedSel<N, MVN_ST_FWD>::NT, lds_bytes, s, true, rider, rider_lds); \
    else if (mode == MVN_ST_INV) launch_walking(kx_strided<N, MVN_ST_INV>, p, nblocks, FxStridedSel<N, MVN_ST_INV>::NT, lds_bytes, s, true, rider, rider_lds); \
    else launch_walking(kx_strided<N, MVN_ST_FWD_MUL_INV>, p, nblocks, FxStridedSel<N, MVN_ST_FWD_MUL_INV>::NT, lds_bytes, s, !FxStridedSel<N, MVN_ST_FWD_MUL_INV>::LDS_FUSED); \
    return;
      MVN_FIXED_STRIDED_LENGTHS(X)
#undef X
      default: throw std::invalid_argument("mvn: no fixed strided kernel for this length");
    }
  }
  mvn_dispatch_tile_width(p.T, [&](auto t) {
    constexpr int T = decltype(t)::value;
    launch_pass(p.is_nyq ? strided_kernel<T, true>(mode) : strided_kernel<T, false>(mode), p, nblocks, nthreads, lds_bytes, s);
  });
}

void launch_dim0_direct(const Dim0DirectParams& p, stream_t s) {
  mvn_dim0_check(p);
  if (p.plane > 0) check_aligned16(p.in, "input");  // (8-byte accesses; the volumes are 16-byte aligned anyway)
  const long main_blocks = mvn_dim0_blocks(p).blocks;
  long nblocks = main_blocks;
  size_t lds = 0;
  if (p.packed) {
    nblocks += mvn_dim0_pairs(p.d1);
    lds = mvn_dim0_dc_lds_bytes(p.d0, p.k);
  }
  if (nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  switch (mvn_dim0_taps_template(p.k)) {
#define X(K) case K: hipLaunchKernelGGL(kd_dim0<K>, dim3((unsigned)nblocks), dim3(MVN_D0_WG), lds, hs(s), p, (unsigned)main_blocks); break;
    MVN_D0_TAP_COUNTS(X)
#undef X
    default: throw std::invalid_argument("mvn: no direct dim0 kernel for this tap count");
  }
  HIP_CHECK(hipGetLastError());
}

void launch_mid_fused(const MidFusedParams& p, stream_t s) {
  mf_check(p);
  const long nblocks = mf_blocks(p);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  const size_t lds = sizeof(cfloat) * (size_t)MF_LDS_CFLOATS;
  if (p.mode == MF_TAPS) {
    launch_pass(kf_mid_taps, p, nblocks, MF_NT, lds, s);
    return;
  }
  ++g_mid_fused_launches;
  switch (mvn_dim0_taps_template(p.k)) {
#define X(K) case K: launch_pass(kf_mid<K>, p, nblocks, MF_NT, lds, s); break;
    MVN_MF_TAP_COUNTS(X)
#undef X
    default: throw std::invalid_argument("mvn: no fused middle pass for this tap count");
  }
}

static unsigned flat_grid(size_t n, int block) {
  size_t g = (n + (size_t)block - 1) / (size_t)block;
  const size_t cap = (size_t)device_cu_count() * 8;  // ~8 blocks per CU of THIS device, grid-stride the rest
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

void launch_scatter_psf(const float* kernel, int k0, int k1, int k2, float* target, int D0,
                        int D1, int D2, long pitch, float scale, stream_t s) {
  const size_t total = (size_t)k0 * k1 * k2;
  hipLaunchKernelGGL(k_scatter_psf, dim3(flat_grid(total, 256)), dim3(256), 0, hs(s), kernel, k0,
                     k1, k2, target, D0, D1, D2, pitch, scale);
  HIP_CHECK(hipGetLastError());
}

void launch_copy3d(float* dst, long drow, long dplane, const float* src, long srow, long splane,
                   int nx, int ny, int nz, stream_t s) {
  if (nx < 1 || ny < 1 || nz < 1) return;
  const long rows = (long)ny * nz;
  const int block = nx >= 256 ? 256 : (nx >= 128 ? 128 : 64);
  const unsigned grid = (unsigned)(rows < 256L * 32 ? rows : 256L * 32);
  hipLaunchKernelGGL(k_copy3d, dim3(grid), dim3(block), 0, hs(s), dst, drow, dplane, src, srow, splane,
                     nx, ny, nz);
  HIP_CHECK(hipGetLastError());
}

void launch_ingest3d(const IngestParams& p, bool u16, stream_t s, bool dst_u16) {
  const long nblocks = mvn_ingest_blocks(p.rows);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  if (dst_u16 && (!u16 || p.use_value)) throw std::invalid_argument("mvn: a uint16 volume takes a uint16 stack");
  if (dst_u16)
    hipLaunchKernelGGL(k_ingest3d_u16, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
  else if (u16)
    hipLaunchKernelGGL(k_ingest3d<uint16_t>, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_ingest3d<float>, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_extract3d(const ExtractParams& p, stream_t s) {
  const long nblocks = mvn_extract_blocks(p);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  hipLaunchKernelGGL(k_extract3d, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long long> g_reflect_launches{0}, g_reflect_volumes{0};
void reflect_counters(long long out[2]) {
  out[0] = g_reflect_launches.load();
  out[1] = g_reflect_volumes.load();
}

void launch_reflect_fill(const ReflectParams& p0, bool u16, stream_t s) {
  mvn_reflect_check(p0);
  ReflectParams p = p0;
  for (int axis = 2; axis >= 0; --axis) {
    p.axis = axis;
    const long nblocks = mvn_ingest_blocks(mvn_reflect_rows_of(p));
    if (nblocks < 1) continue;  // (no margin along this axis)
    if (nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
    ++g_reflect_launches;
    if (u16)
      hipLaunchKernelGGL(k_reflect3d<uint16_t>, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
    else
      hipLaunchKernelGGL(k_reflect3d<float>, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
    HIP_CHECK(hipGetLastError());
  }
  ++g_reflect_volumes;
}

static std::atomic<long long> g_resample_launches{0}, g_normalize_launches{0};
void resample_counters(long long out[2]) {
  out[0] = g_resample_launches.load();
  out[1] = g_normalize_launches.load();
}

void launch_resample(const ResampleParams& p, bool u16, stream_t s) {
  mvn_resample_check(p);
  const long nblocks = mvn_resample_blocks(p);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  ++g_resample_launches;
  if (u16)
    hipLaunchKernelGGL(k_resample3d<uint16_t>, dim3((unsigned)nblocks), dim3(MVN_RS_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_resample3d<float>, dim3((unsigned)nblocks), dim3(MVN_RS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_weights_normalize(const NormalizeParams& p, stream_t s) {
  mvn_normalize_check(p);
  const long nblocks = mvn_normalize_blocks(p);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  ++g_normalize_launches;
  hipLaunchKernelGGL(k_weights_normalize, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long long> g_fuse_raw_launches{0}, g_fuse_volumes_launches{0};
void fuse_counters(long long out[2]) {
  out[0] = g_fuse_raw_launches.load();
  out[1] = g_fuse_volumes_launches.load();
}

void launch_fuse_resampled(const FuseParams& p, stream_t s) {
  mvn_fuse_check(p);
  const long nblocks = mvn_fuse_blocks(p);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  ++g_fuse_raw_launches;
  hipLaunchKernelGGL(k_fuse_resampled, dim3((unsigned)nblocks), dim3(MVN_RS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_fuse_volumes(const FuseVolumesParams& p, stream_t s) {
  mvn_fuse_volumes_check(p);
  const long nblocks = mvn_fuse_volumes_blocks(p);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  ++g_fuse_volumes_launches;
  hipLaunchKernelGGL(k_fuse_volumes, dim3((unsigned)nblocks), dim3(MVN_INGEST_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long long> g_psf_correlate_launches{0};
long long psf_correlate_launches() { return g_psf_correlate_launches.load(); }

static unsigned psf_grid(long nblocks) {
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  return (unsigned)nblocks;
}

void launch_psf_normalize(const PsfNormParams& p, stream_t s) {
  mvn_psf_norm_check(p);
  hipLaunchKernelGGL(k_psf_sum, dim3(psf_grid(p.count)), dim3(MVN_PSF_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_psf_scale, dim3(psf_grid(p.count * mvn_psf_blocks(p.n))), dim3(MVN_PSF_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_psf_pointwise(const PsfPointParams& p, stream_t s) {
  mvn_psf_point_check(p);
  hipLaunchKernelGGL(k_psf_pointwise, dim3(psf_grid(p.V * mvn_psf_blocks(p.n))), dim3(MVN_PSF_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_psf_correlate(const PsfCorrParams& p, stream_t s) {
  mvn_psf_corr_check(p);
  ++g_psf_correlate_launches;
  hipLaunchKernelGGL(k_psf_correlate, dim3(psf_grid((long)p.njobs * p.blocks_per_job)), dim3(MVN_PSF_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long long> g_beads_gather_launches{0}, g_beads_score_launches{0};
void beads_counters(long long out[2]) {
  out[0] = g_beads_gather_launches.load();
  out[1] = g_beads_score_launches.load();
}

void launch_beads_gather(const BeadsParams& p, bool u16, stream_t s) {
  mvn_beads_check(p);
  const unsigned grid = psf_grid((long)mvn_beads_groups(p.nbeads) * mvn_beads_tiles(p));
  ++g_beads_gather_launches;
  if (u16)
    hipLaunchKernelGGL(k_beads_gather<uint16_t>, dim3(grid), dim3(MVN_BEADS_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_beads_gather<float>, dim3(grid), dim3(MVN_BEADS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_beads_reduce(const BeadsParams& p, stream_t s) {
  mvn_beads_check(p);
  hipLaunchKernelGGL(k_beads_reduce, dim3(psf_grid(mvn_beads_tiles(p))), dim3(MVN_BEADS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_beads_remove_min(const BeadsParams& p, stream_t s) {
  mvn_beads_check(p);
  if (!p.minima) throw std::invalid_argument("mvn: beads: null pointer");
  hipLaunchKernelGGL(k_beads_min, dim3(1), dim3(MVN_BEADS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_beads_sub, dim3(psf_grid(mvn_beads_tiles(p))), dim3(MVN_BEADS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_beads_score(const BeadsParams& p, bool u16, stream_t s) {
  mvn_beads_check(p);
  if (!p.records || !p.scores) throw std::invalid_argument("mvn: beads: null pointer");
  ++g_beads_score_launches;
  if (u16)
    hipLaunchKernelGGL(k_beads_score<uint16_t>, dim3(psf_grid(p.nbeads)), dim3(MVN_BEADS_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_beads_score<float>, dim3(psf_grid(p.nbeads)), dim3(MVN_BEADS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
  const long folds = ((long)p.nbeads + MVN_BEADS_WG - 1) / MVN_BEADS_WG;
  hipLaunchKernelGGL(k_beads_score_fold, dim3(psf_grid(folds)), dim3(MVN_BEADS_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long long> g_detect_blur_launches{0}, g_detect_extrema_launches{0};
void detect_counters(long long out[2]) {
  out[0] = g_detect_blur_launches.load();
  out[1] = g_detect_extrema_launches.load();
}

void launch_detect_blur(const DetectParams& p, bool u16, stream_t s) {
  mvn_detect_check_blur(p);
  const unsigned rows = psf_grid(mvn_detect_rows_blocks(p));
  const unsigned cols = psf_grid(mvn_detect_lines_blocks(p, 1)), planes = psf_grid(mvn_detect_lines_blocks(p, 0));
  g_detect_blur_launches += 3;
  if (u16)
    hipLaunchKernelGGL(k_detect_rows<uint16_t>, dim3(rows), dim3(MVN_DETECT_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_detect_rows<float>, dim3(rows), dim3(MVN_DETECT_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_detect_lines<1>, dim3(cols), dim3(MVN_DETECT_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_detect_lines<0>, dim3(planes), dim3(MVN_DETECT_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_detect_extrema(const DetectParams& p, stream_t s) {
  mvn_detect_check_list(p);
  ++g_detect_extrema_launches;
  hipLaunchKernelGGL(k_detect_extrema, dim3(psf_grid(mvn_detect_extrema_blocks(p))), dim3(MVN_DETECT_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_detect_refine(const DetectParams& p, stream_t s) {
  mvn_detect_check_list(p);
  if (p.nfound < 1 || p.nfound > p.list_cap || !p.pos || !p.val || !p.vox)
    throw std::invalid_argument("mvn: detect: nothing to refine");
  hipLaunchKernelGGL(k_detect_refine, dim3(psf_grid(mvn_detect_ceil((long)p.nfound, MVN_DETECT_WG))),
                     dim3(MVN_DETECT_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long long> g_register_match_launches{0}, g_register_ransac_launches{0};
void register_counters(long long out[2]) {
  out[0] = g_register_match_launches.load();
  out[1] = g_register_ransac_launches.load();
}

void launch_register_neighbours(const RegParams& p, stream_t s) {
  mvn_reg_check_neighbours(p);
  hipLaunchKernelGGL(k_reg_neighbours, dim3(psf_grid(mvn_reg_neighbours_blocks(p))), dim3(MVN_REG_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_register_match(const RegParams& p, stream_t s) {
  mvn_reg_check_match(p);
  ++g_register_match_launches;
  hipLaunchKernelGGL(k_reg_match, dim3(psf_grid(mvn_reg_match_blocks(p))), dim3(MVN_REG_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_reg_match_fold, dim3(psf_grid(mvn_reg_fold_blocks(p))), dim3(MVN_REG_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_register_ransac(const RegParams& p, stream_t s) {
  mvn_reg_check_ransac(p);
  ++g_register_ransac_launches;
  hipLaunchKernelGGL(k_reg_ransac, dim3(psf_grid(mvn_reg_ransac_blocks(p))), dim3(MVN_REG_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static unsigned accel_grid(const AccelParams& p, int W) {
  const long nblocks = mvn_accel_blocks(p.n, W);
  if (nblocks < 1 || nblocks > 0x7fffffffL) throw std::invalid_argument("mvn: grid size out of range");
  return (unsigned)nblocks;
}

void launch_accel_a(const AccelParams& p, stream_t s) {
  if (p.RP == p.d2)
    hipLaunchKernelGGL(k_accel_a<4>, dim3(accel_grid(p, 4)), dim3(MVN_ACCEL_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_accel_a<2>, dim3(accel_grid(p, 2)), dim3(MVN_ACCEL_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_accel_reduce(const double* rec, long nrec, float* alpha, stream_t s) {
  hipLaunchKernelGGL(k_accel_reduce, dim3(1), dim3(MVN_ACCEL_WG), 0, hs(s), rec, nrec, alpha);
  HIP_CHECK(hipGetLastError());
}

void launch_accel_b(const AccelParams& p, stream_t s) {
  if (p.RP == p.d2)
    hipLaunchKernelGGL(k_accel_b<4>, dim3(accel_grid(p, 4)), dim3(MVN_ACCEL_WG), 0, hs(s), p);
  else
    hipLaunchKernelGGL(k_accel_b<2>, dim3(accel_grid(p, 2)), dim3(MVN_ACCEL_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

static std::atomic<long> g_tv_launches{0};
long tv_launch_count() { return g_tv_launches.load(); }

void launch_tv(const TvParams& p0, stream_t s) {
  TvParams p = p0;
  mvn_tv_geometry(p);
  const long nblocks = mvn_tv_blocks(p);
  if (p.d0 < 1 || p.d1 < 1 || p.d2 < 1 || p.RP < p.d2 || (long)p.d1 * p.RP > 0x7fffffffL || nblocks < 1 ||
      nblocks > 0x7fffffffL)
    throw std::invalid_argument("mvn: total-variation pass outside its range");
  ++g_tv_launches;
  hipLaunchKernelGGL(k_tv_factor, dim3((unsigned)nblocks), dim3(MVN_TV_WG), 0, hs(s), p);
  HIP_CHECK(hipGetLastError());
}

void launch_divide(const float* view, float* inout, size_t n, stream_t s) {
  hipLaunchKernelGGL(k_divide, dim3(flat_grid(n, 256)), dim3(256), 0, hs(s), view, inout, n);
  HIP_CHECK(hipGetLastError());
}

void launch_update(float* psi, const float* integral, const float* weights, size_t n,
                   double lambda, float min_value, stream_t s) {
  const float linv = lambda > 0 ? (float)(1.f / lambda) : 0.f;
  hipLaunchKernelGGL(k_update, dim3(flat_grid(n, 256)), dim3(256), 0, hs(s), psi, integral,
                     weights, n, lambda, linv, min_value);
  HIP_CHECK(hipGetLastError());
}

void launch_update_legacy_tikhonov(float* image, const float* integral, const float* weights,
                                   size_t n, float lambda_f, float min_value, stream_t s) {
  hipLaunchKernelGGL(k_update_legacy_tikhonov, dim3(flat_grid(n, 256)), dim3(256), 0, hs(s), image,
                     integral, weights, n, lambda_f, min_value);
  HIP_CHECK(hipGetLastError());
}

void launch_axpy1(float* psi, const float* delta, size_t n, stream_t s) {
  hipLaunchKernelGGL(k_axpy1, dim3(flat_grid(n, 256)), dim3(256), 0, hs(s), psi, delta, n);
  HIP_CHECK(hipGetLastError());
}

}  // namespace be
}  // namespace mvn
