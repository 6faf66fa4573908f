/*
 * mvn_engine_api.h -- C ABI of the device-resident engine underneath multiviewnative.h.
 *
 * Not part of the reference's interface: these entry points expose what the reference keeps
 * internal (gpu::plan_store, inc/plan_store.cuh:20-216; the all-on-device RL driver,
 * src/gpu_deconvolve_methods.cuh:345-562; inplace_3d_transform_on_device,
 * inc/cufft_utils.cuh:41-75) so that benches, the multi-GPU launcher and the parity tests can
 * keep data resident in HBM between steps.  Plain pointers and sizes only.  Every function
 * returns 0 on success and a negative value on failure (message via mvn_last_error()).
 */
#ifndef MVN_ENGINE_API_H
#define MVN_ENGINE_API_H

#include <stddef.h>

#include "multiviewnative.h"

typedef struct mvn_engine mvn_engine; /* opaque */

MVN_API const char* mvn_last_error(void);
MVN_API const char* mvn_backend_name(void);

/* inplace_gpu_deconvolve keeps one resident engine per device between calls (same shape and view
 * count are re-used without re-allocating; MVN_ENGINE_CACHE=0 disables it).  This frees them. */
MVN_API int mvn_release_cached_engines(void);

/* Block-after-block callers (Fiji deconvolves a large volume as a sequence of blocks): the
 * asynchronous form of inplace_gpu_deconvolve.  Submit starts the call on a worker thread and
 * returns a ticket; wait blocks until that call is complete (psi written) and returns its status.
 * Submits to one device alternate between two resident engines, so the stacks of block k+1 cross
 * PCIe while block k iterates -- what the reference's interleaved driver
 * (inplace_gpu_deconvolve_iteration_interleaved, src/gpu_deconvolve_methods.cuh:82-326, "not
 * supported yet" there) was meant to do inside one call.  The workspace struct, its view_data array
 * and the int[3] dims are copied at submit; psi and every stack / kernel buffer they point to must
 * stay valid and untouched until the matching wait returns.  The padding policy is the one in
 * force at submit.  Results are those of inplace_gpu_deconvolve, bit for bit.  Every ticket must
 * be waited for exactly once; inplace_gpu_deconvolve == submit + wait on the first engine. */
MVN_API int mvn_deconvolve_submit(imageType* psi, struct workspace input, int device, long long* ticket);
MVN_API int mvn_deconvolve_wait(long long ticket);
/* ---- stacks as the caller has them: device memory, uint16, strides ---------------------------------------------
 * mvn_deconvolve_described is inplace_gpu_deconvolve for stacks that are not dense float32 arrays in host memory.
 * `workspace` keeps its meaning - kernels and every *_dims_ member are host memory, dense float32 / int - while
 * image_, weights_ and psi are read through descriptors:
 *   dtype     MVN_F32 or, for images only, MVN_U16 (what a camera delivers; the conversion to float32 is exact)
 *   location  MVN_HOST or MVN_DEVICE.  A stack in device memory is read (psi: also written) where it lies, by one pass
 *             that converts, embeds and pads (csrc/mvn_ingest.hpp): no copy, no scratch.  A stack in host memory
 *             crosses PCIe as it is - uint16 as uint16, half the bytes - and then goes through the same pass; only
 *             float32 into a volume of its own extents (padding "none", the engine API) is placed by the copy itself.
 *   stride    in ELEMENTS, per dimension of image_dims_.  dense is {d1 * d2, d2, 1}.  Inputs may repeat elements:
 *             a stride of 0 along a dimension, and {0, 0, 0} = one value for every voxel (constant weights); negative
 *             strides are refused.  psi, which is written, needs positive strides that do not overlap.  Stacks in
 *             HOST memory need contiguous rows (stride[2] == 1, stride[1] >= d2; planes anywhere: they cross with
 *             2-D copies) or {0, 0, 0}; any other host layout is refused - the library does not gather on the host.
 * A NULL descriptor array means dense float32 in host memory for every view.
 * The call blocks like inplace_gpu_deconvolve: on return psi is written and the library's streams are drained.
 * `stream` is the hipStream_t the caller produced its device stacks on: the library records an event there and its
 * own streams wait for it before their first read - the host never waits on the caller's stream.  NULL: the stacks
 * are complete when the call is made.
 * Everything else is the blocking call's: the padding policy in force, engine and PSF caches, convergence statistics,
 * the quotient guard, and errors (< 0, message in mvn_last_error(), psi untouched).  The result is bit for bit that of
 * inplace_gpu_deconvolve on the same values as dense float32 host stacks.
 * With any stack in device memory the call runs on the device that owns it (device < 0 picks it; another device,
 * stacks on two devices, or a pointer whose location is not the one described - asked of the runtime's pointer
 * attributes before anything reads it - is an error), ignores MVN_DEVICES and runs resident whatever the memory
 * mode: it is refused with "memory constraints" when mvn_deconvolve_memory's figure (less the embedding scratch when
 * no stack needs it) does not fit.  Calls with host stacks only keep the memory modes - a streamed uint16 view
 * streams uint16, mvn_stream_counters counts the bytes that crossed - and MVN_DEVICES when every descriptor is the
 * default one. */
enum { MVN_F32 = 0, MVN_U16 = 1 };     /* element type */
enum { MVN_HOST = 0, MVN_DEVICE = 1 }; /* where the pointer lives */
typedef struct mvn_stack_desc {
  int dtype;
  int location;
  long long stride[3];
} mvn_stack_desc;
typedef struct mvn_call_desc {
  mvn_stack_desc psi;            /* in/out, MVN_F32 */
  const mvn_stack_desc* image;   /* num_views_ entries, or NULL = all dense host float32 */
  const mvn_stack_desc* weights; /* num_views_ entries (MVN_F32), or NULL = all dense host float32 */
  void* stream;
} mvn_call_desc;
MVN_API int mvn_deconvolve_described(void* psi, struct workspace input, const mvn_call_desc* desc, int device);
/* How uint16 IMAGE stacks of described calls are held on the device for the calls that follow (process-wide, captured
 * at the start of mvn_deconvolve_described / at mvn_engine_set_view_described):
 * 0 (default) converted to float32 on entry, as before - launches and results as without this switch;
 * 1 kept as uint16: the volume (and a streamed view's ring slot) holds 2 bytes per voxel, the divide pass reads them.
 * Results are bit for bit those of mode 0.  float32 images, weights and psi are never affected.  Anything else: error.
 * In mode 1 a uint16 stack in host memory with contiguous rows, under padding "none" (and through the engine API), is
 * placed by the copy itself, with no pass behind it; every other uint16 stack (device memory, other strides, the padded
 * policies) takes the ingest pass in its uint16 -> uint16 form (csrc/mvn_ingest.hpp).  The views of one call may mix
 * element types.  The streamed views of a call share their ring slots: they are kept as uint16 when all of them are
 * uint16 stacks, and converted as in mode 0 otherwise.
 * Out of scope, and unchanged by the mode: weights and psi (float32); float32 images (never narrowed); a uint16 image
 * that is one value for every voxel (strides {0, 0, 0}: converted); the slab engine (mvn_slab_*); mvn_group_* and
 * MVN_DEVICES (which a described call with other than default descriptors does not use anyway); halo mode -
 * mvn_engine_set_view_described on an engine with a halo hook keeps the image as float32, and
 * mvn_engine_set_halo_hook on an engine that holds a uint16 image volume is an error. */
MVN_API int mvn_set_image_storage(int mode);
MVN_API int mvn_get_image_storage(int* mode);
/* mvn_deconvolve_memory for a described call: prices uint16 images at 2 bytes per voxel when the storage mode in force
 * keeps them (only dtype and strides of desc->image are read).  desc == NULL, or mode 0: exactly
 * mvn_deconvolve_memory's figure. */
MVN_API int mvn_deconvolve_memory_described(struct workspace input, const mvn_call_desc* desc, int device,
                                            int streamed_views, size_t* bytes);
/* ---- resampled views: the raw stack and a 3 x 4 matrix ----------------------------------------------------------
 * mvn_deconvolve_resampled is mvn_deconvolve_described for views that are NOT registered yet: image_ of view v is the
 * raw camera stack, desc->image[v] describes it (dtype, location, strides) over geom[v].src_dims, and geom[v] maps the
 * block into it.  image_dims_ / weights_dims_ are the block's extents, which are psi's.  A block's position inside a
 * larger data set is folded into the matrix's fourth column by the caller: the next block of the same data set uses the
 * same raw pointers and another offset.
 *
 * Image.  For block voxel (z, y, x), 0-based integer indices in image_dims_:
 *   coordinate   c_k = ((M[k][0]*z + M[k][1]*y) + M[k][2]*x) + M[k][3], k = 0, 1, 2, in double, no contraction, every
 *                operation rounded once
 *   inside       iff 0 <= c_k <= m_k - 1 for every k, compared in double; a voxel that is not inside gets image 0 and
 *                weight 0
 *   cell         i_k = floor(c_k), f_k = (float)(c_k - (double)i_k); neighbour j_k = min(i_k + 1, m_k - 1) (the clamp is
 *                reached only with f_k == 0: an extent of 1 is no special case)
 *   samples      S(a, b, c): the raw element widened to float32 (uint16 to float is exact)
 *   trilinear    in float32, no contraction, lerp(p, q, f) = p + f * (q - p) (one subtract, one multiply, one add):
 *                a_pq = lerp(S(p, q, i2), S(p, q, j2), f2) for p in {i0, j0}, q in {i1, j1};
 *                b_p = lerp(a_p,i1, a_p,j1, f1);  v = lerp(b_i0, b_j0, f0)
 * Blend weight (Fiji's cosine blend), for inside voxels: d_k = min(c_k, (m_k - 1) - c_k) in double, dk = (float)d_k,
 *   r_k = 0 when dk < border_k; 1 when range_k == 0 or dk >= border_k + range_k; otherwise
 *   0.5f * (1.0f - cosf(pi_f * ((dk - border_k) / range_k)));  w = (r_0 * r_1) * r_2.
 * Normalisation over the views, once per call, after every view has been placed, over the stacks' window only, in
 *   float32: W = ((w_0 + w_1) + ...) + w_{V-1} in view order, then w_v <- W > 0 ? w_v / W : 0, so sum_v w_v <= 1.
 *   Under "reflect" the mirror fill of computed weights runs behind the normalisation.
 *
 * weights_mode 0: the caller's weights stacks (weights_, desc->weights), exactly as in the described call.
 * weights_mode 1: computed and normalised as above; weights_ and desc->weights are ignored (weights_ may be NULL).
 * Raw stacks in device memory are read where they lie; a raw stack in host memory (dense or contiguous rows, or one
 * value) is uploaded as it is into a temporary device buffer for the placement, one view at a time.  The call runs
 * resident on one device whatever the memory mode and MVN_DEVICES say, and holds its images as float32 whatever
 * mvn_set_image_storage says (interpolated values are no integers).  Everything behind the placement is the described
 * call's: padding policy, the loop's switches, caches, statistics.  Errors (< 0, message in mvn_last_error(), psi
 * untouched) beyond the described call's: a NULL geom, a non-finite matrix entry, a negative or non-finite border or
 * range, src_dims < 1, a weights_mode other than 0 or 1.
 * mvn_deconvolve_memory_resampled: mvn_deconvolve_memory_described's figure with float32 images and no streamed views,
 * plus the bytes of the largest raw stack in host memory (the temporary upload); it allocates nothing.
 * Out of scope: interpolation other than trilinear; mvn_deconvolve_submit; streamed views; mvn_group_* / mvn_slab_* /
 * halo mode (mvn_engine_set_view_resampled on an engine with a halo hook is an error); a mix of resampled and plain
 * views in one call; filling the padded margins with real raw data from beyond the block.  Kernels arrive transformed
 * into the block's frame unless mvn_set_kernel_derivation (below) says that they are raw PSFs. */
typedef struct mvn_view_geometry {
  int src_dims[3];       /* extents m0, m1, m2 of the raw stack image_ points to */
  double matrix[12];     /* row-major 3 x 4: raw index c = M * (z, y, x, 1) of block voxel (z, y, x) */
  float blend_border[3]; /* per raw axis, in raw voxels, >= 0: weight 0 within this distance of a face */
  float blend_range[3];  /* per raw axis, in raw voxels, >= 0: width of the cosine ramp behind the border */
} mvn_view_geometry;
MVN_API int mvn_deconvolve_resampled(void* psi, struct workspace input, const mvn_call_desc* desc,
                                     const mvn_view_geometry* geom, int weights_mode, int device);
MVN_API int mvn_deconvolve_memory_resampled(struct workspace input, const mvn_call_desc* desc,
                                            const mvn_view_geometry* geom, int weights_mode, int device, size_t* bytes);
/* Test and bench utilities.  mvn_resample_stack: the resample pass alone - the raw stack src (src_desc over
 * geom->src_dims, NULL = dense float32 in host memory; host or device memory) into two dense float32 HOST arrays of
 * extents out_dims, the image and the unnormalised weights (either may be NULL).
 * mvn_resample_time: ms[0] = milliseconds per pass (image and weights written) into resident volumes of extents out_dims
 * from a resident raw stack of geom->src_dims, uint16 (u16 != 0) or float32, `reps` passes between two stream events;
 * ms[1] = the same for streaming traffic of the output's size, one volume read and two written (a copy of a volume and
 * a clear of a second one).
 * mvn_resample_counters: out[0] = launches of the resample pass, out[1] = launches of the normalisation, since process
 * start. */
MVN_API int mvn_resample_stack(int device, const void* src, const mvn_stack_desc* src_desc, const mvn_view_geometry* geom,
                               const int out_dims[3], float* image_out, float* weights_out);
MVN_API int mvn_resample_time(int device, int u16, const mvn_view_geometry* geom, const int out_dims[3], int reps,
                              float* ms);
MVN_API int mvn_resample_counters(long long out[2]);
/* ---- fusion: the weighted average of the registered views -------------------------------------------------------
 * mvn_fuse_resampled writes F = sum_v w_v I_v / sum_v w_v of num_views RAW views into `out`, a block of extents
 * out_dims.  raw[v] is the raw stack of view v, raw_desc[v] describes it over geom[v].src_dims and geom[v] maps the block
 * into it, all as in mvn_deconvolve_resampled; raw_desc == NULL means dense float32 in host memory for every view.
 *
 * Arithmetic (normative).  For an output voxel take the views in view order; (s_v, w_v) are the trilinear sample and
 * the UNNORMALISED blend weight exactly as mvn_view_geometry defines them above, both 0 when the voxel is not inside
 * view v.  Everything is float32, every operation is rounded once, nothing is contracted into a fused multiply-add:
 *   t_v = w_v * s_v
 *   N   = ((t_0 + t_1) + ...) + t_{V-1}        (starts from t_0 itself, not from 0 + t_0)
 *   W   = ((w_0 + w_1) + ...) + w_{V-1}
 *   F   = W > 0 ? N / W : fill                 (correctly rounded divide)
 * A uint16 output stores F >= 65535 ? 65535 : F > 0 ? rintf(F) : 0 - ties round to even, a NaN becomes 0 - and the
 * same rule applies to `fill`.
 *
 * `out` is MVN_F32 or MVN_U16, in host or device memory, with the strides rules of psi in mvn_deconvolve_described
 * (out_desc == NULL: dense float32 in host memory).  An output in device memory is written where it lies, whatever its
 * (positive, non-overlapping) strides - with stores of 4 elements where rows are contiguous and base and pitches are
 * multiples of 4 elements -, and only its own elements are written: a window of a larger array keeps its surroundings.
 * An output in host memory (contiguous rows) is written into a dense device volume first and copied out.  Raw stacks in
 * device memory are read where they lie; raw stacks in host memory are uploaded into temporaries, all num_views at
 * once.  One kernel reads all views per output voxel; no image and no weights volume is written on the way.
 * The call blocks.  `stream`, the device choice and its checks are those of the described call.  Errors (< 0, message
 * in mvn_last_error(), `out` untouched) are those of the resampled call, plus num_views < 1 and a non-finite fill.
 * mvn_fuse_memory_resampled: the bytes that call would allocate on the device, allocating nothing: 176 bytes per view
 * (the table of the views' records), plus the dense output volume when `out` is in host memory, plus the sum of the raw
 * stacks in host memory (one element for a stack of strides {0, 0, 0}).  An all-device call costs the table alone.
 * mvn_fuse_time: ms[0] = milliseconds per fusion from num_views resident raw stacks of geom[v].src_dims (uint16 when
 * u16 != 0, else float32) into a resident float32 volume of extents out_dims, `reps` passes between two stream events
 * behind one pass that warms up (mvn_fuse_counters' out[0] moves by reps + 1); ms[1] = the same for num_views launches
 * of the resample pass on the same stacks and geometries, each writing an image and a weights volume - the route a
 * fusion took before this entry point, without its combining pass; ms[2] = a plain copy of one volume.
 * mvn_fuse_counters: out[0] = launches of the fusion from raw stacks, out[1] = launches of the fusion of an engine's
 * volumes (psi start, mvn_engine_fuse_psi), since process start. */
MVN_API int mvn_fuse_resampled(void* out, const mvn_stack_desc* out_desc, const int out_dims[3], int num_views,
                               const void* const* raw, const mvn_stack_desc* raw_desc,
                               const mvn_view_geometry* geom, float fill, void* stream, int device);
MVN_API int mvn_fuse_memory_resampled(const mvn_stack_desc* out_desc, const int out_dims[3], int num_views,
                                      const mvn_stack_desc* raw_desc, const mvn_view_geometry* geom,
                                      int device, size_t* bytes);
MVN_API int mvn_fuse_time(int device, int u16, int num_views, const mvn_view_geometry* geom,
                          const int out_dims[3], int reps, float* ms);
MVN_API int mvn_fuse_counters(long long out[2]);
/* Where mvn_deconvolve_resampled starts from (process-wide, captured at the start of that call; no other entry point
 * honours it):
 * 0 (default) the caller's psi - launches and bits as without this switch;
 * 1 psi is OUTPUT only (its pointer and descriptor must still be valid; what it holds is never read): after every view
 *   has been placed and before the weights are normalised, one pass fills psi's window with the F above, s_v and w_v
 *   read from the engine's image volumes and its weights volumes as they stand then - under weights_mode 1 the
 *   unnormalised computed blend weights, so psi starts from exactly mvn_fuse_resampled's float32 result; under
 *   weights_mode 0 the caller's weights.  The margins then follow the padding policy as if that stack had been handed
 *   in: zeros, or the mirror image under "reflect".  No extra volume is held: mvn_deconvolve_memory_resampled is
 *   unchanged.  A call of 0 iterations returns psi unchanged in either mode.
 * A mode other than 0 or 1, or a non-finite fill, is an error. */
MVN_API int mvn_set_psi_start(int mode, float fill);
MVN_API int mvn_get_psi_start(int* mode, float* fill);
/* ---- derived kernels: kernel1 and kernel2 of every view from its raw PSF and its matrix ------------------------------
 * What a caller has is the PSF extracted from beads in the raw view's own voxel grid, and the matrix it hands in anyway.
 * mvn_derive_kernels makes of them, on the device, what a deconvolution takes: kernel1_v, the PSF transformed into the
 * block's frame and normalised, and kernel2_v, the compound kernel of the iteration scheme of Preibisch et al. 2014
 * ("Independent", "Efficient Bayesian", "Optimization I", "Optimization II" in Multiview Reconstruction).
 *
 * Inputs per view v of V: a raw PSF p_v, dense float32 in HOST memory, of ODD extents r_v, centre cr = (r - 1) / 2; and
 * optionally the view's mvn_view_geometry, of which only the linear part A (matrix[4k + 0..2]) is read - the fourth
 * column, src_dims and the blend fields are ignored.  geom == NULL: the PSFs are in the block's frame already.
 *
 * Extents.  All derived kernels of a call share one odd extent triple K, h = (K - 1) / 2.  The caller may give K
 * (out_dims: odd, every entry in 1..257).  out_dims == NULL: K = mvn_psf_extents':
 *   with a geometry, per view B = A^-1 in double as adjugate over determinant (a zero or non-finite determinant is an
 *   error), s_k = (|B[k][0]| cr_0 + |B[k][1]| cr_1) + |B[k][2]| cr_2, h_k(v) = ceil(s_k - 1e-6), K_k = 2 max_v h_k(v) + 1
 *   (a K_k above 257 is an error); without one, K_k = max_v r_v[k].
 * Step 1, transform.  q_v is what mvn_resample_stack returns as image for the raw stack p_v (float32) with src_dims =
 *   r_v, matrix [A | t], border and range 0 and out_dims = K, where t_k = cr_k - ((A[k][0] h_0 + A[k][1] h_1) +
 *   A[k][2] h_2), formed in double on the host, every operation rounded once: the coordinate, inside, floor and lerp
 *   rules of mvn_view_geometry apply unchanged, voxels outside the raw PSF are 0.  Without a geometry q_v is p_v copied
 *   centred into K (an axis with K_k < r_v[k] keeps the central K_k elements).
 * Step 2, normalise.  S = sum q_v in double, in any order; kernel1_v[i] = (float)((double)q_v[i] / S).  S <= 0 or
 *   non-finite is an error ("a kernel without mass").
 * Step 3, kernel2.  Index kernels by the offset d from the centre, P_v = kernel1_v; a value outside an array's extents
 *   is 0; flip(P)(d) = P(-d).  The correlation primitive is
 *     corr(a, b)(d) = sum over t of (double)a(-t) * (double)b(d - t)
 *   with t over a's offsets in raster order (t_0 outermost, ascending), terms whose d - t lies outside b skipped, the sum
 *   started from +0.0 and held in double (the product of two widened floats is exact in double: contraction into a fused
 *   multiply-add cannot change a bit), the result rounded to float32 once.
 *     MVN_PSF_INDEPENDENT         kernel2_v = flip(P_v), bit for bit, no second normalisation - for every V
 *     MVN_PSF_EFFICIENT_BAYESIAN  A_w = corr(flip(P_w), flip(P_w)) on extents 2K - 1, held as float32 (the full
 *                                 autocorrelation of P_w; once per view); C_vw = corr(P_v, A_w) on extents K;
 *                                 T = flip(P_v); for w != v in view order T = T * C_vw (float32, rounded once);
 *                                 kernel2_v = T normalised as in step 2
 *     MVN_PSF_OPTIMIZATION_I      the same with C_vw = corr(P_v, P_w) on extents K; no autocorrelation
 *     MVN_PSF_OPTIMIZATION_II     T = flip(P_v) multiplied by flip(P_v) another V - 1 times (float32, no powf), normalised
 *   With V == 1 the product of the last three types is empty: kernel2 is flip(P_0) normalised once more.
 *
 * mvn_psf_extents: K by the rule above (raw_dims: 3 ints per view).  mvn_derive_kernels: kernel1[v] and kernel2[v] are
 * dense float32 HOST arrays of extents K (out_dims, or NULL = mvn_psf_extents'); either table may be NULL.  The call
 * blocks, checks everything before it touches anything, and writes the outputs last: errors (< 0, message in
 * mvn_last_error(), outputs untouched) are even or < 1 raw extents, a non-finite PSF value, a singular or non-finite
 * linear part, an unknown type, bad out_dims, num_views < 1, a null pointer, and a kernel without mass.
 * Device memory while it runs, all freed before it returns: the raw PSFs, one padded volume of extents K (rows of
 * K_2 + 1), 2 V prod K floats (kernel1, kernel2), V (V - 1) prod K floats (the C_vw, types 1 and 2 only) and
 * V prod (2K - 1) floats (the A_w, type 1 only), plus 64 bytes per correlation and 2048 + 8 bytes per kernel for the sums.
 * The correlations cost prod K multiply-adds per output voxel and are done one output voxel per work item: meant for
 * PSFs of tens of voxels per axis.
 *
 * mvn_set_kernel_derivation (process-wide; captured at the start of mvn_deconvolve_resampled, and read by
 * mvn_deconvolve_memory_resampled; no other entry point honours it): mode 0 (default) - kernels are handed in, launches
 * and bits as without this switch; mode 1 - kernel1_ / kernel1_dims_ of each view are the RAW PSF and its extents,
 * kernel2_ / kernel2_dims_ are ignored and may be NULL, and the call derives both kernels of `type` with geom's linear
 * parts and K = mvn_psf_extents' on its device before it looks up an engine, then continues exactly as if the derived
 * arrays of extents K had been handed in: padding extents, the dim0 form rule, the PSF cache, the uploader thread.
 * mvn_deconvolve_memory_resampled then prices the call with K (it reads dims and matrices only).  The derivation's errors
 * are the call's: psi stays untouched.  A mode other than 0 or 1, or an unknown type, is an error.
 * The derivation cache: process-wide, ONE entry - the last derivation, whichever of the two routes made it.  Its key is
 * the type, V, K, every raw PSF's extents and bytes and every linear part; a hit launches nothing, and the PSF cache
 * then sees identical kernel bytes and re-uses the spectra: the block-after-block case, where only the matrices' fourth
 * columns change.
 * mvn_derive_counters: out[0] = launches of the correlation kernel, out[1] = derivations computed, out[2] = derivations
 * re-used from the cache, since process start.
 * mvn_derive_time (test and bench utility): ms[0] = milliseconds per derivation of `type` for num_views resident PSFs
 * of extents dims (odd; no geometry, K = dims) holding random positive values - all its device work, `reps` derivations
 * between two stream events behind one that warms up; ms[1] = the same for its correlation launches alone (0 for the
 * types that have none).  It bypasses the derivation cache and moves out[0] only.
 * Out of scope: the engine API (mvn_engine_set_view_resampled keeps taking kernels: call mvn_derive_kernels first);
 * every entry point other than the two resampled ones; raw PSFs in device memory.  The raw PSF itself comes from the
 * view's beads through mvn_extract_psf (below). */
enum { MVN_PSF_INDEPENDENT = 0, MVN_PSF_EFFICIENT_BAYESIAN = 1, MVN_PSF_OPTIMIZATION_I = 2, MVN_PSF_OPTIMIZATION_II = 3 };
MVN_API int mvn_psf_extents(int num_views, const int* raw_dims, const mvn_view_geometry* geom, int out_dims[3]);
MVN_API int mvn_derive_kernels(int device, int num_views, const float* const* raw_psf, const int* raw_dims,
                               const mvn_view_geometry* geom, int type, const int out_dims[3],
                               float* const* kernel1, float* const* kernel2);
MVN_API int mvn_set_kernel_derivation(int mode, int type);
MVN_API int mvn_get_kernel_derivation(int* mode, int* type);
MVN_API int mvn_derive_counters(long long out[3]);
MVN_API int mvn_derive_time(int device, int num_views, const int dims[3], int type, int reps, float* ms);
/* ---- bead PSFs: a view's raw PSF from the beads in its raw stack -----------------------------------------------------
 * What a light-sheet caller has is the raw stack of each view and a list of sub-voxel bead positions in it, from the
 * interest points the views were registered with.  mvn_extract_psf averages, on the device, the interpolated
 * neighbourhoods of those beads: the result is exactly what mvn_derive_kernels takes as raw_psf[v].  One call takes ONE
 * view; a caller loops over its views.
 *
 * Inputs.  `raw` and raw_desc describe the raw stack over src_dims = m exactly as in mvn_resample_stack: uint16 or
 * float32, host or device memory, the stride rules of an input stack, raw_desc == NULL = dense float32 in host memory;
 * a stack in device memory is read where it lies, a stack in host memory is uploaded as it is into a temporary.
 * `beads` is num_beads x 3 doubles (z, y, x) in HOST memory, as raw indices.  psf_dims = r, every entry odd and in
 * 1..129, h = (r - 1) / 2.  psf_out is a dense float32 HOST array of extents r; scores_out receives num_beads doubles
 * in HOST memory, or is NULL.  `stream`, the device choice and its checks are those of the described call.
 *
 * Arithmetic (normative).  Every float32 operation is rounded once, nothing is contracted into a fused multiply-add.
 *   bead      for bead b at position p: B_k = floor(p_k), f_k = (float)(p_k - (double)B_k), formed once per bead - the
 *             window is a pure translation, so they are the same for every voxel of it
 *   sample    for PSF voxel j = (j0, j1, j2) the cell's low index along axis k is i_k = B_k + (j_k - h_k), its high index
 *             i_k + 1; both go through mir(i, n), the mirror without repeating the edge sample (numpy.pad's "reflect"):
 *             mir = 0 for n == 1, otherwise q = i mod (2n - 2) taken non-negative and mir = q < n ? q : 2n - 2 - q -
 *             which holds for windows wider than the stack (several reflections).  S is the raw element widened to
 *             float32, and s_b(j) is mvn_view_geometry's trilinear rule on those eight samples: lerp(p, q, f) =
 *             p + f * (q - p) along raw axis 2, then 1, then 0
 *   sum       beads in the order given, in groups of MVN_BEADS_GROUP: P_g(j) = ((+0.0 + (double)s_{32g}(j)) +
 *             (double)s_{32g+1}(j)) + ... in double; T(j) = ((P_0 + P_1) + ...) + P_{G-1}, started from P_0 itself;
 *             psf(j) = (float)(T(j) / (double)num_beads)
 *   The result is the mean window: one bead at integer coordinates returns its neighbourhood bit for bit.
 *   MVN_BEADS_REMOVE_MIN   mn = the minimum of psf over j (exact in any order); psf(j) <- psf(j) - mn in float32: the
 *             smallest value becomes 0, what a camera's offset leaves under the PSF is removed
 *   scores    (scores_out != NULL) against psf BEFORE the minimum is removed: per bead the sums sum s, sum s^2, sum P,
 *             sum P^2 and sum sP over the window, P = psf widened to double, in double and in any order (a product of
 *             two widened floats is exact in double); n = prod r;
 *             score_b = (sum sP - sum s sum P / n) / sqrt((sum s^2 - (sum s)^2 / n) (sum P^2 - (sum P)^2 / n)),
 *             and 0 where that denominator is not positive and finite.  Pearson's correlation of one bead with the
 *             mean, in [-1, 1]: a caller drops merged beads and debris by it and extracts again.
 *
 * The call blocks, checks everything before it touches anything and writes the outputs last: errors (< 0, message in
 * mvn_last_error(), psf_out and scores_out untouched) are those of mvn_resample_stack for the stack and its descriptor
 * (src_dims above 2^30 - 1 as well), num_beads < 1, a null pointer, even psf_dims or psf_dims out of range, an unknown
 * flag bit, a bead position that is not finite or lies outside 0 <= p_k <= m_k - 1 (the message names the bead's
 * index), and a result with a non-finite element ("a non-finite PSF": a non-finite raw sample is the caller's mistake
 * and must not reach the kernel derivation quietly).
 *
 * mvn_extract_memory: the device bytes that call allocates, allocating nothing; it reads only raw_desc, the dims and
 * the counts.  With G = ceil(num_beads / MVN_BEADS_GROUP) and n = prod r:
 *   32 num_beads            the bead records
 *   8 G n                   the G partial volumes in double
 *   4 n + 1028              the result, 256 partial minima and the non-finite flag
 *   (10240 + 8) num_beads   want_scores != 0 only: 256 records of five double sums per bead, and the scores
 *   the raw stack when it is in host memory: one element for strides {0, 0, 0}, m0 m1 m2 elements (the rows as they
 *   are uploaded) otherwise.
 * mvn_extract_counters, since process start: out[0] = launches of the gather, out[1] = launches of the score pass,
 * out[2] = extractions completed (mvn_extract_psf calls that returned 0).  An extraction is one launch of the gather
 * and, with scores_out, one of the score pass.
 * mvn_extract_time (test and bench utility): ms[0] = milliseconds per extraction - all its device work, no scores,
 * flags 0 - from a resident raw stack of src_dims (uint16 when u16 != 0, else float32; every src_dims[k] >=
 * psf_dims[k] + 2) with num_beads beads at reproducible sub-voxel positions at least h + 1 from every face, `reps`
 * extractions between two stream events behind one that warms up (out[0] moves by reps + 1, out[2] does not move);
 * ms[1] = the same for the route a caller had until now: num_beads launches of the resample pass (image only) on the
 * same stack and positions, each writing one volume of extents r through the identity plus the bead's offset, nothing
 * summed; ms[2] = a plain copy of num_beads x prod r floats.
 * The bead positions themselves come from the same raw stack through mvn_detect_beads (below).
 * Out of scope: several views in one call; interpolation other than trilinear; bead lists or the
 * result in device memory; a mode of mvn_set_kernel_derivation that takes bead lists - the extraction happens once per
 * data set, not once per block, and the derivation cache already makes block after block free. */
enum { MVN_BEADS_REMOVE_MIN = 1 }; /* flags */
#define MVN_BEADS_GROUP 32         /* beads per partial sum: part of the arithmetic */
MVN_API int mvn_extract_psf(int device, const void* raw, const mvn_stack_desc* raw_desc, const int src_dims[3],
                            const double* beads, int num_beads, const int psf_dims[3], int flags, float* psf_out,
                            double* scores_out, void* stream);
MVN_API int mvn_extract_memory(const mvn_stack_desc* raw_desc, const int src_dims[3], int num_beads,
                               const int psf_dims[3], int want_scores, int device, size_t* bytes);
MVN_API int mvn_extract_counters(long long out[3]);
MVN_API int mvn_extract_time(int device, int u16, const int src_dims[3], int num_beads, const int psf_dims[3], int reps,
                             float* ms);
/* ---- bead detection: a view's beads from its raw stack ----------------------------------------------------------------
 * mvn_detect_beads finds, on the device, the beads of ONE view's raw stack: the strict extrema of a difference of two
 * Gaussian blurs above a threshold, each with a quadratic sub-voxel fit.  Its positions are what mvn_extract_psf takes
 * as `beads`, so the chain is raw stack -> mvn_detect_beads -> mvn_extract_psf -> mvn_derive_kernels ->
 * mvn_deconvolve_resampled.
 *
 * Inputs.  `raw`, raw_desc, src_dims = m, `stream`, the device choice and their checks are exactly mvn_extract_psf's:
 * uint16 or float32, host or device memory, the stride rules of an input stack, raw_desc == NULL = dense float32 in
 * host memory; a stack in device memory is read where it lies, a stack in host memory is uploaded as it is into a
 * temporary.  prm: sigma1 and sigma2 per raw axis in raw voxels (finite, 0 <= sigma <= 10), a finite threshold, flags.
 * Outputs are HOST memory: *num_found; positions_out, capacity x 3 doubles (z, y, x) as raw indices - the layout of
 * mvn_extract_psf's `beads`; values_out, capacity floats, or NULL; voxels_out, capacity x 3 ints, or NULL.
 *
 * Arithmetic (normative).  Every float32 and double operation is rounded once, nothing is contracted into a fused
 * multiply-add.
 *   taps      for a sigma s, on the host in double: R = ceil(3 s); g_i = exp(-(double)(i i) / ((2 s) s)) for i = -R..R;
 *             S = ((g_{-R} + g_{-R+1}) + ...) + g_R, started from g_{-R} itself; w_i = (float)(g_i / S).  s = 0 gives
 *             R = 0 and w = {1}.  R <= MVN_DETECT_MAX_RADIUS.  mvn_detect_taps returns exactly these taps: taps[j] =
 *             w_{j-R} for j = 0..2R, *radius = R (an error, nothing written, when capacity < 2R + 1 or sigma is refused)
 *   blur      along axis k of a float32 volume u: v(x) = ((w_{-R} u(mir(x-R)) + w_{-R+1} u(mir(x-R+1))) + ...) +
 *             w_R u(mir(x+R)) - taps in ascending order, the sum started from the first product, everything float32;
 *             mir is mvn_extract_psf's mirror (numpy.pad's "reflect", any number of reflections, 0 for an extent of 1)
 *   volumes   L_a = the raw element widened to float32, blurred with sigma_a along axis 2, then axis 1, then axis 0
 *             (a = 1, 2); D = L_1 - L_2 in float32; E = D, or -D under MVN_DETECT_MINIMA
 *   candidate voxel c with 1 <= c_k <= m_k - 2 for every k, E(c) > threshold, and E(c) > E(n) for all 26 neighbours n:
 *             the comparisons are strict, so a plateau yields nothing and a NaN neighbour disqualifies.  A stack with
 *             an extent below 3 has no candidates, and that is no error (*num_found = 0, return value 0)
 *   order     candidates are returned in ascending raster index (c_0 m_1 + c_1) m_2 + c_2, whatever the schedule
 *   fit       in double on E widened, e_k the unit step along k, P = E(c + e_k), M = E(c - e_k):
 *             g_k = (P - M) / 2;  H_kk = (P + M) - 2 E(c);
 *             H_kl = ((E(c+e_k+e_l) - E(c+e_k-e_l)) - (E(c-e_k+e_l) - E(c-e_k-e_l))) / 4  (k < l; H is symmetric);
 *             the cofactors, each a difference of two products:
 *               C00 = H11 H22 - H12 H12   C01 = H02 H12 - H01 H22   C02 = H01 H12 - H02 H11
 *               C11 = H00 H22 - H02 H02   C12 = H01 H02 - H00 H12   C22 = H00 H11 - H01 H01
 *             the determinant along row 0: det = (H00 C00 + H01 C01) + H02 C02;
 *             n_0 = (C00 g_0 + C01 g_1) + C02 g_2,  n_1 = (C01 g_0 + C11 g_1) + C12 g_2,
 *             n_2 = (C02 g_0 + C12 g_1) + C22 g_2;  o_k = (-n_k) / det, that is o = -(adj(H) g) / det H.
 *             If det is zero or not finite, or any o_k is not finite, or any |o_k| > 1, then o = (0, 0, 0)
 *   result    position p_k = (double)c_k + o_k; value E(c); voxel c
 *
 * Capacity and errors.  The call blocks, checks everything before it touches anything and writes the outputs last.
 * *num_found is the number of candidates; if it exceeds `capacity` the call fails, writes *num_found ONLY, and the
 * message states the count (a caller calls again with that capacity).  Every other error returns < 0 with its message
 * in mvn_last_error() and leaves every output, *num_found included, untouched: mvn_extract_psf's errors for the stack
 * and its descriptor; a NULL raw, src_dims, prm, num_found or positions_out; a sigma that is negative, non-finite or
 * above 10; a non-finite threshold; an unknown flag bit; capacity < 1.
 *
 * mvn_detect_dog (test utility): D alone, dense float32 of extents m into HOST memory; three blur launches, no
 * extremum pass, no detection counted; prm's threshold and flags are checked and otherwise unused.
 * mvn_detect_memory: the device bytes mvn_detect_beads allocates, allocating nothing; it reads only raw_desc, the dims
 * and the capacity.  With n = m0 m1 m2:
 *   16 n               four float32 volumes: the blurs along axis 2 and along axis 1 of both sigmas; D reuses the first
 *   1536               the tap table: 2 blurs x 3 axes x 64 floats
 *   8 + 48 capacity    the candidate count; per candidate its raster index (8), position (24), value (4), voxel (12)
 *   the raw stack when it is in host memory: one element for strides {0, 0, 0}, n elements otherwise.
 * mvn_detect_counters, since process start: out[0] = launches of the blur passes (three per detection: one per axis),
 * out[1] = launches of the extremum pass (one per detection), out[2] = detections completed (mvn_detect_beads calls
 * that returned 0).  A stack with an extent below 3 completes a detection without a launch.
 * mvn_detect_time (test and bench utility): on a resident stack of src_dims (uint16 when u16 != 0, else float32) of
 * reproducible non-trivial values, `reps` repetitions between two stream events behind one that warms up: ms[0] = all
 * device work of a detection - the three blur passes, the extremum pass and the fit of the candidates a first run found
 * (at most 2^20; the list is not sorted here); ms[1] = the three blur passes alone; ms[2] = a plain copy of one float32
 * volume of src_dims.  out[0] moves by 3 + 6 (reps + 1), out[1] by 1 + (reps + 1), out[2] does not move.
 * Out of scope: a scale-space search over several sigmas; an iterative re-localisation that moves to a neighbouring
 * voxel; intensity normalisation of the raw stack; several views in one call; outputs in device memory; a mode of
 * mvn_set_kernel_derivation that detects by itself.  Matching the detections across views is mvn_register_beads. */
enum { MVN_DETECT_MINIMA = 1 }; /* flags */
#define MVN_DETECT_MAX_RADIUS 30
typedef struct mvn_detect_params {
  double sigma1[3], sigma2[3]; /* per raw axis, in raw voxels, finite, 0 <= sigma <= 10 */
  float threshold;             /* finite */
  int flags;
} mvn_detect_params;
MVN_API int mvn_detect_beads(int device, const void* raw, const mvn_stack_desc* raw_desc, const int src_dims[3],
                             const mvn_detect_params* prm, int capacity, int* num_found, double* positions_out,
                             float* values_out, int* voxels_out, void* stream);
MVN_API int mvn_detect_taps(double sigma, float* taps, int capacity, int* radius);
MVN_API int mvn_detect_dog(int device, const void* raw, const mvn_stack_desc* raw_desc, const int src_dims[3],
                           const mvn_detect_params* prm, float* dog_out);
MVN_API int mvn_detect_memory(const mvn_stack_desc* raw_desc, const int src_dims[3], int capacity, int device,
                              size_t* bytes);
MVN_API int mvn_detect_counters(long long out[3]);
MVN_API int mvn_detect_time(int device, int u16, const int src_dims[3], const mvn_detect_params* prm, int reps,
                            float* ms);
/* ---- bead registration: the matrix between two views from their beads ------------------------------------------------------
 * mvn_register_beads takes the beads of two views, A and B, as mvn_detect_beads returns them, and finds on the device
 * the affine matrix that maps an index of A to an index of B: geometric-descriptor matching of the two sets, RANSAC
 * over affine models of four pairs, and a least-squares refit.  It produces the one input of the chain that no other
 * call does, so the chain is raw stacks -> mvn_detect_beads -> mvn_register_beads -> mvn_view_geometry ->
 * mvn_extract_psf -> mvn_derive_kernels -> mvn_deconvolve_resampled.
 *
 * Inputs.  `a` and `b`: num_a x 3 and num_b x 3 doubles (z, y, x) in HOST memory, the layout of mvn_detect_beads'
 * positions_out; both counts in 5 .. MVN_REGISTER_MAX_BEADS; every coordinate finite.  prm: see the struct.
 * Outputs, HOST memory.  matrix_out: row-major 3 x 4, M, with b ~ M (a; 1).  With the block frame set to A's frame
 * shifted by the block origin o (block voxel x <-> index x + o of A), B's mvn_view_geometry matrix is M composed with
 * that shift - (L | L o + t) for M = (L | t) - and A's own matrix is the shift alone, (I | o).  *num_candidates: the
 * candidates of step 4.  *num_inliers: the inliers of the result.  pairs_out: NULL, or room for min(num_a, num_b) x 2
 * ints, receives the inlier pairs (i, j) in ascending i.  errors_out: NULL, or 2 doubles, the mean and the maximum
 * residual of the inliers in voxels of B.
 * No model is no error: the call returns 0, writes *num_candidates, sets *num_inliers = 0 and leaves the matrix, the
 * pairs and the errors untouched.
 *
 * Arithmetic (normative).  Every float32 and double operation is rounded once, nothing is contracted into a fused
 * multiply-add.
 *   1 prior       under MVN_REGISTER_PRIOR, T = prm->prior, on the host in double: a'_ik = ((T_k0 z + T_k1 y) + T_k2 x) +
 *                 T_k3 for a_i = (z, y, x); otherwise a' = a.  Steps 2 and 3 of A use a'; steps 5 to 7 use a
 *   2 neighbours  within one set (a', or b): D(i, j) = (dz dz + dy dy) + dx dx in double with d = p_j - p_i.  The
 *                 MVN_REGISTER_NEIGHBOURS = 4 nearest j != i (the index is excluded, not a zero distance), ordered by
 *                 (D, j) ascending: n_0 .. n_3.  mvn_register_neighbours returns them
 *   3 descriptors four per bead, of the neighbour triples (0,1,2), (0,1,3), (0,2,3), (1,2,3) in that order; each is the 9
 *                 values (float)(p_n - p_i), neighbour-major, z y x inside a neighbour: translation invariant.  Rotation
 *                 is the prior's job
 *   4 match       dist(u, v) = ((e_0 e_0 + e_1 e_1) + ...) + e_8 e_8 with e = u - v, in float32, started from the first
 *                 product; d(i, j) = the minimum over the 16 descriptor pairs of bead i of A and bead j of B (a NaN is
 *                 never a minimum).  For each i: j1 = the j of least d, the lower j on a tie, d1 = that distance; d2 =
 *                 the least d over j != j1.  i is a candidate iff d1 * ratio < d2, a float32 product and a strict
 *                 comparison: a lattice (d1 = d2 = 0) yields none.  A j claimed by more than one such i drops all of its
 *                 candidates.  Candidates (i, j1) are kept in ascending i; nC is their number.  nC < 4: no model.
 *                 mvn_register_candidates returns them with (d1, d2) per pair
 *   5 samples     mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, on
 *                 64-bit wrap-around arithmetic.  Draw q of hypothesis h over a range of size n:
 *                 u = mix(seed + 0x9E3779B97F4A7C15 * (16 h + q + 1)), r = ((u >> 32) * n) >> 32.  Hypothesis h takes
 *                 four distinct candidates by draws q = 0..3 over ranges nC - q; after each draw the earlier picks are
 *                 walked in ascending order and r is incremented for every pick <= r.  mvn_register_sample returns them
 *   6 hypothesis  in double; the four samples are (a_m, b_m), m = 0..3.  E has the columns a_1 - a_0, a_2 - a_0, a_3 - a_0
 *                 (E_kc = a_(c+1)k - a_0k) and F likewise from b.  The cofactors of E, each a difference of two products:
 *                   C00 = E11 E22 - E12 E21   C01 = E12 E20 - E10 E22   C02 = E10 E21 - E11 E20
 *                   C10 = E02 E21 - E01 E22   C11 = E00 E22 - E02 E20   C12 = E01 E20 - E00 E21
 *                   C20 = E01 E12 - E02 E11   C21 = E02 E10 - E00 E12   C22 = E00 E11 - E01 E10
 *                 det = (E00 C00 + E01 C01) + E02 C02;  L = (F adj E) / det:
 *                 L_kj = ((F_k0 C_j0 + F_k1 C_j1) + F_k2 C_j2) / det;
 *                 t_k = b_0k - ((L_k0 a_00 + L_k1 a_01) + L_k2 a_02).
 *                 The hypothesis scores 0 if det is zero or not finite or any entry of L or t is not finite; otherwise
 *                 its score is the number of candidates (a, b) with (r_0 r_0 + r_1 r_1) + r_2 r_2 <= max_error *
 *                 max_error, r_k = (((L_k0 a_0 + L_k1 a_1) + L_k2 a_2) + t_k) - b_k.  The best hypothesis has the
 *                 highest score, the lowest h on a tie; a best score < min_inliers: no model
 *   7 refit       on the host in double.  I_0 = the best hypothesis' inliers.  For r = 1 .. MVN_REGISTER_REFITS = 10, over
 *                 I_(r-1) in ascending candidate order: the centroids c_a, c_b (each coordinate summed from the first
 *                 element, then divided by the count); S_aa_kl = the sum of (a_k - c_ak)(a_l - c_al) and S_ba_kl = the
 *                 sum of (b_k - c_bk)(a_l - c_al), each started from the first product; L = (S_ba adj S_aa) / det S_aa
 *                 in the cofactor form of step 6 (E = S_aa, F = S_ba); t_k = c_bk - ((L_k0 c_a0 + L_k1 c_a1) + L_k2 c_a2).
 *                 A det that is zero or not finite, or a non-finite entry: no model.  I_r = the inliers of step 6's
 *                 rule under this model; |I_r| < min_inliers: no model; stop when I_r == I_(r-1).  The result is the last
 *                 model, M = (L | t), and the last I_r; the errors are the mean (summed in order from the first, then
 *                 divided by the count) and the maximum of sqrt of the inliers' squared residuals under that model
 *
 * Errors.  The call blocks, checks everything before it touches anything and writes the outputs last.  Every error
 * returns < 0 with its message in mvn_last_error() and leaves every output untouched: a NULL a, b, prm, matrix_out,
 * num_candidates or num_inliers; a count out of range; a non-finite coordinate, or a non-finite prior entry under the
 * flag; a ratio that is not finite or below 1; a max_error that is not finite or not positive; hypotheses outside
 * 1 .. MVN_REGISTER_MAX_HYPOTHESES; min_inliers < 4; an unknown flag bit; a bad device.  `stream` is accepted for
 * symmetry with the other calls; the inputs are host memory, so nothing is waited for.
 *
 * mvn_register_neighbours (test utility): step 2 on one set p of n points, idx_out n x 4 ints.
 * mvn_register_candidates (test utility): steps 1 to 4; *num candidates into pairs_out, min(num_a, num_b) x 2 ints,
 * and d_out, min(num_a, num_b) x 2 floats (d1, d2); it reads prm's prior, flags and ratio and checks all of prm.
 * mvn_register_sample: the sample of step 5, host only; n >= 4, 0 <= h < MVN_REGISTER_MAX_HYPOTHESES.
 * mvn_register_memory: the device bytes mvn_register_beads allocates, allocating nothing.  With n = num_a + num_b,
 * tiles = ceil(num_b / 64), c = min(tiles, ceil(1024 / ceil(num_a / 256))), chunk = 64 ceil(tiles / c) beads of B and
 * chunks = ceil(num_b / chunk):
 *   184 n                     per bead its position (24), neighbours (16) and descriptors (144)
 *   12 num_a (chunks + 1)     (d1, j1, d2) per bead of A and chunk, and folded
 *   48 min(num_a, num_b)      the candidate records (a, b)
 *   8                         the best (score, h)
 * `hypotheses` is checked and does not enter: a hypothesis lives in registers.
 * mvn_register_counters, since process start: out[0] = launches of the match pass, out[1] = launches of the RANSAC
 * pass, out[2] = registrations completed (mvn_register_beads calls that returned 0, no model included).  A call with
 * nC < 4 launches no RANSAC pass.
 * mvn_register_time (test and bench utility): on reproducible synthetic sets (num_a points in a box, B = the first
 * num_b of them under a small affine map, cyclically when num_b > num_a), `reps` repetitions between two stream events
 * behind one that warms up: ms[0] = the neighbour and descriptor pass of both sets; ms[1] = the match pass and its
 * fold; ms[2] = the RANSAC pass of `hypotheses` hypotheses over min(num_a, num_b) candidate records (pair i with i).
 * out[0] and out[1] move by reps + 1 each, out[2] does not move.
 * Out of scope: a global optimisation over more than two views; rotation-invariant descriptors; rigid or
 * translation-only models; bead lists in device memory; a mode of the resampled call that registers by itself;
 * anisotropy calibration (the caller composes it into the prior). */
enum { MVN_REGISTER_PRIOR = 1 }; /* flags */
#define MVN_REGISTER_NEIGHBOURS 4 /* part of the arithmetic */
#define MVN_REGISTER_REFITS 10    /* part of the arithmetic */
#define MVN_REGISTER_MAX_BEADS 65536
#define MVN_REGISTER_MAX_HYPOTHESES (1 << 24)
typedef struct mvn_register_params {
  double prior[12];        /* row-major 3 x 4, read only under MVN_REGISTER_PRIOR */
  double max_error;        /* inlier bound, in voxels of B; finite, > 0 */
  float ratio;             /* finite, >= 1 */
  int hypotheses;          /* 1 .. MVN_REGISTER_MAX_HYPOTHESES */
  int min_inliers;         /* >= 4 */
  int flags;
  unsigned long long seed;
} mvn_register_params;
MVN_API int mvn_register_beads(int device, const double* a, int num_a, const double* b, int num_b,
                               const mvn_register_params* prm, double matrix_out[12], int* num_candidates,
                               int* num_inliers, int* pairs_out, double* errors_out, void* stream);
MVN_API int mvn_register_neighbours(int device, const double* p, int n, int* idx_out);
MVN_API int mvn_register_candidates(int device, const double* a, int num_a, const double* b, int num_b,
                                    const mvn_register_params* prm, int* num, int* pairs_out, float* d_out);
MVN_API int mvn_register_sample(unsigned long long seed, int h, int n, int out[4]);
MVN_API int mvn_register_memory(int num_a, int num_b, int hypotheses, size_t* bytes);
MVN_API int mvn_register_counters(long long out[3]);
MVN_API int mvn_register_time(int device, int num_a, int num_b, int hypotheses, int reps, float* ms);
/* out[0] = divide passes launched on a uint16 image, out[1] = ingest passes that wrote a uint16 volume, since process start */
MVN_API int mvn_image_storage_counters(long long out[2]);
/* Padding policy of inplace_gpu_deconvolve for the calls that follow (process-wide): "zero"
 * (default: the reference GPU entry's zero_padd with FFT-friendly padded extents), "zero_exact"
 * (exactly image + kernel - 1), "none" (the reference CPU path's cyclic no_padd), "reflect" (the volume, offset
 * and guard of "zero", the margins around image, weights and psi holding the stack's mirror image instead of zeros);
 * NULL or "" returns to the environment variable MVN_PAD_MODE / the default.  See multiviewnative.h. */
MVN_API int mvn_set_pad_mode(const char* mode);
/* The mode last selected with mvn_set_pad_mode ("zero" | "zero_exact" | "none" | "reflect"), or "" when the
 * environment / default decides -- what a caller that switches the policy for one call restores. */
MVN_API const char* mvn_get_pad_mode(void);
/* Memory mode of inplace_gpu_deconvolve / mvn_deconvolve_submit for the calls that follow (process-wide):
 *   "resident" (default)  every stack on the device; a call whose stacks do not fit is refused ("memory
 *                         constraints"), as in the reference's all-on-device branch (src/multiviewnative.cu:94-140)
 *   "auto"                resident when the exact need (mvn_deconvolve_memory with 0 streamed views) fits; otherwise
 *                         the fewest views whose image and weights stacks stay in host memory and cross PCIe into a
 *                         ring of 2 (else 1) device slots for every view update, under the compute of the other
 *                         views -- the reference's min-memory interleaved branch.  Refused only when not even every
 *                         view streamed with one slot fits.
 *   "stream"              every view streamed (the smallest footprint)
 *   "stream:N"            exactly N views streamed (clamped to the view count), ring as in auto; for tests and
 *                         measurements (auto never streams a single view: with one slot that costs what
 *                         resident does)
 * Results are those of the resident call, bit for bit.  NULL or "" returns to the default.  MVN_DEVICES calls
 * (multiviewnative.h) are not affected. */
MVN_API int mvn_set_memory_mode(const char* mode);
/* the mode last selected with mvn_set_memory_mode, or "" when the environment / default decides */
MVN_API const char* mvn_get_memory_mode(void);
/* Caps the device memory the auto / stream planner may use: min(free memory, bytes).  bytes <= 0 removes the
 * cap.  Ignored in resident mode. */
MVN_API int mvn_set_memory_budget(long long bytes);
/* Device bytes a call of inplace_gpu_deconvolve with this workspace allocates on a new engine when
 * `streamed_views` of its views are streamed (0 = resident; > 0 with a ring of 2 slots: a ring of 1 slot needs
 * bytes(1) - bytes(0) less), under the padding policy in force.  Takes the call's own padding and PSF form
 * decisions, allocates nothing; only the dims members of the views are read.  For sizing blocks. */
MVN_API int mvn_deconvolve_memory(struct workspace input, int device, int streamed_views, size_t* bytes);
/* out[0] = calls that streamed views, out[1] = streamed view updates, out[2] = bytes streamed host -> device,
 * all since process start */
MVN_API int mvn_stream_counters(long long out[3]);
/* Convergence of the Richardson-Lucy loop.  For sweep k (one update of every view), over the voxels returned to
 * the caller (the stacks' window inside the padded volume; the whole volume under padding "none" and through the
 * engine API), differenced in float and summed in double:
 *   S_k = sum over the V view updates and voxels of |psi_after - psi_before|,  M_k = max of the same,
 *   P_k = sum of psi_after;  r_k = S_k / P_k, the mean relative L1 change per view update.
 * tolerance < 0: off (default; no statistics, kernels and results as without this switch); 0: statistics of
 * every sweep, all num_iterations_ run; > 0: also stop after the first sweep k with r_k <= tolerance (psi is then
 * the estimate after k sweeps).  A NaN makes r_k NaN, which never stops the loop.  Process-wide, captured by
 * inplace_gpu_deconvolve and mvn_deconvolve_submit at their start.  Multi-device calls (MVN_DEVICES) with
 * statistics on run on one device. */
MVN_API int mvn_set_convergence(double tolerance);   /* < 0 off (default), 0 statistics only, > 0 stop at r_k <= t */
MVN_API int mvn_get_convergence(double* tolerance);
/* Statistics of the last deconvolution this THREAD completed: inplace_gpu_deconvolve, or mvn_deconvolve_wait of
 * its ticket.  *iterations_run = sweeps actually run; stats[3k..3k+2] = {S_k, M_k, P_k} for
 * k < min(capacity, rows); returns the number of rows available (0 when statistics were off), < 0 on error. */
MVN_API int mvn_last_convergence(int* iterations_run, double* stats, int capacity);
/* Acceleration of the Richardson-Lucy loop by vector extrapolation between sweeps (Biggs & Andrews 1997, first
 * order).  With x_k the result of sweep k and y_{k-1} the estimate it started from (x_0 = y_0 = psi as handed in):
 *   g_k = x_k - y_{k-1},   a_k = clamp(sum g_k g_{k-1} / sum g_{k-1} g_{k-1}, 0, 1)  (a_1 = 0; sums in double over
 *   the engine's volume - the padded one under "zero" / "zero_exact"; 0 for an empty or non-finite ratio),
 *   y_k = max(x_k + a_k (x_k - x_{k-1}), minValue)  (float32; y_1 = x_1),
 * and sweep k + 1 starts from y_k.  No extrapolation follows the last sweep run: psi is always a sweep's own
 * result x_k, so 1 or 2 iterations give the bits of the plain loop.  Convergence statistics keep their meaning (r_k
 * is measured inside sweep k) and the tolerance stop works as without acceleration.  The loop needs three more
 * volumes for the duration of the call (mvn_deconvolve_memory and the "auto" planner count them) and two streaming
 * passes per sweep.  mode 0: off (default; launches and results as without this switch); 1: on; anything else is an
 * error.  Process-wide, captured by inplace_gpu_deconvolve, mvn_deconvolve_submit and mvn_deconvolve_described at
 * their start.  Multi-device calls (MVN_DEVICES) with acceleration on run on one device. */
MVN_API int mvn_set_acceleration(int mode);
MVN_API int mvn_get_acceleration(int* mode);
/* The last deconvolution this THREAD completed (as mvn_last_convergence): alphas[k - 1] = a_k for the sweeps run,
 * k - 1 < min(capacity, rows); the entry of the last sweep run is 0 (nothing followed it).  Returns the number of
 * rows available (0 when acceleration was off), < 0 on error. */
MVN_API int mvn_last_acceleration(double* alphas, int capacity);
/* The regulariser of the Richardson-Lucy loop.  MVN_REG_TIKHONOV (default; epsilon ignored): workspace.lambda_ > 0
 * selects the reference's Tikhonov branch, launches and results as without this switch.  MVN_REG_TV: total
 * variation (Dey et al. 2006) - workspace.lambda_ is the TV weight, the Tikhonov branch is off, and the update of
 * view v becomes
 *   psi <- w_v * (next(psi, integral_v * t) - psi) + psi,      t = 1 / (1 - lambda * div(grad psi / |grad psi|_eps))
 * with `next` the clamp chain of the plain loop and t computed from psi as it stands before this view's update.
 * All arithmetic is float32 without contraction, every operation correctly rounded, on the engine's volume (the
 * padded one under "zero" / "zero_exact"), every axis cyclic at the extent of that volume.  For voxel (z, y, x),
 * u = psi:
 *   gz = u[z+1,y,x] - u    gy = u[z,y+1,x] - u    gx = u[z,y,x+1] - u
 *   m  = sqrt(((gx*gx + gy*gy) + gz*gz) + e2)          e2 = (float)epsilon * (float)epsilon
 *   r  = 1.0f / m          px = gx*r   py = gy*r   pz = gz*r
 *   dv = ((px - px[x-1]) + (py - py[y-1])) + (pz - pz[z-1])
 *   t  = 1.0f / (1.0f - (float)lambda * dv)
 * An extent of 1 along an axis makes that neighbour the voxel itself; the row padding of an odd last extent is never
 * read as a neighbour and never written.  |p| <= 1, so |dv| <= 6: a call with TV on and lambda_ >= 1/12 is refused
 * (error, psi untouched), which keeps 1 - lambda dv > 0.5 with no clamp in the kernel.  lambda_ == 0 with TV on is
 * the plain loop: no TV launch, the plain loop's bits.  A non-finite t reaches `next` as a NaN value and becomes
 * minValue through the clamp chain.  One more volume (t) is held while TV is on and lambda_ > 0; mvn_deconvolve_memory
 * and the "auto" planner count it.  Kind 1 needs a finite epsilon > 0; any other kind is an error.  Process-wide,
 * captured by inplace_gpu_deconvolve, mvn_deconvolve_submit and mvn_deconvolve_described at their start.
 * Multi-device calls (MVN_DEVICES) with TV on run on one device. */
enum { MVN_REG_TIKHONOV = 0, MVN_REG_TV = 1 };
MVN_API int mvn_set_regularization(int kind, double epsilon);
MVN_API int mvn_get_regularization(int* kind, double* epsilon);
/* The noise model of the Richardson-Lucy loop: a camera background per view, and the per-sweep likelihood.  An sCMOS
 * frame is Poisson(H psi) + offset; with a background the offset is carried in the forward model instead of being
 * deconvolved as light.  For view v, with `x` the inverse-transform output times `scale`, `b = background[v]` and `y`
 * the image voxel widened to float32:
 *   m = x + b        (float32, one correctly rounded add, never contracted with the multiply by scale;
 *                     with b == 0 the add is NOT performed: m = x, -0 stays -0)
 *   q = quotient_g(y, m, guard)                      (the existing quotient, unchanged)
 *   term = y > 0 ? (y * logf(q) - y) + m : m - y     (float32, no contraction; q is the value written)
 * Per (sweep k, view v) the statistics are summed in double over the voxels handed back to the caller - the stacks'
 * window inside the padded volume; the whole volume under "none" and through the engine API:
 *   D_kv = sum term      Y_kv = sum y      M_kv = sum m
 * D is the Poisson negative log-likelihood of the estimate up to a constant (Csiszar's I-divergence).  The statistics
 * are unweighted.  A NaN anywhere makes D_kv NaN (a poisoned convolution therefore gives NaN).  D_kv is measured
 * against psi as it stands before view v's update of sweep k.
 * mvn_set_background: count 0 or NULL: off (default); 1: the value for every view; otherwise a call whose num_views_
 * != count is refused, psi untouched.  Values finite and >= 0, else error.  mvn_set_likelihood: 0 off (default),
 * 1 on, else error.  With every background 0 and the likelihood off the loop is the plain one, launches and bits;
 * otherwise the divide pass runs its noise-model form (the statistics are always summed then), the records are
 * counted by mvn_deconvolve_memory* and the "auto" planner, the call waits for its rows, and no captured sweep graph
 * (MVN_GRAPH) is used.  Process-wide, captured by inplace_gpu_deconvolve, mvn_deconvolve_submit and
 * mvn_deconvolve_described at their start, like mvn_set_regularization.  Multi-device calls (MVN_DEVICES) with
 * either switch on run on one device. */
MVN_API int mvn_set_background(const float* values, int count);
MVN_API int mvn_get_background(float* values, int capacity); /* returns count */
MVN_API int mvn_set_likelihood(int mode);
MVN_API int mvn_get_likelihood(int* mode);
/* The last deconvolution this THREAD completed (as mvn_last_convergence): stats[3 * (k * V + v) ..] = {D, Y, M} of
 * sweep k, view v, for the sweeps run (a tolerance stop of mvn_set_convergence ends them early), k * V + v <
 * min(capacity_rows, rows); *num_views = V.  Returns the rows available (0 when both switches were off), < 0 on error. */
MVN_API int mvn_last_likelihood(int* iterations_run, int* num_views, double* stats, int capacity_rows);
/* Test and bench utilities of the TV pass.  mvn_tv_factor: t of the dense host volume psi[dims] into the dense host
 * volume t.  mvn_tv_time: ms[0] = milliseconds per launch of the pass on a resident volume of these extents (`reps`
 * launches between two stream events), ms[1] = the same for a plain streaming copy of the volume (one read, one
 * write).  mvn_tv_launch_count: launches of the pass since process start. */
MVN_API int mvn_tv_factor(int device, const int dims[3], const float* psi, double lambda, double epsilon, float* t);
MVN_API int mvn_tv_time(int device, const int dims[3], int reps, float* ms);
MVN_API long mvn_tv_launch_count(void);
/* Padding policy "reflect".  Volume voxel (z, y, x) of image, weights and psi holds the stack's voxel
 * (f(z - o0, n0), f(y - o1, n1), f(x - o2, n2)), o the window's offset (kernel - 1) / 2, n the stack's extents and
 *     f(i, n):  m = i mod 2n (non-negative);  f = m < n ? m : 2n - 1 - m
 * (whole-sample symmetric extension, numpy.pad's "symmetric"; the row padding of an odd last extent stays zero).  The
 * margins are filled in place behind whatever placed the stack, one launch per axis that has a margin; nothing else
 * about the call differs from "zero" (extents, memory, the window of the statistics).  Such a call runs on one device.
 * mvn_reflect_counters: out[0] = launches of the fill, out[1] = volumes filled, since process start.
 * mvn_reflect_time (test and bench utility): ms[0] = milliseconds per fill (all its launches) of a resident volume of
 * extents ext around a window of extents dims at offset off, float32 or (u16 != 0) uint16, `reps` fills between two
 * stream events; ms[1] = the same for a plain streaming copy of that volume (one read, one write). */
MVN_API int mvn_reflect_counters(long long out[2]);
MVN_API int mvn_reflect_time(int device, const int dims[3], const int ext[3], const int off[3], int u16, int reps,
                             float* ms);
/* A resident engine keeps, per view slot, the PSF spectra of the last call together with host
 * copies of the kernels they were made from; a call (or mvn_engine_set_view) that brings
 * bytewise identical kernels for a slot re-uses the spectra (the reference's
 * GPU path recomputes them for every view and iteration, inc/gpu_convolve.cuh:121-124).
 * MVN_PSF_CACHE=0 disables it.  out[0] = spectra re-used, out[1] = spectra prepared, both since
 * process start. */
MVN_API int mvn_psf_cache_counters(long out[2]);
/* passes launched through the long-line (16-column, split-window) kernels since process start
 * (test / diagnostics) */
MVN_API long mvn_split_launch_count(void);
/* launches of the fused middle pass (dim1 forward + direct dim0 leg + dim1 inverse in one pass over the line layout;
   csrc/mvn_mid_fused.hpp) since process start: tests check that the shapes that have it take it */
MVN_API long mvn_mid_fused_launch_count(void);
/* inplace_gpu_deconvolve calls that ran as dim0 slabs on the devices of MVN_DEVICES (multiviewnative.h) since
 * process start - a call that could not be cut that way ran on one device and is not counted */
MVN_API long mvn_multi_device_calls(void);

/* ---- plan_store (inc/plan_store.cuh: get()/add/has_key/empty/size/clear) ---------------- */
MVN_API int mvn_plan_store_add(int device, const int dims[3]);
MVN_API int mvn_plan_store_has_key(int device, const int dims[3]); /* 1 / 0 */
MVN_API int mvn_plan_store_size(void);
MVN_API int mvn_plan_store_empty(void);
MVN_API int mvn_plan_store_clear(void);
/* layout facts of a shape: {h, C, RP, even, rows_T, ax1_T, ax0_T, n_stages(d2 axis),
 * fixed-length kernel used for the last-axis / dim1 / dim0 passes (1/0 each), reserved} */
MVN_API int mvn_plan_describe(int device, const int dims[3], int out[12]);

/* ---- whole 3-D transforms on host buffers (test/bench utility) --------------------------
 * real:  dense [d0][d1][d2] floats.  spec: [d0][d1][d2/2+1] complex64 in the FFTW/cuFFT
 * in-place order (inc/image_stack_utils.h:24-42).  Un-normalised both ways. */
MVN_API int mvn_fft3_r2c(int device, const int dims[3], const float* real, float* spec);
MVN_API int mvn_fft3_c2r(int device, const int dims[3], const float* spec, float* real);
/* times `reps` forward (direction 0) or backward (1) transforms of a resident volume with
 * stream events; returns average milliseconds per transform in *ms */
MVN_API int mvn_fft3_time(int device, const int dims[3], int direction, int reps, float* ms);
/* same, plus the average launch time of every kernel kind (array of mvn_kernel_kind_count()) */
MVN_API int mvn_fft3_profile(int device, const int dims[3], int direction, int reps, float* ms,
                             double* per_kind_ms);

/* Batched transforms, the counterpart of the cufftPlanMany path of the reference's
 * bench/bench_gpu_many_nd_fft.cu:403-463: `batch` stacks of one shape, contiguous in `real`
 * ([batch][d0][d1][d2]), go through ONE cached plan back to back on one stream; `spec` receives
 * [batch][d0][d1][d2/2+1] complex64 in natural bin order. */
MVN_API int mvn_fft3_many_r2c(int device, const int dims[3], int batch, const float* real,
                              float* spec);
/* resident timing of the same sweep over `batch` stacks (direction 0 forward, 1 backward):
 * *ms = average milliseconds per sweep over the batch, stacks already in HBM */
MVN_API int mvn_fft3_many_time(int device, const int dims[3], int batch, int direction, int reps,
                               float* ms);

/* ---- resident RL engine ----------------------------------------------------------------- */
MVN_API int mvn_engine_create(int device, const int dims[3], int num_views, mvn_engine** out);
MVN_API int mvn_engine_destroy(mvn_engine* e);
MVN_API int mvn_engine_set_view(mvn_engine* e, int v, const float* image, const float* weights,
                                const float* kernel1, const int k1dims[3], const float* kernel2,
                                const int k2dims[3]);
MVN_API int mvn_engine_set_psi(mvn_engine* e, const float* psi);
MVN_API int mvn_engine_get_psi(mvn_engine* e, float* psi);
/* The same three for described stacks (mvn_stack_desc above; a NULL descriptor = dense float32 in host memory).  The
 * set_* calls return once the source has been consumed (the caller may free or overwrite it); `stream` as in
 * mvn_call_desc.  Stacks in device memory must be on the engine's device.  get_psi blocks. */
MVN_API int mvn_engine_set_view_described(mvn_engine* e, int v, const void* image, const mvn_stack_desc* image_desc,
                                          const void* weights, const mvn_stack_desc* weights_desc,
                                          const float* kernel1, const int k1dims[3],
                                          const float* kernel2, const int k2dims[3], void* stream);
MVN_API int mvn_engine_set_psi_described(mvn_engine* e, const void* psi, const mvn_stack_desc* d, void* stream);
MVN_API int mvn_engine_get_psi_described(mvn_engine* e, void* psi, const mvn_stack_desc* d);
/* A resampled view (mvn_view_geometry above): `image` is the RAW stack, image_desc describes it over geom->src_dims
 * (NULL: dense float32 in host memory); the engine's extents are the block's.  weights: a stack of the block's extents
 * as in mvn_engine_set_view_described, or NULL - the view's weights are then computed from the geometry,
 * UNNORMALISED: call mvn_engine_normalize_weights once after the last view has been set (it divides the weights of
 * every view of the engine by their sum, in view order, and blocks).  The image is held as float32 whatever
 * mvn_set_image_storage says.  An engine with a halo hook refuses both. */
MVN_API int mvn_engine_set_view_resampled(mvn_engine* e, int v, const void* image, const mvn_stack_desc* image_desc,
                                          const mvn_view_geometry* geom, const void* weights,
                                          const mvn_stack_desc* weights_desc, const float* kernel1, const int k1dims[3],
                                          const float* kernel2, const int k2dims[3], void* stream);
MVN_API int mvn_engine_normalize_weights(mvn_engine* e);
/* psi <- the fusion F of mvn_fuse_resampled (above) of the views as the engine holds them: s_v from its image volumes,
 * w_v from its weights volumes as they stand (before mvn_engine_normalize_weights: the unnormalised computed weights),
 * `fill` where no weight is positive; margins as mvn_engine_set_psi leaves them.  Blocking.  Refused - psi is left as it
 * was - by an engine with a halo hook, with streamed views, or with a uint16 image volume, and for a non-finite fill. */
MVN_API int mvn_engine_fuse_psi(mvn_engine* e, float fill);
/* enqueue `iterations` sequential (Gauss-Seidel) sweeps over the views */
MVN_API int mvn_engine_iterate(mvn_engine* e, int iterations, double lambda, float min_value);
/* resident engine, blocking: stats receives 3 doubles per iteration run ({S_k, M_k, P_k} over the whole volume,
 * see mvn_set_convergence; tolerance as there, < 0 collects nothing) */
MVN_API int mvn_engine_iterate_converge(mvn_engine* e, int iterations, double lambda, float min_value,
                                        double tolerance, int* iterations_run, double* stats);
/* resident engine, blocking: `iterations` sweeps with the extrapolation of mvn_set_acceleration between them.
 * tolerance, *iterations_run and stats as in mvn_engine_iterate_converge; alphas receives one double per sweep run
 * (a_k, the last one 0).  stats and alphas may be NULL.  Refused by an engine in halo mode (a slab of a group). */
MVN_API int mvn_engine_iterate_accelerated(mvn_engine* e, int iterations, double lambda, float min_value,
                                           double tolerance, int* iterations_run, double* stats, double* alphas);
/* the regulariser (mvn_set_regularization) of the mvn_engine_iterate* calls that follow on this engine.  Refused by
 * an engine in halo mode; mvn_engine_set_halo_hook and mvn_engine_compute_delta* are errors on a TV engine. */
MVN_API int mvn_engine_set_regularization(mvn_engine* e, int kind, double epsilon);
/* the noise model (mvn_set_background, mvn_set_likelihood) of the mvn_engine_iterate* calls that follow on this
 * engine: background = one value per view, or NULL for none; likelihood 0 / 1.  Refused by an engine in halo mode;
 * mvn_engine_set_halo_hook and mvn_engine_compute_delta* are errors on an engine in the mode (a background != 0 or the
 * likelihood on).  mvn_engine_last_likelihood drains the stream and hands out the rows of the last iterate call as
 * mvn_last_likelihood does (rows of V views each); returns the rows available. */
MVN_API int mvn_engine_set_noise_model(mvn_engine* e, const float* background, int likelihood);
MVN_API int mvn_engine_last_likelihood(mvn_engine* e, int* iterations_run, double* stats, int capacity_rows);
/* simultaneous (Jacobi) mode, one step: delta = sum_v w_v (next_v - psi) over this engine's
 * views; the caller all-reduces the delta buffer across ranks, then applies it */
MVN_API int mvn_engine_compute_delta(mvn_engine* e, double lambda, float min_value);
MVN_API int mvn_engine_apply_delta(mvn_engine* e);
/* The same step in pieces, so that the all-reduce runs under the compute.  The
 * correction leaves the LAST pass of the last local view and is consumed by plane-local passes
 * (psi += delta, then the forward last-axis and dim1 passes of the next step), so both ends go
 * chunk by chunk over ranges of dim0 planes:
 *   n = mvn_engine_delta_chunks(e, wanted)        (<= wanted; tile alignment of the shape)
 *   mvn_engine_compute_delta_head(e, lambda, minValue)
 *   for c in 0..n-1: mvn_engine_compute_delta_chunk(e, c, n); start all-reduce of floats
 *                    [first, first + count) of the delta buffer (mvn_engine_delta_chunk_range)
 *   for c in 0..n-1: wait for chunk c's all-reduce; mvn_engine_apply_delta_chunk(e, c, n, feed_next)
 * feed_next != 0 also leaves psi's transformed spectrum for the next _head call (another step
 * follows).  Everything is asynchronous on mvn_engine_stream(); an engine created with 0 views
 * contributes zeros (a rank without views still holds a replica of psi). */
MVN_API int mvn_engine_delta_chunks(mvn_engine* e, int wanted);
MVN_API int mvn_engine_delta_chunk_range(mvn_engine* e, int c, int n, size_t* first_float,
                                         size_t* n_floats);
MVN_API int mvn_engine_compute_delta_head(mvn_engine* e, double lambda, float min_value);
MVN_API int mvn_engine_compute_delta_chunk(mvn_engine* e, int c, int n);
MVN_API int mvn_engine_apply_delta_chunk(mvn_engine* e, int c, int n, int feed_next);
MVN_API int mvn_engine_delta_ptr(mvn_engine* e, void** dev_ptr, size_t* n_floats);
/* make the engine write its delta into caller-owned DEVICE memory (same size as the engine's
 * own buffer) so a collective library can reduce it in place; NULL restores the internal one */
MVN_API int mvn_engine_bind_delta(mvn_engine* e, void* dev_ptr);
/* Halo mode: one volume cut into dim0 slabs over several ranks, swept in the REFERENCE's view order
 * (src/multiviewnative.cpp:194-227) - the engine's volume is this rank's planes plus h = (deepest PSF) / 2 halo
 * planes either side (image 1, weights 0, psi anything there).  `fn(user, spectrum, view, conv)` is called on the
 * calling thread right before every convolution's dim0 leg, with the engine's stream drained: it must fill planes
 * [0, h) and [d0 - h, d0) of `spectrum` ([d0][d1][d2/2] complex, DEVICE memory) with the lower neighbour's last
 * and the upper neighbour's first h own planes; mvn_engine_copy_planes moves whole planes between `spectrum` and
 * an exchange buffer (to_buffer bit 0: spectrum -> buffer; bit 1: the buffer is HOST memory; bit 2: only enqueue the
 * copy on the engine's stream, do not wait for it).  Every PSF must have
 * at most 33 planes (direct dim0 leg); NULL switches the mode off.  drain == 0: `fn` is called WITHOUT waiting for the
 * stream and must order everything it does on mvn_engine_stream() itself (copies with bit 2, collectives issued with
 * that stream current): the host then never waits inside a sweep.  libmultiviewnative_amd/sharded.py drives it. */
MVN_API int mvn_engine_set_halo_hook(mvn_engine* e, void (*fn)(void* user, void* spectrum, int view, int conv),
                                     void* user, int drain);
MVN_API int mvn_engine_copy_planes(mvn_engine* e, void* spectrum, int plane0, int nplanes, void* buffer,
                                   int to_buffer);
/* After mvn_engine_set_halo_hook: the first and last `planes` planes of the engine's volume are halo planes that no
 * pass needs to compute - the last-axis and dim1 passes and the dim0 leg then run on the own planes only (a slab of
 * 64 + 2 x 15 planes does the work of 64, not of 94).  split != 0: the leg runs in two parts - first the own planes
 * that do not depend on the halos - and fn is called once more in between, with conv + 4: the halo planes have to be
 * in place (in stream order) only when THAT call returns, so an exchange started at the first call on another
 * stream runs beside the first part (mvn_multi.cpp does that; sharded.py passes 0). */
MVN_API int mvn_engine_set_halo_planes(mvn_engine* e, int planes, int split);
/* 1 / 0: would this engine hold a kernel of these extents in the direct dim0 form (which halo mode needs)?
 * Lets a driver refuse a PSF when it is handed over instead of failing inside the first sweep. */
MVN_API int mvn_engine_would_be_direct(mvn_engine* e, const int kdims[3]);
/* Non-finite values in halo mode.  An FFT-based convolution turns ONE Inf / NaN voxel of its input into a volume of
 * NaN (inc/cpu_convolve.h:256-268), which the update then clamps to minValue everywhere (inc/cpu_kernels.h:40-47,
 * 76-83).  The direct dim0 leg reproduces that through a 4-byte device word per engine, the "poison word": a leg
 * that met a non-finite input stores its epoch (the engine's count of direct legs, so the word never needs clearing)
 * there and the last-axis pass that ends the convolution turns every voxel into NaN when it finds the epoch of its
 * own convolution.  Slabs of one volume on several engines must agree: with bit 1 of `drain` set in
 * mvn_engine_set_halo_hook the hook is called a second time per convolution, right after the dim0 leg and the dim1
 * pass behind it have been enqueued, with conv + 2, and must leave the MAXIMUM of all slabs' words in every slab's
 * word before it returns / in stream order (epochs only grow and the slabs count in step: the maximum is the latest
 * report).  _ptr: the word's device address; _bind: make the engine use caller-owned device memory (4 bytes, zeroed;
 * NULL: back to its own) so that a collective can reduce it in place; _get drains the stream and reads the word;
 * _merge: word = max(word, value). */
MVN_API int mvn_engine_poison_ptr(mvn_engine* e, void** dev_ptr);
MVN_API int mvn_engine_bind_poison(mvn_engine* e, void* dev_ptr);
MVN_API int mvn_engine_poison_get(mvn_engine* e, unsigned* value);
MVN_API int mvn_engine_poison_merge(mvn_engine* e, unsigned value);
MVN_API int mvn_engine_psi_ptr(mvn_engine* e, void** dev_ptr, size_t* n_floats);
MVN_API int mvn_engine_stream(mvn_engine* e, void** hip_stream);
MVN_API int mvn_engine_sync(mvn_engine* e);
/* wall time of `iterations` sweeps measured with events on the engine stream */
MVN_API int mvn_engine_time_iterate(mvn_engine* e, int iterations, double lambda,
                                    float min_value, float* ms);
/* per-kernel event timing: enable (1 = every launch, n > 1 = the launches of every n-th
 * (view, iteration) only, which keeps the events' own cost below 1 %), run, then read totals.
 * kind indexes mvn_kernel_kind_name */
MVN_API int mvn_engine_profile(mvn_engine* e, int enable);
MVN_API int mvn_engine_profile_read(mvn_engine* e, int kind, double* total_ms, long* launches);
MVN_API int mvn_kernel_kind_count(void);
MVN_API const char* mvn_kernel_kind_name(int kind);
/* algorithmic bytes B = 4*d0*d1*2(d2/2+1) of the engine's shape */
MVN_API size_t mvn_engine_B(mvn_engine* e);

/* ---- one volume on several devices of ONE process (what MVN_DEVICES runs inside inplace_gpu_deconvolve) ------
 * The volume is cut into slabs of dim0 planes, one per entry of `devices` (an entry may repeat: two slabs on one
 * device), each an ordinary resident engine on its planes plus `halo_planes` = (deepest PSF) / 2 halo planes either
 * side, each driven by its own host thread; before every dim0 leg a slab pulls its neighbours' boundary planes with
 * peer copies (cyclically: the reference's convolution is cyclic), under the part of the leg that does not need them.
 * The sweep is the reference's view-after-view order (src/multiviewnative.cpp:194-227): results equal the
 * one-device engine's bit for bit.  Needs PSFs of at most 33 planes (direct dim0 leg), an even last extent, at least
 * halo_planes planes per slab, at most 8 slabs.  No communication library: events and hipMemcpyPeerAsync.
 *   mvn_group_create -> mvn_group_load (psi and the workspace's stacks, extents == dims, uploaded slab by slab)
 *   -> mvn_group_iterate (blocking; *ms = wall time of the sweeps, stacks resident) -> mvn_group_get_psi */
typedef struct mvn_group mvn_group; /* opaque */
MVN_API int mvn_group_create(const int* devices, int ndevices, const int dims[3], int halo_planes, int num_views,
                             mvn_group** out);
MVN_API int mvn_group_destroy(mvn_group* g);
MVN_API int mvn_group_load(mvn_group* g, const float* psi, struct workspace input);
MVN_API int mvn_group_iterate(mvn_group* g, int iterations, double lambda, float min_value, float* ms);
MVN_API int mvn_group_get_psi(mvn_group* g, float* psi);

/* ---- slab-decomposed engine: the SEQUENTIAL sweep on several GPUs ------
 * Rank `rank` of `nranks` keeps planes [rank*d0/nranks, (rank+1)*d0/nranks) of psi, of every
 * view and of every weight stack; all host arrays below are those slabs, dense
 * [d0/nranks][d1][d2] (kernels are passed whole).  The reference has no multi-GPU code
 * (src/gpu_deconvolve_methods.cuh runs one device); the arithmetic is the view-after-view sweep
 * of src/multiviewnative.cpp:191-227, pass for pass.
 *
 * Last-axis and dim1 passes are plane-local; the dim0 pass needs whole lines, so every
 * convolution exchanges the half-transformed slab twice.  The exchange is the CALLER's (one
 * all-to-all with equal splits per buffer, e.g. torch.distributed.all_to_all_single over RCCL):
 *
 *   for conv in (0, 1):                       conv 0: psi (*) kernel1, conv 1: quotient (*) kernel2
 *     mvn_slab_pack(h, v, conv)               ... fills A_main / A_nyq
 *     mvn_slab_sync(h); all-to-all A_main -> B_main and A_nyq -> B_nyq
 *     mvn_slab_mid(h, v, conv)                dim0 forward * PSF * inverse, in place on B
 *     mvn_slab_sync(h); all-to-all B_main -> A_main and B_nyq -> A_nyq
 *     mvn_slab_unpack(h, v, conv, lambda, minValue, feed_next)
 *                                             conv 0: view / blurred; conv 1: psi update
 *
 * Buffers hold main_floats / nyq_floats floats (nyq_floats == 0 for odd d2) and are split in
 * `nranks` equal contiguous parts by the all-to-all.  feed_next != 0 says another view update
 * follows (the update pass then leaves psi's last-axis transform for it).  Needs d0 and d1
 * divisible by nranks with quotients >= 2. */
typedef struct mvn_slab mvn_slab; /* opaque */
MVN_API int mvn_slab_create(int device, const int dims[3], int nranks, int rank, int num_views,
                            mvn_slab** out);
MVN_API int mvn_slab_destroy(mvn_slab* h);
MVN_API int mvn_slab_set_view(mvn_slab* h, int v, const float* image_slab,
                              const float* weights_slab, const float* kernel1,
                              const int k1dims[3], const float* kernel2, const int k2dims[3]);
MVN_API int mvn_slab_set_psi(mvn_slab* h, const float* psi_slab);
MVN_API int mvn_slab_get_psi(mvn_slab* h, float* psi_slab);
MVN_API int mvn_slab_buffer_sizes(mvn_slab* h, size_t* main_floats, size_t* nyq_floats);
/* device pointers of the exchange buffers; bind caller-owned device memory (e.g. torch tensors)
 * so that a collective library can work on them in place, all-null returns to engine-owned */
MVN_API int mvn_slab_buffers(mvn_slab* h, void** a_main, void** b_main, void** a_nyq,
                             void** b_nyq);
MVN_API int mvn_slab_bind_buffers(mvn_slab* h, void* a_main, void* b_main, void* a_nyq,
                                  void* b_nyq);
MVN_API int mvn_slab_begin(mvn_slab* h); /* psi was replaced: forget its cached transform */
MVN_API int mvn_slab_pack(mvn_slab* h, int v, int conv);
MVN_API int mvn_slab_mid(mvn_slab* h, int v, int conv);
MVN_API int mvn_slab_unpack(mvn_slab* h, int v, int conv, double lambda, float min_value,
                            int feed_next);
MVN_API int mvn_slab_sync(mvn_slab* h);
MVN_API int mvn_slab_stream(mvn_slab* h, void** hip_stream);

#endif
