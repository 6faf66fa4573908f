"""ctypes binding of the product shared library ``lib/libmultiviewnative.so``.

This is the only way Python touches the hot path: every call goes through the C-ABI declared
in ``include/multiviewnative.h`` / ``include/mvn_engine_api.h``.  There is no fallback -- if the
HIP library has not been built, :func:`lib` raises.

``Binding(path)`` can also wrap the test-only host emulation (``lib/libmvn_emu.so``); only
``tests/`` does that, to validate plans and index math on a box without a GPU.
"""
import ctypes as C
import os

import numpy as np

from .abi import (MVN_DEVICE, CallDesc, DetectParams, RegisterParams, StackDesc, ViewData, ViewGeometry, Workspace,
                  c_float_p, c_int_p, describe_stack, detect_params, fptr, iptr, register_params, view_geometry)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
PRODUCT_SO = os.path.join(LIB_DIR, "libmultiviewnative.so")
EMU_SO = os.environ.get("MVN_EMU_SO") or os.path.join(LIB_DIR, "libmvn_emu.so")  # override: sanitizer build

REFERENCE_ABI_SYMBOLS = [
    "inplace_gpu_deconvolve", "inplace_gpu_convolution", "convolution3DfftCUDAInPlace",
    "convolution3DfftCUDAInPlace_core", "compute_quotient", "compute_final_values",
    "iterate_fft_plain", "iterate_fft_tikhonov",
    "selectDeviceWithHighestComputeCapability", "getCUDAcomputeCapabilityMinorVersion",
    "getCUDAcomputeCapabilityMajorVersion", "getNumDevicesCUDA", "getNameDeviceCUDA",
    "getMemDeviceCUDA",
]
ENGINE_ABI_SYMBOLS = [
    "mvn_last_error", "mvn_backend_name", "mvn_set_pad_mode", "mvn_get_pad_mode", "mvn_set_memory_mode", "mvn_get_memory_mode", "mvn_set_memory_budget", "mvn_deconvolve_memory",
    "mvn_stream_counters", "mvn_release_cached_engines", "mvn_deconvolve_submit", "mvn_deconvolve_wait", "mvn_psf_cache_counters", "mvn_split_launch_count", "mvn_mid_fused_launch_count", "mvn_multi_device_calls", "mvn_group_create", "mvn_group_destroy", "mvn_group_load", "mvn_group_iterate", "mvn_group_get_psi", "mvn_plan_store_add", "mvn_plan_store_has_key",
    "mvn_plan_store_size", "mvn_plan_store_empty", "mvn_plan_store_clear", "mvn_plan_describe",
    "mvn_fft3_r2c", "mvn_fft3_c2r", "mvn_fft3_time", "mvn_fft3_profile", "mvn_fft3_many_r2c", "mvn_fft3_many_time", "mvn_engine_create", "mvn_engine_destroy",
    "mvn_engine_set_view", "mvn_engine_set_psi", "mvn_engine_get_psi", "mvn_engine_iterate",
    "mvn_engine_compute_delta", "mvn_engine_apply_delta", "mvn_engine_delta_ptr",
    "mvn_engine_delta_chunks", "mvn_engine_delta_chunk_range", "mvn_engine_compute_delta_head",
    "mvn_engine_compute_delta_chunk", "mvn_engine_apply_delta_chunk",
    "mvn_engine_bind_delta", "mvn_engine_set_halo_hook", "mvn_engine_set_halo_planes", "mvn_engine_would_be_direct", "mvn_engine_poison_ptr", "mvn_engine_bind_poison", "mvn_engine_poison_get", "mvn_engine_poison_merge", "mvn_engine_copy_planes", "mvn_engine_psi_ptr", "mvn_engine_stream", "mvn_engine_sync", "mvn_engine_time_iterate",
    "mvn_engine_profile", "mvn_engine_profile_read", "mvn_kernel_kind_count",
    "mvn_kernel_kind_name", "mvn_engine_B",
    "mvn_slab_create", "mvn_slab_destroy", "mvn_slab_set_view", "mvn_slab_set_psi", "mvn_slab_get_psi",
    "mvn_slab_buffer_sizes", "mvn_slab_buffers", "mvn_slab_bind_buffers", "mvn_slab_begin",
    "mvn_slab_pack", "mvn_slab_mid", "mvn_slab_unpack", "mvn_slab_sync", "mvn_slab_stream",
    "mvn_set_convergence", "mvn_get_convergence", "mvn_last_convergence", "mvn_engine_iterate_converge",
    "mvn_deconvolve_described", "mvn_engine_set_view_described", "mvn_engine_set_psi_described",
    "mvn_engine_get_psi_described",
    "mvn_set_acceleration", "mvn_get_acceleration", "mvn_last_acceleration", "mvn_engine_iterate_accelerated",
    "mvn_set_regularization", "mvn_get_regularization", "mvn_engine_set_regularization", "mvn_tv_factor",
    "mvn_tv_time", "mvn_tv_launch_count", "mvn_reflect_counters", "mvn_reflect_time",
    "mvn_deconvolve_resampled", "mvn_deconvolve_memory_resampled", "mvn_engine_set_view_resampled",
    "mvn_engine_normalize_weights", "mvn_resample_stack", "mvn_resample_time", "mvn_resample_counters",
    "mvn_set_image_storage", "mvn_get_image_storage", "mvn_deconvolve_memory_described", "mvn_image_storage_counters",
    "mvn_set_background", "mvn_get_background", "mvn_set_likelihood", "mvn_get_likelihood", "mvn_last_likelihood",
    "mvn_engine_set_noise_model", "mvn_engine_last_likelihood",
    "mvn_fuse_resampled", "mvn_fuse_memory_resampled", "mvn_fuse_time", "mvn_fuse_counters", "mvn_set_psi_start",
    "mvn_get_psi_start", "mvn_engine_fuse_psi",
    "mvn_psf_extents", "mvn_derive_kernels", "mvn_set_kernel_derivation", "mvn_get_kernel_derivation",
    "mvn_derive_counters", "mvn_derive_time",
    "mvn_extract_psf", "mvn_extract_memory", "mvn_extract_counters", "mvn_extract_time",
    "mvn_detect_beads", "mvn_detect_taps", "mvn_detect_dog", "mvn_detect_memory", "mvn_detect_counters",
    "mvn_detect_time",
    "mvn_register_beads", "mvn_register_neighbours", "mvn_register_candidates", "mvn_register_sample",
    "mvn_register_memory", "mvn_register_counters", "mvn_register_time",
]
REGISTER_PRIOR = 1                     # MVN_REGISTER_PRIOR
REGISTER_NEIGHBOURS = 4                # MVN_REGISTER_NEIGHBOURS
REGISTER_REFITS = 10                   # MVN_REGISTER_REFITS
REGISTER_MAX_BEADS = 65536             # MVN_REGISTER_MAX_BEADS
REGISTER_MAX_HYPOTHESES = 1 << 24      # MVN_REGISTER_MAX_HYPOTHESES
DETECT_MINIMA = 1       # MVN_DETECT_MINIMA
DETECT_MAX_RADIUS = 30  # MVN_DETECT_MAX_RADIUS
BEADS_REMOVE_MIN = 1  # MVN_BEADS_REMOVE_MIN
BEADS_GROUP = 32      # MVN_BEADS_GROUP
PSF_TYPES = {"independent": 0, "efficient_bayesian": 1, "optimization_1": 2, "optimization_2": 3}


def _caller_stream(tensors):
    """The hipStream_t the device tensors among `tensors` were produced on (torch's current stream of their device), or
    None.  Work on the legacy default stream is waited for here: NULL means 'complete' to the library."""
    dev = [t for t in tensors if not isinstance(t, np.ndarray) and getattr(t, "is_cuda", False)]
    if not dev:
        return None
    import torch
    s = torch.cuda.current_stream(dev[0].device)
    if not s.cuda_stream:
        s.synchronize()
        return None
    return s.cuda_stream


class MvnError(RuntimeError):
    pass


def _dims(shape):
    return (C.c_int * 3)(*[int(s) for s in shape])


class Binding:
    def __init__(self, path):
        if not os.path.exists(path):
            raise MvnError(
                "native library %s is missing -- build it with `python -c 'import "
                "__graft_entry__ as g; g.build()'` (there is no CPU fallback)" % path)
        self.path = path
        self.l = C.CDLL(path)
        l = self.l
        i3 = C.POINTER(C.c_int)
        l.mvn_last_error.restype = C.c_char_p
        l.mvn_backend_name.restype = C.c_char_p
        l.mvn_split_launch_count.restype = C.c_long
        l.mvn_split_launch_count.argtypes = []
        l.mvn_mid_fused_launch_count.restype = C.c_long
        l.mvn_mid_fused_launch_count.argtypes = []
        l.mvn_multi_device_calls.restype = C.c_long
        l.mvn_multi_device_calls.argtypes = []
        l.mvn_group_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]
        l.mvn_group_destroy.argtypes = [C.c_void_p]
        l.mvn_group_load.argtypes = [C.c_void_p, C.POINTER(C.c_float), Workspace]
        l.mvn_group_iterate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_float, C.POINTER(C.c_float)]
        l.mvn_group_get_psi.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.mvn_kernel_kind_name.restype = C.c_char_p
        l.mvn_kernel_kind_name.argtypes = [C.c_int]
        l.mvn_set_pad_mode.argtypes = [C.c_char_p]
        l.mvn_get_pad_mode.restype = C.c_char_p
        l.mvn_get_pad_mode.argtypes = []
        l.mvn_set_memory_mode.argtypes = [C.c_char_p]
        l.mvn_get_memory_mode.restype = C.c_char_p
        l.mvn_get_memory_mode.argtypes = []
        l.mvn_set_memory_budget.argtypes = [C.c_longlong]
        l.mvn_deconvolve_memory.argtypes = [Workspace, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        l.mvn_stream_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.inplace_gpu_deconvolve.argtypes = [c_float_p, Workspace, C.c_int]
        l.inplace_gpu_deconvolve.restype = None
        l.mvn_deconvolve_submit.argtypes = [c_float_p, Workspace, C.c_int, C.POINTER(C.c_longlong)]
        l.mvn_deconvolve_wait.argtypes = [C.c_longlong]
        sd = C.POINTER(StackDesc)
        l.mvn_deconvolve_described.argtypes = [C.c_void_p, Workspace, C.POINTER(CallDesc), C.c_int]
        l.mvn_engine_set_view_described.argtypes = [C.c_void_p, C.c_int, C.c_void_p, sd, C.c_void_p, sd, c_float_p, i3,
                                                    c_float_p, i3, C.c_void_p]
        l.mvn_engine_set_psi_described.argtypes = [C.c_void_p, C.c_void_p, sd, C.c_void_p]
        l.mvn_set_image_storage.argtypes = [C.c_int]
        l.mvn_get_image_storage.argtypes = [C.POINTER(C.c_int)]
        l.mvn_deconvolve_memory_described.argtypes = [Workspace, C.POINTER(CallDesc), C.c_int, C.c_int,
                                                      C.POINTER(C.c_size_t)]
        l.mvn_image_storage_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_engine_get_psi_described.argtypes = [C.c_void_p, C.c_void_p, sd]
        for n in ("inplace_gpu_convolution", "convolution3DfftCUDAInPlace"):
            getattr(l, n).argtypes = [c_float_p, c_int_p, c_float_p, c_int_p, C.c_int]
            getattr(l, n).restype = None
        l.convolution3DfftCUDAInPlace_core.argtypes = [C.c_void_p, c_int_p, C.c_void_p, c_int_p, C.c_int]
        l.convolution3DfftCUDAInPlace_core.restype = None
        l.compute_quotient.argtypes = [c_float_p, c_float_p, C.c_size_t, C.c_int]
        l.compute_quotient.restype = None
        l.compute_final_values.argtypes = [c_float_p, c_float_p, c_float_p, C.c_size_t, C.c_float,
                                           C.c_double, C.c_int]
        l.compute_final_values.restype = None
        l.iterate_fft_plain.argtypes = [c_float_p, c_float_p, c_float_p, c_int_p, c_int_p, C.c_int]
        l.iterate_fft_plain.restype = None
        l.iterate_fft_tikhonov.argtypes = [c_float_p, c_float_p, c_float_p, c_int_p, c_int_p,
                                           C.c_size_t, C.c_float, C.c_double, C.c_int]
        l.iterate_fft_tikhonov.restype = None
        l.getNameDeviceCUDA.argtypes = [C.c_int, C.c_char_p]
        l.getNameDeviceCUDA.restype = None
        l.getMemDeviceCUDA.argtypes = [C.c_int]
        l.getMemDeviceCUDA.restype = C.c_longlong
        l.mvn_plan_store_add.argtypes = [C.c_int, i3]
        l.mvn_plan_store_has_key.argtypes = [C.c_int, i3]
        l.mvn_plan_describe.argtypes = [C.c_int, i3, i3]
        l.mvn_fft3_r2c.argtypes = [C.c_int, i3, c_float_p, c_float_p]
        l.mvn_fft3_c2r.argtypes = [C.c_int, i3, c_float_p, c_float_p]
        l.mvn_fft3_time.argtypes = [C.c_int, i3, C.c_int, C.c_int, C.POINTER(C.c_float)]
        l.mvn_fft3_profile.argtypes = [C.c_int, i3, C.c_int, C.c_int, C.POINTER(C.c_float),
                                       C.POINTER(C.c_double)]
        l.mvn_fft3_many_r2c.argtypes = [C.c_int, i3, C.c_int, c_float_p, c_float_p]
        l.mvn_fft3_many_time.argtypes = [C.c_int, i3, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        l.mvn_engine_create.argtypes = [C.c_int, i3, C.c_int, C.POINTER(C.c_void_p)]
        l.mvn_engine_destroy.argtypes = [C.c_void_p]
        l.mvn_engine_set_view.argtypes = [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, i3,
                                          c_float_p, i3]
        l.mvn_engine_set_psi.argtypes = [C.c_void_p, c_float_p]
        l.mvn_engine_get_psi.argtypes = [C.c_void_p, c_float_p]
        l.mvn_engine_iterate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_float]
        l.mvn_engine_iterate_converge.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_double,
                                                  C.POINTER(C.c_int), C.POINTER(C.c_double)]
        l.mvn_set_convergence.argtypes = [C.c_double]
        l.mvn_get_convergence.argtypes = [C.POINTER(C.c_double)]
        l.mvn_last_convergence.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int]
        l.mvn_set_acceleration.argtypes = [C.c_int]
        l.mvn_get_acceleration.argtypes = [C.POINTER(C.c_int)]
        l.mvn_last_acceleration.argtypes = [C.POINTER(C.c_double), C.c_int]
        l.mvn_engine_iterate_accelerated.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_double,
                                                     C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.mvn_set_regularization.argtypes = [C.c_int, C.c_double]
        l.mvn_get_regularization.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
        l.mvn_engine_set_regularization.argtypes = [C.c_void_p, C.c_int, C.c_double]
        l.mvn_tv_factor.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_double, C.c_double,
                                    C.POINTER(C.c_float)]
        l.mvn_tv_time.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float)]
        l.mvn_set_background.argtypes = [C.POINTER(C.c_float), C.c_int]
        l.mvn_get_background.argtypes = [C.POINTER(C.c_float), C.c_int]
        l.mvn_set_likelihood.argtypes = [C.c_int]
        l.mvn_get_likelihood.argtypes = [C.POINTER(C.c_int)]
        l.mvn_last_likelihood.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int]
        l.mvn_engine_set_noise_model.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        l.mvn_engine_last_likelihood.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int]
        l.mvn_reflect_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_reflect_time.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                       C.c_int, C.POINTER(C.c_float)]
        vg = C.POINTER(ViewGeometry)
        l.mvn_deconvolve_resampled.argtypes = [C.c_void_p, Workspace, C.POINTER(CallDesc), vg, C.c_int, C.c_int]
        l.mvn_deconvolve_memory_resampled.argtypes = [Workspace, C.POINTER(CallDesc), vg, C.c_int, C.c_int,
                                                      C.POINTER(C.c_size_t)]
        l.mvn_engine_set_view_resampled.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(StackDesc), vg,
                                                    C.c_void_p, C.POINTER(StackDesc), c_float_p, i3, c_float_p, i3,
                                                    C.c_void_p]
        l.mvn_engine_normalize_weights.argtypes = [C.c_void_p]
        l.mvn_resample_stack.argtypes = [C.c_int, C.c_void_p, C.POINTER(StackDesc), vg, i3, c_float_p, c_float_p]
        l.mvn_resample_time.argtypes = [C.c_int, C.c_int, vg, i3, C.c_int, C.POINTER(C.c_float)]
        l.mvn_resample_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_fuse_resampled.argtypes = [C.c_void_p, C.POINTER(StackDesc), i3, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(StackDesc), vg, C.c_float, C.c_void_p, C.c_int]
        l.mvn_fuse_memory_resampled.argtypes = [C.POINTER(StackDesc), i3, C.c_int, C.POINTER(StackDesc), vg, C.c_int,
                                                C.POINTER(C.c_size_t)]
        l.mvn_fuse_time.argtypes = [C.c_int, C.c_int, C.c_int, vg, i3, C.c_int, C.POINTER(C.c_float)]
        l.mvn_fuse_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_set_psi_start.argtypes = [C.c_int, C.c_float]
        l.mvn_get_psi_start.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float)]
        l.mvn_engine_fuse_psi.argtypes = [C.c_void_p, C.c_float]
        fpp = C.POINTER(c_float_p)
        l.mvn_psf_extents.argtypes = [C.c_int, i3, vg, i3]
        l.mvn_derive_kernels.argtypes = [C.c_int, C.c_int, fpp, i3, vg, C.c_int, i3, fpp, fpp]
        l.mvn_set_kernel_derivation.argtypes = [C.c_int, C.c_int]
        l.mvn_get_kernel_derivation.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.mvn_derive_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_derive_time.argtypes = [C.c_int, C.c_int, i3, C.c_int, C.c_int, C.POINTER(C.c_float)]
        l.mvn_extract_psf.argtypes = [C.c_int, C.c_void_p, C.POINTER(StackDesc), i3, C.POINTER(C.c_double), C.c_int, i3,
                                      C.c_int, c_float_p, C.POINTER(C.c_double), C.c_void_p]
        l.mvn_extract_memory.argtypes = [C.POINTER(StackDesc), i3, C.c_int, i3, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        l.mvn_extract_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_extract_time.argtypes = [C.c_int, C.c_int, i3, C.c_int, i3, C.c_int, C.POINTER(C.c_float)]
        l.mvn_detect_beads.argtypes = [C.c_int, C.c_void_p, C.POINTER(StackDesc), i3, C.POINTER(DetectParams), C.c_int,
                                       C.POINTER(C.c_int), C.POINTER(C.c_double), c_float_p, C.POINTER(C.c_int),
                                       C.c_void_p]
        l.mvn_detect_taps.argtypes = [C.c_double, c_float_p, C.c_int, C.POINTER(C.c_int)]
        l.mvn_detect_dog.argtypes = [C.c_int, C.c_void_p, C.POINTER(StackDesc), i3, C.POINTER(DetectParams), c_float_p]
        l.mvn_detect_memory.argtypes = [C.POINTER(StackDesc), i3, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        l.mvn_detect_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_detect_time.argtypes = [C.c_int, C.c_int, i3, C.POINTER(DetectParams), C.c_int, C.POINTER(C.c_float)]
        d_p = C.POINTER(C.c_double)
        l.mvn_register_beads.argtypes = [C.c_int, d_p, C.c_int, d_p, C.c_int, C.POINTER(RegisterParams), d_p,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), c_int_p, d_p, C.c_void_p]
        l.mvn_register_neighbours.argtypes = [C.c_int, d_p, C.c_int, c_int_p]
        l.mvn_register_candidates.argtypes = [C.c_int, d_p, C.c_int, d_p, C.c_int, C.POINTER(RegisterParams),
                                              C.POINTER(C.c_int), c_int_p, c_float_p]
        l.mvn_register_sample.argtypes = [C.c_ulonglong, C.c_int, C.c_int, c_int_p]
        l.mvn_register_memory.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        l.mvn_register_counters.argtypes = [C.POINTER(C.c_longlong)]
        l.mvn_register_time.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        l.mvn_tv_launch_count.restype = C.c_long
        l.mvn_tv_launch_count.argtypes = []
        l.mvn_engine_compute_delta.argtypes = [C.c_void_p, C.c_double, C.c_float]
        l.mvn_engine_apply_delta.argtypes = [C.c_void_p]
        l.mvn_engine_delta_chunks.argtypes = [C.c_void_p, C.c_int]
        l.mvn_engine_delta_chunk_range.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t),
                                                   C.POINTER(C.c_size_t)]
        l.mvn_engine_compute_delta_head.argtypes = [C.c_void_p, C.c_double, C.c_float]
        l.mvn_engine_compute_delta_chunk.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.mvn_engine_apply_delta_chunk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        l.mvn_engine_delta_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.mvn_engine_psi_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        l.mvn_engine_bind_delta.argtypes = [C.c_void_p, C.c_void_p]
        l.mvn_engine_set_halo_hook.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        l.mvn_engine_copy_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        l.mvn_engine_set_halo_planes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.mvn_engine_would_be_direct.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        l.mvn_engine_poison_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.mvn_engine_bind_poison.argtypes = [C.c_void_p, C.c_void_p]
        l.mvn_engine_poison_get.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        l.mvn_engine_poison_merge.argtypes = [C.c_void_p, C.c_uint]
        l.mvn_engine_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.mvn_engine_sync.argtypes = [C.c_void_p]
        l.mvn_engine_time_iterate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_float,
                                              C.POINTER(C.c_float)]
        l.mvn_engine_profile.argtypes = [C.c_void_p, C.c_int]
        l.mvn_engine_profile_read.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double),
                                              C.POINTER(C.c_long)]
        vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
        l.mvn_slab_create.argtypes = [C.c_int, i3, C.c_int, C.c_int, C.c_int, vpp]
        l.mvn_slab_destroy.argtypes = [vp]
        l.mvn_slab_set_view.argtypes = [vp, C.c_int, c_float_p, c_float_p, c_float_p, i3, c_float_p, i3]
        l.mvn_slab_set_psi.argtypes = [vp, c_float_p]
        l.mvn_slab_get_psi.argtypes = [vp, c_float_p]
        l.mvn_slab_buffer_sizes.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        l.mvn_slab_buffers.argtypes = [vp, vpp, vpp, vpp, vpp]
        l.mvn_slab_bind_buffers.argtypes = [vp, vp, vp, vp, vp]
        l.mvn_slab_begin.argtypes = [vp]
        l.mvn_slab_pack.argtypes = [vp, C.c_int, C.c_int]
        l.mvn_slab_mid.argtypes = [vp, C.c_int, C.c_int]
        l.mvn_slab_unpack.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_float, C.c_int]
        l.mvn_slab_sync.argtypes = [vp]
        l.mvn_slab_stream.argtypes = [vp, vpp]
        l.mvn_engine_B.argtypes = [C.c_void_p]
        l.mvn_engine_B.restype = C.c_size_t

    # ---- helpers -------------------------------------------------------------------------
    def check(self, rc):
        if rc < 0:
            raise MvnError(self.l.mvn_last_error().decode())
        return rc

    def backend_name(self):
        return self.l.mvn_backend_name().decode()

    def set_pad_mode(self, mode):
        """'zero' | 'zero_exact' | 'none' | 'reflect' (the volume of 'zero', mirrored margins instead of zeros) | None
        (back to MVN_PAD_MODE / the default)."""
        self.check(self.l.mvn_set_pad_mode(mode.encode() if mode else None))

    def get_pad_mode(self):
        """The mode selected with set_pad_mode, None when the environment / default decides."""
        return self.l.mvn_get_pad_mode().decode() or None

    def set_memory_mode(self, mode):
        """'resident' | 'auto' | 'stream' | 'stream:N' | None (back to the default, resident)."""
        self.check(self.l.mvn_set_memory_mode(mode.encode() if mode else None))

    def get_memory_mode(self):
        """The mode selected with set_memory_mode, None when the default (resident) applies."""
        return self.l.mvn_get_memory_mode().decode() or None

    def set_memory_budget(self, nbytes):
        """Cap of the auto / stream planner in bytes; None or <= 0 removes it."""
        self.check(self.l.mvn_set_memory_budget(int(nbytes) if nbytes else 0))

    def deconvolve_memory(self, holder, streamed_views=0, device=0):
        """Device bytes inplace_gpu_deconvolve allocates for this workspace with `streamed_views` views
        streamed (ring of 2 slots), under the padding policy in force."""
        out = C.c_size_t(0)
        self.check(self.l.mvn_deconvolve_memory(holder.ws, device, streamed_views, C.byref(out)))
        return out.value

    def stream_counters(self):
        """(calls that streamed views, streamed view updates, bytes streamed) since process start."""
        out = (C.c_longlong * 3)()
        self.check(self.l.mvn_stream_counters(out))
        return tuple(int(x) for x in out)

    def set_image_storage(self, mode):
        """How uint16 image stacks of described calls are held on the device: 0 (default) converted to float32 on
        entry, 1 kept as uint16 (mvn_engine_api.h).  Results are the same bits."""
        self.check(self.l.mvn_set_image_storage(int(mode)))

    def get_image_storage(self):
        out = C.c_int(0)
        self.check(self.l.mvn_get_image_storage(C.byref(out)))
        return out.value

    def deconvolve_memory_described(self, call, streamed_views=0, device=0):
        """deconvolve_memory for a prepared described call (describe_call), or for a WorkspaceHolder (no descriptors:
        exactly deconvolve_memory): uint16 images are priced at 2 bytes per voxel when the storage mode keeps them."""
        out = C.c_size_t(0)
        desc = C.byref(call.desc) if hasattr(call, "desc") else None
        self.check(self.l.mvn_deconvolve_memory_described(call.ws, desc, device, streamed_views, C.byref(out)))
        return out.value

    def image_storage_counters(self):
        """(divide passes launched on a uint16 image, ingest passes that wrote a uint16 volume) since process start."""
        out = (C.c_longlong * 2)()
        self.check(self.l.mvn_image_storage_counters(out))
        return tuple(int(x) for x in out)

    def set_convergence(self, tolerance):
        """Process-wide convergence tolerance: < 0 off (default), 0 statistics only, > 0 stop at
        S_k / P_k <= tolerance (mvn_engine_api.h)."""
        self.check(self.l.mvn_set_convergence(float(tolerance)))

    def get_convergence(self):
        out = C.c_double(0)
        self.check(self.l.mvn_get_convergence(C.byref(out)))
        return out.value

    def last_convergence(self):
        """(iterations run, float64 array [rows, 3] of {S_k, M_k, P_k}) of the last deconvolution this thread
        completed (inplace_gpu_deconvolve, or the wait of its ticket)."""
        run = C.c_int(0)
        rows = self.l.mvn_last_convergence(C.byref(run), None, 0)
        self.check(rows)
        out = np.zeros((rows, 3), dtype=np.float64)
        if rows:
            self.check(self.l.mvn_last_convergence(C.byref(run), out.ctypes.data_as(C.POINTER(C.c_double)), rows))
        return run.value, out

    def set_acceleration(self, mode):
        """Process-wide acceleration of the RL loop: 0 off (default), 1 vector extrapolation between sweeps
        (mvn_engine_api.h)."""
        self.check(self.l.mvn_set_acceleration(int(mode)))

    def get_acceleration(self):
        out = C.c_int(0)
        self.check(self.l.mvn_get_acceleration(C.byref(out)))
        return out.value

    def last_acceleration(self):
        """float64 array of a_1 .. a_ran of the last deconvolution this thread completed (empty when acceleration
        was off); the entry of the last sweep run is 0."""
        rows = self.check(self.l.mvn_last_acceleration(None, 0))
        out = np.zeros(rows, dtype=np.float64)
        if rows:
            self.check(self.l.mvn_last_acceleration(out.ctypes.data_as(C.POINTER(C.c_double)), rows))
        return out

    def set_regularization(self, kind, epsilon=0.0):
        """Process-wide regulariser of the RL loop: 0 Tikhonov (default; epsilon ignored), 1 total variation with
        workspace.lambda_ as its weight and a finite epsilon > 0 (mvn_engine_api.h)."""
        self.check(self.l.mvn_set_regularization(int(kind), float(epsilon)))

    def get_regularization(self):
        kind, eps = C.c_int(0), C.c_double(0)
        self.check(self.l.mvn_get_regularization(C.byref(kind), C.byref(eps)))
        return kind.value, eps.value

    def set_background(self, values=None):
        """Process-wide camera background of the RL loop's forward model, quotient = image / (H psi + b_v): None or
        empty: off (default); one value: every view; else one per view (mvn_engine_api.h)."""
        vals = np.atleast_1d(np.asarray([] if values is None else values, dtype=np.float32)).ravel()
        self.check(self.l.mvn_set_background(vals.ctypes.data_as(C.POINTER(C.c_float)) if vals.size else None,
                                             int(vals.size)))

    def get_background(self):
        n = self.check(self.l.mvn_get_background(None, 0))
        out = np.zeros(n, dtype=np.float32)
        if n:
            self.check(self.l.mvn_get_background(out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out

    def set_likelihood(self, mode):
        """Process-wide: 1 = the divide pass also sums {D, Y, M} per (sweep, view); 0 off (default)."""
        self.check(self.l.mvn_set_likelihood(int(mode)))

    def get_likelihood(self):
        out = C.c_int(0)
        self.check(self.l.mvn_get_likelihood(C.byref(out)))
        return out.value

    def last_likelihood(self):
        """float64 array [sweeps run, V, 3] of {D, Y, M} of the last deconvolution this thread completed (no rows
        when background and likelihood were off)."""
        run, nv = C.c_int(0), C.c_int(0)
        rows = self.check(self.l.mvn_last_likelihood(C.byref(run), C.byref(nv), None, 0))
        out = np.zeros((rows, 3), dtype=np.float64)
        if rows:
            self.check(self.l.mvn_last_likelihood(C.byref(run), C.byref(nv), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                  rows))
        v = max(nv.value, 1)
        return out.reshape(rows // v, v, 3)

    def tv_factor(self, psi, lambda_, epsilon, device=0):
        """mvn_tv_factor: the total-variation factor t of the float32 volume psi."""
        psi = np.ascontiguousarray(psi, dtype=np.float32)
        assert psi.ndim == 3
        out = np.empty_like(psi)
        dims = (C.c_int * 3)(*psi.shape)
        self.check(self.l.mvn_tv_factor(device, dims, psi.ctypes.data_as(C.POINTER(C.c_float)), float(lambda_),
                                        float(epsilon), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def tv_time(self, shape, reps=10, device=0):
        """mvn_tv_time: (ms per launch of the TV pass, ms per plain copy of the same volume)."""
        ms = (C.c_float * 2)(0, 0)
        dims = (C.c_int * 3)(*shape)
        self.check(self.l.mvn_tv_time(device, dims, int(reps), ms))
        return float(ms[0]), float(ms[1])

    def tv_launch_count(self):
        return int(self.l.mvn_tv_launch_count())

    def reflect_counters(self):
        """mvn_reflect_counters: (launches of the reflect fill, volumes filled) since process start."""
        out = (C.c_longlong * 2)(0, 0)
        self.check(self.l.mvn_reflect_counters(out))
        return int(out[0]), int(out[1])

    def reflect_time(self, dims, ext, off, u16=False, reps=10, device=0):
        """mvn_reflect_time: (ms per reflect fill of a resident volume of extents `ext` around a window of extents `dims`
        at offset `off`, ms per plain copy of that volume)."""
        ms = (C.c_float * 2)(0, 0)
        self.check(self.l.mvn_reflect_time(device, (C.c_int * 3)(*dims), (C.c_int * 3)(*ext), (C.c_int * 3)(*off),
                                           int(bool(u16)), int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- reference ABI, numpy in / numpy out ----------------------------------------------
    def gpu_deconvolve(self, psi, holder, device=0, pad_mode="none"):
        """inplace_gpu_deconvolve on a copy of psi.  `pad_mode` defaults to the CPU path's cyclic
        policy, the one the oracle implements (the library's own default is 'zero', the reference
        GPU entry's; 'reflect' is that volume with mirrored margins); pass pad_mode=False to leave the process-wide
        setting alone.  The setting
        found on entry is restored on exit (the switch is process-wide: not for concurrent callers)."""
        out = np.ascontiguousarray(psi, dtype=np.float32).copy()
        before = self.get_pad_mode()
        if pad_mode is not False:
            self.set_pad_mode(pad_mode)
        try:
            self.l.inplace_gpu_deconvolve(fptr(out), holder.ws, device)
        finally:
            if pad_mode is not False:
                self.set_pad_mode(before)
        return out

    def describe_call(self, psi, views, weights, kernels1, kernels2, lambda_, min_value, iterations,
                      int16_is_uint16=False):
        """The arguments of mvn_deconvolve_described for these objects, as a DescribedCall: `.desc` (mvn_call_desc),
        `.image` / `.weights` (its mvn_stack_desc arrays), `.ws` (the workspace); `.run(device)` makes the call.
        See deconvolve_described for what the objects may be."""
        n = len(views)
        if not (len(weights) == n and len(kernels1) == n and len(kernels2) == n):
            raise ValueError("one weights stack and two kernels per view")
        c = DescribedCall()
        c.binding, c.psi = self, psi
        c.keep = [[np.ascontiguousarray(k, dtype=np.float32) for k in ks] for ks in (kernels1, kernels2)]
        k1, k2 = c.keep
        c.psi_ptr, p_desc, shape, p_dev = describe_stack(psi)
        c.image, c.weights = (StackDesc * n)(), (StackDesc * n)()
        data = (ViewData * n)()
        devices = [p_dev]
        for v in range(n):
            i_ptr, c.image[v], i_shape, i_dev = describe_stack(views[v], int16_is_uint16)
            w_ptr, c.weights[v], w_shape, w_dev = describe_stack(weights[v])
            if i_shape != shape or w_shape != shape:
                raise ValueError("view %d: every stack has psi's shape %r" % (v, shape))
            devices += [i_dev, w_dev]
            dims = [np.array(s_, dtype=np.int32) for s_ in (shape, k1[v].shape, k2[v].shape, shape)]
            c.keep.append(dims)
            d = data[v]
            d.image_, d.weights_ = C.cast(C.c_void_p(i_ptr), c_float_p), C.cast(C.c_void_p(w_ptr), c_float_p)
            d.kernel1_, d.kernel2_ = fptr(k1[v]), fptr(k2[v])
            d.image_dims_, d.kernel1_dims_, d.kernel2_dims_, d.weights_dims_ = [iptr(x) for x in dims]
        c.keep += [data, list(views), list(weights)]
        c.ws = Workspace()
        c.ws.data_ = C.cast(data, C.POINTER(ViewData))
        c.ws.num_views_, c.ws.lambda_, c.ws.minValue_, c.ws.num_iterations_ = (
            n, float(lambda_), float(min_value), int(iterations))
        c.desc = CallDesc()
        c.desc.psi = p_desc
        c.desc.image = C.cast(c.image, C.POINTER(StackDesc))
        c.desc.weights = C.cast(c.weights, C.POINTER(StackDesc))
        owners = [x for x in devices if x is not None]
        c.device = owners[0] if owners else 0
        return c

    def deconvolve_described(self, psi, views, weights, kernels1, kernels2, lambda_, min_value, iterations,
                             device=None, int16_is_uint16=False):
        """mvn_deconvolve_described: inplace_gpu_deconvolve on stacks as the caller has them.  psi, every view and
        every weights stack may be a numpy array (float32; views also uint16; any strides that are multiples of the
        item size) or a torch tensor (CPU or cuda; uint16 views as torch.uint16 - a torch without that type may pass
        torch.int16 tensors holding the same bits with int16_is_uint16=True, otherwise int16 is refused); pointer,
        element type, location and strides are taken from the object, the stream from torch.cuda.current_stream()
        when a tensor is on the device - the stacks need not be complete on the host's side, only enqueued on that
        stream.  Stacks in host memory need contiguous rows, or strides of 0 throughout (np.broadcast_to of a scalar:
        constant weights).  psi (float32, non-overlapping) is updated in place and returned; the process-wide padding
        policy applies.  Kernels are dense float32 host arrays.
        torch is imported only when a tensor is passed, and the rule of INTEGRATION.md section 3 is the caller's:
        import torch BEFORE this library is loaded in the process."""
        return self.describe_call(psi, views, weights, kernels1, kernels2, lambda_, min_value, iterations,
                                  int16_is_uint16).run(device)

    # ---- resampled views (mvn_view_geometry) ----------------------------------------------
    def resample_counters(self):
        """mvn_resample_counters: (launches of the resample pass, launches of the normalisation) since process start."""
        out = (C.c_longlong * 2)(0, 0)
        self.check(self.l.mvn_resample_counters(out))
        return int(out[0]), int(out[1])

    def resample_stack(self, src, geom, out_shape, device=-1, int16_is_uint16=False):
        """mvn_resample_stack: the raw stack `src` (numpy array or torch tensor, float32 or uint16, host or device, as
        deconvolve_described takes them) through `geom` (abi.view_geometry) into (image, unnormalised weights), two
        dense float32 arrays of `out_shape`."""
        ptr, desc, shape, dev = describe_stack(src, int16_is_uint16)
        if shape != tuple(geom.src_dims):
            raise ValueError("the raw stack has shape %r, its geometry says %r" % (shape, tuple(geom.src_dims)))
        if _caller_stream([src]) is not None:  # (the utility takes no stream: the stack must be complete)
            import torch
            torch.cuda.current_stream(src.device).synchronize()
        image, weights = np.empty(out_shape, np.float32), np.empty(out_shape, np.float32)
        self.check(self.l.mvn_resample_stack(int(dev if dev is not None else device), C.c_void_p(ptr), C.byref(desc),
                                             C.byref(geom), _dims(out_shape), fptr(image), fptr(weights)))
        return image, weights

    def resample_time(self, geom, out_shape, u16=True, reps=10, device=0):
        """mvn_resample_time: (ms per resample pass from a resident raw stack of geom.src_dims into volumes of
        `out_shape`, ms per streaming copy that reads one and writes two such volumes)."""
        ms = (C.c_float * 2)(0, 0)
        self.check(self.l.mvn_resample_time(device, int(bool(u16)), C.byref(geom), _dims(out_shape), int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- fusion (mvn_fuse_resampled) -------------------------------------------------------
    def fuse_counters(self):
        """mvn_fuse_counters: (launches of the fusion from raw stacks, launches of the fusion of an engine's volumes)
        since process start."""
        out = (C.c_longlong * 2)(0, 0)
        self.check(self.l.mvn_fuse_counters(out))
        return int(out[0]), int(out[1])

    def _fuse_args(self, out, raws, geoms, int16_is_uint16):
        n = len(raws)
        if len(geoms) != n:
            raise ValueError("one geometry per raw stack")
        o_ptr, o_desc, shape, o_dev = describe_stack(out, int16_is_uint16)
        descs, garr, ptrs = (StackDesc * max(n, 1))(), (ViewGeometry * max(n, 1))(), (C.c_void_p * max(n, 1))()
        devices = [o_dev]
        for v in range(n):
            ptr, descs[v], r_shape, r_dev = describe_stack(raws[v], int16_is_uint16)
            if r_shape != tuple(geoms[v].src_dims):
                raise ValueError("view %d: the raw stack has shape %r, its geometry says %r"
                                 % (v, r_shape, tuple(geoms[v].src_dims)))
            ptrs[v], garr[v] = ptr, geoms[v]
            devices.append(r_dev)
        owners = [x for x in devices if x is not None]
        return o_ptr, o_desc, shape, n, ptrs, descs, garr, (owners[0] if owners else None)

    def fuse_resampled(self, out, raws, geoms, fill=0.0, device=None, int16_is_uint16=False):
        """mvn_fuse_resampled: the weighted average of the RAW views `raws` (numpy arrays or torch tensors, float32 or
        uint16, host or device, as deconvolve_resampled takes them) through `geoms` (abi.view_geometry), with Fiji's
        cosine blend weights, written into `out` (float32 or uint16, numpy array or torch tensor of the block's shape,
        any window of a larger array with positive strides; host memory needs contiguous rows); `fill` where no view
        contributes.  Returns `out`."""
        o_ptr, o_desc, shape, n, ptrs, descs, garr, owner = self._fuse_args(out, raws, geoms, int16_is_uint16)
        stream = _caller_stream([out] + list(raws))
        dev = device if device is not None else (owner if owner is not None else 0)
        self.check(self.l.mvn_fuse_resampled(C.c_void_p(o_ptr), C.byref(o_desc), _dims(shape), n, ptrs, descs, garr,
                                             float(fill), C.c_void_p(stream), int(dev)))
        return out

    def fuse_memory(self, out, raws, geoms, device=0, int16_is_uint16=False):
        """mvn_fuse_memory_resampled: the bytes fuse_resampled would allocate on the device for these objects."""
        o_ptr, o_desc, shape, n, ptrs, descs, garr, owner = self._fuse_args(out, raws, geoms, int16_is_uint16)
        need = C.c_size_t(0)
        self.check(self.l.mvn_fuse_memory_resampled(C.byref(o_desc), _dims(shape), n, descs, garr, int(device),
                                                    C.byref(need)))
        return need.value

    def fuse_time(self, geoms, out_shape, u16=True, reps=10, device=0):
        """mvn_fuse_time: (ms per fusion from len(geoms) resident raw stacks into a resident float32 volume of
        `out_shape`, ms for one resample pass per view on the same stacks, ms per plain copy of one volume)."""
        garr = (ViewGeometry * len(geoms))(*geoms)
        ms = (C.c_float * 3)(0, 0, 0)
        self.check(self.l.mvn_fuse_time(device, int(bool(u16)), len(geoms), garr, _dims(out_shape), int(reps), ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def set_psi_start(self, mode, fill=0.0):
        """Process-wide start of mvn_deconvolve_resampled: 0 the caller's psi (default), 1 the fusion of the views,
        `fill` where no view contributes (mvn_engine_api.h)."""
        self.check(self.l.mvn_set_psi_start(int(mode), float(fill)))

    def get_psi_start(self):
        mode, fill = C.c_int(0), C.c_float(0)
        self.check(self.l.mvn_get_psi_start(C.byref(mode), C.byref(fill)))
        return mode.value, fill.value

    # ---- derived kernels (mvn_derive_kernels) ----------------------------------------------
    @staticmethod
    def _psf_type(type_):
        return PSF_TYPES[type_] if isinstance(type_, str) else int(type_)

    @staticmethod
    def _psf_args(raw_dims, geoms):
        n = len(raw_dims)
        if geoms is not None and len(geoms) != n:
            raise ValueError("one geometry per raw PSF")
        dims = (C.c_int * (3 * max(n, 1)))(*[int(x) for r in raw_dims for x in r])
        garr = (ViewGeometry * max(n, 1))(*geoms) if geoms is not None else None
        return n, dims, garr

    def psf_extents(self, raw_dims, geoms=None):
        """mvn_psf_extents: the common odd extents K of the kernels derived from raw PSFs of extents `raw_dims` (one
        triple per view) under `geoms` (abi.view_geometry per view, only the linear part of the matrix is read; None:
        the PSFs are in the block's frame)."""
        n, dims, garr = self._psf_args(raw_dims, geoms)
        out = (C.c_int * 3)(0, 0, 0)
        self.check(self.l.mvn_psf_extents(n, dims, garr, out))
        return tuple(out)

    def derive_kernels(self, raw_psfs, geoms=None, type_="efficient_bayesian", out_dims=None, device=-1):
        """mvn_derive_kernels: (kernels1, kernels2), two lists of dense float32 arrays of the common extents K, from the
        raw PSFs (float32 arrays of odd extents) and the views' geometries; `type_` is a key of PSF_TYPES or its
        number."""
        raws = [np.ascontiguousarray(p, dtype=np.float32) for p in raw_psfs]
        n, dims, garr = self._psf_args([p.shape for p in raws], geoms)
        K = tuple(int(k) for k in out_dims) if out_dims is not None else self.psf_extents([p.shape for p in raws], geoms)
        k1 = [np.full(K, np.nan, np.float32) for _ in raws]
        k2 = [np.full(K, np.nan, np.float32) for _ in raws]
        tab = lambda arrs: (c_float_p * max(n, 1))(*[fptr(a) for a in arrs])
        self.check(self.l.mvn_derive_kernels(int(device), n, tab(raws), dims, garr, self._psf_type(type_),
                                             _dims(K) if out_dims is not None else None, tab(k1), tab(k2)))
        return k1, k2

    def set_kernel_derivation(self, mode, type_="efficient_bayesian"):
        """Process-wide: 1 makes mvn_deconvolve_resampled take RAW PSFs as kernel1_ and derive both kernels of `type_`
        on the device; 0 (default) takes kernels as handed in (mvn_engine_api.h)."""
        self.check(self.l.mvn_set_kernel_derivation(int(mode), self._psf_type(type_)))

    def get_kernel_derivation(self):
        mode, type_ = C.c_int(0), C.c_int(0)
        self.check(self.l.mvn_get_kernel_derivation(C.byref(mode), C.byref(type_)))
        return mode.value, type_.value

    def derive_counters(self):
        """mvn_derive_counters: (launches of the correlation kernel, derivations computed, derivations re-used)."""
        out = (C.c_longlong * 3)(0, 0, 0)
        self.check(self.l.mvn_derive_counters(out))
        return int(out[0]), int(out[1]), int(out[2])

    def derive_time(self, num_views, dims, type_="efficient_bayesian", reps=3, device=0):
        """mvn_derive_time: (ms per derivation of num_views resident PSFs of extents `dims`, ms of its correlation
        launches alone)."""
        ms = (C.c_float * 2)(0, 0)
        self.check(self.l.mvn_derive_time(int(device), int(num_views), _dims(dims), self._psf_type(type_), int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- bead PSFs (mvn_extract_psf) --------------------------------------------------------
    def extract_psf(self, raw, beads, psf_shape, remove_min=False, scores=False, device=None, int16_is_uint16=False,
                    as_device=False):
        """mvn_extract_psf: the mean of the trilinear windows of extents `psf_shape` (odd) around the `beads` (an
        (N, 3) array of (z, y, x) positions, raw indices) of ONE view's raw stack `raw` (numpy array or torch tensor,
        float32 or uint16, host or device, as deconvolve_resampled takes them).  Returns the PSF as a dense float32
        array - what derive_kernels takes as a raw PSF - or (psf, scores) with scores=True: Pearson's correlation of
        every bead's window with the mean.  remove_min: the smallest value of the result becomes 0.  as_device: describe
        a host array as device memory (the emulation's pointers may be called either)."""
        ptr, desc, shape, dev = describe_stack(raw, int16_is_uint16)
        if as_device:
            desc.location = MVN_DEVICE
        pos = np.ascontiguousarray(beads, dtype=np.float64).reshape(-1, 3)
        psf = np.full(tuple(int(x) for x in psf_shape), np.nan, np.float32)
        sc = np.full(len(pos), np.nan, np.float64) if scores else None
        stream = _caller_stream([raw])
        self.check(self.l.mvn_extract_psf(int(device if device is not None else (dev if dev is not None else -1)),
                                          C.c_void_p(ptr), C.byref(desc), _dims(shape),
                                          pos.ctypes.data_as(C.POINTER(C.c_double)), len(pos), _dims(psf_shape),
                                          BEADS_REMOVE_MIN if remove_min else 0, fptr(psf),
                                          sc.ctypes.data_as(C.POINTER(C.c_double)) if scores else None,
                                          C.c_void_p(stream)))
        return (psf, sc) if scores else psf

    def extract_memory(self, raw, num_beads, psf_shape, scores=False, device=0, int16_is_uint16=False,
                       as_device=False):
        """mvn_extract_memory: the bytes extract_psf would allocate on the device for this stack and these counts."""
        ptr, desc, shape, dev = describe_stack(raw, int16_is_uint16)
        if as_device:
            desc.location = MVN_DEVICE
        need = C.c_size_t(0)
        self.check(self.l.mvn_extract_memory(C.byref(desc), _dims(shape), int(num_beads), _dims(psf_shape),
                                             int(bool(scores)), int(device), C.byref(need)))
        return need.value

    def extract_counters(self):
        """mvn_extract_counters: (launches of the gather, launches of the score pass, extractions completed)."""
        out = (C.c_longlong * 3)(0, 0, 0)
        self.check(self.l.mvn_extract_counters(out))
        return int(out[0]), int(out[1]), int(out[2])

    def extract_time(self, src_shape, num_beads, psf_shape, u16=True, reps=3, device=0):
        """mvn_extract_time: (ms per extraction of num_beads beads from a resident raw stack, ms for one resample pass
        per bead on the same stack and positions, ms per plain copy of num_beads windows)."""
        ms = (C.c_float * 3)(0, 0, 0)
        self.check(self.l.mvn_extract_time(int(device), int(bool(u16)), _dims(src_shape), int(num_beads),
                                           _dims(psf_shape), int(reps), ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # ---- bead detection (mvn_detect_beads) --------------------------------------------------
    def detect_beads(self, raw, sigma1, sigma2, threshold, minima=False, capacity=4096, device=None,
                     int16_is_uint16=False, as_device=False):
        """mvn_detect_beads: the beads of ONE view's raw stack `raw` (numpy array or torch tensor, float32 or uint16,
        host or device) - the strict 26-neighbour maxima (minima=True: minima) above `threshold` of the difference of
        its Gaussian blurs with sigma1 and sigma2 (one value or (z, y, x), raw voxels), in raster order, each with a
        quadratic sub-voxel fit.  Returns (positions (N, 3) float64 as extract_psf takes them, values (N,) float32,
        voxels (N, 3) int32).  More than `capacity` candidates raise MvnError; the message states their number."""
        ptr, desc, shape, dev = describe_stack(raw, int16_is_uint16)
        if as_device:
            desc.location = MVN_DEVICE
        prm = detect_params(sigma1, sigma2, threshold, DETECT_MINIMA if minima else 0)
        n = C.c_int(-1)
        pos = np.full((int(capacity), 3), np.nan, np.float64)
        val = np.full(int(capacity), np.nan, np.float32)
        vox = np.full((int(capacity), 3), -1, np.int32)
        stream = _caller_stream([raw])
        self.check(self.l.mvn_detect_beads(int(device if device is not None else (dev if dev is not None else -1)),
                                           C.c_void_p(ptr), C.byref(desc), _dims(shape), C.byref(prm), int(capacity),
                                           C.byref(n), pos.ctypes.data_as(C.POINTER(C.c_double)), fptr(val), iptr(vox),
                                           C.c_void_p(stream)))
        return pos[:n.value].copy(), val[:n.value].copy(), vox[:n.value].copy()

    def detect_taps(self, sigma):
        """mvn_detect_taps: the 2 R + 1 float32 taps of one sigma, R = ceil(3 sigma)."""
        taps = np.zeros(2 * DETECT_MAX_RADIUS + 1, np.float32)
        r = C.c_int(-1)
        self.check(self.l.mvn_detect_taps(float(sigma), fptr(taps), len(taps), C.byref(r)))
        return taps[:2 * r.value + 1].copy()

    def detect_dog(self, raw, sigma1, sigma2, device=None, int16_is_uint16=False, as_device=False):
        """mvn_detect_dog (test utility): the difference of the two blurs as a dense float32 array."""
        ptr, desc, shape, dev = describe_stack(raw, int16_is_uint16)
        if as_device:
            desc.location = MVN_DEVICE
        prm = detect_params(sigma1, sigma2, 0.0)
        out = np.full(shape, np.nan, np.float32)
        self.check(self.l.mvn_detect_dog(int(device if device is not None else (dev if dev is not None else -1)),
                                         C.c_void_p(ptr), C.byref(desc), _dims(shape), C.byref(prm), fptr(out)))
        return out

    def detect_memory(self, raw, capacity, device=0, int16_is_uint16=False, as_device=False):
        """mvn_detect_memory: the bytes detect_beads would allocate on the device for this stack and capacity."""
        ptr, desc, shape, dev = describe_stack(raw, int16_is_uint16)
        if as_device:
            desc.location = MVN_DEVICE
        need = C.c_size_t(0)
        self.check(self.l.mvn_detect_memory(C.byref(desc), _dims(shape), int(capacity), int(device), C.byref(need)))
        return need.value

    def detect_counters(self):
        """mvn_detect_counters: (launches of the blur passes, launches of the extremum pass, detections completed)."""
        out = (C.c_longlong * 3)(0, 0, 0)
        self.check(self.l.mvn_detect_counters(out))
        return int(out[0]), int(out[1]), int(out[2])

    def detect_time(self, src_shape, sigma1, sigma2, threshold, u16=True, reps=3, device=0):
        """mvn_detect_time: (ms per detection on a resident stack - all its device work, ms for its blur passes alone,
        ms per plain copy of one float32 volume)."""
        ms = (C.c_float * 3)(0, 0, 0)
        prm = detect_params(sigma1, sigma2, threshold)
        self.check(self.l.mvn_detect_time(int(device), int(bool(u16)), _dims(src_shape), C.byref(prm), int(reps), ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # ---- bead registration (mvn_register_beads) ----------------------------------------------
    @staticmethod
    def _beads(p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("bead lists are (N, 3)")
        return p

    def register_beads(self, a, b, max_error, ratio=3.0, hypotheses=1000, min_inliers=4, prior=None, seed=0, device=-1,
                       with_candidates=False):
        """mvn_register_beads: the affine matrix from the beads `a` of one view to the beads `b` of another ((N, 3)
        float64, z y x, as detect_beads returns them) - descriptor matching, RANSAC, a least-squares refit.  `prior`: a
        3 x 4 matrix applied to `a` for the descriptors (the stage rotation).  Returns (matrix (3, 4) float64 with
        b ~ matrix (a; 1), pairs (K, 2) int32 of inliers in ascending i, errors (mean, max) float64); without a model
        (None, an empty pairs array, None).  with_candidates=True appends the number of candidates."""
        a, b = self._beads(a), self._beads(b)
        prm = register_params(max_error, ratio, hypotheses, min_inliers, prior, seed)
        d_p = C.POINTER(C.c_double)
        m = np.full(12, np.nan, np.float64)
        pairs = np.full((max(1, min(len(a), len(b))), 2), -1, np.int32)
        err = np.full(2, np.nan, np.float64)
        nc, ni = C.c_int(-1), C.c_int(-1)
        self.check(self.l.mvn_register_beads(int(device), a.ctypes.data_as(d_p), len(a), b.ctypes.data_as(d_p), len(b),
                                             C.byref(prm), m.ctypes.data_as(d_p), C.byref(nc), C.byref(ni), iptr(pairs),
                                             err.ctypes.data_as(d_p), None))
        if ni.value > 0:
            out = (m.reshape(3, 4), pairs[:ni.value].copy(), err)
        else:
            out = (None, pairs[:0].copy(), None)
        return out + (nc.value,) if with_candidates else out

    def register_neighbours(self, p, device=-1):
        """mvn_register_neighbours (test utility): each point's 4 nearest others by (distance, index), (N, 4) int32."""
        p = self._beads(p)
        idx = np.full((len(p), 4), -1, np.int32)
        self.check(self.l.mvn_register_neighbours(int(device), p.ctypes.data_as(C.POINTER(C.c_double)), len(p), iptr(idx)))
        return idx

    def register_candidates(self, a, b, ratio=3.0, prior=None, device=-1):
        """mvn_register_candidates (test utility): (pairs (K, 2) int32, distances (K, 2) float32 of d1 and d2)."""
        a, b = self._beads(a), self._beads(b)
        prm = register_params(1.0, ratio, 1, 4, prior, 0)
        d_p = C.POINTER(C.c_double)
        cap = max(1, min(len(a), len(b)))
        pairs, d = np.full((cap, 2), -1, np.int32), np.full((cap, 2), np.nan, np.float32)
        n = C.c_int(-1)
        self.check(self.l.mvn_register_candidates(int(device), a.ctypes.data_as(d_p), len(a), b.ctypes.data_as(d_p), len(b),
                                                  C.byref(prm), C.byref(n), iptr(pairs), fptr(d)))
        return pairs[:n.value].copy(), d[:n.value].copy()

    def register_sample(self, seed, h, n):
        """mvn_register_sample: the four candidate indices of hypothesis h over n candidates."""
        out = np.full(4, -1, np.int32)
        self.check(self.l.mvn_register_sample(int(seed), int(h), int(n), iptr(out)))
        return out

    def register_memory(self, num_a, num_b, hypotheses=1000):
        """mvn_register_memory: the bytes register_beads would allocate on the device."""
        need = C.c_size_t(0)
        self.check(self.l.mvn_register_memory(int(num_a), int(num_b), int(hypotheses), C.byref(need)))
        return need.value

    def register_counters(self):
        """mvn_register_counters: (launches of the match pass, launches of the RANSAC pass, registrations completed)."""
        out = (C.c_longlong * 3)(0, 0, 0)
        self.check(self.l.mvn_register_counters(out))
        return int(out[0]), int(out[1]), int(out[2])

    def register_time(self, num_a, num_b, hypotheses, reps=3, device=0):
        """mvn_register_time: ms of (the neighbour and descriptor pass of both sets, the match pass, the RANSAC pass)."""
        ms = (C.c_float * 3)(0, 0, 0)
        self.check(self.l.mvn_register_time(int(device), int(num_a), int(num_b), int(hypotheses), int(reps), ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def resample_call(self, psi, raws, geoms, kernels1, kernels2, lambda_, min_value, iterations, weights=None,
                      int16_is_uint16=False):
        """The arguments of mvn_deconvolve_resampled as a ResampledCall (`.run(device)` makes the call, `.memory()` asks
        mvn_deconvolve_memory_resampled): `raws` are the raw stacks (numpy arrays or torch tensors, float32 or uint16),
        `geoms` their abi.view_geometry; `weights`: None = computed from the geometries and normalised
        (weights_mode 1), else one stack of psi's shape per view (weights_mode 0).  kernels2=None leaves kernel2_ and
        kernel2_dims_ NULL: for calls under set_kernel_derivation(1), where kernels1 are the raw PSFs."""
        n = len(raws)
        if not (len(geoms) == n and len(kernels1) == n and (kernels2 is None or len(kernels2) == n)
                and (weights is None or len(weights) == n)):
            raise ValueError("one geometry and two kernels per view")
        c = ResampledCall()
        c.binding, c.psi, c.mode = self, psi, 1 if weights is None else 0
        c.keep = [[np.ascontiguousarray(k, dtype=np.float32) for k in ks] for ks in (kernels1, kernels2 or [])]
        k1, k2 = c.keep
        c.psi_ptr, p_desc, shape, p_dev = describe_stack(psi)
        c.image, c.weights, c.geom = (StackDesc * n)(), (StackDesc * n)(), (ViewGeometry * n)()
        data = (ViewData * n)()
        devices = [p_dev]
        for v in range(n):
            i_ptr, c.image[v], i_shape, i_dev = describe_stack(raws[v], int16_is_uint16)
            if i_shape != tuple(geoms[v].src_dims):
                raise ValueError("view %d: the raw stack has shape %r, its geometry says %r"
                                 % (v, i_shape, tuple(geoms[v].src_dims)))
            c.geom[v] = geoms[v]
            devices.append(i_dev)
            d = data[v]
            if weights is not None:
                w_ptr, c.weights[v], w_shape, w_dev = describe_stack(weights[v])
                if w_shape != shape:
                    raise ValueError("view %d: weights have psi's shape %r" % (v, shape))
                devices.append(w_dev)
                d.weights_ = C.cast(C.c_void_p(w_ptr), c_float_p)
            dims = [np.array(s_, dtype=np.int32) for s_ in (shape, k1[v].shape, k2[v].shape if k2 else (), shape)]
            c.keep.append(dims)
            d.image_ = C.cast(C.c_void_p(i_ptr), c_float_p)
            d.kernel1_ = fptr(k1[v])
            d.image_dims_, d.kernel1_dims_, d.weights_dims_ = iptr(dims[0]), iptr(dims[1]), iptr(dims[3])
            if k2:
                d.kernel2_, d.kernel2_dims_ = fptr(k2[v]), iptr(dims[2])
        c.keep += [data, list(raws), list(weights or [])]
        c.ws = Workspace()
        c.ws.data_ = C.cast(data, C.POINTER(ViewData))
        c.ws.num_views_, c.ws.lambda_, c.ws.minValue_, c.ws.num_iterations_ = (
            n, float(lambda_), float(min_value), int(iterations))
        c.desc = CallDesc()
        c.desc.psi = p_desc
        c.desc.image = C.cast(c.image, C.POINTER(StackDesc))
        if weights is not None:
            c.desc.weights = C.cast(c.weights, C.POINTER(StackDesc))
        owners = [x for x in devices if x is not None]
        c.device = owners[0] if owners else 0
        return c

    def deconvolve_resampled(self, psi, raws, geoms, kernels1, kernels2, lambda_, min_value, iterations, weights=None,
                             device=None, int16_is_uint16=False):
        """mvn_deconvolve_resampled: the deconvolution from RAW views - each a stack as the camera delivered it plus an
        abi.view_geometry (matrix from block voxel to raw index, blend border and range); the library resamples them
        into psi's frame on the device and, with weights=None, computes and normalises the blend weights there too.
        Stacks may be what deconvolve_described takes.  psi is updated in place and returned."""
        return self.resample_call(psi, raws, geoms, kernels1, kernels2, lambda_, min_value, iterations, weights,
                                  int16_is_uint16).run(device)

    def deconvolve_submit(self, psi, holder, device=0):
        """mvn_deconvolve_submit: starts inplace_gpu_deconvolve on `psi` (C-contiguous float32, updated in
        place by the time deconvolve_wait returns) and returns the ticket.  `psi` and `holder` must be
        kept alive and untouched until then."""
        if not (psi.flags["C_CONTIGUOUS"] and psi.dtype == np.float32):
            raise ValueError("psi must be a C-contiguous float32 array")
        t = C.c_longlong(0)
        self.check(self.l.mvn_deconvolve_submit(fptr(psi), holder.ws, device, C.byref(t)))
        return t.value

    def deconvolve_wait(self, ticket):
        self.check(self.l.mvn_deconvolve_wait(ticket))

    def gpu_deconvolve_inplace(self, psi, holder, device=0):
        """The ABI call exactly as a host program makes it: `psi` (C-contiguous float32) is updated
        in place, the process-wide padding policy applies.  Returns the seconds spent inside the
        call (what the reference's bench times, bench/bench_gpu_deconvolve_synthetic.cu:190-203)."""
        import time
        if not (psi.flags["C_CONTIGUOUS"] and psi.dtype == np.float32):
            raise ValueError("psi must be a C-contiguous float32 array")
        t = time.perf_counter()
        self.l.inplace_gpu_deconvolve(fptr(psi), holder.ws, device)
        return time.perf_counter() - t

    def gpu_convolution(self, image, kernel, device=0, legacy=False):
        im = np.ascontiguousarray(image, dtype=np.float32).copy()
        k = np.ascontiguousarray(kernel, dtype=np.float32)
        idims = np.array(im.shape, np.int32)
        kdims = np.array(k.shape, np.int32)
        f = self.l.convolution3DfftCUDAInPlace if legacy else self.l.inplace_gpu_convolution
        f(fptr(im), iptr(idims), fptr(k), iptr(kdims), device)
        return im

    def compute_quotient(self, view, blurred, device=0):
        view = np.ascontiguousarray(view, dtype=np.float32)
        out = np.ascontiguousarray(blurred, dtype=np.float32).copy()
        self.l.compute_quotient(fptr(view), fptr(out), out.size, device)
        return out

    def compute_final_values(self, psi, integral, weight, min_value, lambda_, device=0):
        psi = np.ascontiguousarray(psi, dtype=np.float32).copy()
        integral = np.ascontiguousarray(integral, dtype=np.float32)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        self.l.compute_final_values(fptr(psi), fptr(integral), fptr(weight), psi.size, min_value,
                                    lambda_, device)
        return psi

    def psf_cache_counters(self):
        out = (C.c_long * 2)()
        self.check(self.l.mvn_psf_cache_counters(out))
        return int(out[0]), int(out[1])

    def iterate_fft(self, image, kernel, min_value=1e-4, lambda_=None, device=0):
        """iterate_fft_plain (lambda_ None; the reference fixes minValue = 1e-4 there) or
        iterate_fft_tikhonov: one legacy RL step on a single stack."""
        im = np.ascontiguousarray(image, dtype=np.float32)
        k = np.ascontiguousarray(kernel, dtype=np.float32)
        out = np.full_like(im, np.nan)
        idims = np.array(im.shape, np.int32)
        kdims = np.array(k.shape, np.int32)
        if lambda_ is None:
            self.l.iterate_fft_plain(fptr(im), fptr(k), fptr(out), iptr(idims), iptr(kdims), device)
        else:
            self.l.iterate_fft_tikhonov(fptr(im), fptr(k), fptr(out), iptr(idims), iptr(kdims),
                                        im.size, min_value, lambda_, device)
        return out

    # ---- transforms ------------------------------------------------------------------------
    def rfft3(self, x, device=0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        d0, d1, d2 = x.shape
        spec = np.empty((d0, d1, d2 // 2 + 1), dtype=np.complex64)
        self.check(self.l.mvn_fft3_r2c(device, _dims(x.shape), fptr(x), fptr(spec.view(np.float32))))
        return spec

    def irfft3(self, spec, d2, device=0):
        spec = np.ascontiguousarray(spec, dtype=np.complex64)
        d0, d1, nc = spec.shape
        assert nc == d2 // 2 + 1
        out = np.empty((d0, d1, d2), dtype=np.float32)
        self.check(self.l.mvn_fft3_c2r(device, _dims((d0, d1, d2)), fptr(spec.view(np.float32)), fptr(out)))
        return out

    def fft3_time(self, shape, direction=0, reps=10, device=0):
        ms = C.c_float(0)
        self.check(self.l.mvn_fft3_time(device, _dims(shape), direction, reps, C.byref(ms)))
        return ms.value

    def rfft3_many(self, stacks, device=0):
        """Forward r2c transform of [batch][d0][d1][d2] stacks through one plan."""
        x = np.ascontiguousarray(stacks, dtype=np.float32)
        batch, d0, d1, d2 = x.shape
        out = np.empty((batch, d0, d1, d2 // 2 + 1), np.complex64)
        self.check(self.l.mvn_fft3_many_r2c(device, _dims((d0, d1, d2)), batch, fptr(x),
                                            out.ctypes.data_as(c_float_p)))
        return out

    def fft3_many_time(self, shape, batch, direction=0, reps=5, device=0):
        ms = C.c_float(0)
        self.check(self.l.mvn_fft3_many_time(device, _dims(shape), batch, direction, reps, C.byref(ms)))
        return ms.value

    def fft3_profile(self, shape, direction=0, reps=10, device=0):
        ms = C.c_float(0)
        n = self.l.mvn_kernel_kind_count()
        per = (C.c_double * n)()
        self.check(self.l.mvn_fft3_profile(device, _dims(shape), direction, reps, C.byref(ms), per))
        return ms.value, {self.l.mvn_kernel_kind_name(k).decode(): per[k] for k in range(n) if per[k] > 0}

    def plan_describe(self, shape, device=0):
        out = (C.c_int * 12)()
        self.check(self.l.mvn_plan_describe(device, _dims(shape), out))
        keys = ["h", "C", "RP", "even", "rows_T", "ax1_T", "ax0_T", "n_stages", "fx_rows", "fx_ax1",
                "fx_ax0", "reserved"]
        return dict(zip(keys, list(out)))

    def engine(self, shape, num_views, device=0):
        return EngineHandle(self, shape, num_views, device)

    def slab_engine(self, shape, nranks, rank, num_views, device=0):
        return SlabHandle(self, shape, nranks, rank, num_views, device)

    def group(self, devices, shape, halo_planes, num_views):
        return GroupHandle(self, devices, shape, halo_planes, num_views)


class DescribedCall:
    """One prepared mvn_deconvolve_described call (Binding.describe_call); keeps what its pointers refer to alive."""

    def run(self, device=None):
        """makes the call (blocking); psi is updated in place and returned"""
        self.desc.stream = _caller_stream([self.psi] + self.keep[-2] + self.keep[-1])
        b = self.binding
        b.check(b.l.mvn_deconvolve_described(C.c_void_p(self.psi_ptr), self.ws, C.byref(self.desc),
                                             int(self.device if device is None else device)))
        return self.psi


class ResampledCall:
    """One prepared mvn_deconvolve_resampled call (Binding.resample_call); keeps what its pointers refer to alive."""

    def run(self, device=None):
        """makes the call (blocking); psi is updated in place and returned"""
        self.desc.stream = _caller_stream([self.psi] + self.keep[-2] + self.keep[-1])
        b = self.binding
        b.check(b.l.mvn_deconvolve_resampled(C.c_void_p(self.psi_ptr), self.ws, C.byref(self.desc), self.geom,
                                             self.mode, int(self.device if device is None else device)))
        return self.psi

    def memory(self, device=0):
        """mvn_deconvolve_memory_resampled: bytes of device memory the call needs (nothing is allocated)"""
        out = C.c_size_t(0)
        b = self.binding
        b.check(b.l.mvn_deconvolve_memory_resampled(self.ws, C.byref(self.desc), self.geom, self.mode, int(device),
                                                    C.byref(out)))
        return out.value


class GroupHandle:
    """One volume as dim0 slabs on several devices of this process (``mvn_group_*``; what MVN_DEVICES runs inside
    ``inplace_gpu_deconvolve``), stacks resident between ``load`` and ``get_psi``."""

    def __init__(self, binding, devices, shape, halo_planes, num_views):
        self.b = binding
        self.shape = tuple(int(s) for s in shape)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        binding.check(binding.l.mvn_group_create(devs, len(devices), _dims(shape), int(halo_planes), int(num_views),
                                                 C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.b.l.mvn_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, psi, holder):
        """psi and the stacks of a ``WorkspaceHolder`` (extents == the group's)"""
        psi = np.ascontiguousarray(psi, dtype=np.float32)
        assert psi.shape == self.shape
        self.b.check(self.b.l.mvn_group_load(self.h, fptr(psi), holder.ws))

    def iterate(self, iterations, lam, min_value):
        """blocking; returns the wall time of the sweeps in ms"""
        ms = C.c_float(0)
        self.b.check(self.b.l.mvn_group_iterate(self.h, int(iterations), float(lam), float(min_value), C.byref(ms)))
        return ms.value

    def get_psi(self):
        out = np.empty(self.shape, np.float32)
        self.b.check(self.b.l.mvn_group_get_psi(self.h, fptr(out)))
        return out


class EngineHandle:
    """Resident RL engine (``mvn_engine_*``)."""

    def __init__(self, binding, shape, num_views, device=0):
        self.b = binding
        self.shape = tuple(int(s) for s in shape)
        self.num_views = num_views
        self.device = device
        h = C.c_void_p()
        binding.check(binding.l.mvn_engine_create(device, _dims(shape), num_views, C.byref(h)))
        self.h = h
        self._keep = []

    def close(self):
        if self.h:
            self.b.l.mvn_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stack(x):
        """A stack as the engine's symbols take it: a tensor as it is; anything else as a numpy array - float32 or
        uint16, and copied to a dense one where the described symbols would refuse its layout in host memory (rows
        that are not contiguous, negative strides), as these methods always did."""
        if not isinstance(x, np.ndarray) and hasattr(x, "data_ptr"):
            return x
        a = np.asarray(x)
        if a.dtype != np.uint16 and a.dtype != np.float32:
            return np.ascontiguousarray(a, dtype=np.float32)
        it = a.itemsize
        ok = a.ndim == 3 and (all(st == 0 for st in a.strides) or (
            all(st >= 0 and st % it == 0 for st in a.strides) and (a.shape[2] == 1 or a.strides[2] == it)
            and (a.shape[1] == 1 or a.strides[1] >= a.shape[2] * it)))
        return a if ok else np.ascontiguousarray(a)

    @staticmethod
    def _plain(a):
        return isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]

    def set_view(self, v, image, weights, kernel1, kernel2):
        """image / weights: dense float32 arrays (the plain symbol), or anything Binding.deconvolve_described takes -
        uint16, strided, torch tensors on the host or the device (mvn_engine_set_view_described)."""
        k = [np.ascontiguousarray(x, dtype=np.float32) for x in (kernel1, kernel2)]
        image, weights = self._stack(image), self._stack(weights)
        if self._plain(image) and self._plain(weights):
            assert image.shape == self.shape and weights.shape == self.shape
            self.b.check(self.b.l.mvn_engine_set_view(self.h, v, fptr(image), fptr(weights), fptr(k[0]),
                                                      _dims(k[0].shape), fptr(k[1]), _dims(k[1].shape)))
            return
        i_ptr, i_desc, i_shape, _ = describe_stack(image)
        w_ptr, w_desc, w_shape, _ = describe_stack(weights)
        assert i_shape == self.shape and w_shape == self.shape
        self.b.check(self.b.l.mvn_engine_set_view_described(
            self.h, v, C.c_void_p(i_ptr), C.byref(i_desc), C.c_void_p(w_ptr), C.byref(w_desc), fptr(k[0]),
            _dims(k[0].shape), fptr(k[1]), _dims(k[1].shape), _caller_stream([image, weights])))

    def set_view_resampled(self, v, raw, geom, kernel1, kernel2, weights=None, int16_is_uint16=False):
        """mvn_engine_set_view_resampled: the raw stack `raw` through `geom` (abi.view_geometry) into view v.
        weights=None: computed from the geometry, unnormalised - call normalize_weights() after the last view."""
        k = [np.ascontiguousarray(x, dtype=np.float32) for x in (kernel1, kernel2)]
        i_ptr, i_desc, i_shape, _ = describe_stack(raw, int16_is_uint16)
        assert i_shape == tuple(geom.src_dims)
        w_ptr, w_desc = None, None
        if weights is not None:
            weights = self._stack(weights)
            w_ptr, w_desc, w_shape, _ = describe_stack(weights)
            assert w_shape == self.shape
        self.b.check(self.b.l.mvn_engine_set_view_resampled(
            self.h, v, C.c_void_p(i_ptr), C.byref(i_desc), C.byref(geom), C.c_void_p(w_ptr),
            C.byref(w_desc) if w_desc is not None else None, fptr(k[0]), _dims(k[0].shape), fptr(k[1]),
            _dims(k[1].shape), _caller_stream([raw] + ([weights] if weights is not None else []))))

    def normalize_weights(self):
        self.b.check(self.b.l.mvn_engine_normalize_weights(self.h))

    def fuse_psi(self, fill=0.0):
        """mvn_engine_fuse_psi: psi <- the fusion of the views as they stand (image and weights volumes), `fill` where
        no weight is positive."""
        self.b.check(self.b.l.mvn_engine_fuse_psi(self.h, float(fill)))

    def set_psi(self, psi):
        psi = self._stack(psi)
        if isinstance(psi, np.ndarray) and psi.dtype == np.uint16:
            psi = psi.astype(np.float32)
        if self._plain(psi):
            assert psi.shape == self.shape
            self.b.check(self.b.l.mvn_engine_set_psi(self.h, fptr(psi)))
            return
        ptr, desc, shape, _ = describe_stack(psi)
        assert shape == self.shape
        self.b.check(self.b.l.mvn_engine_set_psi_described(self.h, C.c_void_p(ptr), C.byref(desc),
                                                           _caller_stream([psi])))

    def get_psi(self, out=None):
        """A new dense float32 array, or psi written into `out`: a float32 numpy array (any non-overlapping strides
        with contiguous rows) or torch tensor (host or device), which is returned.  The call is blocking and has no
        stream of the caller's to order itself behind: for a tensor on the device, torch's current stream of that
        device is synchronised first, so that work enqueued there on `out` has ended before the library writes."""
        if out is None:
            out = np.empty(self.shape, np.float32)
            self.b.check(self.b.l.mvn_engine_get_psi(self.h, fptr(out)))
            return out
        ptr, desc, shape, _ = describe_stack(out)
        assert shape == self.shape
        if not isinstance(out, np.ndarray) and getattr(out, "is_cuda", False):
            import torch
            torch.cuda.current_stream(out.device).synchronize()
        self.b.check(self.b.l.mvn_engine_get_psi_described(self.h, C.c_void_p(ptr), C.byref(desc)))
        return out

    def iterate(self, iterations, lambda_, min_value, sync=True):
        self.b.check(self.b.l.mvn_engine_iterate(self.h, iterations, lambda_, min_value))
        if sync:
            self.sync()

    def iterate_converge(self, iterations, lambda_, min_value, tolerance):
        """mvn_engine_iterate_converge (blocking): (iterations run, float64 array [run, 3] of {S_k, M_k, P_k})."""
        run = C.c_int(0)
        stats = np.zeros((max(int(iterations), 1), 3), dtype=np.float64)
        self.b.check(self.b.l.mvn_engine_iterate_converge(self.h, iterations, lambda_, min_value, float(tolerance),
                                                          C.byref(run),
                                                          stats.ctypes.data_as(C.POINTER(C.c_double))))
        return run.value, (stats[:run.value].copy() if tolerance >= 0 else np.zeros((0, 3)))

    def set_regularization(self, kind, epsilon=0.0):
        """mvn_engine_set_regularization: the regulariser of the iterate* calls that follow."""
        self.b.check(self.b.l.mvn_engine_set_regularization(self.h, int(kind), float(epsilon)))

    def set_noise_model(self, background=None, likelihood=0):
        """mvn_engine_set_noise_model: one background per view (or None) and the likelihood switch of the iterate*
        calls that follow."""
        ptr = None
        if background is not None:
            vals = np.ascontiguousarray(background, dtype=np.float32).ravel()
            assert vals.size == self.num_views, "one background value per view"
            ptr = vals.ctypes.data_as(C.POINTER(C.c_float))
        self.b.check(self.b.l.mvn_engine_set_noise_model(self.h, ptr, int(likelihood)))

    def last_likelihood(self):
        """float64 array [sweeps run, V, 3] of {D, Y, M} of the last iterate* call (drains the stream)."""
        run = C.c_int(0)
        rows = self.b.check(self.b.l.mvn_engine_last_likelihood(self.h, C.byref(run), None, 0))
        out = np.zeros((rows, 3), dtype=np.float64)
        if rows:
            self.b.check(self.b.l.mvn_engine_last_likelihood(self.h, C.byref(run),
                                                             out.ctypes.data_as(C.POINTER(C.c_double)), rows))
        return out.reshape(-1, self.num_views, 3)

    def iterate_accelerated(self, iterations, lambda_, min_value, tolerance=-1.0):
        """mvn_engine_iterate_accelerated (blocking): (iterations run, [run, 3] statistics - empty with
        tolerance < 0 -, float64 array of a_1 .. a_run)."""
        run = C.c_int(0)
        stats = np.zeros((max(int(iterations), 1), 3), dtype=np.float64)
        alphas = np.zeros(max(int(iterations), 1), dtype=np.float64)
        self.b.check(self.b.l.mvn_engine_iterate_accelerated(self.h, iterations, lambda_, min_value, float(tolerance),
                                                             C.byref(run),
                                                             stats.ctypes.data_as(C.POINTER(C.c_double)),
                                                             alphas.ctypes.data_as(C.POINTER(C.c_double))))
        return (run.value, (stats[:run.value].copy() if tolerance >= 0 else np.zeros((0, 3))),
                alphas[:run.value].copy())

    def time_iterate(self, iterations, lambda_, min_value):
        ms = C.c_float(0)
        self.b.check(self.b.l.mvn_engine_time_iterate(self.h, iterations, lambda_, min_value, C.byref(ms)))
        return ms.value

    def compute_delta(self, lambda_, min_value):
        self.b.check(self.b.l.mvn_engine_compute_delta(self.h, lambda_, min_value))

    def apply_delta(self):
        self.b.check(self.b.l.mvn_engine_apply_delta(self.h))

    # the same step in pieces (all-reduce under compute): see include/mvn_engine_api.h
    def delta_chunks(self, wanted):
        return self.b.check(self.b.l.mvn_engine_delta_chunks(self.h, int(wanted)))

    def delta_chunk_range(self, c, n):
        a, cnt = C.c_size_t(), C.c_size_t()
        self.b.check(self.b.l.mvn_engine_delta_chunk_range(self.h, c, n, C.byref(a), C.byref(cnt)))
        return a.value, cnt.value

    def compute_delta_head(self, lambda_, min_value):
        self.b.check(self.b.l.mvn_engine_compute_delta_head(self.h, lambda_, min_value))

    def compute_delta_chunk(self, c, n):
        self.b.check(self.b.l.mvn_engine_compute_delta_chunk(self.h, c, n))

    def apply_delta_chunk(self, c, n, feed_next):
        self.b.check(self.b.l.mvn_engine_apply_delta_chunk(self.h, c, n, 1 if feed_next else 0))

    def _ptr(self, fn):
        p, n = C.c_void_p(), C.c_size_t()
        self.b.check(fn(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def delta_ptr(self):
        return self._ptr(self.b.l.mvn_engine_delta_ptr)

    def bind_delta(self, dev_ptr):
        self.b.check(self.b.l.mvn_engine_bind_delta(self.h, C.c_void_p(dev_ptr)))

    HALO_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int)

    def set_halo_hook(self, fn, drain=True, post=False):
        """fn(spectrum_ptr, view, conv) before every dim0 leg (mvn_engine_set_halo_hook); None switches it off.
        drain=False: fn is called without waiting for the engine's stream and must order its work on it.
        post=True: fn is called again behind the leg with conv + 2, where the slabs merge their poison words."""
        if fn is None:
            self._halo_cb = None
            self.b.check(self.b.l.mvn_engine_set_halo_hook(self.h, None, None, 1))
            return
        self._halo_cb = self.HALO_FN(lambda user, spectrum, view, conv: fn(spectrum, view, conv))
        self.b.check(self.b.l.mvn_engine_set_halo_hook(self.h, C.cast(self._halo_cb, C.c_void_p), None,
                                                       (1 if drain else 0) | (2 if post else 0)))

    def would_be_direct(self, kernel_shape):
        rc = self.b.l.mvn_engine_would_be_direct(self.h, _dims(kernel_shape))
        if rc < 0:
            self.b.check(rc)
        return rc == 1

    def set_halo_planes(self, planes, split=False):
        self.b.check(self.b.l.mvn_engine_set_halo_planes(self.h, int(planes), 1 if split else 0))

    def bind_poison(self, dev_ptr):
        self.b.check(self.b.l.mvn_engine_bind_poison(self.h, C.c_void_p(dev_ptr)))

    def poison_get(self):
        v = C.c_uint(0)
        self.b.check(self.b.l.mvn_engine_poison_get(self.h, C.byref(v)))
        return v.value

    def poison_merge(self, value):
        self.b.check(self.b.l.mvn_engine_poison_merge(self.h, C.c_uint(int(value))))

    def copy_planes(self, spectrum, plane0, nplanes, buffer_ptr, to_buffer, host_buffer=False, wait=True):
        self.b.check(self.b.l.mvn_engine_copy_planes(self.h, C.c_void_p(spectrum), plane0, nplanes,
                                                     C.c_void_p(buffer_ptr),
                                                     (1 if to_buffer else 0) | (2 if host_buffer else 0) |
                                                     (0 if wait else 4)))

    def psi_ptr(self):
        return self._ptr(self.b.l.mvn_engine_psi_ptr)

    def stream(self):
        p = C.c_void_p()
        self.b.check(self.b.l.mvn_engine_stream(self.h, C.byref(p)))
        return p.value

    def sync(self):
        self.b.check(self.b.l.mvn_engine_sync(self.h))

    def profile(self, enable):
        """enable: False/0 off, True/1 every launch, n > 1 the launches of every n-th (view, iteration)."""
        self.b.check(self.b.l.mvn_engine_profile(self.h, int(enable)))

    def profile_read(self):
        out = {}
        for k in range(self.b.l.mvn_kernel_kind_count()):
            ms, n = C.c_double(), C.c_long()
            self.b.check(self.b.l.mvn_engine_profile_read(self.h, k, C.byref(ms), C.byref(n)))
            out[self.b.l.mvn_kernel_kind_name(k).decode()] = (ms.value, n.value)
        return out

    def B(self):
        return self.b.l.mvn_engine_B(self.h)


_product = None


def lib():
    """The product library.  Raises if it has not been built (no fallback)."""
    global _product
    if _product is None:
        _product = Binding(PRODUCT_SO)
    return _product


class SlabHandle:
    """Slab-decomposed RL engine (``mvn_slab_*``): this rank's planes of a volume of `shape`."""

    def __init__(self, binding, shape, nranks, rank, num_views, device=0):
        self.b = binding
        self.shape = tuple(int(s) for s in shape)
        self.nranks, self.rank, self.num_views = nranks, rank, num_views
        self.slab_shape = (self.shape[0] // nranks, self.shape[1], self.shape[2])
        h = C.c_void_p()
        binding.check(binding.l.mvn_slab_create(device, _dims(self.shape), nranks, rank, num_views,
                                                C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.b.l.mvn_slab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _slab(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != self.slab_shape:
            raise ValueError("expected this rank's slab %r, got %r" % (self.slab_shape, a.shape))
        return a

    def set_view(self, v, image_slab, weights_slab, kernel1, kernel2):
        im, w = self._slab(image_slab), self._slab(weights_slab)
        k1 = np.ascontiguousarray(kernel1, dtype=np.float32)
        k2 = np.ascontiguousarray(kernel2, dtype=np.float32)
        self.b.check(self.b.l.mvn_slab_set_view(self.h, v, fptr(im), fptr(w), fptr(k1), _dims(k1.shape),
                                                fptr(k2), _dims(k2.shape)))

    def set_psi(self, psi_slab):
        self.b.check(self.b.l.mvn_slab_set_psi(self.h, fptr(self._slab(psi_slab))))
        self.b.check(self.b.l.mvn_slab_begin(self.h))

    def get_psi(self):
        out = np.empty(self.slab_shape, np.float32)
        self.b.check(self.b.l.mvn_slab_get_psi(self.h, fptr(out)))
        return out

    def buffer_sizes(self):
        a, b = C.c_size_t(0), C.c_size_t(0)
        self.b.check(self.b.l.mvn_slab_buffer_sizes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def buffers(self):
        p = [C.c_void_p() for _ in range(4)]
        self.b.check(self.b.l.mvn_slab_buffers(self.h, *[C.byref(x) for x in p]))
        return [x.value for x in p]

    def bind_buffers(self, a_main, b_main, a_nyq, b_nyq):
        self.b.check(self.b.l.mvn_slab_bind_buffers(self.h, a_main, b_main, a_nyq, b_nyq))

    def pack(self, v, conv):
        self.b.check(self.b.l.mvn_slab_pack(self.h, v, conv))

    def mid(self, v, conv):
        self.b.check(self.b.l.mvn_slab_mid(self.h, v, conv))

    def unpack(self, v, conv, lambda_, min_value, feed_next):
        self.b.check(self.b.l.mvn_slab_unpack(self.h, v, conv, lambda_, min_value, 1 if feed_next else 0))

    def sync(self):
        self.b.check(self.b.l.mvn_slab_sync(self.h))
