"""ctypes mirror of the reference C-ABI structs (``inc/multiviewnative.h:15-35``).

Lays the structs out exactly as JNA does for Fiji (x86-64 SysV, default alignment):
``view_data`` = 8 pointers (64 B); ``workspace`` = ``view_data*`` @0, ``unsigned short``
@8, ``double`` @16, ``float`` @24, ``int`` @28 (32 B), passed BY VALUE to the
deconvolve entry points (``inc/multiviewnative.h:50,66``).
"""
import ctypes as C

import numpy as np

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)


class ViewData(C.Structure):
    _fields_ = [
        ("image_", c_float_p),
        ("kernel1_", c_float_p),
        ("kernel2_", c_float_p),
        ("weights_", c_float_p),
        ("image_dims_", c_int_p),
        ("kernel1_dims_", c_int_p),
        ("kernel2_dims_", c_int_p),
        ("weights_dims_", c_int_p),
    ]


class Workspace(C.Structure):
    _fields_ = [
        ("data_", C.POINTER(ViewData)),
        ("num_views_", C.c_ushort),
        ("lambda_", C.c_double),
        ("minValue_", C.c_float),
        ("num_iterations_", C.c_int),
    ]


assert C.sizeof(ViewData) == 64
assert C.sizeof(Workspace) == 32
assert Workspace.lambda_.offset == 16 and Workspace.minValue_.offset == 24
assert Workspace.num_iterations_.offset == 28


# ---- described stacks (include/mvn_engine_api.h: mvn_stack_desc, mvn_call_desc) --------------------------------
MVN_F32, MVN_U16 = 0, 1
MVN_HOST, MVN_DEVICE = 0, 1


class StackDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int),
        ("location", C.c_int),
        ("stride", C.c_longlong * 3),
    ]


class CallDesc(C.Structure):
    _fields_ = [
        ("psi", StackDesc),
        ("image", C.POINTER(StackDesc)),
        ("weights", C.POINTER(StackDesc)),
        ("stream", C.c_void_p),
    ]


assert C.sizeof(StackDesc) == 32 and StackDesc.stride.offset == 8
assert C.sizeof(CallDesc) == 56
assert (CallDesc.image.offset, CallDesc.weights.offset, CallDesc.stream.offset) == (32, 40, 48)


class ViewGeometry(C.Structure):
    """mvn_view_geometry: a raw stack's extents, the 3 x 4 matrix from block voxel to raw index, and the blend."""
    _fields_ = [
        ("src_dims", C.c_int * 3),
        ("matrix", C.c_double * 12),
        ("blend_border", C.c_float * 3),
        ("blend_range", C.c_float * 3),
    ]


assert C.sizeof(ViewGeometry) == 136 and ViewGeometry.matrix.offset == 16 and ViewGeometry.blend_border.offset == 112


def view_geometry(src_shape, matrix, border=(0, 0, 0), blend_range=(0, 0, 0)):
    """A ViewGeometry from a raw stack's shape, a 3 x 4 (or 12-element) matrix, and per-axis border / range."""
    g = ViewGeometry()
    m = np.asarray(matrix, dtype=np.float64).reshape(12)
    for k in range(3):
        g.src_dims[k] = int(src_shape[k])
        g.blend_border[k] = float(border[k])
        g.blend_range[k] = float(blend_range[k])
    for i in range(12):
        g.matrix[i] = float(m[i])
    return g


class DetectParams(C.Structure):
    """mvn_detect_params: the two sigmas per raw axis, the threshold and the flags of mvn_detect_beads."""
    _fields_ = [
        ("sigma1", C.c_double * 3),
        ("sigma2", C.c_double * 3),
        ("threshold", C.c_float),
        ("flags", C.c_int),
    ]


assert C.sizeof(DetectParams) == 56 and DetectParams.threshold.offset == 48 and DetectParams.flags.offset == 52


def detect_params(sigma1, sigma2, threshold, flags=0):
    """A DetectParams from one sigma or three per set (z, y, x)."""
    p = DetectParams()
    s1 = np.broadcast_to(np.asarray(sigma1, np.float64), (3,))
    s2 = np.broadcast_to(np.asarray(sigma2, np.float64), (3,))
    for k in range(3):
        p.sigma1[k], p.sigma2[k] = float(s1[k]), float(s2[k])
    p.threshold, p.flags = float(threshold), int(flags)
    return p


class RegisterParams(C.Structure):
    """mvn_register_params: the prior, the inlier bound, the ratio, the hypotheses, the flags and the seed of
    mvn_register_beads."""
    _fields_ = [
        ("prior", C.c_double * 12),
        ("max_error", C.c_double),
        ("ratio", C.c_float),
        ("hypotheses", C.c_int),
        ("min_inliers", C.c_int),
        ("flags", C.c_int),
        ("seed", C.c_ulonglong),
    ]


assert C.sizeof(RegisterParams) == 128 and RegisterParams.ratio.offset == 104 and RegisterParams.seed.offset == 120


def register_params(max_error, ratio=3.0, hypotheses=1000, min_inliers=4, prior=None, seed=0, flags=None):
    """A RegisterParams; a `prior` (3 x 4 or 12 elements) sets MVN_REGISTER_PRIOR unless `flags` is given."""
    p = RegisterParams()
    if prior is not None:
        m = np.asarray(prior, dtype=np.float64).reshape(12)
        for i in range(12):
            p.prior[i] = float(m[i])
    p.max_error, p.ratio, p.hypotheses, p.min_inliers = float(max_error), float(ratio), int(hypotheses), int(min_inliers)
    p.flags = int(flags) if flags is not None else (1 if prior is not None else 0)
    p.seed = int(seed)
    return p


def _is_tensor(a):
    # (torch is never imported here: an object that is not a numpy array and has these is taken for a tensor)
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr") and hasattr(a, "stride")


def describe_stack(a, int16_is_uint16=False):
    """(pointer, StackDesc, shape, device index or None) of a numpy array (float32 / uint16, strides that are
    multiples of the item size) or a torch tensor (CPU or cuda; float32 or uint16; int16 only with int16_is_uint16,
    for a torch without uint16: the bits are then read as uint16)."""
    d = StackDesc()
    device = None
    if _is_tensor(a):
        name = str(a.dtype)
        if name == "torch.float32":
            d.dtype = MVN_F32
        elif name == "torch.uint16" or (name == "torch.int16" and int16_is_uint16):
            d.dtype = MVN_U16
        else:
            raise TypeError("stacks are float32 or uint16, not %s" % name)
        ptr, strides, shape = a.data_ptr(), tuple(a.stride()), tuple(a.shape)
        if a.is_cuda:
            d.location = MVN_DEVICE
            device = a.device.index
        else:
            d.location = MVN_HOST
    else:
        a = np.asarray(a)
        if a.dtype == np.float32:
            d.dtype = MVN_F32
        elif a.dtype == np.uint16:
            d.dtype = MVN_U16
        else:
            raise TypeError("stacks are float32 or uint16, not %s" % a.dtype)
        if any(st % a.itemsize for st in a.strides):
            raise ValueError("strides must be multiples of the item size")
        ptr, strides, shape = a.ctypes.data, tuple(st // a.itemsize for st in a.strides), a.shape
        d.location = MVN_HOST
    if len(shape) != 3:
        raise ValueError("stacks are 3-D")
    for k in range(3):
        d.stride[k] = int(strides[k])
    return ptr, d, tuple(int(x) for x in shape), device


def fptr(a):
    return a.ctypes.data_as(c_float_p)


def iptr(a):
    return a.ctypes.data_as(c_int_p)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class WorkspaceHolder:
    """Owns the numpy arrays a ``workspace`` points to (the ABI never copies or frees them)."""

    def __init__(self, views, kernels1, kernels2, weights, lambda_=0.006, min_value=1e-4,
                 iterations=1):
        self.views = [as_f32(v) for v in views]
        self.kernels1 = [as_f32(k) for k in kernels1]
        self.kernels2 = [as_f32(k) for k in kernels2]
        self.weights = [as_f32(w) for w in weights]
        n = len(self.views)
        assert len(self.kernels1) == n and len(self.kernels2) == n and len(self.weights) == n
        self._dims = []
        self.data = (ViewData * n)()
        for v in range(n):
            dims = [np.array(a.shape, dtype=np.int32) for a in
                    (self.views[v], self.kernels1[v], self.kernels2[v], self.weights[v])]
            self._dims.append(dims)
            d = self.data[v]
            d.image_, d.kernel1_, d.kernel2_, d.weights_ = (
                fptr(self.views[v]), fptr(self.kernels1[v]), fptr(self.kernels2[v]),
                fptr(self.weights[v]))
            d.image_dims_, d.kernel1_dims_, d.kernel2_dims_, d.weights_dims_ = (
                iptr(dims[0]), iptr(dims[1]), iptr(dims[2]), iptr(dims[3]))
        self.ws = Workspace()
        self.ws.data_ = C.cast(self.data, C.POINTER(ViewData))
        self.ws.num_views_ = n
        self.ws.lambda_ = float(lambda_)
        self.ws.minValue_ = float(min_value)
        self.ws.num_iterations_ = int(iterations)

    def with_iterations(self, iterations):
        self.ws.num_iterations_ = int(iterations)
        return self
