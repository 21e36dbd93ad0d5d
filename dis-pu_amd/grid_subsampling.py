"""Grid subsampling on the device: every point that falls into a cube of edge sampleDl is replaced by the cube's barycentre, with the
mean feature and the most frequent label of the cube -- the reference's CPython extension `grid_subsampling`
(libs/cpp_wrappers/cpp_subsampling, wrapper.cpp:58-285 over grid_subsampling.cpp:5-106), the KPConv voxel-grid subsampler that thins a
dense, uneven scan to an even spacing before patches are taken from it.

compute() mirrors the wrapper's signature.  The outputs are the reference's bit for bit, with the two things it leaves to
std::unordered_map defined (include/dispu_hip.h: dispu_grid_subsample_plan): rows come in ascending key order, and a tie between label
counts goes to the smallest label.  Kernels: csrc/grid_subsample.hip, csrc/radix_sort.hip; the yardstick is tests/grid_subsample_oracle.py.
A single cloud per call; packed batches of clouds are out of scope."""
import ctypes as C
import math

import numpy as np

METHODS = ("barycenters", "voxelcenters")            # wrapper.cpp:86: both names are accepted, and both compute barycentres (:215)


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _check_args(points, features, classes, sampleDl, method):
    """every check that needs no device (ValueError) -> (n, fdim, ldim)"""
    _req(method in METHODS, "Error parsing method. Valid method names are \"barycenters\" and \"voxelcenters\" (got %r)" % (method,))
    try:
        dl = float(sampleDl)
    except (TypeError, ValueError):
        raise ValueError("sampleDl must be a number, got %r" % (sampleDl,))
    _req(math.isfinite(dl) and dl > 0.0, "sampleDl must be finite and > 0, got %r" % (sampleDl,))
    with np.errstate(over="ignore", under="ignore"):
        dl32 = float(np.float32(dl))                 # the wrapper parses sampleDl as a C float
    _req(math.isfinite(dl32) and dl32 > 0.0, "sampleDl %r is not a positive finite float32" % (sampleDl,))
    for x, name in ((points, "points"), (features, "features"), (classes, "classes")):
        _req(x is None or hasattr(x, "shape"), "%s must be a numpy array or a tensor on a ROCm device" % name)
    _req(points is not None and len(points.shape) == 2 and points.shape[1] == 3, "Wrong dimensions : points.shape is not (N, 3)")
    n = int(points.shape[0])
    _req(n > 0, "points must not be empty")
    _req(n < 2 ** 31, "%d points: at most 2^31 - 1 per call" % n)
    fdim = ldim = 0
    if features is not None:
        _req(len(features.shape) == 2 and features.shape[0] == n, "Wrong dimensions : features.shape is not (N, d)")
        fdim = int(features.shape[1])
    if classes is not None:
        _req(len(classes.shape) in (1, 2) and classes.shape[0] == n, "Wrong dimensions : classes.shape is not (N,) or (N, d)")
        ldim = 1 if len(classes.shape) == 1 else int(classes.shape[1])
    kinds = set(_is_tensor(x) for x in (points, features, classes) if x is not None)
    _req(len(kinds) == 1, "points, features and classes must be all numpy arrays or all tensors")
    return n, fdim, ldim


def _raise_on_status(status, sampleDl, grid):
    """turn a refusal of dispu_grid_subsample_plan into a ValueError"""
    from . import _lib
    if status == 0:
        return
    if status == _lib.GRID_NONFINITE:
        raise ValueError("grid_subsampling: points has a NaN or infinite coordinate")
    if status in (_lib.GRID_AXIS_X, _lib.GRID_AXIS_Y, _lib.GRID_AXIS_Z):
        raise ValueError("grid_subsampling: the %s axis would have more than 2^21 cells of edge %g (voxel keys must stay below 2^63): "
                         "use a larger sampleDl" % ("xyz"[status - _lib.GRID_AXIS_X], sampleDl))
    if status == _lib.GRID_TOO_MANY_POINTS:
        raise ValueError("grid_subsampling: at most 2^31 - 1 points per call")
    raise ValueError("grid_subsampling: unknown refusal %d" % status)


def compute(points, features=None, classes=None, sampleDl=0.1, method="barycenters", verbose=0):
    """points [n,3] float32, features [n,fdim] float32, classes [n] or [n,ldim] int32 -> the subsampled points [m,3], or a tuple with the
    features [m,fdim] and / or the classes [m,ldim] in that order (wrapper.cpp:269-276).  numpy arrays in give numpy arrays out (any
    dtype is converted like PyArray_FROM_OTF does); tensors on a ROCm device in give tensors out, computed on the current stream, and
    must already be float32 / int32.  Rows are in ascending voxel-key order.  The call is synchronous: it reads the bounds and the voxel
    count back."""
    points, features, classes = (x if x is None or _is_tensor(x) else np.asarray(x) for x in (points, features, classes))
    n, fdim, ldim = _check_args(points, features, classes, sampleDl, method)
    import torch
    from . import _lib
    from ._util import f32, i32
    as_numpy = not _is_tensor(points)
    if as_numpy:
        _req(torch.cuda.is_available(), "grid_subsampling needs a ROCm device (there is no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device())
        p = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev)
        f = torch.from_numpy(np.ascontiguousarray(features, np.float32)).to(dev) if fdim else None
        c = torch.from_numpy(np.ascontiguousarray(classes, np.int32)).to(dev) if ldim else None
    else:
        p = f32(points, "points")
        dev = p.device
        f = f32(features, "features") if fdim else None
        c = i32(classes, "classes") if ldim else None
        _req(all(t is None or t.device == dev for t in (f, c)), "points, features and classes live on different devices")
    dl = float(np.float32(sampleDl))
    L = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = L.dispu_grid_subsample_scratch_bytes(n, fdim, ldim)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        m, status, grid = C.c_int(0), C.c_int(0), (C.c_double * 8)()
        _lib.check(L.dispu_grid_subsample_plan(n, _lib.ptr(p), dl, _lib.ptr(scratch), nbytes, C.byref(m), C.byref(status), grid,
                                               _lib.stream_ptr(dev)), "dispu_grid_subsample_plan")
        _raise_on_status(status.value, dl, grid)
        m = m.value
        if verbose:
            print("grid_subsampling: %d -> %d points, dl %g, origin (%g, %g, %g), grid %d x %d x %d, %d sort passes"
                  % (n, m, dl, grid[0], grid[1], grid[2], grid[3], grid[4], grid[5], grid[6]))
        out_p = torch.empty((m, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((m, fdim), dtype=torch.float32, device=dev) if features is not None else None
        out_c = torch.empty((m, ldim), dtype=torch.int32, device=dev) if classes is not None else None
        _lib.check(L.dispu_grid_subsample_emit(n, m, fdim, ldim, _lib.ptr(p), _lib.ptr(f), _lib.ptr(c), _lib.ptr(scratch), nbytes,
                                               _lib.ptr(out_p), _lib.ptr(out_f) if fdim else None, _lib.ptr(out_c) if ldim else None,
                                               _lib.stream_ptr(dev)), "dispu_grid_subsample_emit")
    outs = [out_p] + [o for o in (out_f, out_c) if o is not None]
    if as_numpy:
        outs = [o.cpu().numpy() for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)
