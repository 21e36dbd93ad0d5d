"""Rigid registration: bring one cloud into another's frame by iterative closest point (csrc/icp.hip; dispu_icp_segments in
include/dispu_hip.h, which states the operator).  Several scans of one object taken from different poses become one cloud.  The
reference has no counterpart.

Per iteration and pair: the source under the current motion, its exact nearest target point under the project's rule (a cell-pruned
search over both clouds), the point-to-point or point-to-plane normal equations summed in a fixed order in double, a Cholesky solve
and the update of the motion, all on the device with no read-back between the steps.  The yardstick is tests/icp_oracle.py."""
import collections
import math

import numpy as np
import torch

from . import _lib
from ._util import req
from .segments import Pair, Packed, check_int_range, host_ptr

ITER_MIN, ITER_MAX = 0, 128

Registration = collections.namedtuple("Registration", "transform aligned fitness rmse iterations converged degenerate correspondences")


def _number(v, name, allow_inf):
    ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
    ok = ok and not math.isnan(float(v)) and float(v) >= 0.0 and (allow_inf or math.isfinite(float(v)))
    req(ok, "%s must be a %s number >= 0, got %r" % (name, "non-NaN" if allow_inf else "finite", v))
    return float(v)


def _transforms(t, C, single, dev, name):
    """a [4, 4] (single pair) or [C, 4, 4] tensor, or a list of C [4, 4] tensors -> float64 [C, 16] on dev"""
    if isinstance(t, (list, tuple)):
        req(len(t) == C and all(isinstance(m, torch.Tensor) for m in t), "%s: expected %d [4, 4] tensors" % (name, C))
        req(all(tuple(m.shape) == (4, 4) for m in t), "%s: every transform must be [4, 4]" % name)
        t = torch.stack([m.to(device=dev, dtype=torch.float64) for m in t])
    req(isinstance(t, torch.Tensor), "%s: expected a [4, 4] or [%d, 4, 4] tensor, got %s" % (name, C, type(t).__name__))
    if t.dim() == 2 and single:
        t = t[None]
    req(tuple(t.shape) == (C, 4, 4), "%s: expected shape %s, got %s" % (name, "[4, 4]" if single else "[%d, 4, 4]" % C, tuple(t.shape)))
    req(t.is_floating_point(), "%s must be a floating-point tensor, got %s" % (name, t.dtype))
    return t.to(device=dev, dtype=torch.float64).reshape(C, 16).contiguous()


def icp(source, target, target_normals=None, init=None, max_distance=float("inf"), iterations=30, tolerance=1e-6,
        return_correspondences=False):
    """source, target: float32 [q, 3] and [m, 3] tensors on a ROCm device, or two lists of them (pairs of clouds of any sizes from 1 to
    2^24 points, at most 65535 pairs; lists go through the kernels as ONE packed launch sequence).  target_normals: unit normals of the
    target, shaped like it: given, the residual is point to plane (their sign does not matter), else point to point.
    init: float [4, 4] ([C, 4, 4] or a list for lists) starting motion, default the identity.  max_distance: a source point farther
    than this from its nearest target point is left out of the step (inf: none is).  0 <= iterations <= 128 (0: evaluate init).
    tolerance: a pair stops once its update turns by at most tolerance radians and moves by at most tolerance * the target's
    bounding-box diagonal; 0 runs every iteration.
    -> Registration(transform float64 [4, 4] mapping source coordinates into the target's frame, aligned float32 [q, 3], fitness =
    inliers / q, rmse over the inliers' residuals, iterations applied, converged, degenerate, correspondences int32 [q] (the target index
    per aligned point, -1 for a point beyond max_distance; None unless asked for)); for lists the per-pair fields are tensors of length
    C and transform is [C, 4, 4], aligned and correspondences lists.  Everything stays on the device.  A degenerate pair (too few
    inliers, or equations that do not fix the motion) keeps the motion it had.
    ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    req(target is not None, "icp needs a target")
    b = Pair(source, target, "icp", name="target")
    normals = None
    if target_normals is not None:
        nb = Packed(target_normals, "icp", label="target_normals of cloud %d", dev=b.dev, home="the queries of cloud 0")
        req(nb.single == b.single and nb.C == b.C and np.array_equal(nb.off, b.refs.off), "target_normals must be shaped like target")
        normals = nb
    iterations = check_int_range(iterations, ITER_MIN, ITER_MAX, "iterations")
    max_distance = _number(max_distance, "max_distance", True)
    tolerance = _number(tolerance, "tolerance", False)
    t0 = None if init is None else _transforms(init, b.C, b.single, b.dev, "init")
    max_d2 = float(np.float32(np.float64(max_distance) * np.float64(max_distance)))
    b.pack("dispu_icp_scratch_bytes")
    with torch.cuda.device(b.dev):
        nrm = None if normals is None else normals.pack_like(normals.clouds)
        T = torch.empty((b.C, 4, 4), dtype=torch.float64, device=b.dev)
        aligned = torch.empty((b.nq, 3), dtype=torch.float32, device=b.dev)
        corr = torch.empty((b.nq,), dtype=torch.int32, device=b.dev) if return_correspondences else None
        inl, its, flag = (torch.zeros((b.C,), dtype=torch.int32, device=b.dev) for _ in range(3))
        rmse = torch.zeros((b.C,), dtype=torch.float64, device=b.dev)
        _lib.check(_lib.lib().dispu_icp_segments(*(b.head() + (0 if nrm is None else 1, iterations, max_d2, tolerance,
                                                               _lib.ptr(b.queries.cloud), _lib.ptr(b.refs.cloud), _lib.ptr(nrm), _lib.ptr(t0),
                                                               _lib.ptr(T), _lib.ptr(aligned), _lib.ptr(corr), _lib.ptr(inl), _lib.ptr(rmse),
                                                               _lib.ptr(its), _lib.ptr(flag)) + b.tail())), "dispu_icp_segments")
        b.queries.refuse_non_finite()
        counts = torch.from_numpy(np.diff(b.queries.off).astype(np.float64)).to(b.dev)
        fitness = inl.to(torch.float64) / counts
    one = (lambda v: v[0]) if b.single else (lambda v: v)
    return Registration(one(T), b.queries.split(aligned), one(fitness), one(rmse), one(its), one(flag == 1), one(flag == 2),
                        b.queries.split(corr) if return_correspondences else None)


def apply_transform(points, transform):
    """points: a float32 [n, 3] tensor on a ROCm device or a list of them; transform: [4, 4] ([C, 4, 4] or a list for a list), any float
    dtype -> new float32 tensors: (float)(R p + t) with the products and sums in float64, the rounding of icp's `aligned`."""
    b = Packed(points, "apply_transform")
    t = _transforms(transform, b.C, b.single, b.dev, "transform")
    b.pack(status=False)
    with torch.cuda.device(b.dev):
        out = torch.empty((b.total, 3), dtype=torch.float32, device=b.dev)
        _lib.check(_lib.lib().dispu_rigid_apply_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), _lib.ptr(b.cloud), _lib.ptr(t), _lib.ptr(out),
                                                         _lib.stream_ptr(b.dev)), "dispu_rigid_apply_segments")
    return b.split(out)
