"""Density-based clustering of whole clouds: exact DBSCAN, and "keep the largest cluster(s)" on top of it (csrc/cluster.hip;
dispu_cluster_segments and dispu_cluster_select_segments in include/dispu_hip.h, which states the definition).  The reference has no
counterpart.  Plain Euclidean cluster extraction is dbscan at min_points = 1.

r2 = eps * eps in fp32; a point is core when at least min_points points of its cloud, itself included, lie at d2 <= r2; clusters are
the connected components of the core points under d2 <= r2, numbered by their smallest core index; a non-core point takes the label
of its nearest core point within r2 (ties to the lower index) or is noise, -1.  Clouds of a list never mix.  The labels are a pure
function of the input: identical bytes from run to run.  The yardstick is tests/cluster_oracle.py."""
import numpy as np
import torch

from . import _lib
from .outliers import INT_MAX, RULE_FLAGS, _check_radius, _compact
from .segments import Packed, check_int_range, host_ptr

KEEP_MIN, KEEP_MAX = 1, 32
STATUS_NON_FINITE, STATUS_CAP = 1, 2                             # bits of dispu_cluster_segments' status


def _cluster(b, eps, min_points, core=False, sizes=False):
    """-> labels [total] int32, core bytes or None, sizes [total] int32 or None, nclusters [C] int32, the scratch (its head holds the
    launch counters of include/dispu_hip.h)"""
    L = _lib.lib()
    nbytes = L.dispu_cluster_scratch_bytes(b.C, host_ptr(b.off))
    scratch = b.scratch(nbytes, "dispu_cluster_segments")
    labels = torch.full((b.total,), -1, dtype=torch.int32, device=b.dev)
    d_core = torch.zeros((b.total,), dtype=torch.uint8, device=b.dev) if core else None
    d_sizes = torch.empty((b.total,), dtype=torch.int32, device=b.dev) if sizes else None
    ncl = torch.zeros((b.C,), dtype=torch.int32, device=b.dev)
    _lib.check(L.dispu_cluster_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), eps, min_points, _lib.ptr(b.cloud), _lib.ptr(labels),
                                        _lib.ptr(d_core), _lib.ptr(d_sizes), _lib.ptr(ncl), _lib.ptr(b.status), _lib.ptr(scratch), nbytes,
                                        _lib.stream_ptr(b.dev)), "dispu_cluster_segments")
    return labels, d_core, d_sizes, ncl, scratch


def _refuse(b, status):
    """status: [C] on the host.  The non-finite refusal of the other whole-cloud operations, then the cap bit"""
    status = np.asarray(status)
    b.refuse_non_finite(torch.from_numpy((status & STATUS_NON_FINITE).astype(np.int32)))
    capped = np.nonzero(status & STATUS_CAP)[0]
    if len(capped):
        raise RuntimeError("dispu_cluster_segments: cloud %d left a capped loop short after the last launch" % int(capped[0]))


def _check(eps, min_points):
    return _check_radius(eps), check_int_range(min_points, 1, INT_MAX, "min_points")


def dbscan(points, eps, min_points=10, return_core=False, return_sizes=False):
    """points: a float32 [n, 3] tensor on a ROCm device, or a list of them (clouds of any sizes from 1 to 2^24 points, at most 65535;
    a list goes through the kernels as ONE packed launch sequence)  ->  labels [n] int32 (a list in gives lists out): the cluster of
    every point, 0, 1, ... in the order of the clusters' first core points, -1 for noise.  return_core: also a bool [n], True for a
    core point.  return_sizes: also an int32 vector with one entry per cluster, the points that carry its label.  Returns the labels,
    or a tuple (labels, core, sizes) with the parts asked for, in that order.
    eps is rounded to float32 and must then be finite and > 0 (messages call it the radius); min_points >= 1 counts the point itself.
    ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    b = Packed(points, "dbscan", words=3)
    eps, min_points = _check(eps, min_points)
    b.pack()
    with torch.cuda.device(b.dev):
        labels, core, sizes, ncl, _ = _cluster(b, eps, min_points, core=return_core, sizes=return_sizes)
        host = torch.cat([b.status, ncl]).cpu().numpy()                         # the one read-back
    _refuse(b, host[:b.C])
    res = [b.split(labels)]
    if return_core:
        res.append(b.split(core.bool()))
    if return_sizes:
        per = [sizes[int(b.off[c]):int(b.off[c]) + int(host[b.C + c])] for c in range(b.C)]
        res.append(per[0] if b.single else per)
    return res[0] if len(res) == 1 else tuple(res)


def keep_clusters(points, eps, min_points=1, keep=1, min_size=1, return_index=False, return_labels=False):
    """Keep the points of the `keep` largest clusters of dbscan(points, eps, min_points) among those of at least min_size points
    (size descending, ties to the lower cluster id; 1 <= keep <= 32, min_size >= 1)  ->  the kept points [m, 3] in input order,
    possibly [0, 3] (a list in gives lists out).  return_index: also the kept indices [m] int64, ascending.  return_labels: also the
    labels [n] int32 of ALL points, as dbscan returns them.  Returns the points, or a tuple (points, index, labels) with the parts
    asked for, in that order.  ValueError as for dbscan."""
    b = Packed(points, "keep_clusters", words=3)
    eps, min_points = _check(eps, min_points)
    keep = check_int_range(keep, KEEP_MIN, KEEP_MAX, "keep")
    min_size = check_int_range(min_size, 1, INT_MAX, "min_size")
    b.pack()
    with torch.cuda.device(b.dev):
        L = _lib.lib()
        labels, _, sizes, ncl, _ = _cluster(b, eps, min_points, sizes=True)
        flags = torch.zeros((b.total,), dtype=torch.int32, device=b.dev)
        _lib.check(L.dispu_cluster_select_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), _lib.ptr(labels), _lib.ptr(sizes), _lib.ptr(ncl),
                                                   _lib.ptr(b.status), keep, min_size, _lib.ptr(flags), _lib.stream_ptr(b.dev)),
                   "dispu_cluster_select_segments")
        pts, idx, new_off, status = _compact(b, RULE_FLAGS, flags, None, 0)     # the one read-back
    _refuse(b, status)
    res = [b.split(pts, new_off)]
    if return_index:
        res.append(b.split(idx.long(), new_off))
    if return_labels:
        res.append(b.split(labels))
    return res[0] if len(res) == 1 else tuple(res)
