"""Outlier removal for whole clouds: the statistical filter (mean distance to the k nearest neighbours against the cloud's mean +
std_ratio * std) and the radius filter (fewer than min_neighbors points within radius), in one kernel family (csrc/outliers.hip;
dispu_knn_mean_dist_segments, dispu_radius_count_segments, dispu_outlier_threshold_segments and dispu_compact_segments in
include/dispu_hip.h, which states every definition).  The reference has no counterpart.

The k nearest neighbours are the exact ones of normals.estimate_normals (the same search, at k + 1 with the point itself), distances
in plain fp32 arithmetic; neighbourhoods never cross clouds.  The yardstick is tests/outliers_oracle.py."""
import math

import numpy as np
import torch

from . import _lib
from ._util import req
from .segments import Packed, check_int_range, host_ptr, is_int

K_MIN, K_MAX = 1, 31
INT_MAX = 2 ** 31 - 1
RULE_FLAGS, RULE_MEAN_DIST, RULE_COUNT = 0, 1, 2                 # dispu_compact_segments' rule


def _check_radius(radius):
    req(isinstance(radius, (int, float, np.integer, np.floating)) and not isinstance(radius, bool), "radius must be a number, got %r" % (radius,))
    with np.errstate(over="ignore"):
        r = float(np.float32(radius))
    req(math.isfinite(r) and r > 0.0, "radius must be finite and > 0 as a float32, got %r" % (radius,))
    return r


def _mean_dist(b, k):
    L = _lib.lib()
    nbytes = L.dispu_knn_mean_dist_scratch_bytes(b.C, host_ptr(b.off), k)
    scratch = b.scratch(nbytes, "dispu_knn_mean_dist_segments")
    out = torch.zeros((b.total,), dtype=torch.float32, device=b.dev)
    _lib.check(L.dispu_knn_mean_dist_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), k, _lib.ptr(b.cloud), _lib.ptr(out),
                                              _lib.ptr(b.status), _lib.ptr(scratch), nbytes, _lib.stream_ptr(b.dev)),
               "dispu_knn_mean_dist_segments")
    return out


def _radius_count(b, radius, cap):
    L = _lib.lib()
    nbytes = L.dispu_radius_count_scratch_bytes(b.C, host_ptr(b.off))
    scratch = b.scratch(nbytes, "dispu_radius_count_segments")
    out = torch.zeros((b.total,), dtype=torch.int32, device=b.dev)
    _lib.check(L.dispu_radius_count_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), radius, cap, _lib.ptr(b.cloud), _lib.ptr(out),
                                             _lib.ptr(b.status), _lib.ptr(scratch), nbytes, _lib.stream_ptr(b.dev)),
               "dispu_radius_count_segments")
    return out


def _compact(b, rule, src, stats, min_neighbors):
    """-> (kept points [m, 3], kept local indices [m] int32, new offsets [C + 1] on the host, the status read back with them)"""
    L = _lib.lib()
    nbytes = L.dispu_compact_scratch_bytes(b.C, host_ptr(b.off))
    scratch = b.scratch(nbytes, "dispu_compact_segments")
    pts = torch.empty((b.total, 3), dtype=torch.float32, device=b.dev)
    idx = torch.empty((b.total,), dtype=torch.int32, device=b.dev)
    tail = torch.zeros((2 * b.C + 1,), dtype=torch.int32, device=b.dev)         # new_off [C + 1], then a copy of status [C]: one read-back
    _lib.check(L.dispu_compact_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), _lib.ptr(b.cloud), rule, _lib.ptr(src), _lib.ptr(stats),
                                        min_neighbors, _lib.ptr(b.status), _lib.ptr(pts), _lib.ptr(idx), _lib.ptr(tail), _lib.ptr(scratch),
                                        nbytes, _lib.stream_ptr(b.dev)), "dispu_compact_segments")
    tail[b.C + 1:] = b.status
    host = tail.cpu().numpy()
    new_off = host[:b.C + 1].astype(np.int64)
    return pts[:new_off[-1]], idx[:new_off[-1]], new_off, host[b.C + 1:]


def knn_mean_distance(points, k=16):
    """points: a float32 [n, 3] tensor on a ROCm device, or a list of them (clouds of any sizes from 1 to 2^24 points, at most 65535;
    a list goes through the kernels as ONE packed launch sequence)  ->  [n] float32 (a list in gives a list out): the mean distance of
    every point to its k nearest other points of its own cloud, 1 <= k <= 31; a cloud of n <= k points uses its n - 1 others, a cloud
    of one point gives 0.  ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate
    (after it)."""
    b = Packed(points, "knn_mean_distance", words=3)
    k = check_int_range(k, K_MIN, K_MAX, "k")
    b.pack()
    with torch.cuda.device(b.dev):
        out = _mean_dist(b, k)
        b.refuse_non_finite()
    return b.split(out)


def remove_statistical_outliers(points, k=16, std_ratio=2.0, return_index=False, return_stats=False):
    """Keep the points whose knn_mean_distance(points, k) is at most mean + std_ratio * std of that value over their own cloud (std
    with n - 1 in the denominator, both in float64)  ->  the kept points [m, 3] in input order (a list in gives lists out).
    return_index: also the kept indices [m] int64, ascending.  return_stats: also (mean, std, threshold) per cloud, a float64 [3]
    tensor on the host.  Returns the points, or a tuple (points, index, stats) with the parts asked for, in that order.
    A cloud whose points all coincide keeps everything.  ValueError as for knn_mean_distance; std_ratio must be finite."""
    b = Packed(points, "remove_statistical_outliers", words=3)
    k = check_int_range(k, K_MIN, K_MAX, "k")
    req(isinstance(std_ratio, (int, float, np.integer, np.floating)) and not isinstance(std_ratio, bool) and math.isfinite(float(std_ratio)),
        "std_ratio must be a finite number, got %r" % (std_ratio,))
    b.pack()
    with torch.cuda.device(b.dev):
        L = _lib.lib()
        md = _mean_dist(b, k)
        stats = torch.zeros((b.C, 3), dtype=torch.float64, device=b.dev)
        _lib.check(L.dispu_outlier_threshold_segments(b.C, _lib.ptr(b.d_off), host_ptr(b.off), _lib.ptr(md), _lib.ptr(b.status),
                                                      float(std_ratio), _lib.ptr(stats), _lib.stream_ptr(b.dev)),
                   "dispu_outlier_threshold_segments")
        pts, idx, new_off, status = _compact(b, RULE_MEAN_DIST, md, stats, 0)
        b.refuse_non_finite(torch.from_numpy(status))
    res = [b.split(pts, new_off)]
    if return_index:
        res.append(b.split(idx.long(), new_off))
    if return_stats:
        st = stats.cpu()
        res.append(st[0] if b.single else [st[c] for c in range(b.C)])
    return res[0] if len(res) == 1 else tuple(res)


def radius_neighbor_count(points, radius, cap=None):
    """-> [n] int32 (a list in gives a list out): the number of OTHER points of the point's own cloud at d2 <= radius * radius (fp32,
    the boundary included; duplicates of a point count), at most `cap` (None: exact counts; the search ends early once every point of
    a cell has reached it).  radius is rounded to float32 and must then be finite and > 0; cap >= 1.  ValueError as for
    knn_mean_distance."""
    b = Packed(points, "radius_neighbor_count", words=3)
    r = _check_radius(radius)
    req(cap is None or (is_int(cap) and 1 <= cap <= INT_MAX), "cap must be None or an integer in 1 .. 2^31 - 1, got %r" % (cap,))
    b.pack()
    with torch.cuda.device(b.dev):
        out = _radius_count(b, r, INT_MAX if cap is None else int(cap))
        b.refuse_non_finite()
    return b.split(out)


def remove_radius_outliers(points, radius, min_neighbors=2, return_index=False):
    """Keep the points with at least min_neighbors other points of their cloud within radius (radius_neighbor_count at cap =
    min_neighbors)  ->  the kept points [m, 3] in input order, possibly [0, 3] (a list in gives lists out).  return_index: also the
    kept indices [m] int64, ascending.  min_neighbors >= 1.  ValueError as for radius_neighbor_count."""
    b = Packed(points, "remove_radius_outliers", words=3)
    r = _check_radius(radius)
    req(is_int(min_neighbors) and 1 <= min_neighbors <= INT_MAX, "min_neighbors must be an integer >= 1, got %r" % (min_neighbors,))
    b.pack()
    with torch.cuda.device(b.dev):
        cnt = _radius_count(b, r, int(min_neighbors))
        pts, idx, new_off, status = _compact(b, RULE_COUNT, cnt, None, int(min_neighbors))
        b.refuse_non_finite(torch.from_numpy(status))
    res = [b.split(pts, new_off)]
    if return_index:
        res.append(b.split(idx.long(), new_off))
    return res[0] if len(res) == 1 else tuple(res)
