"""Surface reconstruction from an oriented cloud: the signed distance to the cloud (an IMLS / Hoppe et al. 1992 implicit function, fused
into the cell-pruned k-NN search) and its zero set contoured on a sparse lattice by marching tetrahedra (csrc/signed_distance.hip,
csrc/reconstruct.hip; dispu_signed_distance_*, dispu_lattice_* and dispu_contour_* in include/dispu_hip.h, which states every
definition).  The reference has no counterpart.  The yardstick is tests/reconstruct_oracle.py: both functions return its bytes.

Practical advice: holes appear when `voxel` is below the cloud's point spacing at band=1 (the lattice then has gaps between the
points); use a larger voxel or band=2.  Far from the data the function is still defined (the nearest point's tangent plane), so the
band, not a trimming step, decides how far the surface is followed.  Zero-area faces (f exactly 0 at a lattice vertex, or two vertices
that fp32 collapses) are kept: they keep the connectivity closed."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._util import req
from .segments import MAX_POINTS, Pair, check_cloud, check_int_range, check_support, scratch_buffer

K_MIN, K_MAX = 1, 32
BAND_MIN, BAND_MAX = 1, 3
INDEX_LIMIT = (1 << 20) - 1


def _normals_list(normals, clouds, single, dev, who):
    if single:
        req(isinstance(normals, torch.Tensor), "%s: points is a tensor, so normals must be one too, got %s" % (who, type(normals).__name__))
        normals = [normals]
    req(isinstance(normals, (list, tuple)) and len(normals) == len(clouds), "normals: expected %d tensors, one per cloud" % len(clouds))
    for i, (t, c) in enumerate(zip(normals, clouds)):
        what = "normals of cloud %d" % i
        check_cloud(t, what)
        req(t.device == dev, "%s lives on another device than the queries" % what)
        req(t.shape[0] == c.shape[0], "%s has %d rows but the cloud has %d points" % (what, t.shape[0], c.shape[0]))
        req(bool(torch.isfinite(t).all()), "%s holds a NaN or an infinite component" % what)
    return list(normals)


def signed_distance(queries, points, normals, k=8, support=1.5):
    """queries [q, 3], points [m, 3], normals [m, 3]: float32 tensors on a ROCm device, or three lists of them (pairs of clouds of any
    sizes from 1 to 2^24 points, at most 65535 pairs; lists go through the kernels as ONE packed launch sequence)  ->  f [q] float32,
    the signed distance of every query to the oriented cloud: the Wendland-weighted mean, over the k exact nearest points p_j, of
    (x - p_j) . n_j, the weights reaching support * the k-th neighbour's distance; where every weight is zero (k = 1, coincident or
    equidistant neighbours) the nearest point's tangent plane.  Positive on the side the normals point to.  Lists in give lists out.
    1 <= k <= 32, 1 <= support <= 4.  Normals are used as given: not normalised, a zero row contributes zero.
    ValueError for illegal arguments and non-finite normals (before any launch of the operator) and for a cloud with a NaN or an
    infinite coordinate (after it)."""
    who = "signed_distance"
    b = Pair(queries, points, who, name="points")
    k = check_int_range(k, K_MIN, K_MAX, "k")
    support = check_support(support)
    nrm = _normals_list(normals, b.refs.clouds, b.single, b.dev, who)
    b.pack("dispu_signed_distance_scratch_bytes")
    with torch.cuda.device(b.dev):
        packed_n = b.refs.pack_like(nrm)
        out = torch.empty((b.nq,), dtype=torch.float32, device=b.dev)
        _lib.check(_lib.lib().dispu_signed_distance_segments(*(b.head() + (k, support, _lib.ptr(b.queries.cloud), _lib.ptr(b.refs.cloud),
                                                                           _lib.ptr(packed_n), _lib.ptr(out)) + b.tail())),
                   "dispu_signed_distance_segments")
        b.queries.refuse_non_finite()
    return b.queries.split(out)


def check_voxel(v):
    ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v)) and float(v) > 0
    req(ok and 0 < float(np.float32(v)) < float("inf"), "voxel must be a positive finite number (as float32 too), got %r" % (v,))
    return float(np.float32(v))


def _mark(dev):
    e = torch.cuda.Event(enable_timing=True)
    e.record(torch.cuda.current_stream(dev))
    return e


def reconstruct_surface(points, normals, voxel, k=8, support=1.5, band=1, max_vertices=1 << 24, stages=None):
    """points, normals: float32 [n, 3] tensors on a ROCm device, one cloud with its oriented normals  ->  (verts [V, 3] float32,
    faces [F, 3] int32): the zero set of signed_distance(., points, normals, k, support), contoured by marching tetrahedra on the
    lattice of edge `voxel` over the voxels within `band` (1 .. 3, Chebyshev) of a voxel that holds a point.  Faces are oriented with
    the normals; vertices are welded, one per crossed lattice edge; orders are pinned (vertices by lattice edge, faces by voxel), so
    the output is unique.  A cloud no lattice edge crosses gives V = F = 0.  Several clouds: a Python loop.
    max_vertices: a cap on the number of LATTICE vertices (at most 2^24, what one query segment holds).
    stages: None, or a dict that receives the counts (occupied, voxels, lattice, verts, faces), the lattice's `positions` [nlat, 3] and
    `values` [nlat], and device-event times of the three groups of stages (grid_ms, values_ms, contour_ms; the call then ends with
    a synchronisation).
    ValueError for illegal arguments and non-finite normals (before any launch), for a cloud with a NaN or an infinite coordinate, for
    a voxel size that puts an index (after the band) outside +-(2^20 - 1), and for more than max_vertices lattice vertices."""
    who = "reconstruct_surface"
    check_cloud(points, "points")
    n = int(points.shape[0])
    req(1 <= n <= MAX_POINTS, "points has %d points, expected 1 .. 2^24" % n)
    h = check_voxel(voxel)
    k = check_int_range(k, K_MIN, K_MAX, "k")
    support = check_support(support)
    band = check_int_range(band, BAND_MIN, BAND_MAX, "band")
    max_vertices = check_int_range(max_vertices, 1, MAX_POINTS, "max_vertices")
    dev = points.device
    (nrm,) = _normals_list(normals, [points], True, dev, who)
    points, nrm = points.contiguous(), nrm.contiguous()
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    i64 = dict(dtype=torch.int64, device=dev)          # lattice keys are unsigned 63-bit values: int64 holds them unchanged
    with torch.cuda.device(dev):
        marks = [_mark(dev)] if stages is not None else None
        # occupied voxels
        nb = L.dispu_lattice_voxels_scratch_bytes(n)
        scratch = scratch_buffer(nb, "dispu_lattice_voxels_scratch_bytes", dev, "sizes")
        occ = torch.empty((n,), **i64)
        cnt, status = C.c_int(0), C.c_int(0)
        _lib.check(L.dispu_lattice_voxels(n, _lib.ptr(points), h, band, _lib.ptr(occ), C.byref(cnt), C.byref(status), _lib.ptr(scratch), nb, st),
                   "dispu_lattice_voxels")
        req(status.value != _lib.LATTICE_NONFINITE, "cloud 0 holds a NaN or an infinite coordinate")
        req(status.value != _lib.LATTICE_RANGE,
            "voxel = %r puts the cloud outside the lattice's index range: every index, after the band, must stay in +-(2^20 - 1)" % h)
        nocc = cnt.value
        # active voxels
        nkeys = nocc * (2 * band + 1) ** 3
        nb = L.dispu_lattice_dilate_scratch_bytes(nocc, band)
        del scratch
        scratch = scratch_buffer(nb, "dispu_lattice_dilate_scratch_bytes", dev, "sizes")
        act = torch.empty((nkeys,), **i64)
        cnt64 = C.c_longlong(0)
        _lib.check(L.dispu_lattice_dilate(nocc, _lib.ptr(occ), band, _lib.ptr(act), C.byref(cnt64), _lib.ptr(scratch), nb, st), "dispu_lattice_dilate")
        nvox = cnt64.value
        # lattice vertices and the corner table
        nb = L.dispu_lattice_corners_scratch_bytes(nvox)
        del scratch
        scratch = scratch_buffer(nb, "dispu_lattice_corners_scratch_bytes", dev, "sizes")
        lat = torch.empty((8 * nvox,), **i64)
        corner = torch.empty((nvox, 8), dtype=torch.int32, device=dev)
        _lib.check(L.dispu_lattice_corners(nvox, _lib.ptr(act), _lib.ptr(lat), _lib.ptr(corner), C.byref(cnt64), _lib.ptr(scratch), nb, st),
                   "dispu_lattice_corners")
        nlat = cnt64.value
        del scratch
        req(nlat <= max_vertices, "the lattice has %d vertices, more than max_vertices = %d: use a larger voxel than %r or a smaller band"
            % (nlat, max_vertices, h))
        pos = torch.empty((nlat, 3), dtype=torch.float32, device=dev)
        _lib.check(L.dispu_lattice_positions(nlat, _lib.ptr(lat), h, _lib.ptr(pos), st), "dispu_lattice_positions")
        # values
        if stages is not None:
            marks.append(_mark(dev))
        f = signed_distance(pos, points, nrm, k, support)
        if stages is not None:
            marks.append(_mark(dev))
        # contouring
        nb = L.dispu_contour_count_scratch_bytes(nvox, nlat)
        scratch = scratch_buffer(nb, "dispu_contour_count_scratch_bytes", dev, "sizes")
        num = torch.empty((7 * nlat,), dtype=torch.int32, device=dev)
        start = torch.empty((nvox,), dtype=torch.int32, device=dev)
        nv, nf = C.c_longlong(0), C.c_longlong(0)
        _lib.check(L.dispu_contour_count(nvox, nlat, _lib.ptr(corner), _lib.ptr(f), _lib.ptr(num), _lib.ptr(start), C.byref(nv), C.byref(nf),
                                         _lib.ptr(scratch), nb, st), "dispu_contour_count")
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf.value, 3), dtype=torch.int32, device=dev)
        if nv.value > 0 and nf.value > 0:
            _lib.check(L.dispu_contour_emit(nvox, nlat, h, _lib.ptr(lat), _lib.ptr(corner), _lib.ptr(f), _lib.ptr(num), _lib.ptr(start),
                                            nv.value, nf.value, _lib.ptr(verts), _lib.ptr(faces), st), "dispu_contour_emit")
        if stages is not None:
            marks.append(_mark(dev))
            marks[-1].synchronize()
            stages.update(occupied=nocc, voxels=nvox, lattice=nlat, verts=nv.value, faces=nf.value, positions=pos, values=f,
                          grid_ms=marks[0].elapsed_time(marks[1]), values_ms=marks[1].elapsed_time(marks[2]),
                          contour_ms=marks[2].elapsed_time(marks[3]))
    return verts, faces
