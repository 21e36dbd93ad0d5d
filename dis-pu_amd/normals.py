"""Oriented unit normals for whole clouds: exact k nearest neighbours and a PCA per point, in one kernel family
(csrc/normals.hip, dispu_pca_normals_segments in include/dispu_hip.h).  The reference has no counterpart: it reads and writes bare
x y z; what leaves the upsampler needs a normal per point for surface reconstruction, shading and registration.

The neighbourhood of a point is the k' = min(k, n) points of its own cloud with the smallest (d2, index), d2 in plain fp32 arithmetic,
the point itself included: pc_util.py:83-92's k-NN made deterministic, the rule of upsample.knn_patch_segments.  The normal is the
eigenvector of the smallest eigenvalue of the neighbourhood's covariance, computed in double around the point itself, so a scan at
large coordinates with fine structure loses nothing.  The yardstick is tests/normals_oracle.py."""
import numpy as np
import torch

from . import _lib
from ._util import req

K_MIN, K_MAX = 4, 32
MAX_CLOUDS = 65535
MAX_POINTS = 1 << 24
ORIENT_FORMS = ("viewpoint", "centroid", "reference")


def _host_ptr(a):
    return _lib.C.c_void_p(a.ctypes.data)


def _check_cloud(t, what):
    req(isinstance(t, torch.Tensor), "%s: expected a float32 [n, 3] tensor on a ROCm device, got %s" % (what, type(t).__name__))
    req(t.is_cuda, "%s must live on a ROCm device (dis-pu_amd has no CPU path)" % what)
    req(t.dtype == torch.float32, "%s must be float32, got %s" % (what, t.dtype))
    req(t.dim() == 2 and t.shape[1] == 3, "%s: expected an [n, 3] tensor, got shape %s" % (what, tuple(t.shape)))


def _check_orient(orient, clouds):
    """-> the form's name (or None) after every check that needs no launch"""
    if orient is None:
        return None
    req(isinstance(orient, (tuple, list)) and len(orient) >= 1 and orient[0] in ORIENT_FORMS,
        "orient must be None, ('viewpoint', xyz), ('centroid',) or ('reference', ref_points, ref_normals), got %r" % (orient,))
    form, C = orient[0], len(clouds)
    if form == "centroid":
        req(len(orient) == 1, "('centroid',) takes no argument")
    elif form == "viewpoint":
        req(len(orient) == 2, "('viewpoint', xyz) takes one argument")
        v = np.asarray(orient[1].detach().cpu() if isinstance(orient[1], torch.Tensor) else orient[1], np.float64)
        req(v.shape in ((3,), (C, 3)), "viewpoint: expected 3 numbers, or [%d, 3] (one viewpoint per cloud), got shape %s" % (C, v.shape))
        req(bool(np.all(np.isfinite(v))), "viewpoint must be finite")
    else:
        req(len(orient) == 3, "('reference', ref_points, ref_normals) takes two arguments")
        rp, rn = orient[1], orient[2]
        if C == 1 and isinstance(rp, torch.Tensor):
            rp, rn = [rp], [rn]
        req(isinstance(rp, (list, tuple)) and isinstance(rn, (list, tuple)) and len(rp) == C and len(rn) == C,
            "reference: expected one (ref_points, ref_normals) pair per cloud (%d)" % C)
        for i, (p, m) in enumerate(zip(rp, rn)):
            _check_cloud(p, "reference points %d" % i)
            _check_cloud(m, "reference normals %d" % i)
            req(p.shape[0] >= 1 and p.shape == m.shape, "reference %d: points %s and normals %s must be equal, non-empty shapes"
                % (i, tuple(p.shape), tuple(m.shape)))
            req(p.device == clouds[i].device, "reference %d lives on another device than its cloud" % i)
    return form


def _reference_directions(clouds, ref_points, ref_normals):
    """the reference normal of every point's nearest reference point (three_nn at b = 1 per cloud, column 0, then a gather)"""
    from .tf_interpolate import three_nn
    out = []
    for c, rp, rn in zip(clouds, ref_points, ref_normals):
        _, idx = three_nn(c.reshape(1, -1, 3), rp.contiguous().reshape(1, -1, 3))
        out.append(rn.contiguous()[idx[0, :, 0].long()])
    return torch.cat(out)


def estimate_normals(points, k=16, orient=None, return_variation=False, return_neighbors=False):
    """points: a float32 [n, 3] tensor on a ROCm device, or a list of them (clouds of any sizes from 1 to 2^24 points, at most 65535;
    a list goes through the kernels as ONE packed launch sequence)  ->  unit normals [n, 3] float32 (a list in gives lists out).
    4 <= k <= 32.  A point whose neighbourhood has fewer than 3 points or no extent gets the normal (0, 0, 0) and the variation -1.

    orient: None -- the component of largest magnitude is positive (ties: the lowest axis);
            ("viewpoint", xyz) -- towards the viewpoint (3 numbers, or [C, 3] for one per cloud);
            ("centroid",) -- outwards, away from the cloud's mean (closed objects);
            ("reference", ref_points, ref_normals) -- in agreement with the normal of the nearest reference point (tensors, or lists
            of them, one pair per cloud).  Where the direction is orthogonal to the normal the sign of orient=None stays.
    return_variation: also the surface variation max(l0, 0) / (l0 + l1 + l2) [n] of the covariance's eigenvalues l0 <= l1 <= l2.
    return_neighbors: also the neighbours' indices [n, k] int32 in ascending (distance, index) order, -1 beyond min(k, n).
    Returns the normals, or a tuple (normals, variation, neighbors) with the parts asked for, in that order.
    ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    single = isinstance(points, torch.Tensor)
    clouds = [points] if single else list(points) if isinstance(points, (list, tuple)) else None
    req(clouds is not None, "points must be a float32 [n, 3] tensor on a ROCm device or a list of them, got %s" % type(points).__name__)
    req(len(clouds) >= 1, "estimate_normals needs at least one cloud")
    req(len(clouds) <= MAX_CLOUDS, "at most %d clouds per call, got %d" % (MAX_CLOUDS, len(clouds)))
    for i, c in enumerate(clouds):
        _check_cloud(c, "cloud %d" % i)
        req(1 <= c.shape[0] <= MAX_POINTS, "cloud %d has %d points, expected 1 .. 2^24" % (i, c.shape[0]))
        req(c.device == clouds[0].device, "cloud %d lives on another device than cloud 0" % i)
    req(isinstance(k, (int, np.integer)) and not isinstance(k, bool) and K_MIN <= k <= K_MAX,
        "k must be an integer in %d .. %d, got %r" % (K_MIN, K_MAX, k))
    k = int(k)
    sizes = [int(c.shape[0]) for c in clouds]
    total = sum(sizes)
    req(total * max(k, 3) < 2 ** 31, "a packed batch holds at most 2^31 - 1 output words, got %d points at k = %d" % (total, k))
    form = _check_orient(orient, clouds)

    dev = clouds[0].device
    C = len(clouds)
    off = np.zeros(C + 1, np.int32)
    np.cumsum(sizes, out=off[1:])
    cloud = (clouds[0] if C == 1 else torch.cat(clouds)).contiguous()
    with torch.cuda.device(dev):
        mode, direction = 0, None
        if form == "viewpoint":
            v = np.asarray(orient[1].detach().cpu() if isinstance(orient[1], torch.Tensor) else orient[1], np.float32)
            mode, direction = 2, torch.from_numpy(np.broadcast_to(v.reshape(-1, 3), (C, 3)).copy()).to(dev)
        elif form == "centroid":
            mode, direction = 1, torch.cat([(c.double() - c.double().mean(dim=0, keepdim=True)).float() for c in clouds]).contiguous()
        elif form == "reference":
            rp, rn = orient[1], orient[2]
            if isinstance(rp, torch.Tensor):
                rp, rn = [rp], [rn]
            mode, direction = 1, _reference_directions(clouds, rp, rn).contiguous()
        L = _lib.lib()
        nbytes = L.dispu_pca_normals_scratch_bytes(C, _host_ptr(off), k)
        req(nbytes > 0, "dispu_pca_normals_segments refuses these clouds")
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        d_off = torch.from_numpy(off).to(dev)
        normal = torch.zeros((total, 3), dtype=torch.float32, device=dev)
        variation = torch.zeros((total,), dtype=torch.float32, device=dev) if return_variation else None
        neighbors = torch.full((total, k), -1, dtype=torch.int32, device=dev) if return_neighbors else None
        status = torch.zeros((C,), dtype=torch.int32, device=dev)
        _lib.check(L.dispu_pca_normals_segments(C, _lib.ptr(d_off), _host_ptr(off), k, _lib.ptr(cloud), mode, _lib.ptr(direction),
                                                _lib.ptr(normal), _lib.ptr(variation), _lib.ptr(neighbors), _lib.ptr(status),
                                                _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)), "dispu_pca_normals_segments")
        bad = np.nonzero(status.cpu().numpy())[0]
    req(len(bad) == 0, "cloud %d holds a NaN or an infinite coordinate" % (int(bad[0]) if len(bad) else -1))

    def split(t):
        return t if single else [t[off[c]:off[c + 1]] for c in range(C)]

    res = [split(normal)]
    if return_variation:
        res.append(split(variation))
    if return_neighbors:
        res.append(split(neighbors))
    return res[0] if len(res) == 1 else tuple(res)
