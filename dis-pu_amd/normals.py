"""Oriented unit normals for whole clouds: exact k nearest neighbours and a PCA per point, in one kernel family
(csrc/normals.hip, dispu_pca_normals_segments in include/dispu_hip.h).  The reference has no counterpart: it reads and writes bare
x y z; what leaves the upsampler needs a normal per point for surface reconstruction, shading and registration.

The neighbourhood of a point is the k' = min(k, n) points of its own cloud with the smallest (d2, index), d2 in plain fp32 arithmetic,
the point itself included: pc_util.py:83-92's k-NN made deterministic, the rule of upsample.knn_patch_segments.  The normal is the
eigenvector of the smallest eigenvalue of the neighbourhood's covariance, computed in double around the point itself, so a scan at
large coordinates with fine structure loses nothing.  The yardstick is tests/normals_oracle.py.

orient_consistent makes the signs agree from point to point on shapes where no pointwise rule can (a torus, a handle): propagation
along the minimum spanning forest of the neighbour graph (csrc/orient_consistent.hip, dispu_orient_consistent_segments; the yardstick
is tests/orient_oracle.py)."""
import numpy as np
import torch

from . import _lib
from ._util import req
from .segments import MAX_CLOUDS, Packed, as_list, check_cloud, check_int_range, host_ptr

K_MIN, K_MAX = 4, 32
ORIENT_FORMS = ("viewpoint", "centroid", "reference")


def _split_consistent(orient):
    """('consistent',) or ('consistent', prior) -> (True, prior); any other orient -> (False, orient)"""
    if not (isinstance(orient, (tuple, list)) and len(orient) >= 1 and isinstance(orient[0], str) and orient[0] == "consistent"):
        return False, orient
    req(len(orient) <= 2, "('consistent',) or ('consistent', prior) takes at most one argument")
    prior = orient[1] if len(orient) == 2 else None
    if len(orient) == 2:
        req(isinstance(prior, (tuple, list)) and len(prior) >= 1 and isinstance(prior[0], str) and prior[0] in ORIENT_FORMS,
            "the prior of ('consistent', prior) must be ('viewpoint', xyz), ('centroid',) or ('reference', ref_points, ref_normals), "
            "got %r" % (prior,))
    return True, prior


def _check_orient(orient, clouds):
    """-> the form's name (or None) after every check that needs no launch"""
    if orient is None:
        return None
    req(isinstance(orient, (tuple, list)) and len(orient) >= 1 and isinstance(orient[0], str) and orient[0] in ORIENT_FORMS,
        "orient must be None, ('viewpoint', xyz), ('centroid',), ('reference', ref_points, ref_normals), ('consistent',) or "
        "('consistent', prior), got %r" % (orient,))
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
            check_cloud(p, "reference points %d" % i)
            check_cloud(m, "reference normals %d" % i)
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
            ("consistent",) -- signs that agree from point to point on any shape: orient_consistent(vote="anchor") on the orient=None
            normals and the neighbours of this search;  ("consistent", prior), prior any of the three forms above -- the normals of
            the prior, then orient_consistent(vote="majority"): consistent, and facing the way most of the prior does.
    return_variation: also the surface variation max(l0, 0) / (l0 + l1 + l2) [n] of the covariance's eigenvalues l0 <= l1 <= l2.
    return_neighbors: also the neighbours' indices [n, k] int32 in ascending (distance, index) order, -1 beyond min(k, n).
    Returns the normals, or a tuple (normals, variation, neighbors) with the parts asked for, in that order.
    ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    b = Packed(points, "estimate_normals")
    k = check_int_range(k, K_MIN, K_MAX, "k")
    b.limit(max(k, 3), tail=" at k = %d" % k)
    consistent, orient = _split_consistent(orient)
    want_neighbors, return_neighbors = return_neighbors, return_neighbors or consistent
    form = _check_orient(orient, b.clouds)

    b.pack()
    dev, C, total = b.dev, b.C, b.total
    with torch.cuda.device(dev):
        mode, direction = 0, None
        if form == "viewpoint":
            v = np.asarray(orient[1].detach().cpu() if isinstance(orient[1], torch.Tensor) else orient[1], np.float32)
            mode, direction = 2, torch.from_numpy(np.broadcast_to(v.reshape(-1, 3), (C, 3)).copy()).to(dev)
        elif form == "centroid":
            mode, direction = 1, torch.cat([(c.double() - c.double().mean(dim=0, keepdim=True)).float() for c in b.clouds]).contiguous()
        elif form == "reference":
            rp, rn = orient[1], orient[2]
            if isinstance(rp, torch.Tensor):
                rp, rn = [rp], [rn]
            mode, direction = 1, _reference_directions(b.clouds, rp, rn).contiguous()
        L = _lib.lib()
        nbytes = L.dispu_pca_normals_scratch_bytes(C, host_ptr(b.off), k)
        scratch = b.scratch(nbytes, "dispu_pca_normals_segments")
        normal = torch.zeros((total, 3), dtype=torch.float32, device=dev)
        variation = torch.zeros((total,), dtype=torch.float32, device=dev) if return_variation else None
        neighbors = torch.full((total, k), -1, dtype=torch.int32, device=dev) if return_neighbors else None
        _lib.check(L.dispu_pca_normals_segments(C, _lib.ptr(b.d_off), host_ptr(b.off), k, _lib.ptr(b.cloud), mode, _lib.ptr(direction),
                                                _lib.ptr(normal), _lib.ptr(variation), _lib.ptr(neighbors), _lib.ptr(b.status),
                                                _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)), "dispu_pca_normals_segments")
        b.refuse_non_finite()
    if consistent:                                           # a prior keeps its overall direction: the majority decides per component
        normal = _orient_launch(b, normal, neighbors, k, 0 if orient is None else 1, False, False)[0]
        return_neighbors = want_neighbors
    res = [b.split(normal)]
    if return_variation:
        res.append(b.split(variation))
    if return_neighbors:
        res.append(b.split(neighbors))
    return res[0] if len(res) == 1 else tuple(res)


VOTES = ("anchor", "majority")
_STATUS_TEXT = ((1, "holds a NaN or an infinite normal"), (2, "holds a neighbour index outside -1 .. n - 1"),
                (4, "did not converge (an iteration cap was reached)"))


def _orient_launch(b, normal, neighbors, k, vote, want_flip, want_component):
    """dispu_orient_consistent_segments on a packed batch with its packed normals and neighbours -> (normal_out, flip, component,
    n_components); ValueError for a flagged cloud"""
    dev, C, total = b.dev, b.C, b.total
    with torch.cuda.device(dev):
        L = _lib.lib()
        nbytes = L.dispu_orient_consistent_scratch_bytes(C, host_ptr(b.off), k)
        scratch = b.scratch(nbytes, "dispu_orient_consistent_segments")
        out = torch.empty((total, 3), dtype=torch.float32, device=dev)
        flip = torch.zeros((total,), dtype=torch.uint8, device=dev) if want_flip else None
        component = torch.zeros((total,), dtype=torch.int32, device=dev) if want_component else None
        ncomp = torch.zeros((C,), dtype=torch.int32, device=dev) if want_component else None
        status = torch.zeros((C,), dtype=torch.int32, device=dev)
        _lib.check(L.dispu_orient_consistent_segments(C, _lib.ptr(b.d_off), host_ptr(b.off), k, _lib.ptr(b.cloud), _lib.ptr(normal),
                                                      _lib.ptr(neighbors), vote, 0, _lib.ptr(out), _lib.ptr(flip), _lib.ptr(component),
                                                      _lib.ptr(ncomp), _lib.ptr(status), _lib.ptr(scratch), nbytes, None,
                                                      _lib.stream_ptr(dev)),
                   "dispu_orient_consistent_segments")
        st = status.cpu().numpy()
    bad = np.nonzero(st)[0]
    if len(bad):
        c, bits = int(bad[0]), int(st[bad[0]])
        req(False, "cloud %d %s" % (c, " and ".join(text for bit, text in _STATUS_TEXT if bits & bit)))
    return out, flip, component, ncomp


def orient_consistent(points, normals, k=16, neighbors=None, vote="anchor", return_flips=False, return_components=False):
    """Signs that agree from point to point (Hoppe et al. 1992): the sign is propagated along the minimum spanning forest of the k-NN
    graph weighted by 1 - |n_u . n_v| (csrc/orient_consistent.hip, dispu_orient_consistent_segments in include/dispu_hip.h; the
    yardstick is tests/orient_oracle.py).  The result is a pure function of the input: the forest is unique under the header's edge order.

    points, normals: float32 [n, 3] tensors on a ROCm device, or lists of them (one packed launch sequence; 1 .. 2^24 points per cloud,
    at most 65535 clouds).  Normals of any sign; a zero normal is carried along and never counts in a vote.
    neighbors: int32 [n, k] local indices as estimate_normals(return_neighbors=True) returns them (-1 and the row's own index are
    ignored), or lists of them; None: the lists of the exact search at k.  4 <= k <= 32; with neighbors given k must be their width.
    vote: "anchor" -- per connected component the point with the largest (z, y, x) keeps or turns its normal so that the first non-zero
    of (nz, ny, nx) is positive (on a closed surface: outwards), and the rest follows;  "majority" -- of the two consistent choices the one
    that turns fewer normals: for input that already has a direction (a viewpoint, a centroid, a reference).
    Returns the oriented normals; with return_flips also the flip bytes [n] uint8; with return_components also the component of every
    point [n] int32 (the lowest index of its component) and the number of components (an int, or a list of ints), in that order.
    ValueError for illegal arguments (before any launch) and for a cloud with a non-finite normal or an illegal index (after it)."""
    single, clouds, nrms = isinstance(points, torch.Tensor), as_list(points), as_list(normals)
    req(clouds is not None, "points must be a float32 [n, 3] tensor on a ROCm device or a list of them, got %s" % type(points).__name__)
    req(nrms is not None and isinstance(normals, torch.Tensor) == single, "normals must be a tensor or a list, as points is")
    req(1 <= len(clouds) <= MAX_CLOUDS, "1 .. %d clouds per call, got %d" % (MAX_CLOUDS, len(clouds)))
    req(len(nrms) == len(clouds), "%d clouds and %d sets of normals" % (len(clouds), len(nrms)))
    k = check_int_range(k, K_MIN, K_MAX, "k")
    req(isinstance(vote, str) and vote in VOTES, "vote must be 'anchor' or 'majority', got %r" % (vote,))
    b = Packed(points, "orient_consistent")
    for i, (c, m) in enumerate(zip(clouds, nrms)):
        check_cloud(m, "normals %d" % i)
        req(m.shape == c.shape, "cloud %d has %d points and %d normals" % (i, c.shape[0], m.shape[0]))
        req(m.device == b.dev, "cloud %d lives on another device than cloud 0" % i)
    b.limit(k, unit="neighbour slots", tail=" at k = %d" % k)
    if neighbors is not None:
        nbs = as_list(neighbors)
        req(nbs is not None and isinstance(neighbors, torch.Tensor) == single and len(nbs) == b.C,
            "neighbors must be a tensor or a list of %d tensors, as points is" % b.C)
        for i, (t, c) in enumerate(zip(nbs, clouds)):
            req(isinstance(t, torch.Tensor) and t.is_cuda and t.device == b.dev and t.dtype == torch.int32,
                "neighbors %d must be an int32 tensor on the clouds' device" % i)
            req(tuple(t.shape) == (c.shape[0], k), "neighbors %d: expected shape (%d, %d), got %s" % (i, c.shape[0], k, tuple(t.shape)))
    else:
        nbs = estimate_normals(clouds, k=k, return_neighbors=True)[1]
    b.pack(status=False)
    out, flip, component, ncomp = _orient_launch(b, b.pack_like(nrms), b.pack_like(nbs), k, VOTES.index(vote), return_flips,
                                                 return_components)
    res = [b.split(out)]
    if return_flips:
        res.append(b.split(flip))
    if return_components:
        counts = [int(v) for v in ncomp.cpu().numpy()]
        res += [b.split(component), counts[0] if single else counts]
    return res[0] if len(res) == 1 else tuple(res)
