"""Exact k nearest neighbours from one cloud into another, and per-point attributes (colour, intensity, labels) carried across them:
what brings a scan's attributes onto its upsampled cloud (csrc/attributes.hip; dispu_knn_cross_segments and
dispu_transfer_attributes_segments in include/dispu_hip.h, which states every definition).  The interpolation is pointnet_fp_module's
inverse-distance weighting (Common/pointnet_util.py:204-208) at any k <= 32, carried in double.

The neighbours are the exact ones of the project's rule -- the k smallest (d2, reference index), d2 in plain fp32 arithmetic -- found by
a cell-pruned search over both clouds; neighbourhoods never cross clouds.  The yardstick is tests/attributes_oracle.py."""
import torch

from . import _lib
from ._util import req
from .segments import Pair, check_int_range

K_MIN, K_MAX = 1, 32
MODES = {"idw": 0, "nearest": 1}


def knn_cross(queries, refs, k, return_distance=True):
    """queries, refs: float32 [q, 3] and [m, 3] tensors on a ROCm device, or two lists of them (pairs of clouds of any sizes from 1 to
    2^24 points, at most 65535 pairs; lists go through the kernels as ONE packed launch sequence)  ->  idx [q, k] int32, the k nearest
    reference points of every query in ascending (d2, index) order, -1 beyond min(k, m); with return_distance also d2 [q, k] float32,
    the squared distances, +inf beyond min(k, m): (idx, d2).  Lists in give lists out.  1 <= k <= 32.  ValueError for illegal arguments
    (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    b = Pair(queries, refs, "knn_cross")
    k = check_int_range(k, K_MIN, K_MAX, "k")
    b.width(k)
    b.pack("dispu_knn_cross_scratch_bytes")
    with torch.cuda.device(b.dev):
        idx = torch.empty((b.nq, k), dtype=torch.int32, device=b.dev)
        d2 = torch.empty((b.nq, k), dtype=torch.float32, device=b.dev) if return_distance else None
        _lib.check(_lib.lib().dispu_knn_cross_segments(*(b.head() + (k, _lib.ptr(b.queries.cloud), _lib.ptr(b.refs.cloud), _lib.ptr(idx), _lib.ptr(d2)) + b.tail())),
                   "dispu_knn_cross_segments")
        b.queries.refuse_non_finite()
    return (b.queries.split(idx), b.queries.split(d2)) if return_distance else b.queries.split(idx)


def _attr_list(b, value, name, dtype, dims):
    """the per-cloud attribute tensors of one kind, checked against the references -> a list, or None"""
    if value is None:
        return None
    if b.single:
        req(isinstance(value, torch.Tensor), "%s must be a tensor when queries is one, got %s" % (name, type(value).__name__))
        value = [value]
    req(isinstance(value, (list, tuple)) and len(value) == b.C, "%s: expected %d tensors, one per cloud" % (name, b.C))
    for i, (t, r) in enumerate(zip(value, b.refs.clouds)):
        what = "%s of cloud %d" % (name, i)
        req(isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == dims,
            "%s: expected a %s tensor of %d dimension(s)" % (what, str(dtype).replace("torch.", ""), dims))
        req(t.device == b.dev, "%s lives on another device than the queries" % what)
        req(t.shape[0] == r.shape[0], "%s has %d rows but the cloud has %d reference points" % (what, t.shape[0], r.shape[0]))
        if dims == 2:
            req(t.shape[1] >= 1 and t.shape[1] == value[0].shape[1], "%s has %d columns, expected %d >= 1" % (what, t.shape[1], max(1, value[0].shape[1])))
    return list(value)


def transfer_attributes(queries, refs, features=None, labels=None, k=3, mode="idw"):
    """Carry the attributes of the reference points onto the queries.  queries, refs as for knn_cross; features: float32 [m, F] per
    cloud (F >= 1, the same for every cloud), labels: int32 [m] per cloud; at least one of them.
    mode "idw": every feature is the inverse-distance weighted mean over the k nearest reference points, weights
    1 / max(d2, 1e-10) in double (a query on a reference point takes that point's value to rounding);  "nearest": the row of the
    nearest reference point.  Labels always come from the nearest reference point (equal distances: the smallest index).
    ->  features [q, F] float32, or labels [q] int32, or the tuple (features, labels) when both are given.  Lists in give lists out.
    Feature values are not inspected (a NaN propagates).  ValueError as for knn_cross."""
    b = Pair(queries, refs, "transfer_attributes")
    k = check_int_range(k, K_MIN, K_MAX, "k")
    req(mode in MODES, "mode must be 'idw' or 'nearest', got %r" % (mode,))
    req(features is not None or labels is not None, "transfer_attributes needs features, labels or both")
    feats = _attr_list(b, features, "features", torch.float32, 2)
    labs = _attr_list(b, labels, "labels", torch.int32, 1)
    F = int(feats[0].shape[1]) if feats is not None else 1
    b.width(max(F, k))
    b.pack("dispu_knn_cross_scratch_bytes")
    with torch.cuda.device(b.dev):
        feat = out_feat = lab = out_lab = None
        if feats is not None:
            feat = b.refs.pack_like(feats)
            out_feat = torch.empty((b.nq, F), dtype=torch.float32, device=b.dev)
        if labs is not None:
            lab = b.refs.pack_like(labs)
            out_lab = torch.empty((b.nq,), dtype=torch.int32, device=b.dev)
        _lib.check(_lib.lib().dispu_transfer_attributes_segments(*(b.head() + (k, MODES[mode], _lib.ptr(b.queries.cloud), _lib.ptr(b.refs.cloud), F, _lib.ptr(feat),
                                                                               _lib.ptr(out_feat), _lib.ptr(lab), _lib.ptr(out_lab)) + b.tail())),
                   "dispu_transfer_attributes_segments")
        b.queries.refuse_non_finite()
    res = [b.queries.split(t) for t in (out_feat, out_lab) if t is not None]
    return res[0] if len(res) == 1 else tuple(res)
