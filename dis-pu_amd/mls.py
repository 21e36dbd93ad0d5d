"""Moving-least-squares projection: move the points of one cloud onto the surface another cloud describes (csrc/mls_project.hip;
dispu_mls_project_segments in include/dispu_hip.h, which states the operator).  A cloud against itself loses its noise; an upsampled
cloud against its input is pulled back onto the surface the input describes.  The reference has no counterpart.

Per point: its k exact nearest reference points (the project's rule, found by a cell-pruned search over both clouds), Wendland weights
over support * the k-th distance, a weighted plane fit in double, and the point's projection onto that plane.  Neighbourhoods never
cross clouds.  The yardstick is tests/mls_oracle.py."""
import math

import numpy as np
import torch

from . import _lib
from ._util import req
from .segments import Packed, check_int_range, host_ptr

K_MIN, K_MAX = 4, 32
SUPPORT_MIN, SUPPORT_MAX = 1.0, 4.0
ITER_MIN, ITER_MAX = 1, 8


def check_support(v):
    ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and SUPPORT_MIN <= float(v) <= SUPPORT_MAX
    req(ok and math.isfinite(float(v)), "support must be a number in %g .. %g, got %r" % (SUPPORT_MIN, SUPPORT_MAX, v))
    return float(v)


def mls_project(queries, refs=None, k=16, support=1.0, iterations=1, return_neighbors=False):
    """queries, refs: float32 [q, 3] and [m, 3] tensors on a ROCm device, or two lists of them (pairs of clouds of any sizes from 1 to
    2^24 points, at most 65535 pairs; lists go through the kernels as ONE packed launch sequence); refs=None: every cloud against itself
    ->  the projected positions, new float32 [q, 3] tensors; with return_neighbors also idx [q, k] int32, the last iteration's k nearest
    reference points in ascending (d2, index) order, -1 beyond min(k, m): (points, idx).  Lists in give lists out.
    4 <= k <= 32;  1 <= support <= 4: the weights reach support * the k-th neighbour's distance;  1 <= iterations <= 8: the step is
    repeated on the moved points against the SAME references.  A point whose neighbourhood defines no plane (fewer than three reference
    points or non-zero weights, coincident or collinear neighbours) keeps its position bit for bit.
    ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    who = "mls_project"
    if refs is not None:                                     # as attributes.py pairs them: the shapes of the two arguments first
        if isinstance(queries, torch.Tensor):
            req(isinstance(refs, torch.Tensor), "%s: queries is a tensor, so refs must be one too, got %s" % (who, type(refs).__name__))
        else:
            req(isinstance(queries, (list, tuple)) and isinstance(refs, (list, tuple)),
                "queries and refs must be float32 [n, 3] tensors on a ROCm device or two lists of them, got %s and %s"
                % (type(queries).__name__, type(refs).__name__))
            req(len(queries) >= 1, "%s needs at least one cloud" % who)
            req(len(queries) == len(refs), "%d query clouds but %d reference clouds" % (len(queries), len(refs)))
    q = Packed(queries, who, label="queries of cloud %d", home="the queries of cloud 0")
    r = q if refs is None else Packed(refs, who, label="refs of cloud %d", dev=q.dev, home="the queries of cloud 0")
    k = check_int_range(k, K_MIN, K_MAX, "k")
    support = check_support(support)
    iterations = check_int_range(iterations, ITER_MIN, ITER_MAX, "iterations")
    q.limit(k)
    q.pack()
    if r is not q:
        r.pack(status=False)
    L = _lib.lib()
    nbytes = L.dispu_mls_project_scratch_bytes(q.C, host_ptr(q.off), host_ptr(r.off))
    scratch = q.scratch(nbytes, "dispu_mls_project_scratch_bytes")
    with torch.cuda.device(q.dev):
        out = torch.empty((q.total, 3), dtype=torch.float32, device=q.dev)
        idx = torch.empty((q.total, k), dtype=torch.int32, device=q.dev) if return_neighbors else None
        _lib.check(L.dispu_mls_project_segments(q.C, _lib.ptr(q.d_off), host_ptr(q.off), _lib.ptr(r.d_off), host_ptr(r.off), k, support,
                                                iterations, _lib.ptr(q.cloud), _lib.ptr(r.cloud), _lib.ptr(out), _lib.ptr(idx),
                                                _lib.ptr(q.status), _lib.ptr(scratch), nbytes, _lib.stream_ptr(q.dev)),
                   "dispu_mls_project_segments")
        q.refuse_non_finite()
    return (q.split(out), q.split(idx)) if return_neighbors else q.split(out)
