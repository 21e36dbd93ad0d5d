"""Moving-least-squares projection: move the points of one cloud onto the surface another cloud describes (csrc/mls_project.hip;
dispu_mls_project_segments in include/dispu_hip.h, which states the operator).  A cloud against itself loses its noise; an upsampled
cloud against its input is pulled back onto the surface the input describes.  The reference has no counterpart.

Per point: its k exact nearest reference points (the project's rule, found by a cell-pruned search over both clouds), Wendland weights
over support * the k-th distance, a weighted plane fit in double, and the point's projection onto that plane.  Neighbourhoods never
cross clouds.  The yardstick is tests/mls_oracle.py."""
import torch

from . import _lib
from .segments import SUPPORT_MAX, SUPPORT_MIN, Pair, check_int_range, check_support  # noqa: F401 (the names callers know)

K_MIN, K_MAX = 4, 32
ITER_MIN, ITER_MAX = 1, 8


def mls_project(queries, refs=None, k=16, support=1.0, iterations=1, return_neighbors=False):
    """queries, refs: float32 [q, 3] and [m, 3] tensors on a ROCm device, or two lists of them (pairs of clouds of any sizes from 1 to
    2^24 points, at most 65535 pairs; lists go through the kernels as ONE packed launch sequence); refs=None: every cloud against itself
    ->  the projected positions, new float32 [q, 3] tensors; with return_neighbors also idx [q, k] int32, the last iteration's k nearest
    reference points in ascending (d2, index) order, -1 beyond min(k, m): (points, idx).  Lists in give lists out.
    4 <= k <= 32;  1 <= support <= 4: the weights reach support * the k-th neighbour's distance;  1 <= iterations <= 8: the step is
    repeated on the moved points against the SAME references.  A point whose neighbourhood defines no plane (fewer than three reference
    points or non-zero weights, coincident or collinear neighbours) keeps its position bit for bit.
    ValueError for illegal arguments (before any launch) and for a cloud with a NaN or an infinite coordinate (after it)."""
    b = Pair(queries, refs, "mls_project")
    k = check_int_range(k, K_MIN, K_MAX, "k")
    support = check_support(support)
    iterations = check_int_range(iterations, ITER_MIN, ITER_MAX, "iterations")
    b.queries.limit(k)
    b.pack("dispu_mls_project_scratch_bytes")
    with torch.cuda.device(b.dev):
        out = torch.empty((b.nq, 3), dtype=torch.float32, device=b.dev)
        idx = torch.empty((b.nq, k), dtype=torch.int32, device=b.dev) if return_neighbors else None
        _lib.check(_lib.lib().dispu_mls_project_segments(*(b.head() + (k, support, iterations, _lib.ptr(b.queries.cloud), _lib.ptr(b.refs.cloud),
                                                                       _lib.ptr(out), _lib.ptr(idx)) + b.tail())),
                   "dispu_mls_project_segments")
        b.queries.refuse_non_finite()
    return (b.queries.split(out), b.queries.split(idx)) if return_neighbors else b.queries.split(out)
