"""Sequential float32 numpy restatement of the reference's grid_subsampling (libs/cpp_wrappers/cpp_subsampling/grid_subsampling/
grid_subsampling.cpp:5-106, grid_subsampling.h:10-80, cpp_utils/cloud/cloud.cpp:27-67): the yardstick of dispu_amd.grid_subsampling.

Every operation is one float32 operation with one rounding (x86 g++ without -march never fuses); numpy's float32 scalars do exactly
that.  Two things the reference leaves to std::unordered_map are defined here: rows come in ascending key order, and a tie between
label counts goes to the smallest label (signed).  Keys are signed: `floor(min * (1 / dl)) * dl` is rounded twice and can land a few
ulps above the minimum, a point below it gets cell -1 on that axis; the reference's size_t key then wraps modulo 2^64, which groups
the same points as the signed key does.

compute() walks the points in Python; compute_fast() does the same additions vectorised across voxels, for clouds of 10^5 points and more."""
import numpy as np

F = np.float32
MAX_CELLS = 1 << 21


def grid(points, dl):
    """(origin f32 [3], N int [3]) = (originCorner, (sampleNX, sampleNY, sampleNZ)) of grid_subsampling.cpp:25-32"""
    points = np.asarray(points, F)
    dl = F(dl)
    inv = F(1.0) / dl
    mn, mx = points.min(axis=0), points.max(axis=0)
    origin = np.empty(3, F)
    N = []
    with np.errstate(all="ignore"):
        for c in range(3):
            origin[c] = F(np.floor(F(mn[c] * inv))) * dl
            top = np.floor(F(F(mx[c] - origin[c]) / dl))
            if not top + 1 <= MAX_CELLS:
                raise ValueError("axis %s has more than 2^21 cells" % "xyz"[c])
            N.append(int(top) + 1)
    return origin, N


def keys(points, dl):
    """int64 [n]: mapIdx of every point, grid_subsampling.cpp:53-56, as a signed number"""
    points = np.asarray(points, F)
    dl = F(dl)
    origin, N = grid(points, dl)
    idx = np.floor((points - origin[None, :]).astype(F) / dl).astype(np.int64)      # float32 subtract, float32 divide, floor
    return idx[:, 0] + N[0] * idx[:, 1] + N[0] * N[1] * idx[:, 2]


def passes(points, dl):
    """the 8-bit sorting passes the key range needs: ceil(bit_length(key_max - key_min) / 8) with key_max the last cell of the grid and
    key_min the key of the cell that holds the minimum of every axis (cell -1 where the minimum lies below the rounded origin)"""
    points = np.asarray(points, F)
    dl = F(dl)
    origin, N = grid(points, dl)
    lo = [int(np.floor(F(F(points[:, a].min() - origin[a]) / dl))) for a in range(3)]
    key_min = lo[0] + N[0] * lo[1] + N[0] * N[1] * lo[2]
    return ((N[0] * N[1] * N[2] - 1 - key_min).bit_length() + 7) // 8


def compute_fast(points, features=None, classes=None, sampleDl=0.1):
    """compute() without a Python loop over the points: the same float32 additions in the same order, vectorised ACROSS voxels.  After
    the stable sort, step r adds the r-th point of every voxel that has one to that voxel's sum (one float32 addition each, and within a
    voxel r ascends: ascending point index); a single voxel is one sequential float32 cumsum from 0.  tests/test_grid_subsample_oracle.py
    holds it to compute() byte for byte."""
    points = np.ascontiguousarray(points, F)
    n = points.shape[0]
    data = [points]
    if features is not None:
        features = np.ascontiguousarray(features, F).reshape(n, -1)
        data.append(features)
    if classes is not None:
        classes = np.ascontiguousarray(classes, np.int32).reshape(n, -1)
    k = keys(points, sampleDl)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    counts = np.diff(np.r_[starts, n])
    m = len(starts)
    data = np.concatenate(data, axis=1)[order]                   # [n, 3 + fdim] in summation order
    if m == 1:
        acc = np.cumsum(np.concatenate([np.zeros((1, data.shape[1]), F), data]), axis=0, dtype=F)[-1:]      # ((0 + d0) + d1) + ...
    else:
        vox = np.repeat(np.arange(m), counts)
        rank = np.arange(n) - np.repeat(starts, counts)
        by_rank = np.argsort(rank, kind="stable")
        ends = np.cumsum(np.bincount(rank))
        acc = np.zeros((m, data.shape[1]), F)
        a = 0
        for b in ends:                                           # one step per rank; the voxels of a step are distinct
            j = by_rank[a:b]
            acc[vox[j]] = acc[vox[j]] + data[j]
            a = b
    assert acc.dtype == F
    out_p = acc[:, :3] * (1.0 / counts.astype(np.float64)).astype(F)[:, None]
    out_f = None if features is None else acc[:, 3:] / counts.astype(F)[:, None]
    out_c = None
    if classes is not None:
        out_c = np.empty((m, classes.shape[1]), np.int32)
        vox = np.repeat(np.arange(m), counts)
        for c in range(classes.shape[1]):
            lab = classes[order, c].astype(np.int64)
            o = np.lexsort((lab, vox))
            v, l = vox[o], lab[o]
            head = np.flatnonzero(np.r_[True, (v[1:] != v[:-1]) | (l[1:] != l[:-1])])
            run_v, run_l, run_n = v[head], l[head], np.diff(np.r_[head, n])
            best = np.lexsort((run_l, -run_n, run_v))            # per voxel: the longest run first, the smallest label among equals
            first = best[np.flatnonzero(np.r_[True, run_v[best][1:] != run_v[best][:-1]])]
            out_c[:, c] = run_l[first]
    return np.ascontiguousarray(out_p), (None if out_f is None else np.ascontiguousarray(out_f)), out_c


def compute(points, features=None, classes=None, sampleDl=0.1):
    """-> (points [m,3] f32, features [m,fdim] f32 or None, classes [m,ldim] i32 or None), rows in ascending key order"""
    points = np.ascontiguousarray(points, F)
    n = points.shape[0]
    if features is not None:
        features = np.ascontiguousarray(features, F).reshape(n, -1)
    if classes is not None:
        classes = np.ascontiguousarray(classes, np.int32).reshape(n, -1)
    k = keys(points, sampleDl)
    order = np.argsort(k, kind="stable")             # equal keys keep ascending point index: the reference's summation order
    ks = k[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], n]
    m = len(starts)
    out_p = np.empty((m, 3), F)
    out_f = None if features is None else np.empty((m, features.shape[1]), F)
    out_c = None if classes is None else np.empty((m, classes.shape[1]), np.int32)
    for v, (a, b) in enumerate(zip(starts, ends)):
        ids = order[a:b]
        count = b - a
        acc = np.zeros(3, F)
        for i in ids:
            acc = (acc + points[i]).astype(F)
        out_p[v] = acc * F(1.0 / count)              # point * (1.0 / count): reciprocal in double, to float, float multiply
        if features is not None:
            facc = np.zeros(features.shape[1], F)
            for i in ids:
                facc = (facc + features[i]).astype(F)
            out_f[v] = facc / F(count)
        if classes is not None:
            for c in range(classes.shape[1]):
                vals, cnt = np.unique(classes[ids, c], return_counts=True)     # ascending (signed) labels
                out_c[v, c] = vals[np.argmax(cnt)]                             # the first maximum: the smallest label of a tie
    return out_p, out_f, out_c
