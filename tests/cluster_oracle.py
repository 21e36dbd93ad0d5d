"""The yardstick of dis-pu_amd/clusters.py: the definition of include/dispu_hip.h (dispu_cluster_segments) restated in numpy for ONE
cloud, brute force.  fp32 throughout: r2 = fp32(eps) * fp32(eps) rounded once, d2 as normals_oracle.sqdist_rows forms it (the
arithmetic of the kernels, symmetric bit for bit), the boundary included.  `naive` is a double-loop twin for clouds of at most 40
points that `dbscan` itself is held to (tests/test_cluster_oracle.py)."""
import numpy as np

from normals_oracle import sqdist_rows


def radius2(eps):
    e = np.float32(eps)
    return np.float32(e * e)


def dbscan(p, eps, min_points, chunk=512):
    """-> (labels [n] int32, core [n] bool, sizes [clusters] int32)"""
    p = np.ascontiguousarray(p, np.float32)
    n, r2 = p.shape[0], radius2(eps)
    within = np.zeros((n, n), bool)
    d2 = np.zeros((n, n), np.float32)
    for lo in range(0, n, chunk):
        d2[lo:lo + chunk] = sqdist_rows(p, lo, min(lo + chunk, n))
        within[lo:lo + chunk] = d2[lo:lo + chunk] <= r2
    core = within.sum(1) >= min_points                                       # the point itself included, duplicates counted
    root = np.arange(n)                                                      # quick-find: root[x] is always x's representative
    ci = np.nonzero(core)[0]
    for i in ci:                                                             # a sequential union-find over the core pairs, row by row
        rs = np.unique(root[ci[within[i, ci]]])                              # (i itself is among them)
        if len(rs) > 1:
            root[np.isin(root, rs)] = rs[0]                                  # the smallest representative takes the others' sets
    labels = np.full(n, -1, np.int32)
    ids = {}
    for i in ci:                                                             # numbered by the first core index: the order of a scan
        labels[i] = ids.setdefault(int(root[i]), len(ids))
    for i in np.nonzero(~core)[0]:                                           # borders: the smallest (d2 bits, index) among core points
        cand = ci[within[i, ci]]
        if len(cand):
            labels[i] = labels[cand[np.lexsort((cand, d2[i, cand].view(np.uint32)))[0]]]
    return labels, core, np.bincount(labels[labels >= 0], minlength=len(ids)).astype(np.int32)


def naive(p, eps, min_points):
    """the same by double loops and a flood fill, n <= 40"""
    p = np.ascontiguousarray(p, np.float32)
    n, r2 = p.shape[0], radius2(eps)
    assert n <= 40

    def d2(i, j):
        dx, dy, dz = (np.float32(p[j, a] - p[i, a]) for a in range(3))
        return np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))

    core = [sum(d2(i, j) <= r2 for j in range(n)) >= min_points for i in range(n)]
    labels, k = [-1] * n, 0
    for s in range(n):
        if core[s] and labels[s] < 0:
            labels[s], stack = k, [s]
            while stack:
                i = stack.pop()
                for j in range(n):
                    if core[j] and labels[j] < 0 and d2(i, j) <= r2:
                        labels[j] = k
                        stack.append(j)
            k += 1
    out = list(labels)
    for i in range(n):
        if not core[i]:
            best = None
            for j in range(n):
                if core[j] and d2(i, j) <= r2:
                    key = (int(np.float32(d2(i, j)).view(np.uint32)), j)
                    if best is None or key < best[0]:
                        best = (key, labels[j])
            out[i] = -1 if best is None else best[1]
    sizes = [sum(1 for l in out if l == c) for c in range(k)]
    return np.int32(out), np.array(core, bool), np.int32(sizes)


def keep(labels, sizes, keep_n, min_size):
    """ascending indices of the points in the keep_n largest clusters of size >= min_size: size descending, then id ascending"""
    order = sorted((c for c in range(len(sizes)) if sizes[c] >= min_size), key=lambda c: (-int(sizes[c]), c))[:keep_n]
    return np.nonzero(np.isin(labels, order))[0] if order else np.zeros(0, np.int64)


def shells(n, seed=0, strays=40):
    """two nested sphere shells (radii 1 and 0.5) plus `strays` uniform points in [-1.5, 1.5]^3, float32 [n, 3]"""
    g = np.random.RandomState(seed)
    m = n - strays
    v = g.randn(m, 3)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[m // 2:] *= 0.5
    return np.concatenate([v, g.uniform(-1.5, 1.5, (strays, 3))]).astype(np.float32)


SHELL_CASES = ((500, 0.12, 5), (2000, 0.06, 4), (4200, 0.05, 6), (300, 0.2, 1))      # (n, eps, min_points)
