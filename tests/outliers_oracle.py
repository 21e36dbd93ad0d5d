"""numpy restatement of the outlier filters (include/dispu_hip.h: dispu_knn_mean_dist_segments, dispu_radius_count_segments,
dispu_outlier_threshold_segments, dispu_compact_segments; csrc/outliers.hip) for one cloud: the yardstick of the outlier tests.
d2 is normals_oracle.sqdist_rows (fp32, the kernel's order), the neighbour order a stable sort, the k' terms are added in an explicit
loop in ascending rank (np.sum's pairwise order is not the kernel's), counts are integers, mu and sigma float64."""
import numpy as np

from normals_oracle import far_ellipsoid, lattice, noisy_plane, sphere, sqdist_rows  # noqa: F401  (the seeded clouds, re-exported)


def sorted_d2(p, kmax=32, chunk=512):
    """[n, min(kmax, n)] fp32: per point its smallest d2 in ascending (d2, index) order (a stable sort), its own +0 included"""
    p = np.ascontiguousarray(p, np.float32)
    n = p.shape[0]
    kp = min(kmax, n)
    out = np.zeros((n, kp), np.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d2 = sqdist_rows(p, lo, hi)
        assert d2.dtype == np.float32
        order = np.argsort(d2, axis=1, kind="stable")[:, :kp]
        out[lo:hi] = np.take_along_axis(d2, order, axis=1)
    return out


def mean_dist_from_sorted(sd2, n, k):
    """[n] fp32 from sorted_d2's rows (at least min(k + 1, n) columns): (float)(sum_j sqrt((double)d2_j) / max(k' - 1, 1))"""
    kp = min(k + 1, n)
    assert sd2.shape[0] == n and sd2.shape[1] >= kp
    near = sd2[:, :kp].astype(np.float64)
    s = np.zeros(n, np.float64)
    for j in range(kp):                                         # ascending rank, one double addition per term
        s = s + np.sqrt(near[:, j])
    return (s / np.float64(max(kp - 1, 1))).astype(np.float32)


def mean_dist(p, k):
    """[n] fp32: the mean distance to the k nearest other points, over the k' = min(k + 1, n) smallest (d2, index), self included"""
    return mean_dist_from_sorted(sorted_d2(p, k + 1), len(p), k)


def radius_count(p, radius, cap=None, chunk=512):
    """[n] int32: min(cap, #{j != i: d2_ij <= r2}), r2 = fp32(radius) * fp32(radius) rounded once in fp32"""
    p = np.ascontiguousarray(p, np.float32)
    n = p.shape[0]
    r = np.float32(radius)
    r2 = np.float32(r * r)
    out = np.zeros(n, np.int64)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        out[lo:hi] = (sqdist_rows(p, lo, hi) <= r2).sum(axis=1) - 1     # the point's own d2 is +0
    if cap is not None:
        out = np.minimum(out, cap)
    return out.astype(np.int32)


def threshold(md, ratio):
    """(mu, sigma, mu + ratio * sigma) in float64 from the stored fp32 values; sigma with max(n - 1, 1) below"""
    d = np.asarray(md, np.float32).astype(np.float64)
    n = d.shape[0]
    mu = d.sum() / n
    sigma = np.sqrt(((d - mu) ** 2).sum() / max(n - 1, 1))
    return np.float64(mu), np.float64(sigma), np.float64(mu + np.float64(ratio) * sigma)


def band(md, thr):
    """the smallest relative distance of any mean_dist from the (positive) threshold"""
    assert thr > 0.0
    d = np.asarray(md, np.float32).astype(np.float64)
    return float(np.abs(d - thr).min() / thr)


def statistical_keep(p, k, ratio, md=None):
    """-> (kept indices ascending int64, (mu, sigma, thr), mean_dist)"""
    md = mean_dist(p, k) if md is None else md
    st = threshold(md, ratio)
    return np.nonzero(md.astype(np.float64) <= st[2])[0], st, md


def radius_keep(p, radius, min_neighbors):
    return np.nonzero(radius_count(p, radius, cap=min_neighbors) >= min_neighbors)[0]


# ---- the naive double loops the oracle itself is held to (clouds of <= 40 points) ------------------------------------------------------

def naive_d2(a, b):
    dx, dy, dz = np.float32(b[0]) - np.float32(a[0]), np.float32(b[1]) - np.float32(a[1]), np.float32(b[2]) - np.float32(a[2])
    return np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))


def naive_mean_dist(p, k):
    p = np.asarray(p, np.float32)
    n = len(p)
    out = np.zeros(n, np.float32)
    for i in range(n):
        keys = sorted((naive_d2(p[i], p[j]), j) for j in range(n))[:min(k + 1, n)]
        s = np.float64(0.0)
        for d2, _ in keys:
            s = s + np.sqrt(np.float64(d2))
        out[i] = np.float32(s / np.float64(max(len(keys) - 1, 1)))
    return out


def naive_radius_count(p, radius, cap=None):
    p = np.asarray(p, np.float32)
    r2 = np.float32(np.float32(radius) * np.float32(radius))
    out = np.zeros(len(p), np.int32)
    for i in range(len(p)):
        c = sum(1 for j in range(len(p)) if j != i and naive_d2(p[i], p[j]) <= r2)
        out[i] = c if cap is None else min(c, cap)
    return out


# ---- seeded clouds with planted strays -------------------------------------------------------------------------------------------------

def strays(seed):
    """40 seeded uniform(-1.5, 1.5)^3 draws, kept where the norm is < 0.8 or > 1.2: points off the unit sphere"""
    s = np.random.RandomState(seed).uniform(-1.5, 1.5, (40, 3))
    r = np.linalg.norm(s, axis=1)
    return s[(r < 0.8) | (r > 1.2)].astype(np.float32)


def planted(n, seed):
    """-> (sphere(n, seed) with its strays appended, the number of strays)"""
    s = strays(seed)
    return np.concatenate([sphere(n, seed), s]), len(s)


# ---- the inputs of the threshold-and-mask tests: name -> cloud; every one at MASK_K x MASK_RATIO -------------------------------------------
MASK_K, MASK_RATIO = (7, 8, 16, 31), (1.0, 2.0)
BAND = 1e-9                                                     # no oracle mean_dist may lie this close (relative) to the threshold


def mask_cloud(name):
    if name == "planted2000":
        return planted(2000, 1)[0]
    if name == "planted4097":
        return planted(4097, 2)[0]
    if name == "plane":
        return noisy_plane()
    if name == "ellipsoid":
        return far_ellipsoid()
    raise KeyError(name)


MASK_CLOUDS = ("planted2000", "planted4097", "plane", "ellipsoid")
