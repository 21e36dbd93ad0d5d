"""numpy restatement of dispu_icp_segments / dispu_rigid_apply_segments (include/dispu_hip.h, csrc/icp.hip) for one pair of clouds: the
yardstick of the registration tests.  Correspondences are rank 0 of mls_oracle.neighbors (the smallest (fp32 plain-arithmetic d2, index),
see match()); everything after them in float64: the Jacobian rows written out, A = J^T J, a Cholesky of its own with the header's pivot rule,
Rodrigues, the composition.  apply() is bit for bit the kernel's; the sums are not (numpy adds in another order), which the GPU tests
allow for by a bound from cond(A)."""
import functools

import numpy as np

import mls_oracle as MO
import normals_oracle as NO

PIVOT = 1e-12


def identity():
    return np.eye(4)


def apply(T, pts):
    """[n, 3] fp32: (float)(((T00*x + T01*y) + T02*z) + T03) per row, in float64 from the fp32 points: the kernel's bits"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.ascontiguousarray(pts, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1).astype(np.float32)


def apply64(T, pts):
    """the same motion without the final rounding, float64"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.asarray(pts, np.float32).astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def max_d2_of(max_distance):
    """what the Python entry passes: float32(float64(max_distance)^2)"""
    return np.float32(np.float64(max_distance) * np.float64(max_distance))


def match(cur, target, max_d2=np.inf):
    """-> idx [q] int32 (the nearest target point of every row), d2 [q] fp32, inlier [q] bool.  Column 0 of mls_oracle.neighbors(cur,
    target, 1) -- the smallest (d2, index) over mls_oracle.sqdist_cross -- taken by argmin (the first of equal minima is the lowest
    index) instead of a full stable argsort per row, which is what made a 40-iteration run slow; test_icp_oracle.py holds the two equal
    on clouds full of ties.  Finite clouds only (argmin and argsort place a NaN differently)."""
    cur, target = np.ascontiguousarray(cur, np.float32), np.ascontiguousarray(target, np.float32)
    idx, d2 = np.empty(len(cur), np.int32), np.empty(len(cur), np.float32)
    for lo in range(0, len(cur), 256):
        d = MO.sqdist_cross(cur[lo:lo + 256], target)
        assert d.dtype == np.float32
        j = np.argmin(d, axis=1)
        idx[lo:lo + 256], d2[lo:lo + 256] = j, d[np.arange(len(j)), j]
    return idx, d2, d2 <= np.float32(max_d2)


def equations(cur, target, idx, inlier, normals=None):
    """-> A [6, 6], b [6], e, count of the header's normal equations, about o = target[0]"""
    t64 = np.asarray(target, np.float32).astype(np.float64)
    o = t64[0]
    p = np.asarray(cur, np.float32).astype(np.float64)[inlier] - o
    qv = t64[idx[inlier]] - o
    d = p - qv
    n = len(p)
    if normals is None:                                                         # three rows per point: J = [-[p]x | I]
        J = np.zeros((n, 3, 6))
        J[:, 0, 1], J[:, 0, 2] = p[:, 2], -p[:, 1]
        J[:, 1, 0], J[:, 1, 2] = -p[:, 2], p[:, 0]
        J[:, 2, 0], J[:, 2, 1] = p[:, 1], -p[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
        J, r = J.reshape(-1, 6), d.reshape(-1)
    else:                                                                       # one row per point: J = [(p x n)^T | n^T]
        nn = np.asarray(normals, np.float32).astype(np.float64)[idx[inlier]]
        J = np.concatenate([np.cross(p, nn), nn], axis=1)
        r = (d * nn).sum(axis=1)
    return J.T @ J, J.T @ r, float(r @ r), n


def cholesky(A):
    """-> L, the pivots' ratios d_j / A_jj (what the rule compares with 1e-12), ok"""
    L, ratio, ok = np.zeros((6, 6)), np.zeros(6), True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
            ratio[j] = d / A[j, j]
            if not (d > PIVOT * A[j, j]) or not np.isfinite(d):
                ok = False
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L, ratio, ok


def rodrigues(w):
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-12:
        a, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * K + c * (K @ K)


def step(T, source, target, normals=None, max_d2=np.inf):
    """one update from T -> dict(T: the new transform (T itself when degenerate), degenerate, w, t, A, b, e, count, cond, ratio, idx,
    inlier, cur)"""
    cur = apply(T, source)
    idx, d2, inlier = match(cur, target, max_d2)
    A, b, e, n = equations(cur, target, idx, inlier, normals)
    L, ratio, ok = cholesky(A)
    res = dict(T=np.array(T, np.float64), degenerate=True, w=np.zeros(3), t=np.zeros(3), A=A, b=b, e=e, count=n, ratio=ratio, idx=idx,
               inlier=inlier, cur=cur, cond=np.inf)
    if n < (3 if normals is None else 6) or not ok:
        return res
    with np.errstate(all="ignore"):
        x = np.linalg.solve(L.T, np.linalg.solve(L, -b))
    if not np.isfinite(x).all():
        return res
    w, t = x[:3], x[3:]
    R = rodrigues(w)
    o = np.asarray(target, np.float32).astype(np.float64)[0]
    Tn = np.eye(4)
    Tn[:3, :3] = R @ res["T"][:3, :3]
    Tn[:3, 3] = R @ (res["T"][:3, 3] - o) + o + t
    if not np.isfinite(Tn).all():
        return res
    res.update(T=Tn, degenerate=False, w=w, t=t, cond=float(np.linalg.cond(A)))
    return res


def diagonal(target):
    t = np.asarray(target, np.float32).astype(np.float64)
    return float(np.linalg.norm(t.max(axis=0) - t.min(axis=0)))


def evaluate(T, source, target, max_d2=np.inf, normals=None, matched=None):
    """the outputs of the returned T -> dict(aligned, corr, inliers, rmse, e).  matched: (idx, d2) of match(apply(T, source), target),
    where a caller already has them"""
    cur = apply(T, source)
    if matched is None:
        idx, d2, inlier = match(cur, target, max_d2)
    else:
        idx, d2 = matched
        inlier = d2 <= np.float32(max_d2)
    _, _, e, n = equations(cur, target, idx, inlier, normals)
    return dict(aligned=cur, corr=np.where(inlier, idx, -1).astype(np.int32), inliers=n, rmse=float(np.sqrt(e / n)) if n else 0.0, e=e)


def icp(source, target, normals=None, init=None, max_distance=np.inf, iterations=30, tolerance=1e-6):
    """-> dict(T, aligned, corr, inliers, rmse, iters, flag (0 out of iterations, 1 converged, 2 degenerate), steps: the dicts of step())"""
    T = identity() if init is None else np.array(init, np.float64).reshape(4, 4)
    max_d2, D = max_d2_of(max_distance), diagonal(target)
    flag, iters, steps = 0, 0, []
    for _ in range(iterations):
        if flag:
            break
        s = step(T, source, target, normals, max_d2)
        steps.append(s)
        if s["degenerate"]:
            flag = 2
            break
        T = s["T"]
        iters += 1
        if tolerance > 0 and np.linalg.norm(s["w"]) <= tolerance and np.linalg.norm(s["t"]) <= tolerance * D:
            flag = 1
    out = evaluate(T, source, target, max_d2, normals)
    out.update(T=T, iters=iters, flag=flag, steps=steps)
    return out


# ---- seeded clouds shared by the tests -------------------------------------------------------------------------------------------------

AXIS, ANGLE, SHIFT = np.array([0.3, -0.5, 0.8]), np.deg2rad(10.0), np.array([0.5, -0.3, 0.2])
CAP_SCALE = np.float32([1.0, 0.7, 0.4])


def motion(cloud):
    """the 4 x 4 motion of the moved sources: ANGLE about AXIS through the cloud's centroid, then 0.05 * extent * SHIFT (extent: the
    longest side of the bounding box)"""
    c64 = np.asarray(cloud, np.float32).astype(np.float64)
    cen, extent = c64.mean(axis=0), float((c64.max(axis=0) - c64.min(axis=0)).max())
    R = rodrigues(AXIS / np.linalg.norm(AXIS) * ANGLE)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = cen - R @ cen + 0.05 * extent * SHIFT
    return M


def moved(cloud):
    """every second point of the cloud under motion(cloud), rounded to fp32 -> (source, truth: the points it came from)"""
    truth = np.ascontiguousarray(cloud[::2])
    return apply64(motion(cloud), truth).astype(np.float32), truth


@functools.lru_cache(maxsize=None)
def cap():
    """-> target [3091, 3], its analytic unit normals, source [1546, 3], truth [1546, 3]: an open cap of an ellipsoid"""
    p = NO.sphere(4097) * CAP_SCALE
    p = np.ascontiguousarray(p[p[:, 2] > -0.2])
    g = p.astype(np.float64) / (CAP_SCALE.astype(np.float64) ** 2)
    nrm = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    src, truth = moved(p)
    return p, nrm, src, truth


@functools.lru_cache(maxsize=None)
def far():
    """-> target [2049, 3], analytic normals, source [1025, 3], truth: 2 cm of structure at coordinates of 1000"""
    p = NO.far_ellipsoid(2049)
    g = (p.astype(np.float64) - np.array([1000.0, -500.0, 250.0])) / (np.array([1.0, 0.6, 0.3]) * 0.01) ** 2
    nrm = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    src, truth = moved(p)
    return p, nrm, src, truth


@functools.lru_cache(maxsize=None)
def recovery(plane):
    """the oracle's own run of the recovery case on cap at tolerance 0: 40 iterations point to point, 8 point to plane (computed once
    per process: the CPU tests and the GPU tests share it)"""
    p, nrm, src, _ = cap()
    return icp(src, p, nrm if plane else None, iterations=8 if plane else 40, tolerance=0.0)


@functools.lru_cache(maxsize=None)
def first_step(name, plane):
    """the oracle's first step from the identity on cap or far"""
    p, nrm, src, _ = cap() if name == "cap" else far()
    return step(identity(), src, p, nrm if plane else None)


def coplanar():
    """-> target [400, 3] in the plane z = 0.25 with constant normals, source [150, 3] the same plane's points shifted inside it"""
    r = np.random.RandomState(11)
    t = np.concatenate([r.random_sample((400, 2)), np.full((400, 1), 0.25)], axis=1).astype(np.float32)
    nrm = np.tile(np.float32([[0, 0, 1]]), (400, 1))
    s = (t[:150] + np.float32([0.01, -0.02, 0.0])).astype(np.float32)
    return t, nrm, s


def degenerate_cases():
    """(source, target, normals or None, max_distance, why): each must end with flag 2 and T = init after one step"""
    p, nrm, src, _ = cap()
    ct, cn, cs = coplanar()
    one = np.float32([[0.5, 0.25, -1.0]])
    return [
        (src, p, None, 1e-30, "no inlier, point mode"),
        (src, p, nrm, 1e-30, "no inlier, plane mode"),
        (one + np.float32(0.125), one, None, np.inf, "one-point clouds, point mode"),
        (one + np.float32(0.125), one, np.float32([[0, 0, 1]]), np.inf, "one-point clouds, plane mode"),
        (cs, ct, cn, np.inf, "plane mode onto a coplanar target with constant normals: in-plane motion is free"),
    ]
