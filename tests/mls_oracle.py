"""numpy restatement of dispu_mls_project_segments (include/dispu_hip.h, csrc/mls_project.hip) for one pair of clouds: the yardstick of
the MLS tests.  Neighbours by a stable argsort of the fp32 plain-arithmetic d2 = ((dx*dx + dy*dy) + dz*dz), as normals_oracle.sqdist_rows
forms it; everything after them in float64, sums in ascending rank, numpy.linalg.eigh for the plane."""
import numpy as np

import normals_oracle as NO


def sqdist_cross(q, r):
    """[nq, m] fp32: d2 of every query to every reference point, one rounding per operation, in the kernel's order"""
    d = r[None, :, :] - q[:, None, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def neighbors(q, r, k, chunk=256):
    """-> idx [nq, k] int32 (-1 beyond k' = min(k, m)), d2 [nq, k] float32 (+inf beyond k'): the k' smallest (d2, index), ascending"""
    q, r = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(r, np.float32)
    kp = min(k, len(r))
    idx = np.full((len(q), k), -1, np.int32)
    d2 = np.full((len(q), k), np.inf, np.float32)
    for lo in range(0, len(q), chunk):
        d = sqdist_cross(q[lo:lo + chunk], r)
        assert d.dtype == np.float32
        order = np.argsort(d, axis=1, kind="stable")[:, :kp]
        idx[lo:lo + chunk, :kp] = order
        d2[lo:lo + chunk, :kp] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def step(q, r, k, support=1.0, idx=None, d2=None):
    """one step -> dict(new64 [nq, 3] float64, new32 [nq, 3] float32, ok [nq] (True: moved; False: stayed by rule, new32 = the input's
    bits), evals [nq, 3] ascending, D [nq] float64, idx [nq, k] int32, d2 [nq, k] float32)"""
    q, r = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(r, np.float32)
    if idx is None:
        idx, d2 = neighbors(q, r, k)
    nq, kp = len(q), min(k, len(r))
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    d64 = d2[:, :kp].astype(np.float64)
    D = d64[:, kp - 1].copy()
    rho2 = (float(support) * float(support)) * D
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = d64 / rho2[:, None]
        rr = np.sqrt(r2)
        a = 1.0 - rr
        a2 = a * a
        w = np.where(r2 >= 1.0, 0.0, (a2 * a2) * (4.0 * rr + 1.0))
    live = (w != 0.0).sum(axis=1)
    u = r64[idx[:, :kp]] - q64[:, None, :]
    s0, s1, s2 = np.zeros(nq), np.zeros((nq, 3)), np.zeros((nq, 3, 3))
    for j in range(kp):                                                         # ascending rank
        wu = w[:, j, None] * u[:, j]
        s0 += w[:, j]
        s1 += wu
        s2 += wu[:, :, None] * u[:, j, None, :]
    pre = (kp >= 3) & (live >= 3) & (D != 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = s1 / s0[:, None]
        cov = s2 / s0[:, None, None] - c[:, :, None] * c[:, None, :]
    cov[~pre] = np.eye(3)                                                       # eigh is not asked about rows the rule has settled
    c[~pre] = 0.0
    ev, vec = np.linalg.eigh(cov)
    ok = pre & ~(ev[:, 2] <= 0.0) & ~(ev[:, 1] <= 1e-12 * ev[:, 2])
    nrm = vec[:, :, 0]
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    t = (c * nrm).sum(axis=1)
    new64 = np.where(ok[:, None], q64 + t[:, None] * nrm, q64)
    new32 = np.where(ok[:, None], new64.astype(np.float32), q)
    ev[~pre] = 0.0
    return dict(new64=new64, new32=new32, ok=ok, evals=ev, D=D, idx=idx, d2=d2)


def project(q, r, k, support=1.0, iterations=1):
    """T steps on the moved fp32 positions against the same references -> the last step's dict"""
    cur = np.ascontiguousarray(q, np.float32)
    for _ in range(iterations):
        res = step(cur, r, k, support)
        cur = res["new32"]
    return res


def radial_rms(p):
    """RMS distance of the points from the unit sphere, in float64"""
    return float(np.sqrt(np.mean((np.linalg.norm(np.asarray(p, np.float64), axis=1) - 1.0) ** 2)))


# ---- seeded clouds shared by the tests -------------------------------------------------------------------------------------------------

def noisy_sphere(n, seed, sigma, noise_seed):
    """normals_oracle.sphere(n, seed) + sigma * N(0, 1) per coordinate from RandomState(noise_seed), fp32"""
    return (NO.sphere(n, seed) + sigma * np.random.RandomState(noise_seed).standard_normal((n, 3))).astype(np.float32)


def denoise_self():
    """denoising case 1: a noisy sphere against itself at k = 16, support = 1.5"""
    return noisy_sphere(4097, 0, 0.01, 1)


def denoise_cross():
    """denoising case 2: 8192 points at sigma 0.03 onto the surface of 2049 points at sigma 0.005, k = 16, support = 1.0"""
    return noisy_sphere(8192, 2, 0.03, 3), noisy_sphere(2049, 0, 0.005, 4)


def collinear():
    """the collinear cloud of the normals tests"""
    return (np.arange(200, dtype=np.float32)[:, None] * np.float32([[0.5, 0.25, -1.0]])).astype(np.float32)


def stay_cases():
    """(queries, refs, support, why) of every stay rule: the queries must keep their bits"""
    r = np.random.RandomState(7)
    q = r.random_sample((5, 3)).astype(np.float32)
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    same = np.tile(np.float32([[3, -1, 2]]), (40, 1))
    # small integers: at support 2 every weight is 0.1875 and every sum, quotient and product of the fit is exact, so the covariance is
    # exactly zero for the kernel and the oracle alike.  (With coordinates that round, its sign would be rounding noise.)
    grid = np.float32([[0, 0, 0], [5, -1, 2], [3, 4, -6], [-2, -1, 7], [1, 1, 1]])
    return [
        (q, tri[:1], 2.0, "one reference point: k' < 3"),
        (q, tri[:2], 2.0, "two reference points: k' < 3"),
        (q, tri, 1.0, "three reference points at support 1: the farthest has weight 0, two weights are left"),
        (grid, same, 2.0, "40 coincident reference points: equal weights, zero covariance, l2 <= 0"),
        (same[:3], same, 2.0, "queries on 40 coincident reference points: D == 0"),
        (q, collinear(), 2.0, "collinear reference points: l1 <= 1e-12 l2"),
        (collinear()[:70], collinear(), 1.5, "a collinear cloud against itself"),
    ]
