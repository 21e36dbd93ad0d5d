"""numpy restatement of dispu_pca_normals_segments (include/dispu_hip.h, csrc/normals.hip) for one cloud: the yardstick of the normals
tests.  Neighbours by a stable argsort of the fp32 plain-arithmetic d2 = ((dx*dx + dy*dy) + dz*dz); the covariance of q_j = p_j - p_i
in float64, numpy.linalg.eigh, the sign rules and the variation as the header states them."""
import numpy as np


def sqdist_rows(p, lo, hi):
    """[hi - lo, n] fp32: d2 of points lo .. hi - 1 to every point, one rounding per operation, in the kernel's order"""
    p = np.ascontiguousarray(p, np.float32)
    d = p[None, :, :] - p[lo:hi, None, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def neighbors(p, k, chunk=512):
    """[n, k] int32: per point the min(k, n) smallest (d2, index), ascending, padded with -1"""
    p = np.ascontiguousarray(p, np.float32)
    n = p.shape[0]
    kp = min(k, n)
    out = np.full((n, k), -1, np.int32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d2 = sqdist_rows(p, lo, hi)
        assert d2.dtype == np.float32
        out[lo:hi, :kp] = np.argsort(d2, axis=1, kind="stable")[:, :kp]
    return out


def covariances(p, idx):
    """[n, 3, 3] float64: Cov = sum q q^T / k' - mu mu^T over q_j = p_j - p_i, and k' [n]"""
    p64 = np.asarray(p, np.float32).astype(np.float64)
    valid = idx >= 0
    kp = valid.sum(axis=1)
    q = (p64[np.where(valid, idx, 0)] - p64[:, None, :]) * valid[:, :, None]
    mu = q.sum(axis=1) / kp[:, None]
    cov = np.einsum("nki,nkj->nij", q, q) / kp[:, None, None] - mu[:, :, None] * mu[:, None, :]
    return cov, kp


def canonical_sign(nrm):
    """mode 0 on fp32 vectors: the component of largest magnitude positive, ties to the lowest axis"""
    nrm = np.array(nrm, np.float32)
    a = np.argmax(np.abs(nrm), axis=1)                     # the first of equal maxima
    lead = nrm[np.arange(len(nrm)), a]
    nrm[lead < 0] *= -1
    return nrm


def orient_sign(nrm, direction):
    """modes 1 and 2 after canonical_sign: flip where the dot product (in float64) is negative, keep where it is 0"""
    nrm = np.array(nrm, np.float32)
    dot = np.einsum("ni,ni->n", nrm.astype(np.float64), np.asarray(direction, np.float64))
    nrm[dot < 0] *= -1
    return nrm


def normals(p, k, orient_mode=0, orient=None, idx=None):
    """-> dict(normal [n,3] f32, variation [n] f32, idx [n,k] i32, cov [n,3,3] f64, evals [n,3] f64 ascending, evec [n,3] f64 the
    unsigned eigenvector of evals[:, 0], ok [n] where a normal exists)
    orient_mode 1: orient [n, 3] directions; 2: orient [3] a viewpoint."""
    p = np.ascontiguousarray(p, np.float32)
    if idx is None:
        idx = neighbors(p, k)
    cov, kp = covariances(p, idx)
    w, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0].astype(np.float32)
    ok = (kp >= 3) & (w[:, 2] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(ok, np.maximum(w[:, 0], 0.0) / w.sum(axis=1), -1.0).astype(np.float32)
    nrm = canonical_sign(nrm)
    if orient_mode == 1:
        nrm = orient_sign(nrm, orient)
    elif orient_mode == 2:
        nrm = orient_sign(nrm, np.asarray(orient, np.float32).astype(np.float64)[None, :] - p.astype(np.float64))
    nrm[~ok] = 0
    return dict(normal=nrm, variation=var, idx=idx, cov=cov, evals=w, evec=v[:, :, 0], ok=ok)


# ---- seeded clouds shared by the tests -------------------------------------------------------------------------------------------------

def sphere(n, seed=0):
    """n seeded points on the unit sphere, fp32"""
    v = np.random.RandomState(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def far_ellipsoid(n=2049, seed=0):
    """semi-axes (1, .6, .3) * 0.01 centred at (1000, -500, 250): millimetre structure at large coordinates, where fp32 moments of raw
    coordinates lose everything"""
    v = np.random.RandomState(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (np.array([1.0, 0.6, 0.3]) * 0.01) + np.array([1000.0, -500.0, 250.0])).astype(np.float32)


def noisy_plane(n=1500, seed=0, noise=1e-3):
    r = np.random.RandomState(seed)
    return np.concatenate([r.random_sample((n, 2)), noise * r.standard_normal((n, 1))], axis=1).astype(np.float32)


def lattice(m=17):
    g = np.arange(m, dtype=np.float32)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
