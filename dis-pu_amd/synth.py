"""Synthetic inputs of SURVEY.md section 8(d): spherical-cap patches with the reference's jitter and
patch normalisation (Common/point_operation.py:74-86 sigma = 0.005 jitter; Common/pc_util.py:147-161
centroid / max-radius normalisation).  Pure numpy; deterministic in (seed)."""
import numpy as np


def cap_patch(rng, npoint, jitter=0.005):
    """npoint points on the z > median half of the unit sphere (a 2-manifold patch), jittered."""
    pts = np.empty((0, 3), np.float64)
    while pts.shape[0] < npoint:
        g = rng.standard_normal((4 * npoint, 3))
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        g = g[g[:, 2] > 0.5]
        pts = np.concatenate([pts, g], axis=0)
    pts = pts[:npoint]
    pts = pts + rng.normal(0.0, jitter, pts.shape)
    return pts


def normalize(pts):
    """pc_util.normalize_point_cloud: subtract centroid, divide by the furthest distance."""
    c = pts.mean(axis=0, keepdims=True)
    p = pts - c
    r = np.sqrt((p ** 2).sum(axis=1)).max()
    return p / r, c, r


def patches(batch, npoint=256, seed=0):
    """[batch, npoint, 3] float32 normalised patches."""
    rng = np.random.default_rng(seed)
    out = np.empty((batch, npoint, 3), np.float32)
    for i in range(batch):
        out[i] = normalize(cap_patch(rng, npoint))[0].astype(np.float32)
    return out


def patch_with_gt(batch, npoint=256, ngt=1024, seed=0):
    """(input [batch,npoint,3], ground truth [batch,ngt,3]) drawn from the same cap, same normalisation."""
    rng = np.random.default_rng(seed)
    x = np.empty((batch, npoint, 3), np.float32)
    g = np.empty((batch, ngt, 3), np.float32)
    for i in range(batch):
        p, c, r = normalize(cap_patch(rng, npoint))
        x[i] = p.astype(np.float32)
        g[i] = ((cap_patch(rng, ngt) - c) / r).astype(np.float32)
    return x, g


def icosphere(level, radius=1.0):
    """(verts [V,3] f32, faces [20*4^level, 3] i32): an icosahedron with every triangle split in four `level` times and the
    vertices pushed onto the sphere -- a closed test mesh of any size (level 7: 327680 faces)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = np.array(v, np.float64)
    verts /= np.linalg.norm(verts, axis=1, keepdims=True)
    faces = np.array(f, np.int64)
    for _ in range(level):
        e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=0)
        key = np.sort(e, axis=1)
        uniq, inv = np.unique(key[:, 0] * (1 << 32) + key[:, 1], return_inverse=True)
        a, b = uniq >> 32, uniq & 0xFFFFFFFF
        mid = verts[a] + verts[b]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(3, -1) + verts.shape[0]
        verts = np.concatenate([verts, mid], axis=0)
        v0, v1, v2 = faces[:, 0], faces[:, 1], faces[:, 2]
        m01, m12, m20 = m[0], m[1], m[2]
        faces = np.concatenate([np.stack([v0, m01, m20], 1), np.stack([v1, m12, m01], 1), np.stack([v2, m20, m12], 1),
                                np.stack([m01, m12, m20], 1)], axis=0)
    return (verts * radius).astype(np.float32), faces.astype(np.int32)
