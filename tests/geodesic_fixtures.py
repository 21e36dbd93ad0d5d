"""Meshes with closed-form geodesic distances, built in numpy, shared by tests/test_geodesic.py and tests/test_geodesic_gpu.py.

Every case is (verts [V,3] f64, faces [F,3], seed (face, bary [3]), targets [n,3] f64, target faces [n], expected [n] f64)."""
import math

import numpy as np


def _locate(verts, faces, p):
    """face holding p (within 1e-9 of its plane and inside its barycentric range), and the barycentrics"""
    tv = verts[faces]
    best = None
    for f in range(faces.shape[0]):
        a, b, c = tv[f]
        n = np.cross(b - a, c - a)
        area2 = np.dot(n, n)
        w0 = np.dot(np.cross(c - b, p - b), n) / area2
        w1 = np.dot(np.cross(a - c, p - c), n) / area2
        w2 = 1.0 - w0 - w1
        off = abs(np.dot(p - a, n)) / math.sqrt(area2)
        score = max(-min(w0, w1, w2), 0.0) + off
        if best is None or score < best[0]:
            best = (score, f, np.array([w0, w1, w2]))
    assert best[0] < 1e-9, "point not on the mesh"
    return best[1], best[2]


def grid(nx, ny, jitter=0.0, seed=0):
    """planar grid on [0,1]^2 (z = 0) of nx*ny cells, two triangles each, interior vertices jittered"""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing="ij")
    v = np.stack([xs, ys, np.zeros_like(xs)], -1).reshape(-1, 3)
    inner = (xs > 0) & (xs < 1) & (ys > 0) & (ys < 1)
    j = rng.uniform(-jitter, jitter, (v.shape[0], 2)) * inner.reshape(-1, 1) / max(nx, ny)
    v[:, :2] += j
    f = []
    for i in range(nx):
        for k in range(ny):
            a, b, c, d = i * (ny + 1) + k, (i + 1) * (ny + 1) + k, (i + 1) * (ny + 1) + k + 1, i * (ny + 1) + k + 1
            f += [(a, b, c), (a, c, d)] if (i + k) % 2 == 0 else [(a, b, d), (b, c, d)]
    return v, np.array(f, np.int32)


def planar_case(seed=0, n=40):
    v, f = grid(7, 6, jitter=0.35, seed=seed)
    rng = np.random.default_rng(seed + 1)
    s = np.array([0.43, 0.52, 0.0])
    sf, sb = _locate(v, f, s)
    t = np.concatenate([rng.uniform(0.02, 0.98, (n, 2)), np.zeros((n, 1))], 1)
    tf = np.array([_locate(v, f, p)[0] for p in t])
    return v, f, (sf, sb), t, tf, np.linalg.norm(t - s, axis=1)


def folded_case(angle_deg=100.0, n=30, seed=0):
    """two 1 x 1 rectangles sharing the edge x = 0 (y in [0,1]), opened to a dihedral angle: geodesic = unfolded distance"""
    th = math.radians(angle_deg)
    g, gf = grid(4, 5)
    left = g.copy()
    left[:, 0] = -g[:, 0]                                             # x in [-1, 0], z = 0
    right = np.stack([g[:, 0] * math.cos(math.pi - th), g[:, 1], g[:, 0] * math.sin(math.pi - th)], 1)
    v = np.concatenate([left, right])
    f = np.concatenate([gf[:, ::-1], gf + g.shape[0]])
    # merge the shared edge x = 0
    key = {}
    remap = np.arange(v.shape[0])
    for i, p in enumerate(v):
        kk = (round(p[0], 12), round(p[1], 12), round(p[2], 12))
        if kk in key:
            remap[i] = key[kk]
        else:
            key[kk] = i
    f = remap[f]
    used, inv = np.unique(f, return_inverse=True)
    v, f = v[used], inv.reshape(-1, 3).astype(np.int32)
    rng = np.random.default_rng(seed)
    su = np.array([-0.55, 0.35])                                      # (unfolded x, y): x < 0 left sheet, x > 0 right sheet
    tu = np.stack([rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n)], 1)

    def emb(u):
        if u[0] <= 0:
            return np.array([u[0], u[1], 0.0])
        return np.array([u[0] * math.cos(math.pi - th), u[1], u[0] * math.sin(math.pi - th)])

    s = emb(su)
    t = np.array([emb(u) for u in tu])
    sf, sb = _locate(v, f, s)
    tf = np.array([_locate(v, f, p)[0] for p in t])
    return v, f, (sf, sb), t, tf, np.linalg.norm(tu - su, axis=1)


def cone_fan(theta, n=12, rho=1.0, closed=True):
    """triangles around an apex at the origin whose angles add up to theta (closed fan: rim vertices i, i+1 mod n; open: n
    triangles and n+1 rim vertices, the apex on the boundary).  Convex: rim at z = -h; saddle: rim at z = +-h alternating.
    -> (verts, faces, corner angles, unit in-plane frames per triangle)"""
    m = n if closed else n + 1
    phi = 2 * math.pi * np.arange(m) / n if closed else theta * np.arange(m) / n

    def build(h):
        z = (-h * np.ones(m)) if theta <= 2 * math.pi or not closed else h * (1 - 2 * (np.arange(m) % 2))
        if not closed:
            z = np.zeros(m) if h == 0 else z
        rim = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
        return np.concatenate([[[0.0, 0.0, 0.0]], rim])

    faces = np.array([(0, 1 + i, 1 + (i + 1) % m) for i in range(n)], np.int32)

    def angles(v):
        a = v[faces[:, 1]]
        b = v[faces[:, 2]]
        return np.arccos(np.clip(np.sum(a * b, 1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1), -1, 1))

    if closed:
        lo, hi = 0.0, 50.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            tot = angles(build(mid)).sum()
            if (tot > theta) == (theta > 2 * math.pi):
                hi = mid
            else:
                lo = mid
        v = build(0.5 * (lo + hi))
    else:
        v = build(0.0) if theta <= 2 * math.pi else None
        if v is None:   # an open fan wider than 2 pi: a helicoid-like staircase, each triangle of angle theta / n
            rim = []
            for i in range(m):
                a = theta * i / n
                rim.append([rho * math.cos(a), rho * math.sin(a), 0.15 * a])
            v = np.concatenate([[[0.0, 0.0, 0.0]], np.array(rim)])
    return v, faces, angles(v)


def _fan_point(v, faces, ang, r, a):
    """point at distance r from the apex and unrolled angle a (from the first rim vertex) on the fan"""
    cum = np.concatenate([[0.0], np.cumsum(ang)])
    i = min(int(np.searchsorted(cum, a, side="right") - 1), faces.shape[0] - 1)
    e1 = v[faces[i, 1]] / np.linalg.norm(v[faces[i, 1]])
    w = v[faces[i, 2]] - np.dot(v[faces[i, 2]], e1) * e1
    e2 = w / np.linalg.norm(w)
    loc = a - cum[i]
    return r * (math.cos(loc) * e1 + math.sin(loc) * e2), i


def cone_case(theta, closed=True, n_targets=40, seed=0):
    v, f, ang = cone_fan(theta, closed=closed)
    total = float(ang.sum())
    rng = np.random.default_rng(seed)
    rmax = 0.45 * math.cos(ang.max() / 2)
    a_s, r_s = 0.37 * total, 0.6 * rmax
    s, sf = _fan_point(v, f, ang, r_s, a_s)
    tgt, tf, exp = [], [], []
    for _ in range(n_targets):
        a = rng.uniform(0.01, 0.99) * total
        r = rng.uniform(0.05, 1.0) * rmax
        p, i = _fan_point(v, f, ang, r, a)
        sep = abs(a - a_s)
        if closed:
            sep = min(sep, total - sep)
        d = math.sqrt(max(r_s * r_s + r * r - 2 * r_s * r * math.cos(sep), 0.0)) if sep < math.pi else r_s + r
        tgt.append(p)
        tf.append(i)
        exp.append(d)
    sf2, sb = _locate(v, f, s)
    return v, f, (sf2, sb), np.array(tgt), np.array(tf), np.array(exp)


def cube(n=3):
    """surface of the unit cube [0,1]^3, each side an n x n grid of triangle pairs, outward orientation"""
    g, gf = grid(n, n)
    verts, faces = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            p = np.zeros((g.shape[0], 3))
            o = [i for i in range(3) if i != axis]
            p[:, o[0]], p[:, o[1]], p[:, axis] = g[:, 0], g[:, 1], side
            ff = gf + sum(x.shape[0] for x in verts)
            flip = (side == 0.0) != (axis == 1)
            faces.append(ff[:, ::-1] if flip else ff)
            verts.append(p)
    v = np.concatenate(verts)
    f = np.concatenate(faces)
    key, remap = {}, np.arange(v.shape[0])
    for i, p in enumerate(v):
        kk = tuple(np.round(p, 12))
        remap[i] = key.setdefault(kk, i)
    f = remap[f]
    used, inv = np.unique(f, return_inverse=True)
    return v[used], inv.reshape(-1, 3).astype(np.int32)


def cube_case(n_targets=30, seed=0):
    """seed on the side z = 1 and targets on the side x = 1, both near the middle of their shared edge (x = 1, z = 1):
    unfolding across that edge, the distance is the planar one."""
    v, f = cube(3)
    rng = np.random.default_rng(seed)
    s = np.array([0.88, 0.47, 1.0])
    su = np.array([-(1.0 - s[0]), s[1]])            # unfolded: distance to the edge along -u, y
    tgt, exp = [], []
    for _ in range(n_targets):
        dz, y = rng.uniform(0.01, 0.2), rng.uniform(0.35, 0.65)
        tgt.append([1.0, y, 1.0 - dz])
        exp.append(np.linalg.norm(np.array([dz, y]) - su))
    t = np.array(tgt)
    sf, sb = _locate(v, f, s)
    tf = np.array([_locate(v, f, p)[0] for p in t])
    return v, f, (sf, sb), t, tf, np.array(exp)


def seed_on_edge_case():
    """the planar grid with the seed exactly on an interior edge (one barycentric exactly 0)"""
    v, f = grid(6, 6)
    fs = 30
    a, b = f[fs, 0], f[fs, 1]
    bary = np.array([0.375, 0.625, 0.0])
    s = bary @ v[f[fs]]
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.uniform(0.02, 0.98, (40, 2)), np.zeros((40, 1))], 1)
    tf = np.array([_locate(v, f, p)[0] for p in t])
    del a, b
    return v, f, (fs, bary), t, tf, np.linalg.norm(t - s, axis=1)


def seed_on_vertex_case():
    """a cube seed exactly on a corner vertex (two barycentrics 0); targets on the three sides meeting there, where the
    geodesic is the straight line inside each side"""
    v, f = cube(3)
    corner = int(np.argmin(np.linalg.norm(v - np.array([1.0, 1.0, 1.0]), axis=1)))
    fs, j = next((i, int(np.nonzero(f[i] == corner)[0][0])) for i in range(f.shape[0]) if corner in f[i])
    bary = np.zeros(3)
    bary[j] = 1.0
    rng = np.random.default_rng(4)
    tgt = []
    for side in range(3):
        for _ in range(10):
            p = np.ones(3)
            o = [i for i in range(3) if i != side]
            p[o[0]], p[o[1]] = rng.uniform(0.3, 0.95, 2)
            tgt.append(p)
    t = np.array(tgt)
    tf = np.array([_locate(v, f, p)[0] for p in t])
    return v, f, (fs, bary), t, tf, np.linalg.norm(t - v[corner], axis=1)


CASES = {
    "planar": planar_case,
    "folded_100": lambda: folded_case(100.0),
    "folded_40": lambda: folded_case(40.0),
    "cone_1.5pi": lambda: cone_case(1.5 * math.pi),
    "cone_2.5pi": lambda: cone_case(2.5 * math.pi),
    "cone_3pi": lambda: cone_case(3.0 * math.pi),
    "cone_open_1.5pi": lambda: cone_case(1.5 * math.pi, closed=False),
    "cube_edge": cube_case,
    "seed_on_edge": seed_on_edge_case,
    "seed_on_vertex": seed_on_vertex_case,
}
