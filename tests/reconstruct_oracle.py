"""Sequential numpy restatement of dispu_signed_distance_segments and of the lattice / contouring entries behind
dispu_amd.reconstruct.reconstruct_surface (include/dispu_hip.h, csrc/signed_distance.hip, csrc/reconstruct.hip) for one cloud: the
yardstick of the reconstruction tests.  Neighbours by the project's rule (smallest (fp32 d2, index)); the sums in float64 in ascending
rank; the lattice in fp32 with one rounding per operation; every ordering pinned, so the device must return these bytes."""
import functools
import itertools

import numpy as np

import normals_oracle as NO
import orient_oracle as OO

BIAS = (1 << 20) - 1                                        # a lattice index i is stored as i + BIAS in 21 bits
SJ, SL = 21, 42                                             # key = (l + BIAS) << 42 | (j + BIAS) << 21 | (i + BIAS): ascending (l, j, i)


# ---- the signed distance ----------------------------------------------------------------------------------------------------------------

def neighbors(q, r, k, chunk=512):
    """-> d2 [nq, k'] float32, idx [nq, k'] int64: the k' = min(k, m) smallest (d2 bits, index) per query, ascending"""
    q, r = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(r, np.float32)
    m, kp = len(r), min(k, len(r))
    d2 = np.empty((len(q), kp), np.float32)
    idx = np.empty((len(q), kp), np.int64)
    col = np.arange(m, dtype=np.uint64)[None, :]
    for lo in range(0, len(q), chunk):
        d = r[None, :, :] - q[lo:lo + chunk, None, :]
        sq = d * d
        dd = np.ascontiguousarray((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        assert dd.dtype == np.float32
        keys = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | col       # d2 >= +0: its bits order as the values do
        if m > kp:
            keys = np.partition(keys, kp - 1, axis=1)[:, :kp]
        keys = np.sort(keys, axis=1)
        d2[lo:lo + chunk] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        idx[lo:lo + chunk] = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return d2, idx


def signed_distance(queries, points, normals, k=8, support=1.5):
    """[nq] float32"""
    q = np.ascontiguousarray(queries, np.float32)
    p = np.ascontiguousarray(points, np.float32)
    nr = np.ascontiguousarray(normals, np.float32)
    d2, idx = neighbors(q, p, k)
    kp = d2.shape[1]
    d64 = d2.astype(np.float64)
    rho2 = (float(support) * float(support)) * d64[:, kp - 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = d64 / rho2[:, None]
        inside = r2 < 1.0                                   # NaN (D == 0) and +inf are outside
        rr = np.sqrt(np.where(inside, r2, 0.0))
    a = 1.0 - rr
    a2 = a * a
    w = np.where(inside, (a2 * a2) * (4.0 * rr + 1.0), 0.0)
    u = q.astype(np.float64)[:, None, :] - p.astype(np.float64)[idx]
    nn = nr.astype(np.float64)[idx]
    g = (u[..., 0] * nn[..., 0] + u[..., 1] * nn[..., 1]) + u[..., 2] * nn[..., 2]
    s0, s1 = np.zeros(len(q)), np.zeros(len(q))
    for j in range(kp):                                     # ascending rank
        s0 = s0 + w[:, j]
        s1 = s1 + w[:, j] * g[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(s0 != 0.0, s1 / s0, g[:, 0])
    return f.astype(np.float32)


# ---- Kuhn's six tetrahedra and the case table ---------------------------------------------------------------------------------------------

def tets():
    """[6][4] corner numbers b = bx + 2 by + 4 bz: (0, e_a, e_a + e_b, 7) for the axis permutations in lexicographic order"""
    e = (1, 2, 4)
    return [(0, e[a], e[a] + e[b], 7) for a, b, _ in itertools.permutations(range(3))]


def _corner_xyz(b):
    return np.array([b & 1, (b >> 1) & 1, (b >> 2) & 1], np.float64)


def case_table():
    """[6][16] -> a list of triangles, each three edges (A, d): A the corner number of the edge's lower endpoint, d = B - A in 1 .. 7.
    Bit i of the mask: tet vertex i is negative.  Orientation is decided HERE, once, from the edge midpoints in the unit cube."""
    table = []
    for tet in tets():
        def E(u, v):
            i, j = min(u, v), max(u, v)
            return (tet[i], tet[j] - tet[i])
        row = []
        for mask in range(16):
            neg = [i for i in range(4) if mask >> i & 1]
            pos = [i for i in range(4) if not mask >> i & 1]
            if len(neg) in (1, 3):
                v = neg[0] if len(neg) == 1 else pos[0]
                o = [i for i in range(4) if i != v]
                tris = [(E(v, o[0]), E(v, o[1]), E(v, o[2]))]
            elif len(neg) == 2:
                qd = (E(neg[0], pos[0]), E(neg[0], pos[1]), E(neg[1], pos[1]), E(neg[1], pos[0]))
                tris = [(qd[0], qd[1], qd[2]), (qd[0], qd[2], qd[3])]
            else:
                tris = []
            if tris:
                want = np.mean([_corner_xyz(tet[i]) for i in pos], axis=0) - np.mean([_corner_xyz(tet[i]) for i in neg], axis=0)
                fixed = []
                for tri in tris:
                    a, b, c = ((_corner_xyz(A) + _corner_xyz(A + d)) / 2 for A, d in tri)
                    dot = float(np.dot(np.cross(b - a, c - a), want))
                    assert dot != 0.0
                    fixed.append(tri if dot > 0 else (tri[0], tri[2], tri[1]))
                tris = fixed
            row.append(tris)
        table.append(row)
    return table


def case_bytes():
    """the table as the kernels hold it: [6][16][7] uint8 = triangle count, then up to six edges as (A << 3) | d, zero-filled"""
    out = np.zeros((6, 16, 7), np.uint8)
    for t, row in enumerate(case_table()):
        for mask, tris in enumerate(row):
            out[t, mask, 0] = len(tris)
            for i, (A, d) in enumerate(e for tri in tris for e in tri):
                out[t, mask, 1 + i] = (A << 3) | d
    return out


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------------

def pack_key(i, j, l):
    return ((l + BIAS) << SL) | ((j + BIAS) << SJ) | (i + BIAS)


def unpack_key(key):
    key = np.asarray(key, np.int64)
    m = (1 << 21) - 1
    return (key & m) - BIAS, ((key >> SJ) & m) - BIAS, ((key >> SL) & m) - BIAS


def occupied_voxels(points, voxel, band):
    """sorted unique keys of the voxels that hold a point; ValueError when an index, after the band, leaves +-(2^20 - 1)"""
    p = np.ascontiguousarray(points, np.float32)
    h = np.float32(voxel)
    fi = np.floor(p / h)                                    # fp32, the division correctly rounded
    assert fi.dtype == np.float32
    if not (np.abs(fi) <= np.float32(BIAS - band)).all():
        raise ValueError("voxel = %r puts the cloud outside the lattice's index range of +-(2^20 - 1)" % float(voxel))
    v = fi.astype(np.int64)
    return np.unique(pack_key(v[:, 0], v[:, 1], v[:, 2]))


def dilate(occ, band):
    w = 2 * band + 1
    offs = np.array([(di - band) + ((dj - band) << SJ) + ((dl - band) << SL) for dl in range(w) for dj in range(w) for di in range(w)], np.int64)
    return np.unique((occ[:, None] + offs[None, :]).ravel())


def lattice(act):
    """-> lat [nlat] the sorted unique corner keys, corner [nvox, 8] their numbers"""
    offs = np.array([(b & 1) + (((b >> 1) & 1) << SJ) + ((b >> 2) << SL) for b in range(8)], np.int64)
    keys = act[:, None] + offs[None, :]
    lat = np.unique(keys.ravel())
    return lat, np.searchsorted(lat, keys).astype(np.int64)


def lattice_positions(lat, voxel):
    h = np.float32(voxel)
    i, j, l = unpack_key(lat)
    pos = np.stack([i.astype(np.float32) * h, j.astype(np.float32) * h, l.astype(np.float32) * h], axis=1)
    assert pos.dtype == np.float32
    return pos


def reconstruct(points, normals, voxel, k=8, support=1.5, band=1, max_vertices=1 << 24):
    """-> dict(verts [V, 3] float32, faces [F, 3] int32, f [nlat] float32, nvox, nlat)"""
    occ = occupied_voxels(points, voxel, band)
    act = dilate(occ, band)
    lat, corner = lattice(act)
    if len(lat) > max_vertices:
        raise ValueError("%d lattice vertices, more than max_vertices = %d" % (len(lat), max_vertices))
    pos = lattice_positions(lat, voxel)
    f = signed_distance(pos, points, normals, k, support)
    neg = f < np.float32(0)                                 # exact zeros are non-negative
    nvox = len(act)
    table, T = case_table(), tets()
    slots = np.full((nvox, 6, 2, 3), -1, np.int64)
    for t in range(6):
        mask = sum(neg[corner[:, T[t][i]]].astype(np.int64) << i for i in range(4))
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            if not len(sel):
                continue
            for ti, tri in enumerate(table[t][m]):
                for e, (A, d) in enumerate(tri):
                    slots[sel, t, ti, e] = 7 * corner[sel, A] + (d - 1)
    tris = slots.reshape(-1, 3)
    tris = tris[tris[:, 0] >= 0]                            # (voxel, tet, triangle) ascending
    used = np.unique(tris.ravel())                          # (lattice vertex, d) ascending
    faces = np.searchsorted(used, tris).astype(np.int32).reshape(-1, 3)
    A, d = used // 7, used % 7 + 1
    bkey = lat[A] + (d & 1) + (((d >> 1) & 1) << SJ) + ((d >> 2) << SL)
    B = np.searchsorted(lat, bkey)
    assert (lat[B] == bkey).all()
    fa, fb = f[A].astype(np.float64), f[B].astype(np.float64)
    t = fa / (fa - fb)
    pa, pb = pos[A].astype(np.float64), pos[B].astype(np.float64)
    verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
    return dict(verts=verts.reshape(-1, 3), faces=faces, f=f, nvox=nvox, nlat=len(lat))


# ---- what the tests measure on a mesh ----------------------------------------------------------------------------------------------------------

def edge_stats(faces):
    """-> dict(repeated: directed edges that occur more than once, unpaired: directed edges whose reverse does not occur exactly once,
    E: undirected edges)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(max(a.max(), b.max())) + 1 if len(a) else 1
    code, rev = a * n + b, b * n + a
    u, cnt = np.unique(code, return_counts=True)
    pos = np.searchsorted(u, rev)
    pos = np.minimum(pos, len(u) - 1) if len(u) else pos
    rcnt = np.where(u[pos] == rev, cnt[pos], 0) if len(u) else np.zeros(0, np.int64)
    return dict(repeated=int((cnt > 1).sum()), unpaired=int((rcnt != 1).sum()),
                E=int(len(np.unique(np.minimum(a, b) * n + np.maximum(a, b)))))


def euler(verts, faces):
    return len(verts) - edge_stats(faces)["E"] + len(faces)


def closed(faces):
    s = edge_stats(faces)
    return s["repeated"] == 0 and s["unpaired"] == 0


def unreferenced(verts, faces):
    return len(verts) - len(np.unique(np.asarray(faces).ravel()))


def volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ni,ni->n", a, np.cross(b, c)).sum() / 6.0)


def zero_area(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return int((np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0).sum())


# ---- the seeded cases the CPU and the GPU tests share: every oracle run happens once ------------------------------------------------------

def _up(n):
    return np.tile(np.float32([[0, 0, 1]]), (n, 1))


def _ellipsoid_normals(p):
    """analytic outward normals of normals_oracle.far_ellipsoid: the gradient of the quadric, normalised"""
    g = (p.astype(np.float64) - np.array([1000.0, -500.0, 250.0])) / (np.array([1.0, 0.6, 0.3]) * 0.01) ** 2
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def _estimated_torus():
    """normals estimated and oriented on the CPU by the existing oracles: PCA at k = 16, then the spanning-forest orientation"""
    p, _ = OO.torus(2048)
    est = NO.normals(p, 16)
    return p, OO.orient(p, est["normal"], est["idx"])["normal"]


CASES = {
    # name: (builder of (points, normals), keyword arguments of reconstruct)
    "sphere": (lambda: (NO.sphere(2048),) * 2, dict(voxel=0.1)),
    "torus": (lambda: OO.torus(2048), dict(voxel=0.1)),
    "two_spheres": (lambda: OO.two_spheres(), dict(voxel=0.15)),
    "sphere_fine_band1": (lambda: (NO.sphere(2048),) * 2, dict(voxel=0.05, band=1)),
    "sphere_fine_band2": (lambda: (NO.sphere(2048),) * 2, dict(voxel=0.05, band=2)),
    "noisy_plane": (lambda: (NO.noisy_plane(), _up(1500)), dict(voxel=0.05)),
    "lattice_plane": (lambda: (OO.lattice_plane()[0], _up(len(OO.lattice_plane()[0]))), dict(voxel=1.0)),
    "far_ellipsoid": (lambda: (NO.far_ellipsoid(), _ellipsoid_normals(NO.far_ellipsoid())), dict(voxel=1e-3)),
    "one_point": (lambda: (np.float32([[0.1, 0.2, 0.3]]), _up(1)), dict(voxel=0.25)),
    "estimated_torus": (_estimated_torus, dict(voxel=0.1)),
    "sphere513_band1": (lambda: (NO.sphere(513),) * 2, dict(voxel=0.2, band=1)),
    "sphere513_band2": (lambda: (NO.sphere(513),) * 2, dict(voxel=0.2, band=2)),
    "sphere64_band3": (lambda: (NO.sphere(64),) * 2, dict(voxel=0.2, band=3, k=4, support=2.0)),
}


@functools.lru_cache(maxsize=None)
def case_input(name):
    """-> (points float32 [n, 3], normals float32 [n, 3], keyword arguments)"""
    p, n = CASES[name][0]()
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(n, np.float32), dict(CASES[name][1])


@functools.lru_cache(maxsize=None)
def case_result(name):
    p, n, kw = case_input(name)
    return reconstruct(p, n, **kw)
