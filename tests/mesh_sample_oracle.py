"""Host restatements of the mesh sampler (dis-pu_amd/csrc/mesh_sample.hip, poisson_disk.hip), written from the semantics stated in
include/dispu_hip.h -- independent of the kernel sources.  numpy only.

  sample_surface   Philox draw -> face by binary search over the cumulative areas -> sqrt barycentrics -> fp64 point, fp32 once
  conflicts        per point the lower-index points closer than a radius (fp32 plain-order d2), by brute force inside x windows
  greedy_keep      the SEQUENTIAL greedy dart throwing the kernels must reproduce: a plain loop in index order
  poisson_select   the fp32 bisection around it, and the first m kept indices
  rounds_keep      the parallel-rounds formulation in numpy (what the kernel does), checked against greedy_keep on the CPU
"""
import numpy as np

from sampler_oracle import philox4x32_10

STREAM_SURFACE = 0xD15C5A3D


# ------------------------------------------------------------------------------------------------------------------ surface samples --
def sample_surface(verts, faces, cum, count, seed=0):
    """-> (points [count,3] f32, face [count] i32, bary [count,3] f64)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    fc = np.asarray(faces, np.int64)
    cum = np.asarray(cum, np.float64)
    F = fc.shape[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    w = np.array([philox4x32_10((i & 0xFFFFFFFF, i >> 32, 0, STREAM_SURFACE), key) for i in range(count)], np.uint64).reshape(count, 4)
    u = ((w[:, 0] << np.uint64(21)) | (w[:, 1] >> np.uint64(11))).astype(np.float64) * 2.0 ** -53       # < 2^53: exact
    face = np.clip(np.searchsorted(cum[:F], u, side="right") - 1, 0, F - 1)                              # largest f < F with cum[f] <= u
    r1 = (w[:, 2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r2 = (w[:, 3] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    s = np.sqrt(r1)
    b0 = 1.0 - s
    b1 = s * (1.0 - r2)
    b2 = s * r2
    tv = v[fc[face]]                                                                                     # [count, 3 corners, 3]
    t0 = b0[:, None] * tv[:, 0]
    t1 = b1[:, None] * tv[:, 1]
    t2 = b2[:, None] * tv[:, 2]
    p = (t0 + t1) + t2
    return p.astype(np.float32), face.astype(np.int32), np.stack([b0, b1, b2], axis=1)


# ------------------------------------------------------------------------------------------------------------------ dart throwing ----
def _d2_plain(a, b):
    """fp32 (dx dx + dy dy) + dz dz of a [c,1,3] against b [1,n,3]"""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def conflicts(points, r_max, budget=1 << 22):
    """points [n,3] f32 -> (nbr, d2): per point i a python list of the j < i with d2(i, j) < fl32(r_max r_max), ascending j, and the
    matching list of those fp32 d2.  Brute force over all pairs whose x coordinates differ by at most r_max (a superset: fl(dx dx) >=
    fl(r r) once |dx| >= r, and the later sums only add), in chunks of rows of the x-sorted cloud."""
    p = np.ascontiguousarray(points, np.float32)
    n = p.shape[0]
    r = np.float32(r_max)
    nbr, dd = [[] for _ in range(n)], [[] for _ in range(n)]
    if not r > 0:
        return nbr, dd
    r2 = np.float32(r * r)
    order = np.argsort(p[:, 0], kind="stable")
    q = p[order]
    x = q[:, 0].astype(np.float64)
    I, J, D = [], [], []
    a = 0
    while a < n:
        lo = int(np.searchsorted(x, x[a] - float(r), side="left"))
        e = a + 1
        hi = int(np.searchsorted(x, x[e - 1] + float(r), side="right"))
        while e < n and (e + 1 - a) * (int(np.searchsorted(x, x[e] + float(r), side="right")) - lo) <= budget:
            e += 1
            hi = int(np.searchsorted(x, x[e - 1] + float(r), side="right"))
        d2 = _d2_plain(q[a:e, None, :], q[None, lo:hi, :])
        ii, jj = np.nonzero(d2 < r2)
        oi, oj = order[ii + a], order[jj + lo]
        ok = oj < oi
        I.append(oi[ok]); J.append(oj[ok]); D.append(d2[ii, jj][ok])
        a = e
    I, J, D = np.concatenate(I), np.concatenate(J), np.concatenate(D)
    srt = np.lexsort((J, I))
    I, J, D = I[srt], J[srt], D[srt]
    cuts = np.searchsorted(I, np.arange(n + 1))
    jl, vl = J.tolist(), D.tolist()
    for i in range(n):
        if cuts[i + 1] > cuts[i]:
            nbr[i] = jl[cuts[i]:cuts[i + 1]]
            dd[i] = vl[cuts[i]:cuts[i + 1]]
    return nbr, dd


def greedy_keep(n, nbr, dd, r):
    """The sequential algorithm: keep[i] iff no kept j < i with d2 < fl32(r r) (strict); r <= 0 keeps everything.  (nbr, dd) from
    conflicts() at any r_max >= r.  -> bool [n]"""
    r = np.float32(r)
    keep = [True] * n
    if not r > 0:
        return np.array(keep, bool)
    r2 = float(np.float32(r * r))                                                                        # fp32 product, compared exactly
    for i in range(n):
        for j, d in zip(nbr[i], dd[i]):
            if d < r2 and keep[j]:
                keep[i] = False
                break
    return np.array(keep, bool)


def poisson_keep(points, r):
    p = np.asarray(points, np.float32)
    nbr, dd = conflicts(p, r)
    return greedy_keep(p.shape[0], nbr, dd, r)


def lattice_with_close_pairs(side, extra, seed=0):
    """A cloud whose greedy answer follows from how it is built, at any size: the side^3 lattice of spacing 1 plus `extra` planted
    points, each beside a lattice point of its own -- every other one an exact duplicate, the rest 0.3 away along +x, +y or +z (seeded)
    -- all in seeded index order.  At a radius well inside (0.3, 0.7) the only conflicts are the `extra` isolated pairs (a planted
    point is at least 0.7 from every point but its host), so the later index of each pair is rejected and everything else is kept.
    -> (points f32 [side^3 + extra, 3], keep bool).  tests/test_second_trips.py confirms the rule against poisson_keep at about 5000
    points."""
    rs = np.random.RandomState(seed)
    g = np.arange(side, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    host = rs.permutation(side ** 3)[:extra]
    shift = np.zeros((extra, 3), np.float32)
    near = np.arange(extra) % 2 == 1
    shift[np.nonzero(near)[0], rs.randint(0, 3, int(near.sum()))] = np.float32(0.3)
    pts = np.concatenate([lattice, lattice[host] + shift]).astype(np.float32)
    n = len(pts)
    perm = rs.permutation(n)                                                        # position j holds point perm[j]
    pos = np.empty(n, np.int64)
    pos[perm] = np.arange(n)
    keep = np.ones(n, bool)
    keep[np.maximum(pos[host], pos[side ** 3 + np.arange(extra)])] = False
    return np.ascontiguousarray(pts[perm]), keep


def poisson_select(points, m, r_hi, steps=12):
    """-> (idx [m] i32, r f32, count): lo = 0, hi = r_hi; steps times mid = 0.5f (lo + hi), count(mid) >= m ? lo = mid : hi = mid in
    fp32; the first m kept indices at lo."""
    p = np.asarray(points, np.float32)
    n = p.shape[0]
    nbr, dd = conflicts(p, r_hi)
    lo, hi = np.float32(0.0), np.float32(r_hi)
    for _ in range(steps):
        mid = np.float32(np.float32(0.5) * np.float32(lo + hi))
        if int(greedy_keep(n, nbr, dd, mid).sum()) >= m:
            lo = mid
        else:
            hi = mid
    keep = greedy_keep(n, nbr, dd, lo)
    return np.nonzero(keep)[0][:m].astype(np.int32), lo, int(keep.sum())


def rounds_keep(points, r, max_rounds=1 << 20):
    """The parallel formulation: all points ACTIVE; per round, from a snapshot of the states, an active point with a KEPT conflicting
    lower neighbour becomes REJECTED, one whose conflicting lower neighbours are all REJECTED becomes KEPT.  -> (keep bool [n], rounds)"""
    p = np.asarray(points, np.float32)
    n = p.shape[0]
    r = np.float32(r)
    if not r > 0:
        return np.ones(n, bool), 0
    d2 = _d2_plain(p[:, None, :], p[None, :, :])
    conf = (d2 < np.float32(r * r)) & (np.arange(n)[None, :] < np.arange(n)[:, None])                   # conf[i, j]: j < i conflicts
    ACTIVE, KEPT, REJECTED = 0, 1, 2
    st = np.zeros(n, np.int8)
    for rounds in range(1, max_rounds + 1):
        has_kept = (conf & (st == KEPT)[None, :]).any(axis=1)
        all_rej = ~(conf & (st != REJECTED)[None, :]).any(axis=1)
        act = st == ACTIVE
        new = st.copy()
        new[act & has_kept] = REJECTED
        new[act & ~has_kept & all_rej] = KEPT
        st = new
        if not (st == ACTIVE).any():
            return st == KEPT, rounds
    raise RuntimeError("no fixed point in %d rounds" % max_rounds)


# ------------------------------------------------------------------------------------------------------------------ statistics -------
def nn_distances(points):
    """distance of every point to its nearest other point (float64), brute force"""
    p = np.asarray(points, np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(d2.min(axis=1))


def nn_cv(points):
    d = nn_distances(points)
    return float(d.std() / d.mean())


def min_pair_d2_f32(points):
    """the smallest fp32 plain-order d2 over all pairs"""
    p = np.ascontiguousarray(points, np.float32)
    d2 = _d2_plain(p[:, None, :], p[None, :, :])
    np.fill_diagonal(d2, np.inf)
    return np.float32(d2.min())
