"""numpy restatement of dispu_orient_consistent_segments (include/dispu_hip.h, csrc/orient_consistent.hip) for one cloud: the yardstick of
the orientation tests.  Two programs that must agree bit for bit:

  orient()         sequential Kruskal with a union-find over the edges sorted by (bits of w, min(u, v), max(u, v)), then a walk over the
                   forest from every component's anchor;
  orient_rounds()  the synchronous parallel rounds of the kernels (propose, hook with the cycle-break, pointer jumping with composed
                   parities), then the finish from the parities to the roots.

jump_launch() / jump_model() restate the bounded pointer jump launch by launch (synchronously), for the deep chains of DEEP.

Edges, weights and signs as the header states them: dot = (nx nx' + ny ny') + nz nz' in fp32 with one rounding per operation,
w = max(0, 1 - |dot|) in fp32, s = [dot < 0]."""
import functools

import numpy as np

import normals_oracle as NO


class Edges(object):
    """the undirected union of the directed lists, unique, in ascending key order: lo < hi [m], wbits [m] uint32, s [m] uint8"""

    def __init__(self, normals, nbr):
        nrm = np.ascontiguousarray(normals, np.float32)
        nbr = np.asarray(nbr, np.int64)
        n, k = nbr.shape
        assert ((nbr >= -1) & (nbr < n)).all(), "a neighbour index outside [-1, n)"
        u = np.repeat(np.arange(n, dtype=np.int64), k)
        v = nbr.ravel()
        ok = (v >= 0) & (v != u)
        lo, hi = np.minimum(u[ok], v[ok]), np.maximum(u[ok], v[ok])
        pair = np.unique(lo * n + hi)
        lo, hi = pair // n, pair % n
        a, b = nrm[lo], nrm[hi]
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        w = np.maximum(np.float32(0), np.float32(1) - np.abs(dot))
        assert dot.dtype == np.float32 and w.dtype == np.float32
        wbits = w.view(np.uint32)
        order = np.lexsort((hi, lo, wbits))
        self.n, self.lo, self.hi, self.wbits = n, lo[order], hi[order], wbits[order]
        self.s = (dot < 0).astype(np.uint8)[order]


def kruskal(E):
    """[m] bool: the edges of the minimum spanning forest"""
    parent = list(range(E.n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree = np.zeros(len(E.lo), bool)
    for e, (a, b) in enumerate(zip(E.lo.tolist(), E.hi.tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            tree[e] = True
    return tree


def anchor(points, members):
    """the member with the largest (z, y, x) as fp32, ties to the lowest index"""
    p = np.asarray(points, np.float32)[members]
    return int(members[np.lexsort((members, -p[:, 0], -p[:, 1], -p[:, 2]))[0]])


def anchor_flip(nrm):
    """vote 0: the first non-zero of (nz, ny, nx) is negative"""
    for c in (nrm[2], nrm[1], nrm[0]):
        if c != 0:
            return int(c < 0)
    return 0


def _choose(rel_anchor, f0, rel, nonzero, vote):
    """t with flip = rel ^ t: vote 0 the anchor's rule, vote 1 the choice that flips fewer non-zero normals (ties: vote 0's)"""
    t = int(rel_anchor) ^ f0
    if vote == 1:
        mine = int(((rel ^ t) & nonzero).sum())
        other = int(((rel ^ t ^ 1) & nonzero).sum())
        if other < mine:
            t ^= 1
    return t


def _result(normals, flip, component):
    nrm = np.array(normals, np.float32)
    nrm[flip != 0] = -nrm[flip != 0]
    return dict(normal=nrm, flip=flip.astype(np.uint8), component=component.astype(np.int32), n_components=len(np.unique(component)))


def orient(points, normals, nbr, vote=0, E=None):
    """Kruskal, then a walk from every anchor -> dict(normal, flip, component, n_components, tree)"""
    nrm = np.ascontiguousarray(normals, np.float32)
    E = E or Edges(nrm, nbr)
    n = E.n
    tree = kruskal(E)
    adj = [[] for _ in range(n)]
    for a, b, s in zip(E.lo[tree].tolist(), E.hi[tree].tolist(), E.s[tree].tolist()):
        adj[a].append((b, s))
        adj[b].append((a, s))
    rel = np.full(n, -1, np.int64)                                  # parity of the forest path to the FIRST node met of the component
    component = np.zeros(n, np.int64)
    flip = np.zeros(n, np.uint8)
    nonzero = (nrm != 0).any(axis=1).astype(np.int64)
    for start in range(n):
        if rel[start] >= 0:
            continue
        rel[start] = 0
        members, stack = [start], [start]
        while stack:
            x = stack.pop()
            for y, s in adj[x]:
                if rel[y] < 0:
                    rel[y] = rel[x] ^ s
                    members.append(y)
                    stack.append(y)
        members = np.array(sorted(members), np.int64)
        a = anchor(points, members)
        t = _choose(rel[a], anchor_flip(nrm[a]), rel[members], nonzero[members], vote)
        flip[members] = rel[members] ^ t
        component[members] = members[0]
    out = _result(nrm, flip, component)
    out["tree"] = tree
    return out


JUMP_ITERS, JUMP_LAUNCHES = 64, 4                                  # kOrJumpIters, kOrJumpLaunches of csrc/orient_consistent.hip


def jump_launch(parent, par):
    """A synchronous model of ONE orient_jump_kernel launch: every thread reads the words the launch found, follows at most JUMP_ITERS
    links with the parities composed, and rewrites its own word -> (parent, par, short); short: a thread ended short of its root, the
    flag that lets the next launch work.  (The real launch rewrites in place while others read, so a thread may get further than
    here, never less far.)"""
    x = np.arange(len(parent))
    p, q = parent.copy(), par.copy()
    done = np.zeros(len(parent), bool)
    for _ in range(JUMP_ITERS):
        up = parent[p]
        done |= (p == x) | (up == p)
        act = np.nonzero(~done)[0]
        if len(act) == 0:
            break
        q[act] ^= par[p[act]]
        p[act] = up[act]
    done |= (p == x) | (parent[p] == p)
    return p, q, not done.all()


def jump_model(parent, par):
    """launches until one leaves no thread short, at most JUMP_LAUNCHES -> (parent, par, launches that worked, still short)"""
    for used in range(1, JUMP_LAUNCHES + 1):
        parent, par, short = jump_launch(parent, par)
        if not short:
            break
    return parent, par, used, short


def launches_for_depth(d):
    """what the model needs for a tree of depth d, as arithmetic: a launch leaves no thread short iff d <= JUMP_ITERS + 1, and takes d
    to ceil(d / (JUMP_ITERS + 1)) otherwise (tests/test_orient_oracle.py holds jump_launch to both on chains of up to 274628 nodes).
    Sizes beyond that, 2^24 nodes among them, are bounded by this closed form, not by a run of the model."""
    used = 1
    while d > JUMP_ITERS + 1:
        d = -(-d // (JUMP_ITERS + 1))
        used += 1
    return used


def depths(parent):
    """links from every node to its root, for a forest given by parent (roots point at themselves)"""
    p = parent.copy()
    d = (p != np.arange(len(parent))).astype(np.int64)             # links from x to p[x], doubled until p[x] is the root
    while True:
        up = p[p]
        if (up == p).all():
            return d
        d, p = d + d[p], up


def boruvka_rounds(E, launches=None):
    """the kernels' rounds, synchronous -> (root [n], parity to the root [n], chosen edges [m] bool, rounds).  launches: a list; then
    the flattening of every round is jump_model's, and the list receives (depth of the hooked forest, launches that worked) per round"""
    n, m = E.n, len(E.lo)
    lo, hi, s = E.lo, E.hi, E.s
    parent, par = np.arange(n, dtype=np.int64), np.zeros(n, np.uint8)
    chosen = np.zeros(m, bool)
    rounds = 0
    while True:
        rl, rh = parent[lo], parent[hi]
        idx = np.nonzero(rl != rh)[0]
        if len(idx) == 0:
            break
        rounds += 1
        assert rounds <= max(1, int(np.ceil(np.log2(max(n, 2))))), "more rounds than ceil(log2 n)"
        best = np.full(n, m, np.int64)                              # propose: the position in key order is the key
        np.minimum.at(best, rl[idx], idx)
        np.minimum.at(best, rh[idx], idx)
        roots = np.nonzero(best < m)[0]
        e = best[roots]
        mine = parent[lo[e]] == roots
        a, b = np.where(mine, lo[e], hi[e]), np.where(mine, hi[e], lo[e])
        rb = parent[b]
        hook = ~((best[rb] == e) & (roots < rb))                    # a mutual pair: the lower root stays
        chosen[e] = True
        new_parent, new_par = parent.copy(), par.copy()
        new_parent[roots[hook]] = rb[hook]
        new_par[roots[hook]] = par[a[hook]] ^ par[b[hook]] ^ s[e[hook]]
        parent, par = new_parent, new_par
        if launches is not None:
            depth = int(depths(parent).max())
            parent, par, used, short = jump_model(parent, par)
            assert not short, "a tree deeper than %d launches flatten" % JUMP_LAUNCHES
            launches.append((depth, used))
            continue
        for _ in range(64):                                         # pointer jumping, parities composed
            up = parent[parent]
            if (up == parent).all():
                break
            par, parent = par ^ par[parent], up
        else:
            raise AssertionError("a cycle among the hooks")
    return parent, par, chosen, rounds


def orient_rounds(points, normals, nbr, vote=0, E=None, launches=None):
    """the rounds, then the kernels' finish -> dict(normal, flip, component, n_components, tree, rounds)"""
    nrm = np.ascontiguousarray(normals, np.float32)
    E = E or Edges(nrm, nbr)
    root, rel, chosen, rounds = boruvka_rounds(E, launches)
    rel = rel.astype(np.int64)
    nonzero = (nrm != 0).any(axis=1).astype(np.int64)
    flip = np.zeros(E.n, np.uint8)
    component = np.zeros(E.n, np.int64)
    for r in np.unique(root):
        members = np.nonzero(root == r)[0]
        a = anchor(points, members)
        t = _choose(rel[a], anchor_flip(nrm[a]), rel[members], nonzero[members], vote)
        flip[members] = rel[members] ^ t
        component[members] = members[0]
    out = _result(nrm, flip, component)
    out.update(tree=chosen, rounds=rounds)
    return out


# ---- seeded inputs shared by the tests ------------------------------------------------------------------------------------------------

def random_units(n, seed):
    v = np.random.RandomState(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def torus(n, seed=0, R=1.0, r=0.35):
    """(points, analytic outward normals) of n seeded points on a torus, uniform in area (rejection on R + r cos v)"""
    rs = np.random.RandomState(seed)
    us, vs = [], []
    while sum(len(x) for x in us) < n:
        u, v, t = rs.random_sample(2 * n) * 2 * np.pi, rs.random_sample(2 * n) * 2 * np.pi, rs.random_sample(2 * n)
        keep = t * (R + r) <= R + r * np.cos(v)
        us.append(u[keep])
        vs.append(v[keep])
    u, v = np.concatenate(us)[:n], np.concatenate(vs)[:n]
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    return p.astype(np.float32), nrm


def two_spheres():
    """1500 + 700 points on unit spheres 5 apart -> (points, outward normals)"""
    a, b = NO.sphere(1500, seed=1), NO.sphere(700, seed=2)
    return np.concatenate([a, b + np.float32([5, 0, 0])]), np.concatenate([a, b]).astype(np.float64)


def lattice_plane(m=24, seed=3):
    """an m x m lattice in the plane z = 0 and its normals (0, 0, +-1) with seeded signs: every weight is exactly 0"""
    g = np.arange(m, dtype=np.float32)
    p = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((m, m), np.float32)], axis=-1).reshape(-1, 3)
    sign = np.where(np.random.RandomState(seed).random_sample(m * m) < 0.5, -1.0, 1.0).astype(np.float32)
    return np.ascontiguousarray(p, np.float32), np.stack([np.zeros_like(sign), np.zeros_like(sign), sign], axis=1)


def sheet(rows=200, cols=100, seed=4):
    """a wavy sheet of rows x cols points and the lists of its 8 lattice neighbours in seeded column order, -1 beyond the border:
    20 000 points without a quadratic search; the lists hold -1 in any column"""
    rs = np.random.RandomState(seed)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    p = np.stack([i * 0.05, j * 0.05, 0.3 * np.sin(i * 0.11) * np.cos(j * 0.07)], axis=-1).reshape(-1, 3)
    p += rs.standard_normal(p.shape) * 0.005
    nbr = np.full((rows * cols, 8), -1, np.int32)
    steps = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    for c, (di, dj) in enumerate(steps):
        ii, jj = i + di, j + dj
        ok = (ii >= 0) & (ii < rows) & (jj >= 0) & (jj < cols)
        nbr[:, c] = np.where(ok, ii * cols + jj, -1).reshape(-1)
    perm = np.argsort(rs.random_sample(nbr.shape), axis=1)
    return p.astype(np.float32), np.take_along_axis(nbr, perm, axis=1)


def chain_lists(n, rs):
    """[n, 4] int32: {i - 1, i + 1, -1, -1} in seeded column order, -1 beyond either end"""
    i = np.arange(n, dtype=np.int32)
    nbr = np.stack([i - 1, np.where(i + 1 < n, i + 1, -1), np.full(n, -1, np.int32), np.full(n, -1, np.int32)], axis=1).astype(np.int32)
    return np.take_along_axis(nbr, np.argsort(rs.random_sample(nbr.shape), axis=1), axis=1)


def path(n, seed=19):
    """n points on a line, normals (0, 0, +-1) with seeded signs: every weight is exactly 0, so (min, max) alone orders the edges and
    every node's lightest edge is the one to its LOWER neighbour.  Round one hooks every node but 0 to its lower neighbour (0 and 1
    choose the same edge: the lower root stays): one chain of depth n - 1, node i being i links from the root 0."""
    rs = np.random.RandomState(seed)
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = np.arange(n, dtype=np.float32) * np.float32(0.25)
    sign = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0).astype(np.float32)
    nrm = np.stack([np.zeros_like(sign), np.zeros_like(sign), sign], axis=1)
    return p, nrm, chain_lists(n, rs)


def rising(n, seed=20):
    """the same line with normals that turn in the xy-plane by increments falling from 1.2 to 0.3 rad, signs seeded: the weight
    1 - |cos| falls along the line, so every node's lightest edge is the one to its HIGHER neighbour and the chain hooks upwards
    (n - 1 and n - 2 choose the same edge: n - 2 stays, the root)"""
    rs = np.random.RandomState(seed)
    p = path(n)[0]
    theta = np.concatenate([[0.0], np.cumsum(np.linspace(1.2, 0.3, n - 1))])
    sign = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0)
    nrm = (np.stack([np.cos(theta), np.sin(theta), np.zeros(n)], axis=1) * sign[:, None]).astype(np.float32)
    return p, nrm, chain_lists(n, rs)


# the deep hook trees: 1, 2, 2, 3 and 4 launches of the pointer jump in the model (tests/test_orient_oracle.py: a launch flattens depth
# 65, so 66 points are the last that need one launch), and a chain that hooks upwards
DEEP = ("path_66", "path_67", "path_68", "path_4228", "path_274628", "rising_4300")

# name -> (points, input normals, neighbour lists): the cases of tests/test_orient_gpu.py, which tests/test_orient_oracle.py runs
# through both programs.  Input normals are seeded random unit vectors unless the case says otherwise.
SMALL_N, SMALL_K = (1, 2, 3, 5, 63, 64, 65, 257), (4, 16, 32)
CASES = (["small_n%d_k%d" % (n, k) for n in SMALL_N for k in SMALL_K]
         + ["lattice_plane", "coincident", "zero_normals", "clusters", "helix", "sheet"])


@functools.lru_cache(maxsize=None)
def case(name):
    rs = np.random.RandomState(11)
    if name.startswith("small_"):
        n, k = (int(t[1:]) for t in name.split("_")[1:])
        p = rs.random_sample((257, 3)).astype(np.float32)[:n]
        return p, random_units(n, 12), NO.neighbors(p, k)
    if name == "lattice_plane":
        p, nrm = lattice_plane()
        return p, nrm, NO.neighbors(p, 9)
    if name == "coincident":                                        # 300 equal points among 300 random ones
        p = rs.random_sample((600, 3)).astype(np.float32)
        p[rs.permutation(600)[:300]] = np.float32([0.25, 0.5, 0.75])
        return p, random_units(600, 13), NO.neighbors(p, 16)
    if name == "zero_normals":                                      # one in ten has no normal
        p = NO.sphere(1000, seed=14)
        nrm = random_units(1000, 15)
        nrm[rs.permutation(1000)[:100]] = 0
        return p, nrm, NO.neighbors(p, 8)
    if name == "clusters":                                          # 40 clusters of 30 points, 10 apart: 40 components at k = 8
        centre = np.stack(np.meshgrid(np.arange(4), np.arange(5), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3) * 10.0
        p = (np.repeat(centre, 30, axis=0) + rs.random_sample((1200, 3))).astype(np.float32)
        p = p[rs.permutation(1200)]
        return p, random_units(1200, 16), NO.neighbors(p, 8)
    if name == "helix":                                             # nearly a path at k = 4: the deepest trees
        t = np.arange(4096) * 0.05
        p = np.stack([np.cos(t), np.sin(t), 0.02 * t], axis=1).astype(np.float32)
        return p, random_units(4096, 17), NO.neighbors(p, 4)
    if name == "sheet":
        p, nbr = sheet()
        return p, random_units(len(p), 18), nbr
    if name.startswith("path_"):
        return path(int(name[5:]))
    if name.startswith("rising_"):
        return rising(int(name[7:]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, vote=0):
    """the Kruskal result of a case, computed once"""
    p, nrm, nbr = case(name)
    return orient(p, nrm, nbr, vote)
