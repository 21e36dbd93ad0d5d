"""Float64 CPU oracle of exact geodesic distances on a triangle mesh, for the tests of csrc/geodesic.hip only.

Written from the papers, independently of the kernel and of dis-pu_amd/mesh.py (its own adjacency, its own frames, its own
pruning order): Chen & Han's continuous-Dijkstra window propagation in the sequential, priority-queue form of Xin & Wang,
"Improving Chen and Han's algorithm on the discrete geodesic problem" (ACM TOG 28(4), 2009).

  * A window is an interval of an edge lit by straight lines from one (unfolded) source image I at geodesic distance sigma.
    Windows are popped in ascending order of their lower bound sigma + dist(I, interval) and propagated across the face they
    light; a window whose lower bound exceeds max_dist is never propagated.
  * Vertices keep the best known path length.  A saddle (angle sum >= 2 pi) or boundary vertex becomes a pseudo-source when it
    is settled, and emits windows onto the edges opposite it in its fan.
  * Xin-Wang's filter drops a new window on edge (P, Q) when the known distance of P (or Q) plus the distance along the edge beats
    the window at the window's far (near) end: then it beats the window everywhere along it, and no shortest path uses it.
  * A target t in face f: the least of |s - t| (f holds the seed), d(v) + |v - t| over f's vertices, and over the windows that
    light f: sigma + |I - t| where t is seen through the window, else the path over the nearer window end.  Every candidate is the
    length of a real surface path, so nothing undercuts the geodesic.

geodesic(verts, faces, seed_face, seed_bary, targets, target_faces, max_dist) -> fp64 [n]; +inf beyond max_dist.
"""
import heapq
import math

import numpy as np

_TOL = 1e-12


class Surface(object):
    def __init__(self, verts, faces):
        self.V = np.asarray(verts, np.float64).reshape(-1, 3)
        self.F = np.asarray(faces, np.int64).reshape(-1, 3)
        nv, nf = self.V.shape[0], self.F.shape[0]
        edges = {}
        for f in range(nf):
            for k in range(3):
                a, b = int(self.F[f, k]), int(self.F[f, (k + 1) % 3])
                edges.setdefault((min(a, b), max(a, b)), []).append((f, k))
        self.opp = {}
        self.bnd = np.zeros(nv, bool)
        for (a, b), lst in edges.items():
            if len(lst) > 2:
                raise ValueError("non-manifold edge (%d, %d)" % (a, b))
            if len(lst) == 2:
                self.opp[lst[0]] = lst[1]
                self.opp[lst[1]] = lst[0]
            else:
                self.bnd[a] = self.bnd[b] = True
        self.fan = [[] for _ in range(nv)]
        self.angle = np.zeros(nv)
        for f in range(nf):
            for j in range(3):
                v = int(self.F[f, j])
                self.fan[v].append((f, j))
                p, q, r = self.V[v], self.V[self.F[f, (j + 1) % 3]], self.V[self.F[f, (j + 2) % 3]]
                self.angle[v] += math.atan2(np.linalg.norm(np.cross(q - p, r - p)), np.dot(q - p, r - p))
        self.pseudo = (self.angle >= 2 * math.pi) | self.bnd

    def frame(self, f, k):
        """edge k of face f in 2D: f[k] at (0,0), f[k+1] at (L,0), f[k+2] at (cx, cy>0); returns origin, x axis, y axis, L, c"""
        a, b, c = (self.V[self.F[f, (k + i) % 3]] for i in range(3))
        L = np.linalg.norm(b - a)
        ex = (b - a) / L
        cx = np.dot(c - a, ex)
        ey = c - a - cx * ex
        cy = np.linalg.norm(ey)
        return a, ex, ey / cy, L, (cx, cy)

    def to2d(self, f, k, p):
        a, ex, ey, _, _ = self.frame(f, k)
        d = np.asarray(p, np.float64) - a
        return float(np.dot(d, ex)), float(np.dot(d, ey))


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


class _Run(object):
    def __init__(self, S, max_dist):
        self.S, self.max_dist = S, max_dist
        self.d = {}            # vertex -> best known path length
        self.lit = {}          # face -> windows (sigma, ix, iy, b0, b1, k)
        self.heap = []
        self.tick = 0

    def push(self, key, item):
        heapq.heappush(self.heap, (key, self.tick, item))
        self.tick += 1

    def relax(self, v, dist):
        if dist < self.d.get(v, math.inf):
            self.d[v] = dist
            if self.S.pseudo[v] and dist <= self.max_dist:
                self.push(dist, ("vertex", v, dist))

    def window(self, f, k, sigma, ix, iy, b0, b1):
        """a window on edge k of face f lighting the face g across it; source (ix, iy > 0) and [b0, b1] in f's frame of edge k.
        Stored in g's frame of its edge, where g is at +y and the source below."""
        o = self.S.opp.get((f, k))
        if o is None:
            return
        g, kk = o
        L = self.S.frame(f, k)[3]
        # the twin edge runs the other way (or, on a badly oriented mesh, the same way)
        same = int(self.S.F[g, kk]) == int(self.S.F[f, k])
        if same:
            jx, jy, c0, c1 = ix, -iy, b0, b1
        else:
            jx, jy, c0, c1 = L - ix, -iy, L - b1, L - b0
        c0, c1 = max(c0, 0.0), min(c1, L)
        if not (c1 - c0 > _TOL * L) or not (jy < -_TOL * L):
            return
        lb = sigma + math.hypot(min(max(jx, c0), c1) - jx, jy)
        if lb > self.max_dist:
            return
        if self.pruned(g, kk, sigma, jx, jy, c0, c1, L):
            return
        self.push(lb, ("window", g, kk, sigma, jx, jy, c0, c1))

    def pruned(self, g, k, sigma, ix, iy, c0, c1, L):
        P, Q = int(self.S.F[g, k]), int(self.S.F[g, (k + 1) % 3])
        far = sigma + math.hypot(c1 - ix, iy)
        near = sigma + math.hypot(c0 - ix, iy)
        if self.d.get(P, math.inf) + c1 < far * (1 - _TOL):
            return True
        if self.d.get(Q, math.inf) + (L - c0) < near * (1 - _TOL):
            return True
        return False

    def _emit(self, f, k, sigma, x, y, L):
        """source at (x, y > 0) in f's frame of edge k: a full-edge window lighting the face across"""
        if y > _TOL * L:
            self.window(f, k, sigma, x, y, 0.0, L)

    def propagate(self, f, k, sigma, ix, iy, b0, b1):
        """window on edge k of face f lighting f; (ix, iy < 0) in f's frame of edge k"""
        S = self.S
        self.lit.setdefault(f, []).append((sigma, ix, iy, b0, b1, k))
        _, _, _, L, (cx, cy) = S.frame(f, k)
        va, vb, vc = (int(S.F[f, (k + i) % 3]) for i in range(3))
        xc = ix + (cx - ix) * (-iy) / (cy - iy)
        if b0 < xc < b1:
            self.relax(vc, sigma + math.hypot(cx - ix, cy - iy))
        if b0 <= _TOL * L:
            self.relax(va, sigma + math.hypot(ix, iy))
        if b1 >= L * (1 - _TOL):
            self.relax(vb, sigma + math.hypot(L - ix, iy))
        A, B, C = (0.0, 0.0), (L, 0.0), (cx, cy)
        if b0 < xc:   # through [b0, min(b1, xc)] onto edge k+2 (c -> a)
            self._child(f, (k + 2) % 3, C, A, B, sigma, ix, iy, b0, min(b1, xc))
        if xc < b1:   # through [max(b0, xc), b1] onto edge k+1 (b -> c)
            self._child(f, (k + 1) % 3, B, C, A, sigma, ix, iy, max(b0, xc), b1)

    def _child(self, f, kk, P, Q, R, sigma, ix, iy, x0, x1):
        """rays from I through (x0,0), (x1,0) onto edge kk = P -> Q of f; re-express in edge kk's own frame (P origin, R at +y)"""
        ex, ey = Q[0] - P[0], Q[1] - P[1]
        Lpq = math.hypot(ex, ey)
        ux, uy = ex / Lpq, ey / Lpq
        sg = 1.0 if _cross(ux, uy, R[0] - P[0], R[1] - P[1]) > 0 else -1.0

        def hit(x):
            dx, dy = x - ix, -iy
            den = _cross(ex, ey, dx, dy)
            if abs(den) <= 1e-300:
                return None
            s = _cross(ix - P[0], iy - P[1], dx, dy) / den
            return min(max(s, 0.0), 1.0) * Lpq

        h0, h1 = hit(x0), hit(x1)
        if h0 is None or h1 is None:
            return
        jx = (ix - P[0]) * ux + (iy - P[1]) * uy
        jy = sg * _cross(ux, uy, ix - P[0], iy - P[1])
        lo, hi = min(h0, h1), max(h0, h1)
        # in f's frame of edge kk the source lies on f's side (+y); the child lights the face across
        self.window(f, kk, sigma, jx, jy, lo, hi)

    def vertex_source(self, v, dist):
        S = self.S
        for f, j in S.fan[v]:
            k = (j + 1) % 3                       # the edge opposite v
            _, _, _, L, (cx, cy) = S.frame(f, k)
            self._emit(f, k, dist, cx, cy, L)
            for i in (1, 2):
                w = int(S.F[f, (j + i) % 3])
                self.relax(w, dist + float(np.linalg.norm(S.V[w] - S.V[v])))

    def run(self):
        settled = {}
        while self.heap:
            key, _, item = heapq.heappop(self.heap)
            if key > self.max_dist:
                break
            if item[0] == "vertex":
                _, v, dist = item
                if self.d[v] != dist or settled.get(v, math.inf) <= dist:
                    continue
                settled[v] = dist
                self.vertex_source(v, dist)
            else:
                _, g, k, sigma, ix, iy, b0, b1 = item
                L = self.S.frame(g, k)[3]
                if self.pruned(g, k, sigma, ix, iy, b0, b1, L):       # the filter again, with what is known by now
                    continue
                self.propagate(g, k, sigma, ix, iy, b0, b1)


def geodesic(verts, faces, seed_face, seed_bary, targets, target_faces, max_dist, surface=None):
    S = surface if surface is not None else Surface(verts, faces)
    bary = np.asarray(seed_bary, np.float64).reshape(3)
    fs = int(seed_face)
    s = bary @ S.V[S.F[fs]]
    run = _Run(S, float(max_dist))
    zeros = [j for j in range(3) if bary[j] == 0.0]
    src_faces = {fs}
    if len(zeros) >= 2:                               # a vertex seed: a pseudo-source at distance 0
        v = int(S.F[fs, [j for j in range(3) if j not in zeros][0]])
        run.d[v] = 0.0
        run.vertex_source(v, 0.0)
        src_faces = {f for f, _ in S.fan[v]}
    else:
        for f in ([fs] + ([S.opp[(fs, (zeros[0] + 1) % 3)][0]] if zeros and (fs, (zeros[0] + 1) % 3) in S.opp else [])):
            src_faces.add(f)
            for j in range(3):
                w = int(S.F[f, j])
                run.relax(w, float(np.linalg.norm(S.V[w] - s)))
            for k in range(3):
                x, y = S.to2d(f, k, s)
                run._emit(f, k, 0.0, x, y, S.frame(f, k)[3])
    run.run()
    T = np.asarray(targets, np.float64).reshape(-1, 3)
    tf = np.asarray(target_faces, np.int64).reshape(-1)
    out = np.full(T.shape[0], math.inf)
    for q in range(T.shape[0]):
        t, f = T[q], int(tf[q])
        best = math.inf
        if f in src_faces:
            best = float(np.linalg.norm(t - s))
        for j in range(3):
            v = int(S.F[f, j])
            if v in run.d:
                best = min(best, run.d[v] + float(np.linalg.norm(S.V[v] - t)))
        for sigma, ix, iy, b0, b1, k in run.lit.get(f, []):
            tx, ty = S.to2d(f, k, t)
            x = ix + (tx - ix) * (-iy) / (ty - iy) if ty - iy > 0 else math.nan
            if b0 <= x <= b1:
                best = min(best, sigma + math.hypot(tx - ix, ty - iy))
            else:
                best = min(best, sigma + math.hypot(b0 - ix, iy) + math.hypot(tx - b0, ty),
                           sigma + math.hypot(b1 - ix, iy) + math.hypot(tx - b1, ty))
        out[q] = best if best <= max_dist else math.inf
    return out
