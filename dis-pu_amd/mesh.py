"""Mesh metrics of the evaluator: point-to-surface distance (P2F) and disk uniformity.

Counterpart of the reference's CGAL tool evaluation_code/evaluation.cpp (P2F by an AABB tree, seeds on the surface, disk
membership, `<pred>_point2mesh_distance.txt` / `_radius.txt` / `_disk_idx.txt`) and of the sklearn post-processing in
evaluate.py:53-101 (analyze_uniform).  The geometry runs in csrc/mesh_eval.hip; this module loads meshes, builds the face
tiles once per mesh, draws seeds on the host and reads / writes the CGAL tool's files.

Disk membership has two modes (mesh_metrics(disks=...), evaluate_pair / evaluate_dirs, tools/evaluate.py --disks):
  * "euclidean" (the default): q is in disk (i, j) iff the straight-line distance between seed i and the projected point q is at
    most r_j (disk_members, fp32).  That is CGAL's own pre-filter (evaluation.cpp:95) and a lower bound of the geodesic: on smooth
    parts at these radii the two agree to about 0.1 % (sphere of radius 0.88, r = 0.157: chord / arc = 0.9987); across creases and
    thin features a Euclidean disk can hold extra points;
  * "geodesic": CGAL's membership (Surface_mesh_shortest_path, evaluation.cpp:85-115): the points that pass the straight-line
    pre-filter at max(radii) are kept iff their exact fp64 geodesic distance on the polyhedral surface from the seed's face location
    is at most (double)r_j (geodesic_disk_members, csrc/geodesic.hip: Chen-Han / Xin-Wang window propagation, one workgroup per
    seed).  The `_disk_idx.txt` written in this mode is the one the CGAL tool writes for the same seeds.  It needs an
    edge-manifold mesh (ValueError otherwise); its tables are built on first use (Mesh.geodesic_tables).
Where CGAL outputs exist, evaluate.evaluate_dirs(use_cgal_files=True) reads them instead.

Semantics that differ from the CGAL tool, on purpose:
  * seeds come from a NumPy generator: CGAL::Random's stream cannot be reproduced, so seeded results match each other, not the
    CGAL tool's, and uniformity is a statistic over a different random set of 1000 disks;
  * the nearest other disk member replaces sklearn's 2-NN (`dis[:, 1]`): the same value, 0 for duplicated points as in sklearn.
"""
import os

import numpy as np
import torch

from . import _lib
from ._util import f32, i32, req

DEFAULT_PERCENTAGES = (0.008, 0.012)     # evaluation.cpp:259, evaluate.py:46


# ------------------------------------------------------------------------------------------------------------- OFF files ----
def load_off(path):
    """OFF file -> (verts [V,3] float32, faces [F,3] int32).  Counts may follow `OFF` on the same line or the next; blank lines
    and `#` comments are skipped; a trailing edge count is accepted.  Faces other than triangles raise ValueError (the CGAL
    tool's AABB triangle primitive cannot take them either)."""
    with open(path) as f:
        toks = []
        for line in f:
            line = line.split("#", 1)[0].strip()
            if line:
                toks.append(line)
    req(len(toks) > 0 and toks[0].split()[0].upper().endswith("OFF"), "%s: not an OFF file (no OFF header)" % path)
    head = toks[0].split()[1:]
    rest = toks[1:]
    if not head:
        req(len(rest) > 0, "%s: missing the vertex / face counts" % path)
        head, rest = rest[0].split(), rest[1:]
    req(len(head) >= 2, "%s: malformed counts line %r" % (path, " ".join(head)))
    try:
        nv, nf = int(head[0]), int(head[1])
    except ValueError:
        raise ValueError("%s: malformed counts line %r" % (path, " ".join(head)))
    req(nv >= 0 and nf >= 0 and len(rest) >= nv + nf, "%s: expected %d vertex and %d face lines, found %d lines"
        % (path, nv, nf, len(rest)))
    try:
        verts = np.array([[float(x) for x in rest[i].split()[:3]] for i in range(nv)], dtype=np.float64).reshape(nv, 3)
    except ValueError:
        raise ValueError("%s: malformed vertex line" % path)
    faces = np.empty((nf, 3), np.int64)
    for k in range(nf):
        vals = rest[nv + k].split()
        try:
            cnt = int(vals[0])
            idx = [int(v) for v in vals[1:1 + cnt]]
        except (ValueError, IndexError):
            raise ValueError("%s: malformed face line %d" % (path, k))
        req(cnt == 3, "%s: face %d has %d vertices; only triangle meshes are supported" % (path, k, cnt))
        req(len(idx) == 3, "%s: face %d lists fewer than 3 vertex indices" % (path, k))
        faces[k] = idx
    req(nf == 0 or (faces.min() >= 0 and faces.max() < nv), "%s: face vertex index out of range" % path)
    return verts.astype(np.float32), faces.astype(np.int32)


def save_off(path, verts, faces):
    """(verts [V,3] float32, faces [F,3] int32) as arrays or tensors -> an OFF file that load_off reads back to the same arrays:
    every coordinate with the 9 significant digits that name one float32."""
    v = np.ascontiguousarray(verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else verts, dtype=np.float32)
    f = np.ascontiguousarray(faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else faces)
    req(v.ndim == 2 and v.shape[1] == 3, "verts: expected a [V, 3] array, got shape %s" % (v.shape,))
    req(f.ndim == 2 and f.shape[1] == 3 and np.issubdtype(f.dtype, np.integer), "faces: expected an integer [F, 3] array, got %s %s" % (f.dtype, f.shape))
    req(len(f) == 0 or (f.min() >= 0 and f.max() < len(v)), "faces: vertex index out of range")
    with open(path, "w") as out:
        out.write("OFF\n%d %d 0\n" % (len(v), len(f)))
        out.writelines("%.9g %.9g %.9g\n" % (float(r[0]), float(r[1]), float(r[2])) for r in v)
        out.writelines("3 %d %d %d\n" % (int(r[0]), int(r[1]), int(r[2])) for r in f)


def _morton3(q):
    """interleave the low 10 bits of three non-negative ints -> 30-bit Morton code"""
    def spread(v):
        v = v.astype(np.uint64) & 0x3FF
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    return spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)


def face_tiles(verts, faces):
    """Host side of the face layout of dispu_point_to_mesh: faces sorted by the 30-bit Morton code of their centroids inside the
    mesh's bounding box (stable), -> (tris [F,12] f32 = v0.xyz 0 v1.xyz 0 v2.xyz 0 in that order, order [F] i32 = the original
    face index of each entry, box [T,8] f32 = min.xyz 0 max.xyz 0 over the vertices of each tile of 64 consecutive entries)."""
    v = np.asarray(verts, np.float32)
    fc = np.asarray(faces, np.int64)
    F = fc.shape[0]
    tv = v[fc].astype(np.float64)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    q = np.clip(((tv.mean(axis=1) - lo) / np.maximum(hi - lo, 1e-30) * 1023.0).astype(np.int64), 0, 1023)
    order = np.argsort(_morton3(q), kind="stable")
    T = (F + _lib.MESH_TILE - 1) // _lib.MESH_TILE
    tris = np.zeros((F, 3, 4), np.float32)
    tris[:, :, :3] = v[fc[order]]
    tv32 = tris[:, :, :3].reshape(F, 9)
    tv32 = np.concatenate([tv32, np.repeat(tv32[-1:], T * _lib.MESH_TILE - F, axis=0)], axis=0).reshape(T, _lib.MESH_TILE * 3, 3)
    box = np.zeros((T, 2, 4), np.float32)
    box[:, 0, :3] = tv32.min(axis=1)
    box[:, 1, :3] = tv32.max(axis=1)
    return tris.reshape(F, 12), order.astype(np.int32), box.reshape(T, 8)


def geodesic_tables(verts, faces):
    """Host tables of the exact geodesic disks (csrc/geodesic.hip), all fp64 geometry:
      verts64 [V,3] f64; faces [F,3] i32;
      twin [F,3] i32: for edge k of face f (f[k] -> f[k+1]) the half-edge g*3 + k' of the other face on that edge, -1 on a boundary;
      edge_geo [F,3,3] f64: (L, cx, cy) of edge k: its length and the opposite vertex f[k+2] in the frame with f[k] at the origin
        and f[k+1] at (L, 0), cy > 0;
      angle_sum [V] f64, boundary [V] bool, pseudo [V] i32: 1 where a shortest path may turn (angle sum >= 2 pi, or a boundary
        vertex: the pseudo-sources of Chen & Han / Xin & Wang);
      fan_off [V+1] i64, fan [3F] i32: per vertex, the corners f*3 + j (faces[f, j] == v) of the faces around it, ascending.
    Twins come from sorting the undirected edge keys; an edge shared by more than two faces raises ValueError (CGAL's Surface_mesh
    cannot hold such a mesh either), and so does a degenerate (zero-area) face."""
    v = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    F, V = fc.shape[0], v.shape[0]
    a, b = fc, np.roll(fc, -1, axis=1)                               # edge k: f[k] -> f[k+1]
    key = (np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.concatenate([[True], ks[1:] != ks[:-1]])
    gid = np.cumsum(start) - 1
    cnt = np.bincount(gid)
    if cnt.size and cnt.max() > 2:
        e = int(ks[np.argmax(start & (cnt[gid] > 2))])
        raise ValueError("non-manifold mesh: edge (%d, %d) is shared by %d faces; geodesic disks need an edge-manifold mesh"
                         % (e // V, e % V, int(cnt.max())))
    twin = np.full(3 * F, -1, np.int64)
    pair = np.nonzero(start[:-1] & ~start[1:])[0] if ks.size > 1 else np.zeros(0, np.int64)
    twin[order[pair]] = order[pair + 1]
    twin[order[pair + 1]] = order[pair]
    twin = twin.reshape(F, 3)
    p0, p1, p2 = v[a], v[b], v[np.roll(fc, -2, axis=1)]             # [F,3,3]: f[k], f[k+1], f[k+2] per edge k
    e = p1 - p0
    L = np.linalg.norm(e, axis=2)
    cr = np.linalg.norm(np.cross(e, p2 - p0), axis=2)
    if np.any(L <= 0) or np.any(cr <= 0):
        raise ValueError("degenerate face %d: geodesic disks need faces of positive area" % int(np.nonzero((L <= 0).any(1) | (cr <= 0).any(1))[0][0]))
    geo = np.stack([L, np.einsum("fkc,fkc->fk", p2 - p0, e) / L, cr / L], axis=2)
    # corner angle at f[k] between edges k and k-1
    u, w = p1 - p0, np.roll(p0, 1, axis=1) - p0                      # roll: f[k-1] - f[k]
    ang = np.arctan2(np.linalg.norm(np.cross(u, w), axis=2), np.einsum("fkc,fkc->fk", u, w))
    angle_sum = np.bincount(fc.reshape(-1), weights=ang.reshape(-1), minlength=V)
    boundary = np.zeros(V, bool)
    bd = (twin < 0)
    boundary[a[bd]] = True
    boundary[b[bd]] = True
    pseudo = ((angle_sum >= 2.0 * np.pi) | boundary).astype(np.int32)
    corner = np.argsort(fc.reshape(-1), kind="stable")
    fan_off = np.zeros(V + 1, np.int64)
    fan_off[1:] = np.cumsum(np.bincount(fc.reshape(-1), minlength=V))
    return {"verts64": v, "faces": fc.astype(np.int32), "twin": twin.astype(np.int32), "edge_geo": geo, "angle_sum": angle_sum,
            "boundary": boundary, "pseudo": pseudo, "fan_off": fan_off, "fan": corner.astype(np.int32)}


class Mesh(object):
    """A triangle mesh resident on the device in the face layout of dispu_point_to_mesh (include/dispu_hip.h): faces sorted by the
    Morton code of their centroids (a one-time host sort, the counterpart of CGAL's AABB-tree build), tiles of 64 with fp32 boxes.

    Host attributes: verts [V,3] f32, faces [F,3] i32, areas [F] f64 (per face), total_area (f64 sum, evaluation.cpp:148-150),
    cum_areas [F+1] f64 (normalised cumulative areas, :152-157)."""

    def __init__(self, verts, faces, device=None):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        fc = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
        req(fc.shape[0] > 0, "Mesh needs at least one face")
        req(fc.min() >= 0 and fc.max() < v.shape[0], "Mesh: face vertex index out of range")
        if device is None:
            device = torch.device("cuda:0")
        device = torch.device(device)
        req(device.type == "cuda", "Mesh must live on a ROCm device (dis-pu_amd has no CPU path)")
        self.device = device
        self.verts, self.faces = v, fc.astype(np.int32)
        tv = v[fc].astype(np.float64)                                    # [F, 3, 3]
        self.areas = 0.5 * np.linalg.norm(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]), axis=1)
        self.total_area = float(np.sum(self.areas))
        cum = np.zeros(fc.shape[0] + 1, np.float64)
        cum[1:] = np.cumsum(self.areas / self.total_area) if self.total_area > 0 else np.arange(1, fc.shape[0] + 1) / fc.shape[0]
        self.cum_areas = cum
        tris, order, box = face_tiles(v, fc)
        self.order = order
        self.tris = torch.from_numpy(tris).to(device)
        self.face_ids = torch.from_numpy(order).to(device)
        self.tile_box = torch.from_numpy(box).to(device)

    @classmethod
    def from_off(cls, path, device=None):
        v, f = load_off(path)
        return cls(v, f, device)

    @property
    def num_faces(self):
        return self.faces.shape[0]

    def geodesic_tables(self):
        """The host tables and device copies of geodesic_tables(verts, faces), built on the first call and cached (Euclidean users
        never pay for them).  Raises ValueError on a non-manifold mesh."""
        g = getattr(self, "_geodesic", None)
        if g is None:
            g = geodesic_tables(self.verts, self.faces)
            for k in ("verts64", "faces", "twin", "edge_geo", "pseudo", "fan_off", "fan"):
                g["dev_" + k] = torch.from_numpy(np.ascontiguousarray(g[k])).to(self.device)
            self._geodesic = g
        return g

    def surface_points(self, face_ids, bary):
        """b0 v0 + b1 v1 + b2 v2 of each (face, barycentrics) in float64 (CGAL's shortest_paths.point, evaluation.cpp:253)."""
        fid = np.asarray(face_ids, np.int64)
        b = np.asarray(bary, np.float64).reshape(-1, 3)
        req(fid.shape[0] == b.shape[0], "face_ids and barycentrics differ in length")
        req(fid.size == 0 or (fid.min() >= 0 and fid.max() < self.num_faces), "seed face id out of range")
        tv = self.verts[self.faces[fid]].astype(np.float64)
        return np.einsum("nk,nkc->nc", b, tv)


# ------------------------------------------------------------------------------------------------------------- P2F ----------
def point_to_mesh(points, mesh, brute_force=False):
    """points [n,3] device f32 -> (dist [n] f32, proj [n,3] f32, face [n] i32): the closest point of the mesh surface to every
    point (evaluation.cpp:202-214).  Smallest distance wins, exact ties go to the lowest face index; dist / proj are evaluated in
    fp64 for the winning face.  brute_force=True visits every face tile (the pruned default gives identical outputs)."""
    p = f32(points, "points")
    req(p.dim() == 2 and p.shape[1] == 3, "points must be of shape (#points,3)")
    req(p.device == mesh.device, "points and mesh live on different devices")
    n = p.shape[0]
    dev = p.device
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    proj = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    flags = _lib.MESH_BRUTE_FORCE if brute_force else 0
    _lib.check(_lib.lib().dispu_point_to_mesh(n, _lib.ptr(p), mesh.num_faces, _lib.ptr(mesh.tris), _lib.ptr(mesh.face_ids),
                                              _lib.ptr(mesh.tile_box), _lib.ptr(dist), _lib.ptr(proj), _lib.ptr(face), flags,
                                              _lib.stream_ptr(dev)), "dispu_point_to_mesh")
    return dist, proj, face


def mean_std(x):
    """x [n] device f32 -> (mean, std) of the non-NaN entries as Python floats (np.nanmean / np.nanstd, ddof 0)."""
    x = f32(x, "x").reshape(-1)
    req(x.numel() > 0, "mean_std needs at least one value")
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().dispu_row_mean_std(1, x.numel(), _lib.ptr(x), _lib.ptr(out), _lib.stream_ptr(x.device)), "dispu_row_mean_std")
    m, s = out.cpu().tolist()
    return m, s


# ------------------------------------------------------------------------------------------------------------- seeds / disks --
def find_surface(cum_areas, u):
    """evaluation.cpp:117-125 vectorised: the face i with cum[i] <= u < cum[i+1], 0 when there is none."""
    u = np.asarray(u, np.float64)
    i = np.searchsorted(cum_areas, u, side="right") - 1
    ok = (i >= 0) & (i < len(cum_areas) - 1)
    return np.where(ok, i, 0).astype(np.int32)


def sample_surface_seeds(mesh, count=1000, seed=0):
    """Seeds on the surface as (face_ids [count] i32, bary [count,3] f64): per seed a face chosen with probability proportional
    to its area (find_surface, evaluation.cpp:117-125,239) and barycentrics U(0.01, 1) normalised to sum 1 (:241-243), drawn
    in that order from numpy.random.default_rng(seed).  CGAL::Random's stream cannot be reproduced, so the seeds (and the
    uniformity that depends on them) are not those of the CGAL tool."""
    req(int(count) > 0, "seed count must be positive")
    rng = np.random.default_rng(seed)
    r = rng.random((int(count), 4))
    fid = find_surface(mesh.cum_areas, r[:, 0])
    b = 0.01 + 0.99 * r[:, 1:]
    return fid, b / b.sum(axis=1, keepdims=True)


def disk_radii(mesh, percentages=DEFAULT_PERCENTAGES):
    """sqrt(total_area * pct / pi) per percentage (evaluation.cpp:259-266), with CGAL's float percentages and float radii."""
    pct = np.asarray(percentages, np.float32).astype(np.float64)
    return np.sqrt(mesh.total_area * pct / np.pi).astype(np.float32)


def _dev_f32(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def disk_members(seed_points, points, radii):
    """Euclidean disks: seed_points [S,3], points [n,3] (the projected points) device f32, radii [R] -> (offsets [S*R+1] i64,
    members [offsets[-1]] i32) on the device, CSR rows seed-major (i*R + j, the `_disk_idx.txt` line order), members ascending.
    q is in disk (i, j) iff d2(seed i, q) <= fl32(r_j * r_j) (include/dispu_hip.h: dispu_disk_count)."""
    s, p = f32(seed_points, "seed_points"), f32(points, "points")
    req(s.dim() == 2 and s.shape[1] == 3 and p.dim() == 2 and p.shape[1] == 3, "seed_points and points must be (#points,3)")
    req(p.shape[0] > 0, "points must not be empty")
    dev = p.device
    r = f32(_dev_f32(np.asarray(radii, np.float32).reshape(-1), dev) if not isinstance(radii, torch.Tensor) else radii, "radii").reshape(-1)
    S, n, R = s.shape[0], p.shape[0], r.shape[0]
    req(R > 0, "at least one radius")
    offsets = torch.empty(S * R + 1, dtype=torch.int64, device=dev)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    _lib.check(L.dispu_disk_count(S, n, R, _lib.ptr(s), _lib.ptr(p), _lib.ptr(r), _lib.ptr(offsets), st), "dispu_disk_count")
    total = int(offsets[S * R].item())
    members = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    _lib.check(L.dispu_disk_fill(S, n, R, _lib.ptr(s), _lib.ptr(p), _lib.ptr(r), _lib.ptr(offsets), _lib.ptr(members), st), "dispu_disk_fill")
    return offsets, members[:total]


def uniformity(points, offsets, members, radii, percentages=DEFAULT_PERCENTAGES, N=None):
    """analyze_uniform (evaluate.py:53-101) on the device: points [n,3] f32 (projected points), CSR (offsets [S*R+1] i64, members
    i32) with R = len(radii) disks per seed -> np.float64 [R], NaN for a radius whose disks all hold fewer than 5 points.
    N (default n) sets the expected count pct * N."""
    p = f32(points, "points")
    req(p.dim() == 2 and p.shape[1] == 3 and p.shape[0] > 0, "points must be of shape (#points,3)")
    dev = p.device
    rad = np.asarray(radii, np.float64).reshape(-1)
    pct = np.asarray(percentages, np.float64).reshape(-1)
    R = rad.shape[0]
    req(R > 0 and pct.shape[0] == R, "need one percentage per radius")
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or not isinstance(members, torch.Tensor) or not members.is_cuda:
        raise ValueError("offsets / members must live on a ROCm device (dis-pu_amd has no CPU path)")
    req(offsets.dtype == torch.int64 and members.dtype == torch.int32, "offsets must be int64 and members int32")
    offsets, members = offsets.contiguous(), members.contiguous()
    M = offsets.shape[0] - 1
    req(M > 0 and M % R == 0, "offsets must hold S*R + 1 row starts")
    S = M // R
    n = p.shape[0]
    N = n if N is None else int(N)
    mem = members if members.numel() > 0 else torch.zeros(1, dtype=torch.int32, device=dev)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    rad_d = torch.from_numpy(rad).to(dev)
    pct_d = torch.from_numpy(pct).to(dev)
    nbytes = L.dispu_disk_uniformity_scratch_bytes(S, R)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(R, dtype=torch.float64, device=dev)
    _lib.check(L.dispu_disk_uniformity(S, R, n, _lib.ptr(p), _lib.ptr(offsets), _lib.ptr(mem), _lib.ptr(rad_d), _lib.ptr(pct_d), N,
                                       _lib.ptr(scratch), nbytes, _lib.ptr(out), st), "dispu_disk_uniformity")
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- geodesic disks -
GEODESIC_ARENA = 4096                 # windows per seed in the first pass; an overflowing seed is rerun with 4x as many
_GEODESIC_ARENA_MAX = 1 << 22
_GEODESIC_SCRATCH_BUDGET = 256 << 20  # bytes of window arena per launch (seeds are launched in chunks that fit)


def _seed_arrays(mesh, seed_faces, seed_bary):
    fid = np.ascontiguousarray(seed_faces, np.int64).reshape(-1)
    bary = np.ascontiguousarray(seed_bary, np.float64).reshape(-1, 3)
    req(fid.shape[0] == bary.shape[0], "seed_faces and seed_bary differ in length")
    req(fid.size == 0 or (fid.min() >= 0 and fid.max() < mesh.num_faces), "seed face id out of range")
    req(np.all(bary >= 0.0) and np.all(np.abs(bary.sum(axis=1) - 1.0) <= 1e-9), "seed barycentrics must be >= 0 and sum to 1")
    return fid.astype(np.int32), bary


def _geodesic_launch(T, fid, bary, p, pf, cand_off, cand, a, b, max_dist, cap, dist, status):
    """seeds [a, b) (consecutive: their candidate rows are a view of the CSR) in chunks whose arenas fit the scratch budget"""
    L, st, dev = _lib.lib(), _lib.stream_ptr(p.device), p.device
    per = max(1, _GEODESIC_SCRATCH_BUDGET // max(1, L.dispu_geodesic_scratch_bytes(1, cap)))
    for c0 in range(a, b, per):
        c1 = min(b, c0 + per)
        sf = torch.from_numpy(fid[c0:c1]).to(dev)
        sb = torch.from_numpy(np.ascontiguousarray(bary[c0:c1])).to(dev)
        nbytes = L.dispu_geodesic_scratch_bytes(c1 - c0, cap)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.dispu_geodesic_distances(
            c1 - c0, _lib.ptr(sf), _lib.ptr(sb), _lib.ptr(T["dev_verts64"]), _lib.ptr(T["dev_faces"]), _lib.ptr(T["dev_twin"]),
            _lib.ptr(T["dev_edge_geo"]), _lib.ptr(T["dev_pseudo"]), _lib.ptr(T["dev_fan_off"]), _lib.ptr(T["dev_fan"]), p.shape[0],
            _lib.ptr(p), _lib.ptr(pf), _lib.C.c_void_p(cand_off.data_ptr() + 8 * c0), _lib.ptr(cand), float(max_dist), int(cap),
            _lib.ptr(scratch), nbytes, _lib.ptr(dist), _lib.C.c_void_p(status.data_ptr() + 4 * c0), st), "dispu_geodesic_distances")


def geodesic_distances(mesh, seed_faces, seed_bary, points, point_faces, max_dist, arena=GEODESIC_ARENA):
    """Exact geodesic distances from seeds on the surface (face ids [S], barycentrics [S,3] f64; zeros allowed: a seed on an edge or a
    vertex) to the points [n,3] (device f32, on the surface: point_to_mesh's proj) in their faces point_faces [n] (device i32) whose
    straight-line distance to the seed is at most max_dist (widened by 2^-12 relative: the pre-filter must not drop a point the
    geodesic keeps).  -> (cand_off [S+1] i64, cand i32: per seed its candidate points ascending, dist f64 aligned with cand: the
    geodesic distance, +inf above max_dist), all on the device.  csrc/geodesic.hip; a seed whose window arena (`arena` windows)
    overflows is rerun with 4x the arena, never truncated."""
    T = mesh.geodesic_tables()
    p, pf = f32(points, "points"), i32(point_faces, "point_faces").reshape(-1)
    req(p.dim() == 2 and p.shape[1] == 3 and p.shape[0] > 0, "points must be of shape (#points,3)")
    req(pf.shape[0] == p.shape[0], "point_faces must hold one face per point")
    req(int(pf.min().item()) >= 0 and int(pf.max().item()) < mesh.num_faces, "point face id out of range")
    req(p.device == mesh.device and pf.device == mesh.device, "points and mesh live on different devices")
    req(float(max_dist) >= 0.0, "max_dist must be >= 0")
    req(int(arena) > 0, "arena must be positive")
    fid, bary = _seed_arrays(mesh, seed_faces, seed_bary)
    S, dev = fid.shape[0], p.device
    seed_pts = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
    rc = np.float32(float(max_dist) * (1.0 + 2.0 ** -12))
    cand_off, cand = disk_members(seed_pts, p, np.array([rc], np.float32)) if S else (torch.zeros(1, dtype=torch.int64, device=dev),
                                                                                     torch.zeros(0, dtype=torch.int32, device=dev))
    total = int(cand_off[S].item())
    dist = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
    cand_buf = cand if cand.numel() > 0 else torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(max(S, 1), dtype=torch.int32, device=dev)
    todo, cap = np.arange(S), int(arena)
    while todo.size:
        runs = np.split(todo, np.nonzero(np.diff(todo) != 1)[0] + 1)
        for r in runs:
            _geodesic_launch(T, fid, bary, p, pf, cand_off, cand_buf, int(r[0]), int(r[-1]) + 1, max_dist, cap, dist, status)
        st = status.cpu().numpy()[:S]
        todo = todo[st[todo] != 0]
        if todo.size:
            req(cap < _GEODESIC_ARENA_MAX, "geodesic disks: %d seeds still overflow a %d-window arena" % (todo.size, cap))
            cap *= 4
    return cand_off, cand, dist[:total]


def geodesic_disk_members(mesh, seed_faces, seed_bary, points, point_faces, radii, arena=GEODESIC_ARENA):
    """Geodesic disks, the CGAL tool's membership (evaluation.cpp:85-115): point q is in disk (i, j) iff its straight-line distance to
    seed i passes the pre-filter at max(radii) and geodesic(seed i, q) <= (double)fl32(r_j).  Same arguments as geodesic_distances
    with the float radii [R]; -> (offsets [S*R+1] i64, members i32) on the device, in disk_members' CSR layout (rows i*R + j,
    members ascending)."""
    r = np.asarray(radii, np.float32).reshape(-1)
    req(r.shape[0] > 0, "at least one radius")
    cand_off, cand, dist = geodesic_distances(mesh, seed_faces, seed_bary, points, point_faces, float(r.max()), arena)
    S, R, dev = cand_off.shape[0] - 1, r.shape[0], cand_off.device
    rd = torch.from_numpy(r).to(dev)
    offsets = torch.empty(S * R + 1, dtype=torch.int64, device=dev)
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    d = dist if dist.numel() > 0 else torch.zeros(1, dtype=torch.float64, device=dev)
    c = cand if cand.numel() > 0 else torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.dispu_geodesic_disk_count(S, R, _lib.ptr(cand_off), _lib.ptr(d), _lib.ptr(rd), _lib.ptr(offsets), st),
               "dispu_geodesic_disk_count")
    total = int(offsets[S * R].item())
    members = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    _lib.check(L.dispu_geodesic_disk_fill(S, R, _lib.ptr(cand_off), _lib.ptr(c), _lib.ptr(d), _lib.ptr(rd), _lib.ptr(offsets),
                                          _lib.ptr(members), st), "dispu_geodesic_disk_fill")
    return offsets, members[:total]


# ------------------------------------------------------------------------------------------------------------- CGAL files -----
def cgal_paths(pred_path):
    """the three files the CGAL tool writes beside a prediction (evaluation.cpp:194-197,262,303)."""
    stem = os.path.splitext(pred_path)[0]
    return stem + "_point2mesh_distance.txt", stem + "_radius.txt", stem + "_disk_idx.txt"


def write_cgal_files(pred_path, points, dist, proj, radii, offsets, members):
    """Write `_point2mesh_distance.txt` (x y z d px py pz per point), `_radius.txt` and `_disk_idx.txt` (`count:i i ... ` per
    disk) in the CGAL tool's layout, with %.9g (float32 round trip) instead of its 6 digits.  Host arrays."""
    p2m, rad, idx = cgal_paths(pred_path)
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    tab = np.concatenate([pts, np.asarray(dist, np.float32).reshape(-1, 1), np.asarray(proj, np.float32).reshape(-1, 3)], axis=1)
    np.savetxt(p2m, tab, fmt="%.9g", delimiter=" ")
    with open(rad, "w") as f:
        f.write("".join("%.9g " % r for r in np.asarray(radii, np.float32)) + "\n")
    off = np.asarray(offsets, np.int64)
    mem = np.asarray(members, np.int64)
    with open(idx, "w") as f:
        for k in range(off.shape[0] - 1):
            row = mem[off[k]:off[k + 1]]
            f.write("%d:%s\n" % (row.shape[0], "".join("%d " % q for q in row)))


def read_cgal_files(pred_path):
    """-> dict(points [n,3], dist [n], proj [n,3] float32 (np.loadtxt + float32 as pc_util.load), radii [R] float64 of the
    nearest float32 (the CGAL tool's radii are floats), offsets [M+1] i64, members i32) from the CGAL tool's three files.
    A member index outside the projected points raises."""
    p2m, rad, idx = cgal_paths(pred_path)
    tab = np.loadtxt(p2m, ndmin=2).astype(np.float32)
    req(tab.shape[1] >= 7, "%s: expected 7 columns (x y z d px py pz)" % p2m)
    radii = np.atleast_1d(np.loadtxt(rad)).astype(np.float32).astype(np.float64)
    counts, members = [], []
    with open(idx) as f:
        for line in f:
            if not line.strip():
                continue
            head, _, body = line.partition(":")
            row = [int(t) for t in body.split()]
            req(int(head) == len(row), "%s: count %s does not match its %d indices" % (idx, head, len(row)))
            counts.append(len(row))
            members.extend(row)
    n = tab.shape[0]
    mem = np.asarray(members, np.int64)
    req(mem.size == 0 or (mem.min() >= 0 and mem.max() < n), "%s: member index outside the %d projected points" % (idx, n))
    req(len(counts) % max(radii.shape[0], 1) == 0, "%s: %d disks is not a multiple of %d radii" % (idx, len(counts), radii.shape[0]))
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return {"points": tab[:, :3], "dist": tab[:, 3].copy(), "proj": np.ascontiguousarray(tab[:, 4:7]), "radii": radii,
            "offsets": off, "members": mem.astype(np.int32)}


# ------------------------------------------------------------------------------------------------------------- one cloud ------
DISK_MODES = ("euclidean", "geodesic")


def mesh_metrics(pred, mesh, seeds=1000, seed=0, percentages=DEFAULT_PERCENTAGES, disks="euclidean"):
    """P2F and uniformity of one predicted cloud pred [n,3] (device f32, raw coordinates: the mesh's frame) against `mesh`.
    seeds: a count (sample_surface_seeds(mesh, seeds, seed)) or user-given (face_ids, bary) / an [S,4] array of
    (face_id, b0, b1, b2) rows.  disks: "euclidean" (disk_members, the default) or "geodesic" (geodesic_disk_members, CGAL's
    membership).  Returns a dict with the scalars and the device arrays behind them."""
    req(disks in DISK_MODES, "disks must be one of %s, got %r" % (DISK_MODES, disks))
    p = f32(pred, "pred")
    if isinstance(seeds, (int, np.integer)):
        fid, bary = sample_surface_seeds(mesh, int(seeds), seed)
    elif isinstance(seeds, tuple) and len(seeds) == 2:
        fid, bary = seeds
    else:
        a = np.asarray(seeds, np.float64).reshape(-1, 4)
        fid, bary = a[:, 0].astype(np.int64), a[:, 1:]
    seed_pts = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(p.device)
    dist, proj, face = point_to_mesh(p, mesh)
    radii = disk_radii(mesh, percentages)
    if disks == "geodesic":
        offsets, members = geodesic_disk_members(mesh, fid, bary, proj, face, radii)
    else:
        offsets, members = disk_members(seed_pts, proj, radii)
    uni = uniformity(proj, offsets, members, radii.astype(np.float64), np.asarray(percentages, np.float64), N=p.shape[0])
    m, s = mean_std(dist)
    return {"p2f avg": m, "p2f std": s, "uniform": uni, "dist": dist, "proj": proj, "face": face, "radii": radii,
            "offsets": offsets, "members": members}
