"""The evaluator's mesh kernels, each ALONE through the C ABI against tests/mesh_oracle.py (plain numpy, held to hand-computed cases and
to analyze_uniform by tests/test_mesh_eval.py), on every path their launch code takes and with exact ties wherever a choice can meet one.

Entries under test: csrc/mesh_eval.hip (dispu_point_to_mesh, dispu_disk_count, dispu_disk_fill, dispu_disk_uniformity and its
scratch_bytes) and the two membership entries at the end of csrc/geodesic.hip (dispu_geodesic_disk_count, dispu_geodesic_disk_fill;
dispu_geodesic_distances is not called: candidates and distances are made by hand).  dispu_row_mean_std is in test_cloud_ops_gpu.py.

Every output is pre-filled with a sentinel and sits between guards of it (train_ops_oracle.Guarded; the int32, int64 and float64
outputs are views of such a buffer), and so does every input: a kernel that writes one element outside its rows, leaves one unwritten, or
changes an input fails the test, and a read past an input's end meets the sentinel (-12345, or its bits).  No call passes an index or a
shape its entry point does not refuse on the host.

Standards.
  P2F              pruned == DISPU_MESH_BRUTE_FORCE == NULL tile boxes, bit for bit on dist, proj and face, for every mesh and point count.
                   Against mesh_oracle.point_to_mesh (float64), with scale = max(1, largest |coordinate| of mesh and points):
                   dist within 2e-6 scale; |p - proj| against dist within the same, everywhere; proj within 1e-5 scale and face equal
                   where the oracle's second-best face is more than 1e-6 scale behind, which holds for nine tenths of every mesh's points
                   or more (asserted here and, from the oracle alone, in test_mesh_eval.py); where faces that share a vertex tie at exactly 0
                   in float32 and float64 alike, the lowest index of them.  Duplicated meshes: never the copy's index, dist and proj as
                   bits those of the mesh alone.
  disks            index-exact against disk_members_fp32 / geodesic_disk_members: offsets whole, then every row.
  uniformity       against mesh_oracle.uniform_terms (the nearest other member from float32 d2, which is exact in any order; float64 and
                   math.fsum after it): kept exact; term within (c + 8) 2^-52 |want| for a disk of c members -- the terms of its sum are not
                   negative, so any order of adding c of them is within (c - 1) 2^-53 relative, and 8 covers the roundings of the square
                   root, difference, square and divisions; a skipped disk has term 0 and kept 0; out[j] within (S + 8) 2^-52 |want| plus the
                   mean of its disks' term bounds, NaN for a radius without a kept disk; two runs equal as bits, scratch included.
Every float comparison prints its worst error as a fraction of its bound before it asserts (pytest -s).

Paths and the case that reaches each (the host or kernel branch is named; nothing is instrumented):
  point_to_mesh_kernel<false>, flags 0 with boxes        every P2F case, first call
  point_to_mesh_kernel<true>, by the flag / by NULL boxes  every P2F case, second and third call (`(flags & BRUTE) || !tile_box`)
  `pi >= n` in a workgroup of 4 waves                    n = 1, 3, 5, 63, 257 of every mesh (n = 4: a full workgroup)
  one tile, partial and full: `e < F`, T = 1, 2          test_point_to_mesh[ico2_1], [ico2_20], [ico2_63], [ico2_64], [ico2_65]
  second trip of `t += 64` / `c0 += 64`, `min(t, T - 1)`  [ico4_4096] (T = 64: one trip, full), [ico4_4097] (T = 65: lane 0 alone in the second,
                                                          63 lanes clamped to T - 1), [ico4_5120] (T = 80)
  the slack term of box_lower_bound at pmag, bmag = 40    [offset]: radius 0.5 about (37.5, -20.25, 11)
  slivers of length 1 and width 1e-4                      [rungs]: 200 of them as the rungs of a ladder (mesh_oracle.sliver_rungs says why
                                                          they share no edge)
  faces without area                                      [rungs_zero]: a == b, b == c, a == c, a == b == c, and three distinct, exactly
                                                          collinear float32 vertices in three orders; a quarter of the points lie nearest to
                                                          one of them, 40 or more are decided by one, every one of the seven decides a point
  faces whose area is what rounding left                  [rungs_collinear]: float64-collinear triples rounded to float32
  exact float32 ties between faces, either tile order     test_point_to_mesh_exact_ties[copy_after], [copy_before]; the shared-vertex rule of
                                                          every closed mesh
  host refusals, n == 0                                   test_point_to_mesh_refusals
  `i >= S`, `q < n` of disk_count / disk_fill             test_disks: S = 1, 3, 5, 6, 7 (never a multiple of the 4 waves), n = 1, 63, 64, 65, 200;
                                                          radius 1e5 (rows exactly 0 .. n - 1; the guard values lie within it), r with a point
                                                          exactly on it and one a float32 beyond, 0 with a seed on a point
  disk_scan_kernel, M = S R                               test_disk_scan_sizes: 1, 1023 (idle threads), 1024 (full), 1025 (per = 2, threads from
                                                          513 on start beyond M + 1), 2049 and 3000 (per = 3); through disk_scan_launch:
                                                          test_geodesic_disks_scan_1025
  S == 0 (`offsets[0] = 0` only), refusals                test_disks_empty_and_refusals, test_geodesic_disks_empty_and_refusals
  `i >= S`, `c < e` of geo_count / geo_fill               test_geodesic_disks: rows of 0, 1, 63, 64, 65, 200 candidates, S = 6, R = 1, 3, the
                                                          empty row first, in the middle, last; +inf, 0, exactly (double)radii[j], the next double
  disk_uniformity_kernel: `c < 5`; `a0 += 256`; tiles     test_disk_uniformity: c = 0, 4 / 5, 6; 255, 256 (one trip), 257 (a second, of one member);
                                                          1024 (one LDS tile), 1025 (a second of one member: the coincident twin of member 0, or
                                                          a member whose nearest other is elsewhere)
  disk_uniformity_mean_kernel                             S = 1, 63 (idle lanes), 65, 130 (second and third trip); kept and skipped disks
                                                          alternate along the seeds; S = 65: radius 1 without a kept disk -> NaN; N = n and N != n
  refusals of dispu_disk_uniformity                       test_disk_uniformity_refusals: scratch one byte short, NULL, S, R, n, N <= 0
Not reached, as far as can be seen from outside: the "three edges" fallback at the end of tri_closest (the faces without area resolve in
the vertex and edge regions -- with a == b: d1 = d3 = 0 and d4 = d2, so the point goes to vertex a (d2 <= 0), to vertex c (d6 >= 0), or
to edge ac through `vb <= 0` with vb = 0; exactly collinear vertices give a zero normal, every weight 0, and likewise an edge), and the
clamp of a member index into [0, n) in disk_uniformity_kernel (no row here holds an index outside the points).

A bug found and fixed.  test_point_to_mesh[rungs] (and [rungs_zero], [rungs_collinear]) failed on the kernel as it was: on each of the
three meshes 4 of 333 points, on or next to the interior of a sliver, came back with the next rung as their face, dist off by up to
0.0078, 0.0087 and 0.0036 (1139, 1344 and 530 times the bound).  The fp32 search formed the
face-region weights as d1 d4 - d3 d2, two products of about |ab| |ac| |ap| |bp| that cancel to |ab x ac| |ap x bp|; on a sliver of
aspect 1e4 nothing but rounding was left, and the point's own face lost.  tri_closest now forms them as (ab x ac) . (ap x bp).  Output
change: where two faces are within float32 rounding of each other the winner can differ from before (Icosahedron with its 8192 network
outputs: 1 face, fandisk: 2 faces, 18 of 32768 on a 81920-face sphere; P2F mean 2.5919458534e-3 -> 2.5919458553e-3); nothing else
moves.  What remains of the conditioning is the float32 one: on a sliver of aspect A the fp32 closest point is good to about
A 2^-24 of its length, so faces closer together than that are told apart no better than before.

Mutations (each alone, on a scratch build of the two kernel files) and the tests of this file that fail under each, all others passing:
  key from `e`, the tile entry (face = face_ids[e] of     test_point_to_mesh_exact_ties[copy_before] (all 333 points report the copy), [copy_after]
  the winner), for face_ids[e]                            and test_point_to_mesh[ico2_20], [ico2_63], [ico2_64], [ico2_65], [ico4_4096],
                                                          [ico4_4097], [ico4_5120], [offset]: the shared-vertex rule (exact ties; 2 .. 9 points each)
  `q < n &&` dropped in disk_count_kernel                 test_disks[1-1-1], [3-63-2], [6-65-3], [7-200-2] (every n % 64 != 0; [5-64-1] passes),
                                                          test_disk_scan_sizes (all six, n = 65), test_disks_empty_and_refusals
  `min(b + per, M)` in disk_scan_kernel                   test_disks (all but [1-1-1]), test_disk_scan_sizes (all but [1-1]: with M = 1 the last
                                                          count is the total), test_disks_empty_and_refusals, test_geodesic_disks (all six),
                                                          test_geodesic_disks_scan_1025
  `c <= 5` in disk_uniformity_kernel                      test_disk_uniformity (all eight: kept differs at exactly the 5-member disks)
  `t != a` for `b0 + t != a`                              test_disk_uniformity (all eight: the terms of the 1025-member disks, by 3e9 bounds or more)
  `dist[c] < r` in geo_in                                 test_geodesic_disks (all six), test_geodesic_disks_scan_1025
  v and w swapped in the face region of tri_closest       test_point_to_mesh (all twelve), test_point_to_mesh_exact_ties (both)
The refusal tests pass under every mutation that leaves their kernels alone.

Measured on an MI355X: every index of every disk and every kept flag as the oracle has it; pruned, brute force and NULL boxes equal in
every bit.  Worst error as a fraction of its bound: P2F dist 0.021 (2.3e-7 absolute; [offset] 0.014, 1.1e-6; the sliver meshes 0.018),
proj 0.003 ([offset] 0.005), |p - proj| against dist 0.023; near-ties 0 .. 7.8 % of a mesh's points; uniformity term 0.12 (the
6-member disks, 8.9e-16 absolute; the 1024- and 1025-member disks 0.0007), out 0.0009.  No bound stated above had to be widened."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_oracle as MO  # noqa: E402
import train_ops_oracle as TO  # noqa: E402
from train_ops_oracle import F32, INVALID, SENT, Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
          np.dtype(np.int64): torch.int64}


@pytest.fixture(autouse=True)
def _release():
    yield
    TO.release()


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


def run(L, dev, name, *args):
    """one entry of the C ABI on the current stream, synchronised -> its return code."""
    rc = getattr(L.lib(), name)(*(args + (L.stream_ptr(dev),)))
    torch.cuda.synchronize()
    return rc


def ok(L, dev, name, *args):
    L.check(run(L, dev, name, *args), name)


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def gin(dev, a, g=64):
    """a host array of float32 / float64 / int32 / int64 as a guarded device buffer, bit for bit (the guards and the buffer's own
    element type stay float32: what lies past the end reads as the sentinel, or as its bits)."""
    a = np.ascontiguousarray(a)
    G = Guarded(dev, a.nbytes // 4, g=g)
    if a.size:
        G.t[g:g + G.n].view(_TORCH[a.dtype]).copy_(torch.from_numpy(a.reshape(-1)))
        torch.cuda.synchronize()
    G.host = a.reshape(-1).view(np.uint32).copy()
    return G


def gout(dev, count, dtype):
    """a guarded output of `count` elements of dtype, every 32-bit word of it the sentinel."""
    return Guarded(dev, count * np.dtype(dtype).itemsize // 4)


def as_(G, dtype):
    return np.ascontiguousarray(G.body()).view(dtype)


def unread(G):
    """an input after the launch: guards intact, every bit as it was."""
    return G.guards_intact() and np.array_equal(np.ascontiguousarray(G.body()).view(np.uint32), G.host)


def untouched(G):
    return G.guards_intact() and bool((G.body() == F32(SENT)).all())


def exact_rows(off, mem, want, what):
    """a CSR against a list of rows: offsets whole, then every row."""
    want_off = np.concatenate([[0], np.cumsum([len(r) for r in want])]).astype(np.int64)
    bad = np.nonzero(off != want_off)[0]
    assert off.shape == want_off.shape and not len(bad), "%s: offsets differ at %s: got %s, want %s" % (
        what, bad[:4], off[bad[:4]], want_off[bad[:4]])
    if mem is not None:
        flat = np.concatenate([np.asarray(r, np.int32) for r in want] + [np.zeros(0, np.int32)])
        bad = np.nonzero(mem != flat)[0]
        assert mem.shape == flat.shape and not len(bad), "%s: %d members differ, first at %d (row %d): got %d, want %d" % (
            what, len(bad), bad[0], int(np.searchsorted(want_off, bad[0], side="right") - 1), mem[bad[0]], flat[bad[0]])


def near(got, want, bound, what):
    """|got - want| <= bound per element, the worst fraction printed first."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert np.isfinite(got).all(), what + ": not finite"
    err = np.abs(got - want)
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("[measured] %s: worst error %.4f of its bound (largest absolute error %.3e)" % (what, frac, err.max() if err.size else 0.0))
    assert (err <= bound).all(), "%s: %d elements beyond the bound, worst %.3f of it (first at %d)" % (
        what, int((err > bound).sum()), frac, int(np.argmax(err > bound)))
    return frac


# ------------------------------------------------------------------------------------------- dispu_point_to_mesh ----
class Layout(object):
    """mesh.face_tiles' layout of a mesh in guarded device buffers; `relabel` renames the faces (face_ids = relabel[order])."""

    def __init__(self, dev, verts, faces, relabel=None):
        from dispu_amd import mesh as M
        tris, order, box = M.face_tiles(verts, faces)
        self.F = faces.shape[0]
        assert tris.shape == (self.F, 12) and box.shape == ((self.F + 63) // 64, 8)
        ids_ = order if relabel is None else np.asarray(relabel, np.int32)[order]
        self.tris, self.ids, self.box = gin(dev, tris), gin(dev, ids_.astype(np.int32)), gin(dev, box)

    def unread(self):
        return unread(self.tris) and unread(self.ids) and unread(self.box)


def p2f_call(L, dev, lay, pts, flags, box=True):
    n = pts.shape[0]
    gp = gin(dev, pts)
    dist, proj, face = gout(dev, n, F32), gout(dev, 3 * n, F32), gout(dev, n, np.int32)
    ok(L, dev, "dispu_point_to_mesh", n, gp.ptr(), lay.F, lay.tris.ptr(), lay.ids.ptr(), lay.box.ptr() if box else None, dist.ptr(),
       proj.ptr(), face.ptr(), flags)
    assert dist.guards_intact() and proj.guards_intact() and face.guards_intact(), "point_to_mesh n %d wrote outside its outputs" % n
    assert unread(gp) and lay.unread()
    return dist.body(), proj.body().reshape(n, 3), as_(face, np.int32)


def p2f_three(L, dev, lay, pts, what):
    """the pruned kernel, the brute-force flag and the NULL-box route: bit-identical on all three outputs -> the pruned result."""
    a = p2f_call(L, dev, lay, pts, 0)
    b = p2f_call(L, dev, lay, pts, L.MESH_BRUTE_FORCE)
    c = p2f_call(L, dev, lay, pts, 0, box=False)
    for other, name in ((b, "brute force"), (c, "NULL boxes")):
        for x, y, out in zip(a, other, ("dist", "proj", "face")):
            same = np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
            assert same, "%s n %d: %s of the pruned kernel and of %s differ in bits" % (what, pts.shape[0], out, name)
    return a


def p2f_sets(L, dev, lay, case, what):
    """every point set of the case (n = 1, 3, 4, 5, 63, 257) through the three routes -> dist, proj, face over case['points']."""
    got = [p2f_three(L, dev, lay, pts, what) for pts in case["sets"]]
    return tuple(np.concatenate([g[k] for g in got]) for k in range(3))


def p2f_check(what, got, case, max_face=None):
    d, q, f = got
    pts, s = case["points"].astype(np.float64), case["scale"]
    rd, rq, rf, gap = case["dist"], case["proj"], case["face"], case["gap"]
    clear = gap > 1e-6 * s
    share = 1.0 - clear.mean()
    print("[measured] %s: %.1f %% of %d points within 1e-6 x %.3g of a second face" % (what, 100.0 * share, len(d), s))
    assert share <= 0.10, "%s: %.1f %% of the points are near-ties" % (what, 100.0 * share)
    near(d, rd, 2e-6 * s, what + " dist")
    near(np.linalg.norm(q[clear] - rq[clear], axis=1), np.zeros(int(clear.sum())), 1e-5 * s, what + " proj")
    near(np.linalg.norm(pts - q, axis=1), d, 2e-6 * s, what + " |p - proj| against dist")
    assert f.min() >= 0 and f.max() < (case["faces"].shape[0] if max_face is None else max_face), what + ": face out of range"
    bad = np.nonzero(clear & (f != rf))[0]
    assert not len(bad), "%s: face differs at %d clear points, first %d: got %d, want %d (gap %.3e)" % (
        what, len(bad), bad[0], f[bad[0]], rf[bad[0]], gap[bad[0]])
    # faces that share a vertex tie at exactly 0 in float32 and in float64: the lowest index of them
    zero = (rd == 0.0) & (gap == 0.0) & (d == 0.0)
    bad = np.nonzero(zero & (f != rf))[0]
    assert not len(bad), "%s: at %d points on a shared vertex the face is not the lowest tied index, first %d: got %d, want %d" % (
        what, len(bad), bad[0], f[bad[0]], rf[bad[0]])


@pytest.mark.parametrize("name", MO.P2F_MESHES)
def test_point_to_mesh(dev, L, name):
    """paths: see the table; every mesh with every point count, pruned == brute == NULL boxes, then the float64 oracle."""
    case = MO.p2f_case(name)
    lay = Layout(dev, case["verts"], case["faces"])
    got = p2f_sets(L, dev, lay, case, "point_to_mesh " + name)
    p2f_check("point_to_mesh " + name, got, case)
    if case["favour"] is not None:
        decided = np.isin(case["face"], case["favour"]) & (case["gap"] > 1e-6 * case["scale"])
        assert decided.sum() >= 40, "only %d points are decided by an appended face" % decided.sum()


@pytest.mark.parametrize("swap", [False, True], ids=["copy_after", "copy_before"])
def test_point_to_mesh_exact_ties(dev, L, swap):
    """icosphere(2) with its face list twice: face i and face i + F0 are the same three float32 vertices in the same order, so their
    float32 d2 are equal bit for bit and only the face index decides.  copy_after: ids in list order, where the stable Morton sort
    puts i before i + F0 in the tiles.  copy_before: the two halves trade names (face_ids = (order + F0) mod 2 F0), so the entry
    that comes first in every tile carries the higher index."""
    base = MO.p2f_case(MO.P2F_DUP_BASE)
    v, f2 = MO.duplicated(base["verts"], base["faces"])
    F0 = base["faces"].shape[0]
    relabel = (np.arange(2 * F0) + F0) % (2 * F0) if swap else None
    what = "point_to_mesh duplicated (%s)" % ("copy first in the tiles" if swap else "copy second in the tiles")
    alone = p2f_sets(L, dev, Layout(dev, base["verts"], base["faces"]), base, "point_to_mesh " + MO.P2F_DUP_BASE)
    got = p2f_sets(L, dev, Layout(dev, v, f2, relabel), base, what)
    high = np.nonzero(got[2] >= F0)[0]
    assert not len(high), "%s: %d points report the copy (face >= %d), first %d -> %d" % (what, len(high), F0, high[0], got[2][high[0]])
    p2f_check(what, got, base, max_face=F0)
    for x, y, out in zip(got, alone, ("dist", "proj", "face")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), (
            "%s: %s differs in bits from the run on the mesh alone" % (what, out))


def test_point_to_mesh_refusals(dev, L):
    case = MO.p2f_case("ico2_65")
    lay = Layout(dev, case["verts"], case["faces"])
    pts = case["sets"][-1]
    gp = gin(dev, pts)
    dist, proj, face = gout(dev, 257, F32), gout(dev, 3 * 257, F32), gout(dev, 257, np.int32)

    def call(n=257, F=lay.F, tris=lay.tris.ptr(), fid=lay.ids.ptr(), flags=0):
        return run(L, dev, "dispu_point_to_mesh", n, gp.ptr(), F, tris, fid, lay.box.ptr(), dist.ptr(), proj.ptr(), face.ptr(), flags)

    assert call(n=-1) == INVALID and call(F=0) == INVALID and call(F=-3) == INVALID
    assert call(tris=None) == INVALID and call(fid=None) == INVALID
    assert call(flags=L.MESH_BRUTE_FORCE, n=-1) == INVALID and call(flags=L.MESH_BRUTE_FORCE, fid=None) == INVALID
    assert call(n=0) == 0 and call(n=0, flags=L.MESH_BRUTE_FORCE) == 0
    assert untouched(dist) and untouched(proj) and untouched(face)
    assert call() == 0 and not untouched(dist) and not untouched(proj) and not untouched(face)
    assert dist.guards_intact() and proj.guards_intact() and face.guards_intact() and unread(gp) and lay.unread()


# ------------------------------------------------------------------------------ dispu_disk_count, dispu_disk_fill ----
def disks_call(L, dev, seeds, points, radii, want):
    """count, offsets compared whole, then fill into a buffer of the ORACLE's size (never one sized by what the kernel counted).
    The points sit before 256 guard floats: 64 whole points of sentinel, as far as any lane of the last trip could read."""
    S, n, R = seeds.shape[0], points.shape[0], radii.shape[0]
    what = "disks S %d n %d R %d" % (S, n, R)
    gs, gp, gr = gin(dev, seeds), gin(dev, points, g=256), gin(dev, radii)
    off = gout(dev, S * R + 1, np.int64)
    ok(L, dev, "dispu_disk_count", S, n, R, gs.ptr(), gp.ptr(), gr.ptr(), off.ptr())
    assert off.guards_intact(), what + ": dispu_disk_count wrote outside offsets"
    exact_rows(as_(off, np.int64), None, want, what)
    total = sum(len(r) for r in want)
    mem = gout(dev, total, np.int32)
    before = as_(off, np.int64).copy()
    ok(L, dev, "dispu_disk_fill", S, n, R, gs.ptr(), gp.ptr(), gr.ptr(), off.ptr(), mem.ptr())
    assert mem.guards_intact() and off.guards_intact(), what + ": dispu_disk_fill wrote outside members"
    assert np.array_equal(as_(off, np.int64), before) and unread(gs) and unread(gp) and unread(gr)
    exact_rows(as_(off, np.int64), as_(mem, np.int32), want, what)


DISKS = [(1, 1, 1), (3, 63, 2), (5, 64, 1), (6, 65, 3), (7, 200, 2)]


@pytest.mark.parametrize("case", DISKS, ids=ids(DISKS))
def test_disks(dev, L, case):
    """paths: `i >= S` (S is never a multiple of the 4 waves), `q < n` in the last trip (n = 1, 63, 65, 200), n below, at and above one
    wave.  Radii: 1e5 (every row exactly 0 .. n - 1), r with a point exactly on it and one a float32 outside, 0 with a seed on a point."""
    S, n, R = case
    seeds, points, radii = MO.disk_case(S, n, R)
    want = MO.disk_members_fp32(seeds, points, radii)
    for i in range(S):
        assert np.array_equal(want[i * R], np.arange(n))                      # the 1e5 rows
    disks_call(L, dev, seeds, points, radii, want)


SCANS = [(1, 1), (341, 3), (1024, 1), (205, 5), (683, 3), (1000, 3)]          # S * R = 1, 1023, 1024, 1025, 2049, 3000


@pytest.mark.parametrize("case", SCANS, ids=ids(SCANS))
def test_disk_scan_sizes(dev, L, case):
    """disk_scan_kernel's 1024 threads over M = S R counts: M = 1 and 1023 (one entry each, idle threads), 1024 (full), 1025 (two
    each; the threads from 513 on start beyond M + 1), 2049 and 3000 (three each, the tail idle / the last thread short)."""
    S, R = case
    seeds, points, radii = MO.disk_case(S, 65, R)
    disks_call(L, dev, seeds, points, radii, MO.disk_members_fp32(seeds, points, radii))


def test_disks_empty_and_refusals(dev, L):
    seeds, points, radii = MO.disk_case(6, 65, 3)
    gs, gp, gr = gin(dev, seeds), gin(dev, points, g=256), gin(dev, radii)
    off, mem = gout(dev, 6 * 3 + 1, np.int64), gout(dev, 6 * 3 * 65, np.int32)

    def count(S=6, n=65, R=3):
        return run(L, dev, "dispu_disk_count", S, n, R, gs.ptr(), gp.ptr(), gr.ptr(), off.ptr())

    def fill(S=6, n=65, R=3):
        return run(L, dev, "dispu_disk_fill", S, n, R, gs.ptr(), gp.ptr(), gr.ptr(), off.ptr(), mem.ptr())

    for f in (count, fill):
        assert f(S=-1) == INVALID and f(n=0) == INVALID and f(n=-2) == INVALID and f(R=0) == INVALID and f(R=-1) == INVALID
    assert untouched(off) and untouched(mem)
    # S == 0: offsets[0] = 0 and nothing else
    assert count(S=0) == 0 and fill(S=0) == 0
    o = as_(off, np.int64)
    assert o[0] == 0 and (np.ascontiguousarray(off.body())[2:] == F32(SENT)).all() and off.guards_intact() and untouched(mem)
    assert count() == 0 and fill() == 0 and off.guards_intact() and mem.guards_intact()
    assert as_(off, np.int64)[-1] == sum(len(r) for r in MO.disk_members_fp32(seeds, points, radii))


# ---------------------------------------------------------- dispu_geodesic_disk_count, dispu_geodesic_disk_fill ----
def geodesic_call(L, dev, off, cand, dist, radii, what):
    S, R = off.shape[0] - 1, radii.shape[0]
    want = MO.geodesic_disk_members(off, cand, dist, radii)
    go, gc, gd, gr = gin(dev, off), gin(dev, cand), gin(dev, dist), gin(dev, radii)
    out = gout(dev, S * R + 1, np.int64)
    ok(L, dev, "dispu_geodesic_disk_count", S, R, go.ptr(), gd.ptr(), gr.ptr(), out.ptr())
    assert out.guards_intact(), what + ": dispu_geodesic_disk_count wrote outside offsets"
    exact_rows(as_(out, np.int64), None, want, what)
    mem = gout(dev, sum(len(r) for r in want), np.int32)
    ok(L, dev, "dispu_geodesic_disk_fill", S, R, go.ptr(), gc.ptr(), gd.ptr(), gr.ptr(), out.ptr(), mem.ptr())
    assert mem.guards_intact() and out.guards_intact(), what + ": dispu_geodesic_disk_fill wrote outside members"
    assert unread(go) and unread(gc) and unread(gd) and unread(gr)
    exact_rows(as_(out, np.int64), as_(mem, np.int32), want, what)
    return want


GEO_ORDERS = {"empty_first": (0, 1, 63, 64, 65, 200), "empty_middle": (65, 200, 1, 0, 64, 63), "empty_last": (200, 64, 1, 65, 63, 0)}
GEO = [(R, o) for R in (1, 3) for o in sorted(GEO_ORDERS)]


@pytest.mark.parametrize("case", GEO, ids=ids(GEO))
def test_geodesic_disks(dev, L, case):
    """paths: `i >= S` (S = 6 in two workgroups of 4 waves), `c < e` in rows of 0, 1, 63, 65 and 200 candidates, an empty row (no trip of
    the loop) first, in the middle and last; distances +inf, 0, exactly (double)radii[j] (a member) and the next double (not one)."""
    R, order = case
    radii = np.array([0.25, 0.1, 0.4], np.float32)[:R]
    lengths = GEO_ORDERS[order]
    off, cand, dist = MO.geodesic_case(lengths, radii, seed=R)
    want = geodesic_call(L, dev, off, cand, dist, radii, "geodesic disks R %d %s" % (R, order))
    # the at-the-radius candidates are members, the ones a double above are not (the inputs hold both in every row they fit in)
    for i, c in enumerate(lengths):
        if c >= 2:
            j = i % R
            row = want[i * R + j].tolist()
            assert int(cand[off[i]]) in row and int(cand[off[i] + 1]) not in row


def test_geodesic_disks_scan_1025(dev, L):
    """S R = 1025 through dispu_geodesic_disk_count: disk_scan_launch is the scan of dispu_disk_count (two entries per thread)."""
    lengths = [(7 * i) % 5 for i in range(205)]
    radii = np.array([0.25, 0.1, 0.4, 0.05, 0.3], np.float32)
    off, cand, dist = MO.geodesic_case(lengths, radii, seed=5)
    geodesic_call(L, dev, off, cand, dist, radii, "geodesic disks S 205 R 5")


def test_geodesic_disks_empty_and_refusals(dev, L):
    radii = np.array([0.25, 0.1, 0.4], np.float32)
    off, cand, dist = MO.geodesic_case(MO.GEO_ROWS, radii, seed=9)
    go, gc, gd, gr = gin(dev, off), gin(dev, cand), gin(dev, dist), gin(dev, radii)
    out, mem = gout(dev, 6 * 3 + 1, np.int64), gout(dev, 3 * int(off[-1]), np.int32)

    def count(S=6, R=3):
        return run(L, dev, "dispu_geodesic_disk_count", S, R, go.ptr(), gd.ptr(), gr.ptr(), out.ptr())

    def fill(S=6, R=3):
        return run(L, dev, "dispu_geodesic_disk_fill", S, R, go.ptr(), gc.ptr(), gd.ptr(), gr.ptr(), out.ptr(), mem.ptr())

    for f in (count, fill):
        assert f(S=-1) == INVALID and f(R=0) == INVALID and f(R=-1) == INVALID
    assert untouched(out) and untouched(mem)
    assert count(S=0) == 0 and fill(S=0) == 0
    assert as_(out, np.int64)[0] == 0 and (np.ascontiguousarray(out.body())[2:] == F32(SENT)).all() and out.guards_intact()
    assert untouched(mem)
    assert count() == 0 and fill() == 0 and out.guards_intact() and mem.guards_intact()


# -------------------------------------------------------------------------------------------- dispu_disk_uniformity ----
class Uniformity(object):
    """one hand-built CSR over MO.uniformity_points() in guarded buffers, with the scratch and the output."""

    def __init__(self, L, dev, S, N):
        self.S, self.R, self.N = S, 2, N
        self.pts = MO.uniformity_points()
        self.rows = MO.uniformity_rows(S, self.pts.shape[0])
        off = np.concatenate([[0], np.cumsum([len(r) for r in self.rows])]).astype(np.int64)
        mem = np.concatenate(self.rows).astype(np.int32)
        self.gp, self.go, self.gm = gin(dev, self.pts), gin(dev, off), gin(dev, mem)
        self.gr, self.gc = gin(dev, MO.UNI_RADII), gin(dev, MO.UNI_PCT)
        self.nbytes = L.lib().dispu_disk_uniformity_scratch_bytes(S, self.R)
        assert self.nbytes == S * self.R * 12                                   # S R doubles of term, then S R ints of kept
        self.scratch, self.out = gout(dev, S * self.R * 3, F32), gout(dev, self.R, np.float64)

    def call(self, L, dev, **kw):
        a = dict(S=self.S, R=self.R, n=self.pts.shape[0], N=self.N, scratch=self.scratch.ptr(), nbytes=self.nbytes)
        a.update(kw)
        return run(L, dev, "dispu_disk_uniformity", a["S"], a["R"], a["n"], self.gp.ptr(), self.go.ptr(), self.gm.ptr(), self.gr.ptr(),
                   self.gc.ptr(), a["N"], a["scratch"], a["nbytes"], self.out.ptr())

    def results(self):
        M = self.S * self.R
        raw = np.ascontiguousarray(self.scratch.body())
        return raw[:2 * M].view(np.float64).copy(), raw[2 * M:].view(np.int32).copy(), as_(self.out, np.float64).copy()

    def intact(self):
        return (self.scratch.guards_intact() and self.out.guards_intact() and unread(self.gp) and unread(self.go) and unread(self.gm)
                and unread(self.gr) and unread(self.gc))


UNI = [(S, N) for S in (1, 63, 65, 130) for N in (1100, 8192)]


@pytest.mark.parametrize("case", UNI, ids=ids(UNI))
def test_disk_uniformity(dev, L, case):
    """paths: c < 5 (0, 4) / c = 5, 6; one trip of 256 members (255, 256), a second (257: one member in it); one LDS tile (1024), a
    second of one member (1025); disk_uniformity_mean_kernel at S < 64, S = 65 and 130 (a second and third trip of its lanes), kept
    and skipped disks alternating along the seeds, and a radius without any kept disk (S = 65, radius 1) -> NaN."""
    S, N = case
    u = Uniformity(L, dev, S, N)
    kept, term, mean = MO.uniform_terms(u.rows, MO.UNI_RADII, u.pts, MO.UNI_PCT, N)
    assert u.call(L, dev) == 0 and u.intact()
    t1, k1, o1 = u.results()
    what = "disk_uniformity S %d N %d" % (S, N)
    assert np.array_equal(k1, kept), "%s: kept differs at disks %s" % (what, np.nonzero(k1 != kept)[0][:8])
    c = np.array([len(r) for r in u.rows], np.float64)
    skipped = kept == 0
    assert (t1[skipped] == 0.0).all(), what + ": a skipped disk has a term"
    tb = (c + 8.0) * U52 * np.abs(term)
    for size in sorted(set(c[~skipped].astype(int))):
        sel = c == size
        near(t1[sel], term[sel], tb[sel], "%s term of the %d-member disks" % (what, size))
    for j in range(u.R):
        sel = np.nonzero(kept[j::u.R])[0] * u.R + j
        if not sel.size:
            assert np.isnan(o1[j]) and np.isnan(mean[j]), "%s: out[%d] = %r without a kept disk" % (what, j, o1[j])
            continue
        bound = (S + 8.0) * U52 * abs(mean[j]) + tb[sel].sum() / sel.size
        near(o1[j:j + 1], mean[j:j + 1], bound, "%s out[%d] over %d kept disks" % (what, j, sel.size))
    if S == 65:
        assert np.isnan(o1[1])
    # run to run: bit-identical, scratch included
    u.scratch.t.fill_(SENT)
    u.out.t.fill_(SENT)
    assert u.call(L, dev) == 0 and u.intact()
    t2, k2, o2 = u.results()
    assert np.array_equal(t1.view(np.uint64), t2.view(np.uint64)) and np.array_equal(k1, k2)
    assert np.array_equal(o1.view(np.uint64), o2.view(np.uint64))


def test_disk_uniformity_refusals(dev, L):
    u = Uniformity(L, dev, 63, 1100)
    assert L.lib().dispu_disk_uniformity_scratch_bytes(0, 2) == 0 and L.lib().dispu_disk_uniformity_scratch_bytes(63, 0) == 0
    assert u.call(L, dev, nbytes=u.nbytes - 1) == INVALID and u.call(L, dev, scratch=None) == INVALID
    for name in ("S", "R", "n", "N"):
        assert u.call(L, dev, **{name: 0}) == INVALID and u.call(L, dev, **{name: -1}) == INVALID, name
    assert untouched(u.scratch) and untouched(u.out) and u.intact()
    assert u.call(L, dev, nbytes=u.nbytes + 5) == 0 and not untouched(u.scratch) and not untouched(u.out) and u.intact()
