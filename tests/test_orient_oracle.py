"""CPU tests of tests/orient_oracle.py, the yardstick of dispu_orient_consistent_segments: the emulated parallel rounds against the
sequential Kruskal on every case of the GPU tests, Kruskal against an independent Prim, and what the propagation is for -- outward
normals on a torus, where no pointwise hint can give them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_oracle as NO  # noqa: E402
import orient_oracle as O  # noqa: E402


def same(a, b):
    return (np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["component"], b["component"])
            and a["n_components"] == b["n_components"] and np.array_equal(a["normal"].view(np.uint32), b["normal"].view(np.uint32))
            and np.array_equal(a["tree"], b["tree"]))


@pytest.mark.parametrize("name", O.CASES)
def test_rounds_equal_kruskal(name):
    p, nrm, nbr = O.case(name)
    E = O.Edges(nrm, nbr)
    for vote in (0, 1):
        want = O.expected(name, vote)
        got = O.orient_rounds(p, nrm, nbr, vote, E=E)
        assert same(got, want), (name, vote)
    assert got["rounds"] <= max(1, int(np.ceil(np.log2(max(len(p), 2)))))


def prim(E):
    """the minimum spanning forest by Prim from every unvisited node, with the same strict order -> [m] bool"""
    import heapq
    adj = [[] for _ in range(E.n)]
    for e, (a, b) in enumerate(zip(E.lo.tolist(), E.hi.tolist())):
        adj[a].append((e, b))                                       # e is the edge's position in key order
        adj[b].append((e, a))
    seen = np.zeros(E.n, bool)
    tree = np.zeros(len(E.lo), bool)
    for start in range(E.n):
        if seen[start]:
            continue
        seen[start] = True
        heap = list(adj[start])
        heapq.heapify(heap)
        while heap:
            e, y = heapq.heappop(heap)
            if seen[y]:
                continue
            seen[y] = True
            tree[e] = True
            for item in adj[y]:
                heapq.heappush(heap, item)
    return tree


@pytest.mark.parametrize("name", [c for c in O.CASES if c.startswith("small_") and int(c.split("_")[1][1:]) <= 200])
def test_kruskal_equals_prim(name):
    _, nrm, nbr = O.case(name)
    E = O.Edges(nrm, nbr)
    assert np.array_equal(O.kruskal(E), prim(E))


def test_kruskal_equals_prim_with_ties_and_components():
    rs = np.random.RandomState(5)
    p = np.concatenate([rs.random_sample((90, 3)), rs.random_sample((90, 3)) + 50]).astype(np.float32)
    nrm = np.zeros((180, 3), np.float32)
    nrm[:, 2] = np.where(rs.random_sample(180) < 0.5, -1, 1)        # every weight 0: (lo, hi) alone decides
    E = O.Edges(nrm, NO.neighbors(p, 6))
    tree = O.kruskal(E)
    assert np.array_equal(tree, prim(E)) and tree.sum() == 178


@pytest.mark.parametrize("n,k", [(1024, 8), (2048, 12), (4096, 16)])
def test_torus_is_oriented_outwards(n, k):
    """PCA normals with the canonical sign, then the propagation: every normal agrees with the analytic one.  ('centroid' alone
    reaches 71 % here: the inner half of the tube faces the centroid.)"""
    p, true = O.torus(n, seed=n)
    ref = NO.normals(p, k)
    out = O.orient(p, ref["normal"], ref["idx"], vote=0)
    assert out["n_components"] == 1
    assert ((out["normal"].astype(np.float64) * true).sum(axis=1) > 0).all()
    d = p.astype(np.float64) - p.astype(np.float64).mean(axis=0)
    centroid = NO.orient_sign(ref["normal"], d)
    assert ((centroid.astype(np.float64) * true).sum(axis=1) > 0).mean() < 0.8
    rounds = O.orient_rounds(p, ref["normal"], ref["idx"], vote=0)
    assert same(rounds, out)


def test_two_spheres_are_two_components_all_outwards():
    p, true = O.two_spheres()
    ref = NO.normals(p, 10)
    out = O.orient(p, ref["normal"], ref["idx"], vote=0)
    assert out["n_components"] == 2
    assert set(out["component"].tolist()) == {0, 1500}
    assert ((out["normal"].astype(np.float64) * true).sum(axis=1) > 0).all()
    assert same(O.orient_rounds(p, ref["normal"], ref["idx"], vote=0), out)


def test_lattice_plane_with_random_signs_comes_out_plus_z():
    p, nrm, nbr = O.case("lattice_plane")
    E = O.Edges(nrm, nbr)
    assert not E.wbits.any()                                        # every weight ties at exactly 0
    for fn in (O.orient, O.orient_rounds):
        out = fn(p, nrm, nbr, vote=0)
        assert out["n_components"] == 1
        assert np.array_equal(out["normal"], np.tile(np.float32([0, 0, 1]), (len(p), 1)))
        assert np.array_equal(out["flip"], (nrm[:, 2] < 0).astype(np.uint8))


def test_majority_vote_keeps_the_prior_direction():
    """a sphere oriented outwards with one point in five flipped: the vote mends the flipped ones and keeps 'outwards'; vote 0 depends on
    the anchor alone"""
    p = NO.sphere(800, seed=21)
    nrm = p.copy()
    bad = np.random.RandomState(22).permutation(800)[:160]
    nrm[bad] *= -1
    out = O.orient(p, nrm, NO.neighbors(p, 8), vote=1)
    assert np.array_equal(out["normal"], p) and np.array_equal(np.nonzero(out["flip"])[0], np.sort(bad))
    inward = O.orient(p, -p, NO.neighbors(p, 8), vote=1)            # consistent already: nothing flips, whatever the anchor says
    assert not inward["flip"].any()
    assert O.orient(p, -p, NO.neighbors(p, 8), vote=0)["flip"].all()   # the anchor (the top) points down: vote 0 turns all
