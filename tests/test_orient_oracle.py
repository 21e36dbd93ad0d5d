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


# ---- the deep hook trees and the model of the pointer jump's launches ------------------------------------------------------------------
def hooked_chain(name):
    """(depth of the forest round one hooks, launches the model needs to flatten it, rounds) of a DEEP case"""
    p, nrm, nbr = O.case(name)
    launches = []
    out = O.orient_rounds(p, nrm, nbr, 0, launches=launches)
    assert out["n_components"] == 1 and len(launches) == out["rounds"] == 1
    return launches[0] + (out,)


@pytest.mark.parametrize("name", O.DEEP)
def test_deep_chains_both_programs_and_the_jump_model_agree(name):
    """Kruskal, the rounds with pointer doubling and the rounds with the launch model give the same flips; the chain is as deep as the
    case claims"""
    p, nrm, nbr = O.case(name)
    n = len(p)
    E = O.Edges(nrm, nbr)
    depth, used, modelled = hooked_chain(name)
    assert depth == (n - 1 if name.startswith("path_") else n - 2)
    for vote in (0, 1):
        want = O.expected(name, vote)
        assert same(O.orient_rounds(p, nrm, nbr, vote, E=E), want), (name, vote)
    assert same(modelled, O.expected(name, 0))
    assert 0.4 * n < O.expected(name, 0)["flip"].sum() < 0.6 * n + 2               # the parities are live: about half the normals turn
    if name.startswith("path_"):
        assert not E.wbits.any()                                    # every weight exactly 0
    else:                                                           # the fp32 weight bits strictly decrease along the line
        assert np.array_equal(E.lo[np.lexsort((E.hi, E.lo))] + 1, E.hi[np.lexsort((E.hi, E.lo))])
        assert (np.diff(E.wbits[np.lexsort((E.hi, E.lo))].astype(np.int64)) < 0).all()


def test_jump_model_launch_counts():
    """A launch of the model follows 64 links from the parent, so it flattens depth 65 and leaves depth d at ceil(d / 65): a chain of n
    points hooks to depth n - 1, so 66 points need one launch and 67 two (one size below where a count of n - 2 would put it), 4228
    three, 274628 four.  65^4 > 2^24: no tree of 2^24 nodes needs a fifth."""
    assert (O.JUMP_ITERS, O.JUMP_LAUNCHES) == (64, 4)
    step = O.JUMP_ITERS + 1
    for n, want in ((66, 1), (67, 2), (68, 2), (step ** 2 + 1, 2), (step ** 2 + 2, 3), (4228, 3), (step ** 3 + 1, 3), (step ** 3 + 2, 4),
                    (274628, 4)):
        depth, used, _ = hooked_chain("path_%d" % n)
        assert (depth, used) == (n - 1, want) and O.launches_for_depth(depth) == want, n
    assert hooked_chain("rising_4300")[:2] == (4298, 3)
    # one launch on a chain: depth d -> ceil(d / 65), and short exactly when some d > 65
    for n in (60, 66, 67, 4228):
        parent = np.maximum(np.arange(n) - 1, 0)
        par = np.random.RandomState(n).randint(0, 2, n).astype(np.uint8)
        par[0] = 0
        p1, q1, short = O.jump_launch(parent, par)
        d = np.arange(n)
        assert np.array_equal(p1, np.maximum(d - step, 0)) and short == (n - 1 > step)
        assert np.array_equal(O.depths(p1), -(-d // step))
        to_root = np.bitwise_xor.accumulate(par)                    # parity of node i to the root
        assert np.array_equal(q1, to_root ^ to_root[p1])            # the composed parity is the parity to the new parent
    # any tree's deepest node sees only its own chain of ancestors, so the chain is the worst tree of its depth
    assert O.launches_for_depth((1 << 24) - 1) == 4 and O.launches_for_depth(step ** 4) == 4 and O.launches_for_depth(step ** 4 + 1) == 5
    assert step ** O.JUMP_LAUNCHES > 1 << 24


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
