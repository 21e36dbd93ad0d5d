"""CPU tests of tests/icp_oracle.py alone: the conditions the GPU tests of dispu_icp_segments rest on.  The oracle recovers a known motion
on the cap to fp32 resolution in both modes, its first-step normal equations are as well conditioned as the GPU tests' bound on T
assumes, it flags every degenerate case with pivots far from the threshold, and its apply is the stated arithmetic."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_oracle as O  # noqa: E402


def test_clouds_are_the_stated_ones():
    p, nrm, src, truth = O.cap()
    assert p.shape == (3091, 3) and src.shape == (1546, 3) and p.dtype == src.dtype == nrm.dtype == np.float32
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    fp, fn, fs, _ = O.far()
    assert fp.shape == (2049, 3) and fs.shape == (1025, 3)
    assert abs(float((fp.max(axis=0) - fp.min(axis=0)).max()) - 0.02) < 1e-3 and np.abs(fp).max() > 999
    M = O.motion(p)                                                             # a proper rigid motion of 10 degrees
    assert np.allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-15) and abs(np.trace(M[:3, :3]) - (1 + 2 * np.cos(np.deg2rad(10)))) < 1e-14


def test_match_is_rank_0_of_the_mls_oracle():
    """the correspondences are mls_oracle.neighbors at k = 1, ties included: the lattice (every distance tied many times over), 40
    coincident points, and the cap under its motion"""
    import mls_oracle as MO
    import normals_oracle as NO
    r = np.random.RandomState(0)
    dup = r.random_sample((1040, 3)).astype(np.float32)
    dup[r.permutation(1040)[:40]] = np.float32([0.25, 0.5, 0.75])
    p, _, src, _ = O.cap()
    half = (NO.lattice(9)[::3] + np.float32(0.5)).astype(np.float32)            # cell centres: eight lattice points at one distance
    for q, t in ((half, NO.lattice(9)), (NO.sphere(300), dup), (dup[:300], dup), (src[:400], p)):
        idx, d2, inlier = O.match(q, t, 0.3)
        want_i, want_d = MO.neighbors(q, t, 1)
        assert idx.dtype == np.int32 and np.array_equal(idx, want_i[:, 0]) and d2.tobytes() == want_d[:, 0].tobytes()
        assert np.array_equal(inlier, want_d[:, 0] <= np.float32(0.3))
    assert len(set(O.match(half, NO.lattice(9))[1])) == 1                       # the ties are there


def test_point_mode_recovers_the_motion_on_cap():
    _, _, _, truth = O.cap()
    r = O.recovery(False)
    err = np.abs(r["aligned"].astype(np.float64) - truth).max()
    print("point mode, 40 iterations: rmse %.3g, max |aligned - truth| %.3g" % (r["rmse"], err))
    assert r["flag"] == 0 and r["iters"] == 40 and r["inliers"] == 1546
    assert r["rmse"] <= 2e-7 and err <= 1e-6


def test_plane_mode_recovers_the_motion_on_cap_within_five_iterations():
    p, nrm, src, truth = O.cap()
    r = O.recovery(True)
    five = O.evaluate(r["steps"][4]["T"], src, p, normals=nrm)
    err = np.abs(five["aligned"].astype(np.float64) - truth).max()
    print("plane mode, 5 iterations: rmse %.3g, max |aligned - truth| %.3g" % (five["rmse"], err))
    assert five["rmse"] <= 2e-7 and err <= 1e-6
    assert r["rmse"] <= 2e-7 and np.abs(r["aligned"].astype(np.float64) - truth).max() <= 1e-6


def test_first_step_is_well_conditioned():
    """the bound of the GPU tests on T is summation error times cond(A).  Point to point on far is the case measured when the bound was
    set (6.6e4); point to plane on far, with the analytic normals used here, has cond 2.5e5: the GPU bound takes whatever the oracle
    reports, so that case is printed, not held to 1e5"""
    conds = {(n, pl): O.first_step(n, pl)["cond"] for n in ("cap", "far") for pl in (False, True)}
    print({k: "%.3g" % v for k, v in conds.items()})
    assert conds[("cap", False)] <= 1e2 and conds[("cap", True)] <= 1e2
    assert conds[("far", False)] <= 1e5
    assert np.isfinite(conds[("far", True)])
    for n in ("cap", "far"):
        for pl in (False, True):
            s = O.first_step(n, pl)
            assert not s["degenerate"] and s["ratio"].min() > 1e-3              # nine orders above the pivot rule


def test_every_degenerate_case_is_flagged_far_from_the_threshold():
    for src, tgt, nrm, max_distance, why in O.degenerate_cases():
        init = O.motion(tgt) if len(tgt) > 1 else O.identity()
        for T0 in (O.identity(), init):
            s = O.step(T0, src, tgt, nrm, O.max_d2_of(max_distance))
            assert s["degenerate"] and np.array_equal(s["T"], T0), why
            if s["count"] >= (3 if nrm is None else 6):                         # flagged by a pivot: an exact zero, not a near miss
                bad = ~(s["ratio"] > O.PIVOT)
                first = int(np.argmax(bad))
                assert bad.any() and (s["ratio"][:first] > 1e-3).all(), why
                assert s["A"][first, first] == 0.0, why
        r = O.icp(src, tgt, nrm, max_distance=max_distance, iterations=3)
        assert r["flag"] == 2 and r["iters"] == 0 and np.array_equal(r["T"], O.identity()), why
    t, _, s = O.coplanar()                                                      # the same pair point to point is an ordinary problem
    st = O.step(O.identity(), s, t)
    assert not st["degenerate"] and st["ratio"].min() > 1e-2


def test_apply_by_hand():
    T = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float64)     # 90 degrees about z, then (1, 2, 3)
    pts = np.float32([[1, 0, 0], [0, 1, 0], [0.5, 0.25, -2]])
    assert np.array_equal(O.apply(T, pts), np.float32([[1, 3, 3], [0, 2, 3], [0.75, 2.5, 1]]))
    assert O.apply(O.identity(), pts).tobytes() == pts.tobytes()
    R = O.rodrigues(np.array([0, 0, np.pi / 2]))
    assert np.abs(R - T[:3, :3]).max() < 1e-15
    assert np.array_equal(O.rodrigues(np.zeros(3)), np.eye(3))
    assert O.max_d2_of(0.1) == np.float32(0.1 * 0.1) and O.max_d2_of(np.inf) == np.float32(np.inf)
