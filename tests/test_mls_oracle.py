"""CPU tests that hold tests/mls_oracle.py, the yardstick of the MLS projection, to facts that need no GPU: a plane is a fixed surface,
every stay rule fires on the input made for it, and the operator denoises (the figures of the two denoising cases are printed)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mls_oracle as M  # noqa: E402


def plane(n, seed):
    xy = np.random.RandomState(seed).random_sample((n, 2))
    return np.concatenate([xy, np.zeros((n, 1))], axis=1).astype(np.float32)


def test_points_on_a_clean_plane_do_not_move():
    refs = plane(2000, 0)
    q = plane(300, 1) * np.float32(0.8) + np.float32([0.1, 0.1, 0.0])           # inside the sheet
    for k, support in ((16, 1.0), (16, 1.5), (4, 2.0), (32, 1.0)):
        res = M.step(q, refs, k, support)
        assert res["ok"].all()
        assert np.abs(res["new64"] - q.astype(np.float64)).max() <= 1e-12
        assert np.array_equal(res["new32"].view(np.uint32), q.view(np.uint32))


def test_lifted_points_land_on_the_plane():
    refs = plane(2000, 0)
    q = plane(300, 1) * np.float32(0.8) + np.float32([0.1, 0.1, 0.0])
    q[:, 2] = (0.05 * np.random.RandomState(2).standard_normal(300)).astype(np.float32)
    res = M.step(q, refs, 16, 1.5)
    assert res["ok"].all()
    assert np.abs(res["new64"][:, 2]).max() <= 1e-12                            # onto z = 0 ...
    assert np.abs(res["new64"][:, :2] - q[:, :2].astype(np.float64)).max() <= 1e-12   # ... straight down
    self_res = M.step(refs, refs, 16, 1.0)                                      # the plane against itself
    assert np.array_equal(self_res["new32"].view(np.uint32), refs.view(np.uint32))


def test_every_stay_rule():
    for q, r, support, why in M.stay_cases():
        for k in (4, 16):
            res = M.step(q, r, k, support)
            assert not res["ok"].any(), why
            assert np.array_equal(res["new32"].view(np.uint32), q.view(np.uint32)), why
            assert np.array_equal(res["new64"], q.astype(np.float64)), why
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    res = M.step(np.float32([[0.2, 0.3, 0.5]]), tri, 4, 2.0)                    # the same three points at support 2: a plane, z = 0
    assert res["ok"].all() and np.abs(res["new64"] - np.float32([[0.2, 0.3, 0.0]]).astype(np.float64)).max() <= 1e-12
    assert np.array_equal(res["idx"], np.int32([[0, 2, 1, -1]]))                # (0, 1, 0) is nearer to (0.2, 0.3) than (1, 0, 0)


def test_iterations_are_chained_steps():
    p = M.denoise_self()[:500]
    three = M.project(p, p, 16, 1.5, iterations=3)
    cur = p
    for _ in range(3):
        cur = M.step(cur, p, 16, 1.5)["new32"]
    assert np.array_equal(three["new32"].view(np.uint32), cur.view(np.uint32))


def test_denoising_a_noisy_sphere():
    p = M.denoise_self()
    res = M.step(p, p, 16, 1.5)
    before, after = M.radial_rms(p), M.radial_rms(res["new64"])
    print("self: radial RMS %.4f -> %.4f" % (before, after))
    assert after < 0.5 * before
    assert M.radial_rms(res["new32"]) < 0.5 * before


def test_denoising_across_clouds():
    q, r = M.denoise_cross()
    res = M.step(q, r, 16, 1.0)
    before, after = M.radial_rms(q), M.radial_rms(res["new64"])
    print("cross: radial RMS %.4f -> %.4f" % (before, after))
    assert after < 0.25 * before
    assert M.radial_rms(res["new32"]) < 0.25 * before
