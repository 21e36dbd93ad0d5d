"""CPU tests of tests/loss_oracle.py: the explicit-index float64 formulas the GPU tests of the loss kernels rest on
(tests/test_train_loss_gpu.py) are held to autograd of the project's training oracle (oracle/train_oracle.py: chamfer, repulsion,
pu_loss) at 1e-12, and the helpers around them to hand-built cases.  No kernel runs here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_oracle as LO  # noqa: E402

from oracle import oracle as O  # noqa: E402
from oracle import train_oracle as T  # noqa: E402

F64 = torch.float64
SHAPES = [(3, 100, 300), (2, 1024, 1024), (17, 64, 33)]


def rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("B,n_gt,n_pred", SHAPES)
@pytest.mark.parametrize("coef", [1000.0, 10.0])
def test_chamfer_matches_autograd(B, n_gt, n_pred, coef):
    gt, pred = LO.jittered_pair(B, n_gt, n_pred, seed=B + n_gt)
    radius = np.random.default_rng(B).uniform(0.5, 2.0, B).astype(np.float32)
    i_gt, i_pred = LO.nearest(gt, pred)["idx"], LO.nearest(pred, gt)["idx"]
    value, dpred = LO.chamfer_value_grad(gt, pred, i_gt, i_pred, radius, coef)
    pt = torch.tensor(pred, dtype=F64, requires_grad=True)
    v = T.chamfer(pt, torch.tensor(gt, dtype=F64), torch.tensor(radius, dtype=F64))
    (coef * v).backward()
    assert abs(value - float(v.detach())) <= 1e-12 * abs(float(v.detach()))
    assert np.abs(pt.grad.numpy()).max() > 0
    assert rel(dpred, pt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("B,M", [(3, 100), (2, 1024), (17, 64), (1, 5)])
def test_repulsion_matches_autograd(B, M):
    _, pred = LO.jittered_pair(B, M, M, seed=M)
    if M < 1024:
        pred = (pred * (M / 1024.0) ** 0.5).astype(np.float32)    # keep the density of a 1024-point patch: the 0.07 balls are not all empty
    idx, cnt = O.query_ball_point(0.07, 20, pred, pred)
    scale = 1.0 / (B * M * 4)
    out, dpred = LO.repulsion_value_grad(pred, idx, 0.001, scale)
    pt = torch.tensor(pred, dtype=F64, requires_grad=True)
    v = T.repulsion(pt)
    v.backward()
    assert abs(out.sum() * scale - float(v.detach())) <= 1e-12 * abs(float(v.detach()))
    assert np.abs(pt.grad.numpy()).max() > 0 and (cnt > 1).any()
    assert rel(dpred, pt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("epoch", [0, 15, 25, 35])
@pytest.mark.parametrize("use_repulse,rep_w", [(True, 1.0), (True, 0.5), (False, 1.0)])
def test_pu_loss_terms_match_the_oracle(epoch, use_repulse, rep_w):
    B, n = 3, 256
    gt, fine = LO.jittered_pair(B, n, n, seed=11)
    _, coarse = LO.jittered_pair(B, n, n, seed=11, sigma=0.05)
    radius = np.array([1.0, 1.3, 0.7], np.float32)
    total, terms = T.pu_loss(torch.tensor(coarse, dtype=F64), torch.tensor(fine, dtype=F64), torch.tensor(gt, dtype=F64), radius,
                             epoch=epoch, repulsion_w=rep_w, use_repulse=use_repulse)
    cd = [LO.chamfer_value_grad(gt, p, LO.nearest(gt, p)["idx"], LO.nearest(p, gt)["idx"], radius, 1.0)[0] for p in (coarse, fine)]
    rep = None
    if use_repulse:
        idx, _ = O.query_ball_point(0.07, 20, fine, fine)
        rep = LO.repulsion_value_grad(fine, idx, 0.001, 1.0)[0]
    got = LO.pu_loss_terms(cd[0], cd[1], rep, B * n, T.weight_fine(epoch), rep_w)
    want = [float(terms["dis_coarse_cd"]), float(terms["dis_fine_cd"]), float(terms["repulsion_loss"]), float(total), T.weight_fine(epoch)]
    assert got[4] == {0: 0.01, 15: 0.1, 25: 0.5, 35: 1.0}[epoch]
    if use_repulse:
        assert got[2] > 0
    else:
        assert got[2] == 0.0
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1e-300), (got, want)


def test_chamfer_by_hand():
    """one cloud, two gt points, three pred points, indices that are NOT the arg-mins: the formulas hold for any indices."""
    gt = np.array([[[0, 0, 0], [1, 0, 0]]], np.float32)
    pred = np.array([[[0, 1, 0], [2, 0, 0], [0, 0, 3]]], np.float32)
    i_gt, i_pred = np.array([[2, 2]]), np.array([[0, 1, 1]])
    value, dpred = LO.chamfer_value_grad(gt, pred, i_gt, i_pred, np.array([2.0], np.float32), 10.0)
    # gt -> pred: |(0,0,-3)|^2 = 9, |(1,0,-3)|^2 = 10; pred -> gt: 1, 1, |(-1,0,3)|^2 = 10
    assert value == ((9 + 10) / 2 + (1 + 1 + 10) / 3) / 2.0
    want = 2 * 10.0 * np.array([[0, 1, 0], [1, 0, 0], [-1, 0, 3]], np.float64) / (2.0 * 3 * 1)
    want[2] += -2 * 10.0 * (np.array([0, 0, -3.0]) + np.array([1, 0, -3.0])) / (2.0 * 2 * 1)
    assert np.allclose(dpred[0], want, rtol=1e-15, atol=0)


def test_repulsion_by_hand():
    """three points on a line, ns = 6: the dropped first slot, a repeated neighbour and an inactive hinge."""
    pred = np.array([[[0, 0, 0], [0.01, 0, 0], [0.5, 0, 0]]], np.float32)
    p = pred.astype(np.float64)
    idx = np.array([[[0, 1, 1, 1, 1, 1], [0, 1, 2, 0, 0, 2], [2, 2, 2, 2, 2, 2]]])
    h = 0.001
    out, dpred = LO.repulsion_value_grad(pred, idx, h, 1.0)
    d01 = (p[0, 1, 0] - p[0, 0, 0]) ** 2
    # point 0: sorted d = 0 (self, dropped), then point 1 four times; point 1: self dropped, then point 0 three times and point 2
    # (d = 0.49^2 > h: nothing); point 2: all slots are itself
    assert np.allclose(out[0], [4 * (h - d01), 3 * (h - d01), 4 * h], rtol=1e-15)
    e = p[0, 1] - p[0, 0]
    want = np.zeros((3, 3))
    want[0] += 4 * 2 * e
    want[1] -= 4 * 2 * e
    want[1] += 3 * 2 * (-e)
    want[0] -= 3 * 2 * (-e)
    assert np.allclose(dpred[0], want, rtol=1e-15, atol=0) and not dpred[0, 2].any()
    ties = LO.near_ties(pred, idx=idx, h=h)
    assert ties["first"][0, 0] == 1.0 and np.isinf(ties["first"][0, 2]) and np.isinf(ties["fifth"][0, 0])
    assert np.allclose(ties["hinge"][0, 2], 1.0) and np.allclose(ties["hinge"][0, 0], (h - d01) / h)
    assert np.isinf(ties["fifth"][0, 1])                           # point 1: its 5th and 6th sorted slots both hold point 2


def test_nearest_and_near_ties():
    a = np.array([[[0, 0, 0], [1, 0, 0], [5, 5, 5]]], np.float32)
    b = np.array([[[0, 0, 1], [0, 0, -1], [1, 0, 2]]], np.float32)
    nn = LO.nearest(a, b)
    assert nn["idx"].tolist() == [[0, 0, 2]]                      # lowest index on the exact tie of row 0
    assert nn["best"].tolist() == [[1.0, 2.0, 50.0]] and nn["second"][0, 0] == 1.0 and nn["second_idx"][0, 0] == 1
    gap = LO.near_ties(a, b)
    assert gap[0, 0] == 0.0 and gap[0, 1] == 0.0 and 0 < gap[0, 2] < 1
    assert np.isinf(LO.near_ties(a, b[:, :1])).all()
    assert np.array_equal(LO.sq_dist_to(a, b, nn["idx"]), nn["best"])


def test_jittered_pair_shapes():
    for B, n_gt, n_pred in [(1, 1, 1), (3, 300, 100), (2, 513, 4096), (5, 8, 5)]:
        gt, pred = LO.jittered_pair(B, n_gt, n_pred, seed=1)
        assert gt.shape == (B, n_gt, 3) and pred.shape == (B, n_pred, 3) and gt.dtype == pred.dtype == np.float32
        assert np.isfinite(gt).all() and np.isfinite(pred).all()
        # pred stays near gt: every pred point within a few sigma of some gt point
        assert LO.nearest(pred, gt)["best"].max() <= 3 * (6 * 0.02) ** 2
