"""The trainer's loss and glue kernels, each ALONE against float64 (tests/loss_oracle.py, numpy with explicit indices), then the
trainer's loss head isolated from the generator.

Entries under test (csrc/train_fused.hip, csrc/train_ops.hip): dispu_chamfer_loss_grad, dispu_repulsion_loss_grad,
dispu_pu_loss_finalize, dispu_transpose_batched, dispu_sigmoid_offset(_grad), dispu_dup_sum_grad, dispu_add3.  The end-to-end step of
tests/test_train_gpu.py visits them at one shape (B = 2, 1024/1024 points, epoch 0) behind a generator whose fp32 branch flips force
loose bounds; here every kernel gets its own inputs at the shapes where its loops, tails, offsets and scale factors can go wrong.

Bounds:
  * values and gradients of single kernels: 1e-5 of the largest entry of the float64 reference (the bound tests/test_train_gpu.py
    states for every backward kernel alone); loss scalars 1e-5 relative;
  * copy / integer kernels (transpose_batched, add3), sentinels and guard regions: bit-exact;
  * where the DEVICE picks indices (nn_distance in front of the Chamfer kernel, the trainer's loss head) each device arg-min index
    must be a float64 arg-min or within 1e-5 relative of one (fp32 squared distances are good to a few 1e-7), and the gradient
    reference is built on the device's indices, so no row is left out of a Chamfer comparison; the loss head's ball-query slots must
    EQUAL the host oracle's (same fp32 arithmetic).  For the repulsion term of the loss head a row may be left out of the GRADIENT
    comparison only when a float64 gap of the REFERENCE that decides its top-k / hinge branch is below 1e-5 relative
    (tests/loss_oracle.py:near_ties), at most 0.1 % of the rows of a tensor, asserted; values are never left out.
Every comparison prints its measured error next to its bound (pytest -s shows them).

Measured on an MI355X (worst case of each group, relative as above; bound 1e-5 unless exact):
  chamfer_loss_grad alone   value 6.4e-7 (1030 x 8 x 5; 1.2e-7 at 64 x 1024 x 1024), dpred 1.4e-7 (64 x 1024 x 1024), 1.9e-7 with
                            1024 atomics on one row, 9.3e-8 at random indices
  nn_distance + chamfer     value 6.3e-8, dpred 1.3e-7; 0 of 65536 + 65536 device indices differ from the float64 arg-min at B = 64;
                            rows left out: 0
  repulsion_loss_grad       per shape in test_repulsion_loss_grad; hand-built cases exact
  pu_loss_finalize          9.7e-8 over nrep x weight_fine x repulsion_w
  sigmoid_offset / _grad    8.6e-8 / 9.9e-8;  dup_sum_grad 1.6e-7;  transpose_batched, add3: bit-exact
  loss head                 terms 1.7e-7, dcoarse 4.1e-7, dfine 5.5e-7; ball-query slots equal to the oracle's in every case; rows of
                            dfine left out: 9 of 65536 at B = 64 (three rows whose 5th and 6th nearest slots tie inside the hinge,
                            and the two points each of them chooses between), 0 everywhere else"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_oracle as LO  # noqa: E402

from oracle import generator as OG  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 1                     # hipErrorInvalidValue
H, BALL, NS = 0.001, 0.07, 20    # get_repulsion_loss: hinge width, ball radius, slots (loss_utils.py:271-298)
TIE = 1e-5                      # the near-tie margin
SENT = -12345.0                 # guard value around output buffers

_KEEP = []     # device tensors created inline in a launch's argument list must outlive the launch


def dv(a, dev, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del _KEEP[:]


def p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def N_(t):
    return t.detach().cpu().numpy()


def close(a, ref, rel, what=""):
    ref = np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(np.asarray(a, np.float64) - ref).max()
    print("[measured] %s: max err %.3e of scale %.3e = %.2e (bound %.0e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e > %.0e)" % (what, err, scale, err / scale, rel)


def scalar_close(a, ref, rel, what=""):
    err = abs(float(a) - float(ref))
    print("[measured] %s: %.9g vs %.9g, rel err %.2e (bound %.0e)" % (what, float(a), float(ref), err / max(abs(float(ref)), 1e-300), rel))
    assert err <= rel * abs(float(ref)), "%s: %.9g vs %.9g" % (what, float(a), float(ref))


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


class Guarded(object):
    """a device float buffer of `n` elements with `g` guard elements of SENT on either side; `fill` goes into the body."""

    def __init__(self, dev, n, fill=SENT, g=64):
        self.n, self.g = n, g
        self.t = torch.full((n + 2 * g,), SENT, dtype=torch.float32, device=dev)
        if isinstance(fill, np.ndarray):
            self.t[g:g + n] = torch.from_numpy(np.ascontiguousarray(fill, F32).reshape(-1)).to(dev)
        else:
            self.t[g:g + n] = fill
        _KEEP.append(self.t)

    def ptr(self):
        return p(self.t, self.g)

    def body(self):
        return N_(self.t[self.g:self.g + self.n])

    def guards_intact(self):
        a = N_(self.t)
        return bool((a[:self.g] == F32(SENT)).all() and (a[self.g + self.n:] == F32(SENT)).all())


# ------------------------------------------------------------------------------------------ host-side inputs ----
@functools.lru_cache(maxsize=None)
def pair(B, n_gt, n_pred, seed):
    return LO.jittered_pair(B, n_gt, n_pred, seed)


@functools.lru_cache(maxsize=None)
def host_nn(B, n_gt, n_pred, seed):
    gt, pred = pair(B, n_gt, n_pred, seed)
    return LO.nearest(gt, pred), LO.nearest(pred, gt)


def radii(B, seed):
    return np.random.default_rng(1000 + seed).uniform(0.5, 2.0, B).astype(F32)


def repulsion_cloud(B, M, seed):
    """the `pred` of jittered_pair at the point density of a 1024-point patch (smaller clouds are shrunk: at the patch's own scale
    their 0.07 balls would all be empty and the gradient identically zero); the five-point cloud a little further (x 0.8), until some of
    its points are closer than sqrt(h) and their hinges active while most balls still hold fewer than 5 points."""
    _, pred = pair(B, M, M, seed)
    return pred if M >= 1024 else (pred * (M / 1024.0) ** 0.5 * (0.8 if M < NS else 1.0)).astype(F32)


def grid_cloud(B, spacing):
    """B clouds of 4 x 4 x 4 = 64 points on a cubic grid (cloud b shifted by b): every pair is at least `spacing` apart."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(64, 3).astype(np.float64) * spacing
    return np.stack([g - 1.5 * spacing + 0.01 * b for b in range(B)]).astype(F32)


# ------------------------------------------------------------------------------- dispu_chamfer_loss_grad alone ----
def run_chamfer(dev, L, gt, pred, d_gt, i_gt, d_pred, i_pred, radius, coef):
    """-> (value float32, dpred [B, n_pred, 3]).  dpred starts as a sentinel (the entry zero-fills it) between guards; value sits in
    the middle of a sentinel array."""
    B, n_gt, n_pred = gt.shape[0], gt.shape[1], pred.shape[1]
    val = Guarded(dev, 1, g=4)
    dp = Guarded(dev, B * n_pred * 3, fill=777.0)
    L.check(L.lib().dispu_chamfer_loss_grad(B, n_gt, p(dv(gt, dev)), n_pred, p(dv(pred, dev)), p(dv(d_gt, dev)), p(dv(i_gt, dev, torch.int32)),
                                            p(dv(d_pred, dev)), p(dv(i_pred, dev, torch.int32)), p(dv(radius, dev)), coef, val.ptr(), dp.ptr(),
                                            L.stream_ptr(dev)), "chamfer_loss_grad")
    torch.cuda.synchronize()
    assert val.guards_intact(), "chamfer_loss_grad wrote around value[0]"
    assert dp.guards_intact(), "chamfer_loss_grad wrote around dpred"
    return val.body()[0], dp.body().reshape(B, n_pred, 3)


CD_SHAPES = [(1, 1, 1), (2, 1024, 1024), (3, 100, 300), (3, 300, 100), (2, 513, 4096), (16, 64, 64), (17, 64, 33), (64, 1024, 1024),
             (1030, 8, 5)]
CD_COEFS = [1000.0, 10.0, 1000.0 * 0.5]


@pytest.mark.parametrize("case", range(len(CD_SHAPES)), ids=["%dx%dx%d" % s for s in CD_SHAPES])
def test_chamfer_loss_grad(dev, L, case):
    """value and gradient for host-side float64 arg-mins (distances rounded to fp32): the kernel isolated from nn_distance.  B = 64
    is four trips of the value kernel's clouds loop per wave, 17 a ragged last trip, 1030 a second pass over the 1024 LDS slots;
    100 / 300 / 513 / 33 / 5 leave tails in its 8 x 64 unroll; n_gt != n_pred in both orders."""
    B, n_gt, n_pred = CD_SHAPES[case]
    coef = CD_COEFS[case % 3]
    gt, pred = pair(B, n_gt, n_pred, 20 + case)
    a, b = host_nn(B, n_gt, n_pred, 20 + case)
    radius = radii(B, case)
    value, dpred = run_chamfer(dev, L, gt, pred, a["best"].astype(F32), a["idx"], b["best"].astype(F32), b["idx"], radius, coef)
    ref_v, ref_d = LO.chamfer_value_grad(gt, pred, a["idx"], b["idx"], radius, coef)
    scalar_close(value, ref_v, 1e-5, "chamfer value %s" % (CD_SHAPES[case],))
    close(dpred, ref_d, 1e-5, "chamfer dpred %s coef %g" % (CD_SHAPES[case], coef))


def test_chamfer_loss_grad_all_gt_points_pull_one_row(dev, L):
    """every gt point's nearest pred point is row 0: 1024 atomics on one address per cloud and coordinate."""
    B, n = 2, 1024
    gt, pred = pair(B, n, n, 3)
    pred = pred.copy()
    pred[:, 1:, 0] += 10.0                       # every other pred point is far away ...
    pred[:, 0] = (0.0, 0.0, -1.0)                # ... and row 0 sits off-centre, so that the 1024 pulls add up instead of cancelling
    a, b = LO.nearest(gt, pred), LO.nearest(pred, gt)
    assert not a["idx"].any()
    radius = radii(B, 77)
    value, dpred = run_chamfer(dev, L, gt, pred, a["best"].astype(F32), a["idx"], b["best"].astype(F32), b["idx"], radius, 1000.0)
    ref_v, ref_d = LO.chamfer_value_grad(gt, pred, a["idx"], b["idx"], radius, 1000.0)
    assert np.abs(ref_d[:, 0]).max() == np.abs(ref_d).max()          # the contended row carries the largest entries
    scalar_close(value, ref_v, 1e-5, "chamfer value, one row")
    close(dpred, ref_d, 1e-5, "chamfer dpred, one row")
    close(dpred[:, 0], ref_d[:, 0], 1e-5, "chamfer dpred, the contended row")


def test_chamfer_loss_grad_any_indices(dev, L):
    """the entry differentiates at the indices it is GIVEN (arbitrary in-range rows, not arg-mins), n_gt != n_pred."""
    B, n_gt, n_pred = 3, 200, 77
    gt, pred = pair(B, n_gt, n_pred, 5)
    rng = np.random.default_rng(5)
    i_gt = rng.integers(0, n_pred, (B, n_gt)).astype(np.int32)
    i_pred = rng.integers(0, n_gt, (B, n_pred)).astype(np.int32)
    d_gt, d_pred = LO.sq_dist_to(gt, pred, i_gt).astype(F32), LO.sq_dist_to(pred, gt, i_pred).astype(F32)
    radius = radii(B, 5)
    value, dpred = run_chamfer(dev, L, gt, pred, d_gt, i_gt, d_pred, i_pred, radius, 10.0)
    ref_v, ref_d = LO.chamfer_value_grad(gt, pred, i_gt, i_pred, radius, 10.0)
    scalar_close(value, ref_v, 1e-5, "chamfer value, random indices")
    close(dpred, ref_d, 1e-5, "chamfer dpred, random indices")


# --------------------------------------------------- dispu_nn_distance + dispu_chamfer_loss_grad, as Trainer._chamfer ----
def check_device_argmin(a, b, i_dev, what):
    """every device index of a's points into b: in range, and a float64 arg-min or within TIE of one.  -> number of near-tie rows"""
    nn = LO.nearest(a, b)
    i_dev = np.asarray(i_dev)
    assert i_dev.min() >= 0 and i_dev.max() < b.shape[1], what
    d_dev = LO.sq_dist_to(a, b, i_dev)
    differ = i_dev != nn["idx"]
    assert (d_dev <= nn["best"] * (1.0 + TIE)).all(), "%s: %d device indices are not arg-mins" % (what, int((d_dev > nn["best"] * (1.0 + TIE)).sum()))
    ties = int((LO.rel_gap(nn["best"], nn["second"]) < TIE).sum())
    print("[measured] %s: %d of %d device indices differ from the float64 arg-min, %d rows with a gap below %.0e"
          % (what, int(differ.sum()), differ.size, ties, TIE))
    return nn, ties


@pytest.mark.parametrize("B,n", [(4, 1024), (64, 1024)])
def test_nn_distance_then_chamfer_loss_grad(dev, L, B, n):
    gt, pred = pair(B, n, n, 31)
    radius = radii(B, 31)
    coef = 1000.0 * 0.1
    tg, tp = dv(gt, dev), dv(pred, dev)
    d_gt, d_pred = torch.empty((B, n), dtype=torch.float32, device=dev), torch.empty((B, n), dtype=torch.float32, device=dev)
    i_gt, i_pred = torch.empty((B, n), dtype=torch.int32, device=dev), torch.empty((B, n), dtype=torch.int32, device=dev)
    val = Guarded(dev, 1, g=4)
    dp = Guarded(dev, B * n * 3, fill=777.0)
    st = L.stream_ptr(dev)
    L.check(L.lib().dispu_nn_distance(B, n, p(tg), n, p(tp), p(d_gt), p(i_gt), p(d_pred), p(i_pred), L.ARITH_CONTRACT, st), "nn_distance")
    L.check(L.lib().dispu_chamfer_loss_grad(B, n, p(tg), n, p(tp), p(d_gt), p(i_gt), p(d_pred), p(i_pred), p(dv(radius, dev)), coef, val.ptr(),
                                            dp.ptr(), st), "chamfer_loss_grad")
    torch.cuda.synchronize()
    assert val.guards_intact() and dp.guards_intact()
    ig, ip = N_(i_gt), N_(i_pred)
    a, _ = check_device_argmin(gt, pred, ig, "gt -> pred")
    b, _ = check_device_argmin(pred, gt, ip, "pred -> gt")
    ref_v, _ = LO.chamfer_value_grad(gt, pred, a["idx"], b["idx"], radius, coef)        # the value is continuous across ties
    scalar_close(val.body()[0], ref_v, 1e-5, "chained chamfer value B=%d" % B)
    _, ref_d = LO.chamfer_value_grad(gt, pred, ig, ip, radius, coef)
    close(dp.body().reshape(B, n, 3), ref_d, 1e-5, "chained chamfer dpred B=%d (no row left out)" % B)


# ------------------------------------------------------------------------------------- dispu_repulsion_loss_grad ----
def run_repulsion(dev, L, pred, idx, scale, prefill=None):
    B, M = pred.shape[0], pred.shape[1]
    out = Guarded(dev, B * M)
    dp = Guarded(dev, B * M * 3, fill=0.0 if prefill is None else prefill)
    L.check(L.lib().dispu_repulsion_loss_grad(B * M, M, NS, H, scale, p(dv(pred, dev)), p(dv(idx, dev, torch.int32)), out.ptr(), dp.ptr(),
                                              L.stream_ptr(dev)), "repulsion_loss_grad")
    torch.cuda.synchronize()
    assert out.guards_intact() and dp.guards_intact()
    return out.body().reshape(B, M), dp.body().reshape(B, M, 3)


REP_TOL = 1e-5       # the differences p_j - p_i of close fp32 points are exact (Sterbenz): nothing is lost where the points are close


@pytest.mark.parametrize("B,M", [(2, 1024), (3, 100), (1, 5), (64, 1024)])
def test_repulsion_loss_grad(dev, L, B, M):
    """value and gradient for the host oracle's ball-query slots; the gradient into zeros and on top of a prefill; and the replaced
    pair dispu_repulsion / dispu_repulsion_grad as a cross-check (out bit for bit, dpred to atomics order).
    Measured worst gradient error on an MI355X, of the largest reference entry (bound 1e-5): 2 x 1024: 6.5e-8, 3 x 100: 9.8e-8,
    1 x 5: 2.0e-8, 64 x 1024: 1.5e-7; onto a prefill: 1.3e-7, 1.4e-7, 3.6e-8, 1.6e-7; out: at most 1.5e-7 of 4h; against
    dispu_repulsion_grad: at most 1.5e-7."""
    pred = repulsion_cloud(B, M, 40 + M)
    idx, cnt = O.query_ball_point(BALL, NS, pred, pred)
    padded = float((cnt < 5).mean())
    print("[measured] repulsion %dx%d: %.1f %% of the balls hold fewer than 5 points" % (B, M, 100 * padded))
    assert padded >= 0.25, "the padded-slot path is not exercised"
    scale = 1.0 / (B * M * 4.0)
    ref_out, ref_d = LO.repulsion_value_grad(pred, idx, H, scale)
    assert np.abs(ref_d).max() > 0
    out, dpred = run_repulsion(dev, L, pred, idx, scale)
    close(out, ref_out, 1e-5, "repulsion out %dx%d" % (B, M))
    close(dpred, ref_d, REP_TOL, "repulsion dpred %dx%d" % (B, M))
    pre = (np.random.default_rng(M).standard_normal((B, M, 3)) * np.abs(ref_d).max()).astype(F32)
    out2, dpred2 = run_repulsion(dev, L, pred, idx, scale, prefill=pre)
    assert np.array_equal(out2, out)
    close(dpred2, pre.astype(np.float64) + ref_d, REP_TOL, "repulsion prefill + dpred %dx%d" % (B, M))
    # the older two launches
    tp, ti = dv(pred, dev), dv(idx, dev, torch.int32)
    o1 = torch.empty(B * M, dtype=torch.float32, device=dev)
    g1 = torch.zeros((B * M, 3), dtype=torch.float32, device=dev)
    st = L.stream_ptr(dev)
    L.check(L.lib().dispu_repulsion(B * M, M, NS, 0, H, p(tp), p(ti), p(o1), st), "repulsion")
    L.check(L.lib().dispu_repulsion_grad(B * M, M, NS, H, scale, p(tp), p(ti), p(g1), st), "repulsion_grad")
    torch.cuda.synchronize()
    assert np.array_equal(N_(o1).reshape(B, M), out), "out differs from dispu_repulsion's"
    close(dpred, N_(g1).reshape(B, M, 3).astype(np.float64), 1e-6, "repulsion dpred against dispu_repulsion_grad %dx%d" % (B, M))


def _four_h():
    h = F32(H)
    return ((h + h) + h) + h


def test_repulsion_coincident_points(dev, L):
    """a cloud of coincident points: every d = 0, out = 4h, gradient exactly 0."""
    pred = np.tile(np.array([0.3, -0.2, 0.1], F32), (2, 64, 1))
    idx, cnt = O.query_ball_point(BALL, NS, pred, pred)
    assert (cnt == NS).all()
    out, dpred = run_repulsion(dev, L, pred, idx, 1.0 / (2 * 64 * 4))
    assert _four_h() == F32(4) * F32(H)
    assert (out == _four_h()).all() and not dpred.any()
    ref_out, ref_d = LO.repulsion_value_grad(pred, idx, H, 1.0)
    assert not ref_d.any() and np.allclose(ref_out, 4 * H, rtol=1e-15)


def test_repulsion_isolated_points(dev, L):
    """spacing above the ball radius: every ball holds only its own point, all 20 slots are the point itself: out = 4h (what the
    reference computes for an isolated point), gradient exactly 0."""
    pred = grid_cloud(2, 0.1)
    idx, cnt = O.query_ball_point(BALL, NS, pred, pred)
    assert (cnt == 1).all() and (idx == np.arange(64)[None, :, None]).all()
    out, dpred = run_repulsion(dev, L, pred, idx, 1.0 / (2 * 64 * 4))
    assert (out == _four_h()).all() and not dpred.any()
    ref_out, ref_d = LO.repulsion_value_grad(pred, idx, H, 1.0)
    assert not ref_d.any() and np.allclose(ref_out, 4 * H, rtol=1e-15)


def test_repulsion_distinct_far_slots(dev, L):
    """hand-built slots: 20 distinct points, all farther than sqrt(h): out exactly 0, dpred keeps its prefill bit for bit."""
    pred = grid_cloud(2, 0.1)                                        # 0.1 > sqrt(0.001) = 0.0316
    idx = ((np.arange(64)[:, None] + 1 + np.arange(NS)[None, :]) % 64).astype(np.int32)[None].repeat(2, 0)
    assert (idx != np.arange(64)[None, :, None]).all()
    pre = np.random.default_rng(1).standard_normal((2, 64, 3)).astype(F32)
    out, dpred = run_repulsion(dev, L, pred, idx, 1.0, prefill=pre)
    assert not out.any()
    assert np.array_equal(dpred.view(np.uint32), pre.view(np.uint32))
    ref_out, ref_d = LO.repulsion_value_grad(pred, idx, H, 1.0)
    assert not ref_out.any() and not ref_d.any()


def test_repulsion_one_neighbour_in_every_slot(dev, L):
    """hand-built slots: one neighbour closer than sqrt(h) repeated 20 times: its term counts four times in out and in both rows'
    gradients, as the gather in the reference does."""
    pred = grid_cloud(2, 0.1).astype(np.float64)
    pred[:, 1::2] = pred[:, 0::2] + np.array([0.006, -0.008, 0.0])          # partners 0.01 apart, pairs 0.1 apart (rows 2k, 2k+1)
    pred = pred.astype(F32)
    idx = (np.arange(64) ^ 1).astype(np.int32)[None, :, None].repeat(2, 0).repeat(NS, 2)
    scale = 1.0 / (2 * 64 * 4)
    ref_out, ref_d = LO.repulsion_value_grad(pred, idx, H, scale)
    d = ((pred[:, 1::2].astype(np.float64) - pred[:, 0::2].astype(np.float64)) ** 2).sum(-1)
    assert np.allclose(ref_out[:, 0::2], 4 * (H - d), rtol=1e-12) and np.allclose(ref_out[:, 1::2], 4 * (H - d), rtol=1e-12)
    e = pred[:, 1::2].astype(np.float64) - pred[:, 0::2].astype(np.float64)
    assert np.allclose(ref_d[:, 0::2], 2 * 4 * 2 * scale * e, rtol=1e-12)          # four from its own slots, four from the partner's
    out, dpred = run_repulsion(dev, L, pred, idx, scale)
    close(out, ref_out, 1e-5, "repulsion out, one neighbour x 20")
    close(dpred, ref_d, REP_TOL, "repulsion dpred, one neighbour x 20")


def test_repulsion_exact_tie_keeps_the_earlier_slot(dev, L):
    """six DIFFERENT neighbours at exactly the same distance (+-0.01 along the axes: the same fp32 and float64 square for each) in
    slots 1..6 behind the point itself: tf.nn.top_k puts the lower index first among equals, so slots 1..4 carry the terms and slots
    5, 6 none.  An unstable selection sends the gradient to other rows."""
    M = 7
    pred = np.zeros((1, M, 3), F32)
    for k in range(6):
        pred[0, 1 + k, k // 2] = F32(0.01) * (1 if k % 2 == 0 else -1)
    idx = np.tile(np.arange(M, dtype=np.int32)[None, :, None], (1, 1, NS))         # rows 1..6: every slot is the point itself
    idx[0, 0] = [0, 1, 2, 3, 4, 5, 6] + [1] * (NS - 7)                              # padded like a ball query: the first hit repeats
    scale = 0.25
    ref_out, ref_d = LO.repulsion_value_grad(pred, idx, H, scale)
    d = float(F32(0.01)) ** 2
    assert np.isclose(ref_out[0, 0], 4 * (H - d), rtol=1e-12) and not ref_d[0, 5:].any() and ref_d[0, 1:5].any(-1).all()
    assert np.allclose(ref_d[0, 1, 0], -2 * scale * float(F32(0.01)), rtol=1e-12)
    out, dpred = run_repulsion(dev, L, pred, idx, scale)
    close(out, ref_out, 1e-5, "repulsion out, six-way tie")
    close(dpred, ref_d, REP_TOL, "repulsion dpred, six-way tie")
    assert not dpred[0, 5:].any(), "a slot behind its equals received a gradient"


# ---------------------------------------------------------------------------------------- dispu_pu_loss_finalize ----
WFS = [0.01, 0.1, 0.5, 1.0]


def run_finalize(dev, L, cd, rep, nrep, wf, rep_w):
    """as the trainer calls it: cd = loss_vals[0:2], out = loss_vals + 2 (loss_vals has 8 floats; here guards follow)."""
    lv = Guarded(dev, 8, g=8)
    lv.t[lv.g:lv.g + 2] = torch.from_numpy(np.asarray(cd, F32)).to(dev)
    L.check(L.lib().dispu_pu_loss_finalize(lv.ptr(), p(rep) if rep is not None else None, nrep, wf, rep_w, p(lv.t, lv.g + 2),
                                           L.stream_ptr(dev)), "pu_loss_finalize")
    torch.cuda.synchronize()
    body = lv.body()
    assert lv.guards_intact() and body[7] == F32(SENT), "pu_loss_finalize wrote past out[4]"
    assert np.array_equal(body[:2], np.asarray(cd, F32)), "cd[0..1] did not survive the aliased call"
    return body[2:7]


@pytest.mark.parametrize("nrep", [1, 63, 1024, 1025, 65536])
def test_pu_loss_finalize(dev, L, nrep):
    rng = np.random.default_rng(nrep)
    rep = rng.uniform(0.0, 4 * H, nrep).astype(F32)
    more = np.concatenate([rep, np.full(64, 1e6, F32)])              # anything read past nrep would show
    t = dv(more, dev)
    for k, wf in enumerate(WFS):
        for rep_w in (1.0, 0.5, 0.0):
            cd = rng.uniform(1e-3, 5e-2, 2).astype(F32)
            out = run_finalize(dev, L, cd, t, nrep, wf, rep_w)
            ref = LO.pu_loss_terms(cd[0], cd[1], rep, nrep, F32(wf), F32(rep_w))
            for j in range(4):
                scalar_close(out[j], ref[j], 1e-5, "pu_loss out[%d] nrep=%d wf=%g rep_w=%g" % (j, nrep, wf, rep_w))
            assert out[4] == F32(wf)
            if rep_w == 0.0:
                assert out[2] == 0.0


@pytest.mark.parametrize("wf", WFS)
def test_pu_loss_finalize_without_repulsion(dev, L, wf):
    """rep = NULL: out[2] exactly 0 and out[3] = out[0] + wf * out[1] in fp32 (as two roundings or as one fused multiply-add)."""
    cd = np.array([0.0123, 0.00456], F32)
    out = run_finalize(dev, L, cd, None, 0, wf, 1.0)
    assert out[2] == 0.0 and not np.signbit(out[2])
    assert out[0] == F32(1000) * cd[0] and out[1] == F32(1000) * cd[1] and out[4] == F32(wf)
    two = out[0] + F32(wf) * out[1]
    fused = F32(float(out[0]) + float(F32(wf)) * float(out[1]))
    assert out[3] == two or out[3] == fused, (out[3], two, fused)
    ref = LO.pu_loss_terms(cd[0], cd[1], None, 0, F32(wf), 1.0)
    scalar_close(out[3], ref[3], 1e-5, "pu_loss without repulsion wf=%g" % wf)


# ---------------------------------------------------------------------------------------- dispu_transpose_batched ----
T_SHAPES = [(1, 1), (3, 64), (31, 33), (32, 32), (134, 24), (256, 2048), (2048, 256), (480, 128)]


def test_transpose_batched(dev, L):
    """one launch over eight matrices packed at non-zero offsets with gaps: bit-exact against numpy.transpose, the gaps of dst
    untouched.  256 x 2048 is 512 tiles on 64 workgroups (the stride loop), 31 x 33 / 3 x 64 / 134 x 24 have ragged tiles."""
    rng = np.random.default_rng(12)
    desc, off = [], 5
    for k, (K, Nn) in enumerate(T_SHAPES):
        desc.append((off, K, Nn))
        off += K * Nn + (3, 7, 1, 64, 13, 2, 33, 9)[k]
    total = off
    src = rng.standard_normal(total).astype(F32)
    want = np.full(total, SENT, F32)
    for o, K, Nn in desc:
        want[o:o + K * Nn] = src[o:o + K * Nn].reshape(K, Nn).T.reshape(-1)
    dst = Guarded(dev, total)
    ts, td = dv(src, dev), dv(np.array(desc, np.int32), dev, torch.int32)
    st = L.stream_ptr(dev)
    assert L.lib().dispu_transpose_batched(0, p(td), p(ts), dst.ptr(), st) == 0
    torch.cuda.synchronize()
    assert (dst.body() == F32(SENT)).all(), "count = 0 wrote something"
    L.check(L.lib().dispu_transpose_batched(len(desc), p(td), p(ts), dst.ptr(), st), "transpose_batched")
    torch.cuda.synchronize()
    got = dst.body()
    for o, K, Nn in desc:
        assert np.array_equal(got[o:o + K * Nn].view(np.uint32), want[o:o + K * Nn].view(np.uint32)), "W^T of the %d x %d matrix" % (K, Nn)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "a gap between the matrices was written"
    assert dst.guards_intact() and np.array_equal(N_(ts), src)
    # a sub-range of the descriptors (the pointer may start anywhere in the table)
    dst2 = Guarded(dev, total)
    L.check(L.lib().dispu_transpose_batched(2, p(td, 3 * 4), p(ts), dst2.ptr(), st), "transpose_batched")
    torch.cuda.synchronize()
    want2 = np.full(total, SENT, F32)
    for o, K, Nn in desc[4:6]:
        want2[o:o + K * Nn] = want[o:o + K * Nn]
    assert np.array_equal(dst2.body().view(np.uint32), want2.view(np.uint32))


# ------------------------------------------------------------------------------- dispu_sigmoid_offset / _grad ----
Z_SPECIAL = [0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]


def sigmoid64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def test_sigmoid_offset_and_grad(dev, L):
    rng = np.random.default_rng(21)
    z = np.concatenate([rng.standard_normal(1000) * 3, Z_SPECIAL]).astype(F32)
    total = z.size
    assert total % 256 != 0
    base = rng.uniform(-1, 1, total).astype(F32)
    g = rng.standard_normal(total).astype(F32)
    g[1000:] = rng.uniform(1.0, 2.0, len(Z_SPECIAL)) * np.where(np.arange(len(Z_SPECIAL)) % 2, 1, -1)   # no small factor hides a bad dz
    s = sigmoid64(z)
    st = L.stream_ptr(dev)
    tz, tb, tg = dv(z, dev), dv(base, dev), dv(g, dev)
    out = Guarded(dev, total)
    L.check(L.lib().dispu_sigmoid_offset(total, p(tz), p(tb), out.ptr(), st), "sigmoid_offset")
    off0 = Guarded(dev, total)
    L.check(L.lib().dispu_sigmoid_offset(total, p(tz), p(dv(np.zeros(total, F32), dev)), off0.ptr(), st), "sigmoid_offset")
    torch.cuda.synchronize()
    assert out.guards_intact() and off0.guards_intact()
    assert np.isfinite(out.body()).all() and np.isfinite(off0.body()).all()
    close(out.body(), base.astype(np.float64) + (s - 0.5), 1e-5, "sigmoid_offset")
    close(off0.body(), s - 0.5, 1e-5, "sigmoid_offset, base = 0")
    assert off0.body().min() >= -0.5 and off0.body().max() <= 0.5, "the offset left [-0.5, 0.5]"
    # gradient: dz = dout s (1 - s); without dbase, then accumulating onto a prefilled dbase
    ref_dz = g.astype(np.float64) * s * (1.0 - s)
    dz = Guarded(dev, total)
    L.check(L.lib().dispu_sigmoid_offset_grad(total, p(tz), p(tg), dz.ptr(), None, st), "sigmoid_offset_grad")
    torch.cuda.synchronize()
    assert dz.guards_intact() and np.isfinite(dz.body()).all()
    assert np.array_equal(N_(tz), z) and np.array_equal(N_(tg), g) and np.array_equal(N_(tb), base)      # nothing else was written
    close(dz.body(), ref_dz, 1e-5, "sigmoid_offset_grad dz")
    # fp32 s is exactly 1 once exp(-z) < 2^-25 (z > 17.4) and exactly 0 once exp(-z) overflows (z < -88.8): dz must be 0 there
    sat = (z >= 20.0) | (z <= -89.0)
    assert sat.sum() == 8 and not dz.body()[sat].any(), dz.body()[sat]
    pre = rng.standard_normal(total).astype(F32)
    dz2, db = Guarded(dev, total), Guarded(dev, total, fill=pre)
    L.check(L.lib().dispu_sigmoid_offset_grad(total, p(tz), p(tg), dz2.ptr(), db.ptr(), st), "sigmoid_offset_grad")
    torch.cuda.synchronize()
    assert dz2.guards_intact() and db.guards_intact()
    assert np.array_equal(dz2.body(), dz.body())
    assert np.array_equal(db.body(), pre + g), "dbase != prefill + dout"


# ------------------------------------------------------------------------------------------- dispu_dup_sum_grad ----
@pytest.mark.parametrize("nclouds,n", [(1, 1), (3, 100), (8, 256)])
@pytest.mark.parametrize("up", [1, 2, 4, 16])
def test_dup_sum_grad(dev, L, nclouds, n, up):
    """dH[cloud, i] = sum_r dZ[(cloud * up + r) * n + i] (copy-major), strided rows on both sides."""
    for co in (1, 24, 256):
        rng = np.random.default_rng(nclouds * 1000 + up * 10 + co)
        lddz, lddh = co + 3, co + 5
        dZ = rng.standard_normal((nclouds * up * n, lddz)).astype(F32)
        ref = dZ.reshape(nclouds, up, n, lddz)[..., :co].astype(np.float64).sum(1).reshape(nclouds * n, co)
        dH = Guarded(dev, nclouds * n * lddh)
        L.check(L.lib().dispu_dup_sum_grad(nclouds, n, co, up, p(dv(dZ, dev)), lddz, dH.ptr(), lddh, L.stream_ptr(dev)), "dup_sum_grad")
        torch.cuda.synchronize()
        got = dH.body().reshape(nclouds * n, lddh)
        assert dH.guards_intact() and (got[:, co:] == F32(SENT)).all(), "dup_sum_grad wrote outside its columns"
        close(got[:, :co], ref, 1e-5, "dup_sum_grad %dx%d up=%d co=%d" % (nclouds, n, up, co))


# --------------------------------------------------------------------------------------------------- dispu_add3 ----
@pytest.mark.parametrize("total", [1, 255, 256 * 37 + 11])
def test_add3(dev, L, total):
    """out = (a + b) + c, the kernel's association, bit for bit; also in place over a (generator.py calls it so)."""
    rng = np.random.default_rng(total)
    a, b, c = (rng.standard_normal(total).astype(F32) * s for s in (1.0, 1e-3, 1e3))
    want = (a + b) + c
    ta, tb, tc = dv(a, dev), dv(b, dev), dv(c, dev)
    out = Guarded(dev, total)
    st = L.stream_ptr(dev)
    L.check(L.lib().dispu_add3(total, p(ta), p(tb), p(tc), out.ptr(), st), "add3")
    torch.cuda.synchronize()
    assert out.guards_intact() and np.array_equal(out.body().view(np.uint32), want.view(np.uint32))
    ia = Guarded(dev, total, fill=a)
    L.check(L.lib().dispu_add3(total, ia.ptr(), p(tb), p(tc), ia.ptr(), st), "add3")
    torch.cuda.synchronize()
    assert ia.guards_intact() and np.array_equal(ia.body().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(N_(tb), b) and np.array_equal(N_(tc), c)


# -------------------------------------------------------------------------------------------- argument refusals ----
def test_wrappers_refuse_invalid_arguments(dev, L):
    """only arguments a wrapper refuses BEFORE launching; every pointer that is passed is a real buffer of sufficient size."""
    lib, st = L.lib(), L.stream_ptr(dev)
    f = torch.full((4096,), SENT, dtype=torch.float32, device=dev)
    i = torch.zeros((4096,), dtype=torch.int32, device=dev)
    _KEEP.extend([f, i])
    F, I = p(f), p(i)

    def chamfer(b=2, n_gt=8, n_pred=8, gt=F, pred=F, d_gt=F, i_gt=I, d_pred=F, i_pred=I, radius=F, value=F, dpred=F):
        return lib.dispu_chamfer_loss_grad(b, n_gt, gt, n_pred, pred, d_gt, i_gt, d_pred, i_pred, radius, 1.0, value, dpred, st)

    for kw in (dict(b=0), dict(b=-1), dict(n_gt=0), dict(n_pred=0), dict(n_gt=-3), dict(gt=None), dict(pred=None), dict(d_gt=None),
               dict(i_gt=None), dict(d_pred=None), dict(i_pred=None), dict(radius=None), dict(value=None), dict(dpred=None)):
        assert chamfer(**kw) == INVALID, kw

    def repulsion(rows=8, n=8, ns=NS, pred=F, idx=I, out=F, dpred=F):
        return lib.dispu_repulsion_loss_grad(rows, n, ns, H, 1.0, pred, idx, out, dpred, st)

    for kw in (dict(rows=-1), dict(n=0), dict(n=-8), dict(ns=19), dict(ns=21), dict(ns=5), dict(ns=0), dict(pred=None), dict(idx=None),
               dict(out=None), dict(dpred=None)):
        assert repulsion(**kw) == INVALID, kw
    assert repulsion(rows=0) == 0

    assert lib.dispu_pu_loss_finalize(None, None, 0, 0.5, 1.0, F, st) == INVALID
    assert lib.dispu_pu_loss_finalize(F, None, 0, 0.5, 1.0, None, st) == INVALID
    assert lib.dispu_pu_loss_finalize(F, F, 0, 0.5, 1.0, p(f, 8), st) == INVALID
    assert lib.dispu_pu_loss_finalize(F, F, -5, 0.5, 1.0, p(f, 8), st) == INVALID

    assert lib.dispu_transpose_batched(-1, I, F, p(f, 2048), st) == INVALID
    assert lib.dispu_transpose_batched(1, None, F, p(f, 2048), st) == INVALID
    assert lib.dispu_transpose_batched(1, I, None, p(f, 2048), st) == INVALID
    assert lib.dispu_transpose_batched(1, I, F, None, st) == INVALID

    assert lib.dispu_sigmoid_offset(-1, F, F, F, st) == INVALID and lib.dispu_sigmoid_offset(0, F, F, F, st) == 0
    assert lib.dispu_sigmoid_offset_grad(-1, F, F, F, None, st) == INVALID and lib.dispu_sigmoid_offset_grad(0, F, F, F, None, st) == 0
    assert lib.dispu_add3(-1, F, F, F, F, st) == INVALID and lib.dispu_add3(0, F, F, F, F, st) == 0
    for args in ((-1, 4, 4, 2), (2, 0, 4, 2), (2, 4, 0, 2), (2, 4, 4, 0), (2, -4, 4, 2), (2, 4, 4, -1)):
        assert lib.dispu_dup_sum_grad(args[0], args[1], args[2], args[3], F, 8, p(f, 2048), 8, st) == INVALID, args
    assert lib.dispu_dup_sum_grad(0, 4, 4, 2, F, 8, p(f, 2048), 8, st) == 0
    torch.cuda.synchronize()
    assert bool((f == SENT).all()) and not bool(i.any()), "a refused call wrote to its buffers"


# ------------------------------------------------------------- the trainer's loss head, isolated from the generator ----
def loss_head_reference(ws, gt, radius, wf, use_repulse, rep_w):
    """float64 loss terms and gradients at the DEVICE's own fp32 coarse / fine.  Chamfer: the device's arg-min indices, each checked
    to be a float64 arg-min (or within TIE of one), carry the gradient; the values use the float64 arg-mins.  Repulsion: the host
    oracle's ball query on the device's fine cloud, which the device's own slots must equal.  -> dict(terms [4], dcoarse, dfine, skip (rows of dfine left out), M)"""
    B = gt.shape[0]
    coarse, fine = N_(ws["coarse"]).reshape(B, -1, 3), N_(ws["fine"]).reshape(B, -1, 3)
    M = fine.shape[1]
    cds, grads = [], []
    for slot, (cloud, coef) in enumerate(((coarse, 1000.0), (fine, 1000.0 * wf))):
        ig, ip = N_(ws["cd"][slot]["i_gt"]).reshape(B, -1), N_(ws["cd"][slot]["i_pred"]).reshape(B, -1)
        a, _ = check_device_argmin(gt, cloud, ig, "loss head slot %d, gt -> pred" % slot)
        b, _ = check_device_argmin(cloud, gt, ip, "loss head slot %d, pred -> gt" % slot)
        cds.append(LO.chamfer_value_grad(gt, cloud, a["idx"], b["idx"], radius, coef)[0])
        grads.append(LO.chamfer_value_grad(gt, cloud, ig, ip, radius, coef)[1])
    rep = None
    skip = np.zeros((B, M), bool)
    if use_repulse:
        idx, _ = O.query_ball_point(BALL, NS, fine, fine)
        rep, dr = LO.repulsion_value_grad(fine, idx, H, rep_w / (B * M * 4.0))
        grads[1] = grads[1] + dr
        # rows whose branch an fp32 evaluation may take differently, judged on the reference alone: a float64 gap below TIE between
        # two sorted slots of which one is (nearly) inside the hinge, or between a kept d and h
        t = LO.near_ties(fine, idx=idx, h=H)
        d = t["d"]
        live = H * (1.0 + TIE)
        assert np.array_equal(N_(ws["ball"]).reshape(B, M, NS), idx), "the trainer's ball query differs from the oracle's"
        kinds = dict(first=(t["first"] < TIE) & (d[..., 0] < live), fifth=(t["fifth"] < TIE) & (d[..., 4] < live),
                     hinge=(t["hinge"] < TIE).any(-1))
        risky = kinds["first"] | kinds["fifth"] | kinds["hinge"]
        print("[measured] loss head: risky repulsion rows by kind: %s" % {k: int(v.sum()) for k, v in kinds.items()})
        # what such a row can change: its own sum, and the rows of the two slots it chooses between (of the slot whose hinge toggles)
        js, bi = t["j"], np.broadcast_to(np.arange(B)[:, None], risky.shape)
        for kind, slots in (("first", (0, 1)), ("fifth", (4, 5))):
            for s_ in slots:
                np.logical_or.at(skip, (bi, js[..., s_]), kinds[kind])
        for s_ in range(4):
            np.logical_or.at(skip, (bi, js[..., 1 + s_]), t["hinge"][..., s_] < TIE)
        skip |= risky
        print("[measured] loss head: %d risky repulsion rows, %d of %d dfine rows left out" % (int(risky.sum()), int(skip.sum()), skip.size))
        assert skip.sum() <= 1e-3 * skip.size, "more than 0.1 % of the rows of dfine left out"
    terms = LO.pu_loss_terms(cds[0], cds[1], None if rep is None else rep.reshape(-1), B * M, wf, rep_w)
    return dict(terms=terms[:4], dcoarse=grads[0], dfine=grads[1], skip=skip, M=M)


def check_loss_head(tr, B, N, gt, radius, terms, what):
    from dispu_amd.train import weight_fine
    ws = tr._ws[(B, N)]
    wf = weight_fine(tr.epoch)
    ref = loss_head_reference(ws, gt, radius, wf, tr.opts.use_repulse, float(tr.opts.repulsion_w))
    got = [float(terms[k]) for k in ("dis_coarse_cd", "dis_fine_cd", "repulsion_loss", "pu_loss")]
    assert float(terms["weight_fine"]) == wf
    for k, g, r in zip(("dis_coarse_cd", "dis_fine_cd", "repulsion_loss", "pu_loss"), got, ref["terms"]):
        if r == 0.0:
            assert g == 0.0, (k, g)
        else:
            scalar_close(g, r, 1e-5, "%s %s" % (what, k))
    M = ref["M"]
    close(N_(ws["dcoarse"]).reshape(B, M, 3), ref["dcoarse"], 1e-5, "%s dcoarse" % what)
    keep = ~ref["skip"]
    dfine = N_(ws["dfine"]).reshape(B, M, 3)
    scale = np.abs(ref["dfine"]).max()
    err = np.abs(dfine.astype(np.float64) - ref["dfine"])[keep].max()
    print("[measured] %s dfine: max err %.3e of scale %.3e = %.2e (bound 1e-05), %d rows left out" % (what, err, scale, err / scale, int((~keep).sum())))
    assert err <= 1e-5 * scale, "%s dfine: rel %.2e" % (what, err / scale)
    return ref


def make_trainer(dev, epoch, use_repulse=True, repulsion_w=1.0):
    from dispu_amd.train import Trainer, TrainOpts
    opts = TrainOpts()
    opts.use_repulse, opts.repulsion_w = use_repulse, repulsion_w
    tr = Trainer(opts=opts, params=OG.init_params(seed=1234, bias_scale=0.05, bn_random=True), device=dev)
    tr.epoch = epoch
    return tr


def loss_head(dev, tr, B, N, seed):
    from dispu_amd import synth
    x, gt = synth.patch_with_gt(B, N, 4 * N, seed=seed)
    radius = radii(B, seed)
    tr.zero_grad()
    tr.forward(dv(x, dev))
    terms = tr.loss_backward(dv(gt, dev), dv(radius, dev))
    torch.cuda.synchronize()                    # read dcoarse / dfine BEFORE backward(), which adds dfine into dcoarse
    return gt, radius, terms


@pytest.mark.parametrize("epoch,B,N", [(0, 2, 256), (15, 1, 256), (25, 3, 256), (35, 17, 64), (15, 64, 256)])
def test_loss_head(dev, epoch, B, N):
    """pu_loss terms, dcoarse and dfine of Trainer.loss_backward against float64 at the device's own coarse / fine: every value of
    weight_fine once, every batch shape once.  No generator branch enters, so there is no row-wise allowance."""
    tr = make_trainer(dev, epoch)
    gt, radius, terms = loss_head(dev, tr, B, N, seed=50 + B)
    ref = check_loss_head(tr, B, N, gt, radius, terms, "loss head epoch %d B=%d N=%d" % (epoch, B, N))
    assert ref["terms"][2] > 0


def test_loss_head_without_repulsion(dev):
    tr = make_trainer(dev, 25, use_repulse=False)
    gt, radius, terms = loss_head(dev, tr, 2, 256, seed=61)
    assert float(terms["repulsion_loss"]) == 0.0
    ref = check_loss_head(tr, 2, 256, gt, radius, terms, "loss head, no repulsion")       # dfine = the Chamfer-only reference
    assert ref["terms"][2] == 0.0 and not ref["skip"].any()


def test_loss_head_repulsion_weight(dev):
    tr = make_trainer(dev, 35, repulsion_w=0.5)
    gt, radius, terms = loss_head(dev, tr, 2, 256, seed=62)
    check_loss_head(tr, 2, 256, gt, radius, terms, "loss head, repulsion_w = 0.5")


def test_loss_head_new_targets_on_one_forward(dev):
    """targets replaced between two loss_backward calls on one forward: the second result must not contain the first (dcoarse has
    had dfine added by backward() in between, dfine holds the first loss's repulsion atomics)."""
    from dispu_amd import synth
    tr = make_trainer(dev, 25)
    B, N = 2, 256
    gt1, radius1, _ = loss_head(dev, tr, B, N, seed=63)
    tr.backward()
    torch.cuda.synchronize()
    _, gt2 = synth.patch_with_gt(B, N, 4 * N, seed=64)
    radius2 = radii(B, 64)
    assert not np.array_equal(gt1, gt2)
    tr.zero_grad()
    terms = tr.loss_backward(dv(gt2, dev), dv(radius2, dev))
    torch.cuda.synchronize()
    check_loss_head(tr, B, N, gt2, radius2, terms, "loss head, second targets")
