"""Losses of the reference's training graph (Common/loss_utils.py: chamfer :45-64, hausdorff_loss :67-84,
earth_mover :170-176, get_uniform_loss :238-267, get_repulsion_loss :271-298) on the hot-path ops.  Same names / arguments /
return values (scalar tensors).  chamfer and earth_mover are differentiable w.r.t. the point sets through the registered
gradients of nn_distance / match_cost, hausdorff through them and the max reductions (the reference only logs it,
DisPU/model.py:76,79); the repulsion term here is forward-only (its gradient kernel is used by train.py); the uniform term
is differentiable through its fused value + gradient kernel (csrc/uniform_loss.hip)."""
import ctypes
import math

import torch

from . import _lib
from .tf_approxmatch import approx_match, match_cost
from .tf_grouping import query_ball_point
from .tf_nndistance import nn_distance
from .tf_sampling import farthest_point_sample
from ._util import f32, req


def _row_mean_max(x):
    b, n = x.shape
    mean = torch.empty((b,), dtype=torch.float32, device=x.device)
    mx = torch.empty((b,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dispu_row_mean_max(b, n, _lib.ptr(x.contiguous()), _lib.ptr(mean), _lib.ptr(mx),
                                             _lib.stream_ptr(x.device)), "dispu_row_mean_max")
    return mean, mx


class _RowMean(torch.autograd.Function):
    """mean over axis 1 with the HIP reduction forward; d/dx = g / n."""

    @staticmethod
    def forward(ctx, x):
        ctx.n = x.shape[1]
        return _row_mean_max(x)[0]

    @staticmethod
    def backward(ctx, g):
        return (g / ctx.n).unsqueeze(1).expand(-1, ctx.n).contiguous()


class _RowMax(torch.autograd.Function):
    """max over axis 1 with the HIP reduction forward; the gradient goes to the maximal entries, split evenly among ties
    (tf.reduce_max's rule)."""

    @staticmethod
    def forward(ctx, x):
        mx = _row_mean_max(x)[1]
        ctx.save_for_backward(x, mx)
        return mx

    @staticmethod
    def backward(ctx, g):
        x, mx = ctx.saved_tensors
        hit = (x == mx.unsqueeze(1)).to(x.dtype)
        return hit * (g / hit.sum(1)).unsqueeze(1)


def chamfer(pred, gt, radius=1.0, forward_weight=1.0, threshold=None, return_hd=False):
    """loss_utils.py:45-64: mean_b[(fw * mean(dist gt->pred) + mean(dist pred->gt)) / radius]."""
    if threshold is not None:
        raise NotImplementedError("threshold is never set by the reference's training graph (DisPU/model.py:75-79)")
    dists_forward, _, dists_backward, _ = nn_distance(gt, pred)
    cd = forward_weight * _RowMean.apply(dists_forward) + _RowMean.apply(dists_backward)
    return (cd / radius).sum() / cd.shape[0]


def hausdorff_loss(pred, gt, radius=1.0, forward_weight=1.0, threshold=None):
    """loss_utils.py:67-84: max_b[(fw * max(dist gt->pred) + max(dist pred->gt)) / radius]."""
    if threshold is not None:
        raise NotImplementedError("threshold is never set by the reference's training graph")
    dists_forward, _, dists_backward, _ = nn_distance(gt, pred)
    hd = forward_weight * _RowMax.apply(dists_forward) + _RowMax.apply(dists_backward)
    return (hd / radius).max()


def earth_mover(pcd1, pcd2, radius=1.0):
    """loss_utils.py:170-176: mean_b(match_cost / radius / num_points); approx_match carries no gradient."""
    assert pcd1.shape[1] == pcd2.shape[1]
    num_points = float(pcd1.shape[1])
    match = approx_match(pcd1.detach(), pcd2.detach())
    cost = match_cost(pcd1, pcd2, match) / radius
    return (cost / num_points).sum() / cost.shape[0]


def get_repulsion_loss(pred, nsample=20, radius=0.07, knn=False, use_l1=False, h=0.001):
    """loss_utils.py:271-298: ball query (radius, nsample) around every point, squared distances to the grouped
    neighbours, the 4 nearest non-first ones, mean(max(0, h - d))."""
    if knn:
        raise NotImplementedError("knn=True is dead code in the reference (hard-coded (30,1024) constant, loss_utils.py:275)")
    p = pred.detach().contiguous()
    b, n, _ = p.shape
    idx, _ = query_ball_point(radius, nsample, p, p)
    if use_l1:
        h = float(h) ** 0.5 * 2
    per_point = torch.empty((b, n), dtype=torch.float32, device=p.device)
    _lib.check(_lib.lib().dispu_repulsion(b * n, n, nsample, 1 if use_l1 else 0, float(h), _lib.ptr(p), _lib.ptr(idx),
                                          _lib.ptr(per_point), _lib.stream_ptr(p.device)), "dispu_repulsion")
    return _row_mean_max(per_point)[0].sum() / (b * 4.0)


UNIFORM_PERCENTAGES = (0.004, 0.006, 0.008, 0.010, 0.012)      # loss_utils.py:238 (the defaults of get_uniform_loss)
UNIFORM_MAX_LEVELS, UNIFORM_MAX_NS = 8, 64                      # csrc/uniform_loss.hip: a ball's members sit one per lane


def uniform_min_points(percentages=UNIFORM_PERCENTAGES):
    """the smallest cloud get_uniform_loss accepts: int(N * 0.05) >= 1 and int(N * p) >= 2 for every level."""
    n = 1
    while int(n * 0.05) < 1 or any(int(n * p) < 2 for p in percentages):
        n += 1
    return n


def uniform_levels(n, percentages=UNIFORM_PERCENTAGES, radius=1.0):
    """The host-side quantities of get_uniform_loss (loss_utils.py:239-251) for clouds of n points, in Python double arithmetic as
    the reference computes them -> dict(npoint = int(n * 0.05), ns[l] = int(n * p_l), r[l] = sqrt(p_l * radius),
    e[l] = sqrt(pi * radius^2 * p_l / ns_l), w[l] = (100 p_l)^2).  ValueError where the reference's own graph fails (top_k(., 2) of a
    ball of one slot, a sample of zero seeds) or the kernel's limits are passed."""
    percentages = [float(p) for p in percentages]
    req(1 <= len(percentages) <= UNIFORM_MAX_LEVELS, "get_uniform_loss expects 1..%d percentages" % UNIFORM_MAX_LEVELS)
    req(all(p > 0 for p in percentages) and radius > 0, "get_uniform_loss expects positive percentages and radius")
    npoint = int(n * 0.05)
    req(npoint >= 1, "FarthestPointSample expects positive npoint")
    ns = [int(n * p) for p in percentages]
    req(min(ns) >= 2, "input must have at least k columns")       # tf.nn.top_k(., 2) on a ball of one slot
    req(max(ns) <= min(UNIFORM_MAX_NS, n), "get_uniform_loss: at most min(%d, n) slots per ball, got %d" % (UNIFORM_MAX_NS, max(ns)))
    return dict(npoint=npoint, ns=ns, r=[math.sqrt(p * radius) for p in percentages],
                e=[math.sqrt(math.pi * (radius ** 2) * p / k) for p, k in zip(percentages, ns)],
                w=[math.pow(p * 100, 2) for p in percentages])


class UniformTables(object):
    """the host arrays dispu_uniform_loss_grad reads (ns [L] int32; levels [L][4] float32 = r | e | value factor | gradient factor)
    for b clouds of n points; `scale` multiplies the gradient.  A launch tape records their addresses: keep the object alive."""

    def __init__(self, b, n, percentages=UNIFORM_PERCENTAGES, radius=1.0, scale=1.0):
        lv = uniform_levels(n, percentages, radius)
        L = len(lv["ns"])
        self.nlevels, self.npoint, self.ns_list = L, lv["npoint"], lv["ns"]
        self.ns = (ctypes.c_int * L)(*lv["ns"])
        rows = []
        for l in range(L):
            vfac = lv["w"][l] / lv["ns"][l]                        # mean over the slots; the mean over (level, cloud, seed) is the finalize's
            rows += [lv["r"][l], lv["e"][l], vfac, scale * vfac / (L * max(b, 1) * lv["npoint"])]
        self.levels = (ctypes.c_float * (4 * L))(*rows)
        self.slots = sum(lv["ns"])


def uniform_loss_grad_raw(pcd, seeds, tables, dpcd=None, want_slots=False, arith=_lib.ARITH_CONTRACT):
    """one dispu_uniform_loss_grad launch -> (partial [L, b * npoint], idx_out | None, cnt_out | None); dpcd accumulates."""
    b, n, _ = pcd.shape
    balls = b * tables.npoint
    partial = torch.empty((tables.nlevels, balls), dtype=torch.float32, device=pcd.device)
    idx = torch.zeros((balls * tables.slots,), dtype=torch.int32, device=pcd.device) if want_slots else None
    cnt = torch.empty((tables.nlevels, balls), dtype=torch.int32, device=pcd.device) if want_slots else None
    _lib.check(_lib.lib().dispu_uniform_loss_grad(b, n, tables.npoint, tables.nlevels, ctypes.addressof(tables.ns), ctypes.addressof(tables.levels),
                                                  _lib.ptr(pcd), _lib.ptr(seeds), _lib.ptr(partial), _lib.ptr(dpcd), _lib.ptr(idx), _lib.ptr(cnt),
                                                  int(arith), _lib.stream_ptr(pcd.device)), "dispu_uniform_loss_grad")
    return partial, idx, cnt


class _UniformLoss(torch.autograd.Function):
    """value = mean of the kernel's partials; the same launch leaves d value / d pcd (seeds, slots and partners held fixed)."""

    @staticmethod
    def forward(ctx, pcd, seeds, tables):
        grad = torch.zeros_like(pcd)
        partial, _, _ = uniform_loss_grad_raw(pcd, seeds, tables, dpcd=grad)
        ctx.save_for_backward(grad)
        return partial.sum() / partial.numel()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def get_uniform_loss(pcd, percentages=[0.004, 0.006, 0.008, 0.010, 0.012], radius=1.0):
    """loss_utils.py:238-267: farthest-point seeds (5 % of the cloud), per percentage p a ball query (sqrt(p radius), int(N p) slots),
    every slot's distance u to its nearest other slot, mean((u - e)^2 / (e + 1e-8)) * (100 p)^2 with e = sqrt(pi radius^2 p / int(N p)),
    averaged over the percentages.  Differentiable w.r.t. pcd.  The seeds are computed once (the reference recomputes the same ones
    per level); squared distances come from coordinate differences (deviations)."""
    pcd = f32(pcd, "pcd")
    req(pcd.dim() == 3 and pcd.shape[2] == 3, "get_uniform_loss expects (batch_size, num_points, 3) pcd shape")
    b, n, _ = pcd.shape
    tables = UniformTables(b, n, percentages, radius)
    seeds = farthest_point_sample(tables.npoint, pcd.detach())
    return _UniformLoss.apply(pcd, seeds, tables)
