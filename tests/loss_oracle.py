"""Float64 oracle of the trainer's loss head, for tests only (dis-pu_amd/train.py:loss_backward; csrc/train_fused.hip:
chamfer_value_kernel, chamfer_grad_kernel, repulsion_loss_grad_kernel, pu_loss_finalize_kernel).

Plain numpy with explicit indices, written from the formulas of DisPU/model.py:75-87 and Common/loss_utils.py:45-64,271-298 and
not from the kernels: the arg-min / ball-query indices are ARGUMENTS (the kernels take them as inputs too), so a reference is exact
for whatever indices it is given and no autograd graph is needed.  Inputs are float32 arrays, widened to float64 before any
arithmetic.  tests/test_loss_oracle.py holds these functions to autograd of oracle/train_oracle.py at 1e-12.

  nearest              float64 arg-min of one cloud set against another, with the best and second-best squared distance
  chamfer_value_grad   CD(gt, pred) and d(coef * CD)/d pred for given arg-min indices
  repulsion_value_grad per-point hinge sums and scale * d(sum)/d pred for given ball-query slots
  pu_loss_terms        the five outputs of dispu_pu_loss_finalize
  near_ties            relative gaps that tell where an fp32 evaluation may legitimately pick another branch
  jittered_pair        the synthetic (gt, pred) clouds of the GPU tests
"""
import numpy as np


def _f64(a):
    return np.asarray(a, np.float64)


def rel_gap(lo, hi):
    """(hi - lo) / hi for 0 <= lo <= hi; 0 where both are 0 (an exact tie), inf where hi is inf (no second candidate)."""
    lo, hi = _f64(lo), _f64(hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(np.isinf(hi), np.inf, np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, 1.0), 0.0))
    return g


def nearest(a, b):
    """For every point of a [B, n, 3] its nearest point of b [B, m, 3] by the squared distance in float64 (differences first,
    no |a|^2 - 2ab + |b|^2 expansion), one cloud at a time -> dict(idx int32 [B, n] (lowest index on exact ties), best [B, n],
    second [B, n] (inf for m == 1), second_idx [B, n] (-1 for m == 1))."""
    a, b = _f64(a), _f64(b)
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    idx = np.empty((B, n), np.int32)
    best = np.empty((B, n))
    second = np.full((B, n), np.inf)
    second_idx = np.full((B, n), -1, np.int32)
    rows = np.arange(n)
    for c in range(B):
        d = ((a[c][:, None, :] - b[c][None, :, :]) ** 2).sum(-1)                # [n, m]
        i0 = d.argmin(1)
        idx[c], best[c] = i0, d[rows, i0]
        if m > 1:
            d[rows, i0] = np.inf
            i1 = d.argmin(1)
            second[c], second_idx[c] = d[rows, i1], i1
    return dict(idx=idx, best=best, second=second, second_idx=second_idx)


def sq_dist_to(a, b, idx):
    """|a[c, k] - b[c, idx[c, k]]|^2 in float64 -> [B, n]."""
    a, b = _f64(a), _f64(b)
    bi = np.arange(a.shape[0])[:, None]
    return ((a - b[bi, np.asarray(idx, np.int64)]) ** 2).sum(-1)


def chamfer_value_grad(gt, pred, i_gt, i_pred, radius, coef):
    """gt [B, n_gt, 3], pred [B, n_pred, 3], i_gt [B, n_gt] (rows of pred), i_pred [B, n_pred] (rows of gt), radius [B].
      value = mean_b[(mean_k |gt_k - pred[i_gt_k]|^2 + mean_j |pred_j - gt[i_pred_j]|^2) / radius_b]
      dpred[b, j] = 2 coef (pred_j - gt[i_pred_j]) / (radius_b n_pred B), and scattered to row i_gt_k:
                    -2 coef (gt_k - pred[i_gt_k]) / (radius_b n_gt B)
    -> (value float, dpred float64 [B, n_pred, 3]) with dpred = d(coef * value)/d pred at fixed indices."""
    gt, pred, radius = _f64(gt), _f64(pred), _f64(radius)
    i_gt, i_pred = np.asarray(i_gt, np.int64), np.asarray(i_pred, np.int64)
    B, n_gt, n_pred = gt.shape[0], gt.shape[1], pred.shape[1]
    assert i_gt.shape == (B, n_gt) and i_pred.shape == (B, n_pred) and radius.shape == (B,)
    assert i_gt.min() >= 0 and i_gt.max() < n_pred and i_pred.min() >= 0 and i_pred.max() < n_gt
    bi = np.arange(B)[:, None]
    from_gt = gt - pred[bi, i_gt]                       # [B, n_gt, 3]
    from_pred = pred - gt[bi, i_pred]                   # [B, n_pred, 3]
    per_cloud = ((from_gt ** 2).sum(-1).mean(1) + (from_pred ** 2).sum(-1).mean(1)) / radius
    value = float(per_cloud.mean())
    r = radius[:, None, None]
    dpred = 2.0 * coef * from_pred / (r * n_pred * B)
    np.add.at(dpred, (np.broadcast_to(bi, i_gt.shape), i_gt), -2.0 * coef * from_gt / (r * n_gt * B))
    return value, dpred


def _repulsion_sorted(pred, idx):
    pred, idx = _f64(pred), np.asarray(idx, np.int64)
    B, M = pred.shape[0], pred.shape[1]
    assert idx.shape[:2] == (B, M) and idx.min() >= 0 and idx.max() < M
    bi = np.arange(B)[:, None, None]
    diff = pred[bi, idx] - pred[:, :, None, :]          # p_j - p_i  [B, M, ns, 3]
    d = (diff ** 2).sum(-1)
    order = np.argsort(d, axis=-1, kind="stable")       # earlier slot first on ties, as tf.nn.top_k
    return pred, idx, diff, d, order


def repulsion_value_grad(pred, idx, h, scale):
    """pred [B, M, 3], idx [B, M, ns] ball-query slots (cloud-local rows of pred, padded slots repeat a neighbour).
    Per point the squared distances to its slots, stable ascending sort, slots 1..4 kept (the first is dropped, as
    tf.nn.top_k(-d, 5)[..., 1:]):  out[i] = sum max(0, h - d);  for each kept slot with h - d > 0:  +2 scale (p_j - p_i) to row i and
    the negative to row j (a padded slot that repeats one neighbour counts once per slot).
    -> (out float64 [B, M], dpred float64 [B, M, 3]) with dpred = scale * d(sum out)/d pred at fixed slots."""
    pred, idx, diff, d, order = _repulsion_sorted(pred, idx)
    B, M = pred.shape[0], pred.shape[1]
    keep = order[..., 1:5]
    dk = np.take_along_axis(d, keep, -1)                                        # [B, M, 4]
    out = np.maximum(0.0, h - dk).sum(-1)
    active = (h - dk) > 0
    jk = np.take_along_axis(idx, keep, -1)
    ek = np.take_along_axis(diff, keep[..., None], 2)                           # [B, M, 4, 3]
    c = 2.0 * scale * ek * active[..., None]
    dpred = c.sum(2)
    np.add.at(dpred, (np.broadcast_to(np.arange(B)[:, None, None], jk.shape), jk), -c)
    return out, dpred


def pu_loss_terms(cd_coarse, cd_fine, rep, nrep, wf, rep_w):
    """The five outputs of dispu_pu_loss_finalize (model.py:75-87): 1000 cd_coarse | 1000 cd_fine | rep_w * sum(rep[:nrep]) /
    (4 nrep) (0 without a repulsion term: rep is None) | the first + wf * the second + the third | wf."""
    c, f = 1000.0 * float(cd_coarse), 1000.0 * float(cd_fine)
    r = 0.0 if rep is None else float(rep_w) * float(_f64(rep).reshape(-1)[:nrep].sum()) / (4.0 * nrep)
    return np.array([c, f, r, c + float(wf) * f + r, float(wf)], np.float64)


def near_ties(a, b=None, idx=None, h=None):
    """Relative gaps, in float64, that say where an fp32 evaluation of the same distances may pick another branch.

    near_ties(a, b): arg-min rows of the Chamfer term -> gap [B, n] = (second - best) / second between the best and second-best
    candidate of every point of a among the points of b (0: exact tie; inf: b has one point).

    near_ties(pred, idx=idx, h=h): the repulsion term -> dict of
      first   [B, M]    gap between the 1st and 2nd sorted slot (which one is dropped),
      fifth   [B, M]    gap between the 5th and 6th sorted slot (which one is kept last),
      hinge   [B, M, 4] |h - d| / h of every kept slot (whether its hinge is active);
      d, j    [B, M, ns] the sorted squared distances and the points in those slots;
    `first` and `fifth` are inf where the two slots hold the same point: the choice between them changes nothing."""
    if idx is None:
        nn = nearest(a, b)
        return rel_gap(nn["best"], nn["second"])
    pred, idx, diff, d, order = _repulsion_sorted(a, idx)
    ds = np.take_along_axis(d, order, -1)
    js = np.take_along_axis(idx, order, -1)
    first = np.where(js[..., 0] == js[..., 1], np.inf, rel_gap(ds[..., 0], ds[..., 1]))
    if ds.shape[-1] > 5:
        fifth = np.where(js[..., 4] == js[..., 5], np.inf, rel_gap(ds[..., 4], ds[..., 5]))
    else:
        fifth = np.full(first.shape, np.inf)
    return dict(first=first, fifth=fifth, hinge=np.abs(h - ds[..., 1:5]) / h, d=ds, j=js)


def jittered_pair(B, n_gt, n_pred, seed, sigma=0.02):
    """(gt [B, n_gt, 3], pred [B, n_pred, 3]) float32: gt from dispu_amd.synth (normalised spherical-cap patches), pred a permuted
    copy of gt's points (repeated where n_pred > n_gt) + N(0, sigma): a cloud that looks like a generator output."""
    from dispu_amd import synth
    _, gt = synth.patch_with_gt(B, max(16, n_gt // 4), n_gt, seed=seed)
    rng = np.random.default_rng(seed + 7919)
    pred = np.empty((B, n_pred, 3), np.float32)
    for c in range(B):
        take = np.concatenate([rng.permutation(n_gt) for _ in range((n_pred + n_gt - 1) // n_gt)])[:n_pred]
        pred[c] = (gt[c][take].astype(np.float64) + rng.normal(0.0, sigma, (n_pred, 3))).astype(np.float32)
    return gt, pred
