"""Float64 oracle of the uniform term of the training loss, for tests only (dis-pu_amd/loss_utils.py:get_uniform_loss;
csrc/uniform_loss.hip: uniform_loss_grad_kernel, pu_loss_finalize_u_kernel).

Plain numpy with explicit indices, written from the formulas of Common/loss_utils.py:238-267 and not from the kernel: the seeds and the
ball-query slots are ARGUMENTS (the kernel's own are checked bit for bit against the ball-query oracle), so a reference is exact for
whatever slots it is given and no autograd graph is needed.  Inputs are float32 arrays, widened to float64 before any arithmetic.
tests/test_uniform_oracle.py holds these functions to a float64 autograd restatement of the reference's graph at 1e-8.

  host_levels          npoint, ns_l, r_l, e_l, (100 p_l)^2 in Python double arithmetic, as the reference computes them
  uniform_value_grad   value, per-ball partials, gradient at fixed slots and partners, and the near-tie report
  pu_loss_terms_u      the six outputs of dispu_pu_loss_finalize_u
"""
import math

import numpy as np

from loss_oracle import pu_loss_terms, rel_gap

DEFAULT_PERCENTAGES = [0.004, 0.006, 0.008, 0.010, 0.012]


def host_levels(n, percentages=DEFAULT_PERCENTAGES, radius=1.0):
    """loss_utils.py:239-251 for clouds of n points."""
    ns = [int(n * p) for p in percentages]
    return dict(npoint=int(n * 0.05), ns=ns, r=[math.sqrt(p * radius) for p in percentages],
                e=[math.sqrt(math.pi * (radius ** 2) * p / k) if k else float("nan") for p, k in zip(percentages, ns)],
                w=[math.pow(p * 100, 2) for p in percentages])


def uniform_value_grad(pcd, slots, percentages=DEFAULT_PERCENTAGES, radius=1.0, scale=1.0, levels=None):
    """pcd [B, N, 3]; slots[l] int [B, S, ns_l]: the ball-query slots of level l around the S seeds (cloud-local rows of pcd, unused
    slots repeat the first hit).  For slot i of a ball, with a = idx[i]:
        D_i = min over slots t != i of |x_a - x_idx[t]|^2 (differences first), the lowest t on exact ties; c = idx[t*]
        u_i = sqrt(D_i + 1e-8),  q_i = (u_i - e_l)^2 / (e_l + 1e-8)
        value_l = (100 p_l)^2 mean_(b, s, i) q_i,  value = mean_l value_l
        k = scale (100 p_l)^2 / (L B S ns_l);  g = k ((u_i - e_l) / ((e_l + 1e-8) u_i)) 2 (x_a - x_c): +g to row a, -g to row c,
        nothing where a == c.
    `levels` (hand-built cases): dict(ns, e, w) that replaces the quantities derived from the percentages.
    -> dict(value float, partial [L, B * S] = (100 p_l)^2 / ns_l * sum_i q_i (value = partial.mean()), grad [B, N, 3] float64,
            abs_grad [B, N, 3] = the sum of |contributions| per entry, u[l] [B, S, ns_l], partner[l] [B, S, ns_l] (the point c),
            gap[l] [B, S, ns_l] = the float64 relative gap (second - best) / second between D_i and the smallest distance to a slot
            holding a DIFFERENT point than c (inf where there is none): where it is tiny an fp32 evaluation may legitimately take the
            other partner)."""
    x = np.asarray(pcd, np.float64)
    B, N, _ = x.shape
    lv = levels if levels is not None else host_levels(N, percentages, radius)
    L = len(lv["ns"])
    S = np.asarray(slots[0]).shape[1]
    grad, abs_grad = np.zeros((B, N, 3)), np.zeros((B, N, 3))
    partial = np.empty((L, B * S))
    us, partners, gaps = [], [], []
    bi = np.arange(B)[:, None, None]
    for l in range(L):
        idx = np.asarray(slots[l], np.int64)
        ns, e, w = lv["ns"][l], lv["e"][l], lv["w"][l]
        assert idx.shape == (B, S, ns) and ns >= 2 and idx.min() >= 0 and idx.max() < N
        pts = x[bi, idx]                                                        # [B, S, ns, 3]
        diff = pts[:, :, :, None, :] - pts[:, :, None, :, :]                    # x_a(i) - x_idx[t]   [B, S, ns(i), ns(t), 3]
        d = (diff ** 2).sum(-1)
        d[:, :, np.arange(ns), np.arange(ns)] = np.inf                          # t != i
        t = d.argmin(-1)                                                        # first minimum: the lowest slot on ties
        D = np.take_along_axis(d, t[..., None], -1)[..., 0]
        c = np.take_along_axis(idx, t, -1)                                      # [B, S, ns]
        other = np.where(idx[:, :, None, :] == c[..., None], np.inf, d)         # slots holding another point than the partner
        gaps.append(rel_gap(D, other.min(-1)))
        u = np.sqrt(D + 1e-8)
        q = (u - e) ** 2 / (e + 1e-8)
        partial[l] = (w / ns * q.sum(-1)).reshape(-1)
        k = scale * w / (L * B * S * ns)
        xd = np.take_along_axis(diff, t[..., None, None], 3)[:, :, :, 0, :]     # x_a - x_c
        g = (k * (u - e) / ((e + 1e-8) * u) * 2.0)[..., None] * xd * (idx != c)[..., None]
        rows = np.broadcast_to(bi, idx.shape)
        np.add.at(grad, (rows, idx), g)
        np.add.at(grad, (rows, c), -g)
        np.add.at(abs_grad, (rows, idx), np.abs(g))
        np.add.at(abs_grad, (rows, c), np.abs(g))
        us.append(u)
        partners.append(c)
    return dict(value=float(partial.mean()), partial=partial, grad=grad, abs_grad=abs_grad, u=us, partner=partners, gap=gaps)


def near_tie_rows(res, slots, shape, tol=1e-5):
    """bool [B, N]: the rows a slot with a partner gap below tol touches (the member's row and both candidate partners cannot be told
    apart here, so every member of such a ball's slot and its partner are marked)."""
    B, N = shape
    mask = np.zeros((B, N), bool)
    for idx, c, gap in zip(slots, res["partner"], res["gap"]):
        idx = np.asarray(idx, np.int64)
        hit = gap < tol
        if hit.any():
            b = np.broadcast_to(np.arange(B)[:, None, None], idx.shape)
            ball = hit.any(-1)[..., None] & np.ones_like(hit)                   # the whole ball: the other partner is one of its members
            mask[b[ball], idx[ball]] = True
            mask[b[hit], c[hit]] = True
    return mask


def pu_loss_terms_u(cd_coarse, cd_fine, rep, nrep, wf, rep_w, upart, uniform_w):
    """The six outputs of dispu_pu_loss_finalize_u: pu_loss_terms' five with the uniform term uniform_w * mean(upart) added to the
    fourth (pu_loss), and that term itself."""
    t = pu_loss_terms(cd_coarse, cd_fine, rep, nrep, wf, rep_w)
    un = float(uniform_w) * float(np.asarray(upart, np.float64).mean())
    return np.array([t[0], t[1], t[2], t[3] + un, t[4], un], np.float64)
