"""float64 numpy reference of the EMD term of the training loss, `emd_w * earth_mover(fine, gt, radius)` (DisPU/model.py:77,
Common/loss_utils.py:170-176), GIVEN a transport plan `match` [b, m, n] (approx_match carries no gradient, tf_approxmatch.py:22):

  cost_b        = sum_{k,l} sqrt(d2(k,l)) match[b,l,k]                                 matchcost, tf_approxmatch_g.cu:183-225
  grad1[b,k,:]  = sum_l match[b,l,k] (p1_k - p2_l) / sqrt(max(d2(k,l), 1e-20))        matchcostgrad1, :270-291
  dis_fine_emd  = emd_w * mean_b(cost_b / radius_b / m)
  d(wf * dis_fine_emd)/d p1[b,k,:] = emd_w * wf / (B * m) / radius_b * grad1[b,k,:]
  pu_loss       = ((c + wf * (f + e)) + r) [+ u]       the term inside the weight_fine parenthesis, next to dis_fine_cd

Inputs are taken as they are (float32 clouds and plans are widened exactly); nothing here runs an auction.  Held to the project's C
oracle (oracle.match_cost / match_cost_grad) and to a float64 torch autograd restatement by tests/test_emd_oracle.py."""
import numpy as np


def _f64(a):
    return np.asarray(a, np.float64)


def sqdist(xyz1, xyz2):
    """d2 [b, n, m] of the coordinate differences, float64."""
    d = _f64(xyz1)[:, :, None, :] - _f64(xyz2)[:, None, :, :]
    return (d * d).sum(-1)


def match_cost(xyz1, xyz2, match):
    """cost [b] = sum_{k,l} sqrt(d2(k,l)) match[b,l,k]; match [b, m, n]."""
    return (np.sqrt(sqdist(xyz1, xyz2)) * _f64(match).transpose(0, 2, 1)).sum((1, 2))


def match_cost_grad1(xyz1, xyz2, match):
    """grad1 [b, n, 3] with the reference's clamp: the direction is divided by sqrt(max(d2, 1e-20)), so a prediction that coincides
    with a ground-truth point gets a zero contribution from that pair (0 * 1e10), never a NaN."""
    p1, p2 = _f64(xyz1), _f64(xyz2)
    d = p1[:, :, None, :] - p2[:, None, :, :]
    w = _f64(match).transpose(0, 2, 1) / np.sqrt(np.maximum((d * d).sum(-1), 1e-20))
    return (w[..., None] * d).sum(2)


def emd_value(cost, radius, m, emd_w=10.0):
    """dis_fine_emd = emd_w * mean_b(cost_b / radius_b / m) (loss_utils.py:170-176 with the literal of model.py:77)."""
    cost = _f64(cost)
    r = np.ones_like(cost) if radius is None else _f64(radius)
    return float(emd_w) * float((cost / r / float(m)).mean())


def grad_scale(radius, b, m, emd_w=10.0, wf=1.0):
    """[b]: the factor of grad1 in d(wf * dis_fine_emd)/d p1 = coef / radius_b, coef = emd_w * wf / (b * m)."""
    r = np.ones(b) if radius is None else _f64(radius)
    return float(emd_w) * float(wf) / (float(b) * float(m)) / r


def emd_value_grad(xyz1, xyz2, match, radius, emd_w=10.0, wf=1.0):
    """-> dict(cost [b], grad1 [b, n, 3], value (dis_fine_emd, without wf), grad [b, n, 3] = d(wf * value)/d xyz1)."""
    b, m = np.shape(xyz2)[0], np.shape(xyz2)[1]
    cost, g1 = match_cost(xyz1, xyz2, match), match_cost_grad1(xyz1, xyz2, match)
    return dict(cost=cost, grad1=g1, value=emd_value(cost, radius, m, emd_w),
                grad=grad_scale(radius, b, m, emd_w, wf)[:, None, None] * g1)


def pu_loss_terms_e(cd_coarse, cd_fine, rep, nrep, wf, rep_w, upart, uniform_w, cost, radius, m, emd_w):
    """The seven outputs of dispu_pu_loss_finalize_e in float64: 1000 cd_coarse | 1000 cd_fine | rep_w * sum(rep) / (4 nrep) (0: rep is
    None) | pu_loss | wf | uniform_w * mean(upart) (0: upart is None) | dis_fine_emd."""
    c, f = 1000.0 * float(cd_coarse), 1000.0 * float(cd_fine)
    r = 0.0 if rep is None else float(rep_w) * float(_f64(rep).reshape(-1)[:nrep].sum()) / (4.0 * nrep)
    u = 0.0 if upart is None else float(uniform_w) * float(_f64(upart).mean())
    e = emd_value(cost, radius, m, emd_w)
    return np.array([c, f, r, ((c + float(wf) * (f + e)) + r) + u, float(wf), u, e], np.float64)


def pu_loss_f32(c, f, e, r, u, wf):
    """the entry's stated order in float32, operation by operation: ((c + wf * (f + e)) + r) [+ u] (u None: no uniform term)."""
    F = np.float32
    pu = F(F(c) + F(F(wf) * F(F(f) + F(e))))
    pu = F(pu + F(r))
    return pu if u is None else F(pu + F(u))
