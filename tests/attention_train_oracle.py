"""Float64 oracle of the training attention (csrc/attention_train.hip: dispu_attention_fwd_lse, dispu_attention_bwd), for tests only.

Plain numpy, written from the three ops of Common/ops.py:326-339 (matmul(transpose_b), softmax, matmul) and from the formulas in the
header comment of the kernel file, not from the kernels.  Queries are [b, m, 64], keys and values [b, nk, 64]; m != nk is allowed.

  forward        (O, lse2) float64: O = softmax(scale Q K^T) V, lse2[q] = log2 sum_k exp(scale Q[q].K[k])
  backward       (dQ, dK, dV, D) float64 from the explicit formulas (no autograd):
                     P = softmax(scale Q K^T)   D = rowsum(dO o O)   dS = P o (dO V^T - D)
                     dQ = scale dS K            dK = scale dS^T Q    dV = P^T dO
  recompute_f32  the same ALGORITHM with every intermediate rounded to float32: s2 = (scale log2 e) Q K^T, lse2, P = exp2(s2 - lse2),
                 D, dS and the products.  It states what the algorithm costs in float32 whoever implements it: P is recomputed from
                 one float per query, so an error of s2 or lse2 of eps32 |s2| becomes a RELATIVE error of P of ln 2 eps32 |s2|.
  three_op_f32   float32 torch autograd of the three ops on the CPU: what the trainer's flash_attn = False arithmetic costs.
  dq_cancelled   the size of the terms that cancel in dQ (for inputs whose dQ is analytically zero)
  cloud_errors   per cloud: max |got - ref| / max |ref|

Input builders (all return float32 q [b, m, 64], k, v [b, nk, 64], do [b, m, 64]); cloud c's V is scaled by 2^((5 c) % 13 - 6) and its
dO by 2^((3 c) % 7 - 3), which scales the outputs linearly and changes no conditioning:
  benign         randn * 1.5 (the inputs of tests/test_train_fused_gpu.py)
  ascending      logits strictly increasing along the key index for every query: the running maximum moves on every tile
  descending     strictly decreasing: the maximum never moves after the first tile
  one_hot        query i is aligned with key hot_keys(nk)[i % ..]: key 0, key 31, key nk - 1 and one key of every 32-key tile; the
                 dominance grows with i from a lead of 0.66 nats to saturation (P == 1 in float32, dS cancels)
  equal_keys     all K rows of a cloud equal: P == 1 / nk, O the mean of V, lse2 == s2 + log2 nk, dQ analytically zero
  zero_q         Q == 0: lse2 == log2 nk, O the column mean of V, dK == 0
  k_offset       benign plus one common offset on every key of a cloud, sized so that max |s2| is `target` (what conv_kv's bias does):
                 the softmax does not change analytically, the exponent arithmetic does
  big_logits     randn * mult for Q and K
"""
import numpy as np

F32 = np.float32
LOG2E = 1.4426950408889634
D = 64


def _f64(a):
    return np.asarray(a, np.float64)


def _t(a):
    return np.swapaxes(a, -1, -2)


# ------------------------------------------------------------------------------------------------ formulas ----
def _softmax(q, k, scale):
    s = np.matmul(q, _t(k)) * float(scale)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(-1, keepdims=True)
    return e / l, (mx[..., 0] + np.log(l[..., 0])) * LOG2E


def forward(q, k, v, scale):
    """-> (O [b, m, 64], lse2 [b, m]) float64, lse2 in the log2 domain."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    P, lse2 = _softmax(q, k, scale)
    return np.matmul(P, v), lse2


def backward(q, k, v, do, scale):
    """-> (dQ [b, m, 64], dK [b, nk, 64], dV [b, nk, 64], D [b, m]) float64."""
    q, k, v, do = _f64(q), _f64(k), _f64(v), _f64(do)
    P, _ = _softmax(q, k, scale)
    Dv = (do * np.matmul(P, v)).sum(-1)
    dS = P * (np.matmul(do, _t(v)) - Dv[..., None])
    return float(scale) * np.matmul(dS, k), float(scale) * np.matmul(_t(dS), q), np.matmul(_t(P), do), Dv


def dq_cancelled(q, k, v, do, scale):
    """per cloud [b]: max over (query, channel) of scale sum_k |dS[q][k]| |K[k][d]|, the magnitude of what dQ adds up."""
    q, k, v, do = _f64(q), _f64(k), _f64(v), _f64(do)
    P, _ = _softmax(q, k, scale)
    Dv = (do * np.matmul(P, v)).sum(-1)
    dS = P * (np.matmul(do, _t(v)) - Dv[..., None])
    return (float(scale) * np.matmul(np.abs(dS), np.abs(k))).reshape(q.shape[0], -1).max(-1)


def recompute_f32(q, k, v, do, scale):
    """the flash algorithm in float32 -> dict(O, lse2, D, dQ, dK, dV), float32 arrays.  Every line is one rounded float32 operation
    (the matrix products accumulate in float32)."""
    q, k, v, do = (np.asarray(a, F32) for a in (q, k, v, do))
    scale = F32(scale)
    s2 = np.matmul(q * (scale * F32(LOG2E)), _t(k))                      # log2 domain, as the row statistic is kept
    mx = s2.max(-1, keepdims=True)
    e = np.exp2(s2 - mx)
    l = e.sum(-1, keepdims=True, dtype=F32)
    O = np.matmul(e, v) / l
    lse2 = mx + np.log2(l)                                               # the ONE float per query the backward gets
    P = np.exp2(s2 - lse2)                                               # recomputed, not e / l
    Dv = (do * O).sum(-1, keepdims=True, dtype=F32)
    dS = P * (np.matmul(do, _t(v)) - Dv)
    out = dict(O=O, lse2=lse2[..., 0], D=Dv[..., 0], dQ=np.matmul(dS, k) * scale, dK=np.matmul(_t(dS), q) * scale, dV=np.matmul(_t(P), do))
    assert all(a.dtype == F32 for a in out.values())
    return out


def three_op_f32(q, k, v, do, scale):
    """float32 torch autograd of matmul(transpose_b) / softmax / matmul on the CPU -> dict(O, dQ, dK, dV)."""
    import torch
    tq, tk, tv = (torch.tensor(np.asarray(a, F32), requires_grad=True) for a in (q, k, v))
    out = torch.matmul(torch.softmax(torch.matmul(tq, tk.transpose(1, 2)) * float(scale), dim=-1), tv)
    out.backward(torch.tensor(np.asarray(do, F32)))
    return dict(O=out.detach().numpy(), dQ=tq.grad.numpy(), dK=tk.grad.numpy(), dV=tv.grad.numpy())


def s2_max(q, k, scale):
    """max |scale log2(e) Q.K| over all clouds, float64."""
    return float(np.abs(np.matmul(_f64(q), _t(_f64(k)))).max() * float(scale) * LOG2E)


def cloud_errors(got, ref, floor=None):
    """got, ref [b, ...] -> [b]: max |got - ref| of a cloud over max |ref| of the same cloud (not below `floor` [b] where given)."""
    ref = _f64(ref)
    b = ref.shape[0]
    assert np.shape(got) == ref.shape, "shape %s vs %s" % (np.shape(got), ref.shape)
    size = np.abs(ref).reshape(b, -1).max(-1)
    if floor is not None:
        size = np.maximum(size, floor)
    return np.abs(_f64(got) - ref).reshape(b, -1).max(-1) / np.maximum(size, 1e-300)


# ---------------------------------------------------------------------------------------------- input builders ----
def v_scale(b):
    return (2.0 ** ((5 * np.arange(b)) % 13 - 6)).astype(F32)


def do_scale(b):
    return (2.0 ** ((3 * np.arange(b)) % 7 - 3)).astype(F32)


def _vdo(rng, b, m, nk):
    v = rng.standard_normal((b, nk, D)).astype(F32) * F32(1.5) * v_scale(b)[:, None, None]
    do = rng.standard_normal((b, m, D)).astype(F32) * do_scale(b)[:, None, None]
    return v, do


def benign(rng, b, m, nk):
    q = rng.standard_normal((b, m, D)).astype(F32) * F32(1.5)
    k = rng.standard_normal((b, nk, D)).astype(F32) * F32(1.5)
    return (q, k) + _vdo(rng, b, m, nk)


def _monotone(rng, b, m, nk, sign):
    """K[j] = u g(j) + noise with a dense unit vector u per cloud and g linear in j; every query's component along u is 2..3 and the
    noise is small against one step of g, so the logits are strictly monotone in j for every query.  The logits span about 9 in all."""
    u = rng.standard_normal((b, 1, D))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    step = 24.0 / nk
    g = sign * (np.arange(nk) - (nk - 1) / 2.0) * step
    k = u * g[None, :, None] + rng.standard_normal((b, nk, D)) * (0.02 * step)
    q = rng.standard_normal((b, m, D)) * 0.5
    q += u * (rng.uniform(2.0, 3.0, (b, m, 1)) - (q * u).sum(-1, keepdims=True))
    return (q.astype(F32), k.astype(F32)) + _vdo(rng, b, m, nk)


def ascending(rng, b, m, nk):
    return _monotone(rng, b, m, nk, 1.0)


def descending(rng, b, m, nk):
    return _monotone(rng, b, m, nk, -1.0)


def hot_keys(nk):
    """key 0, key 31, key nk - 1, one key of every tile of 32 (so of every wave's tile in every stage of the split shape) and eight
    more, so that even 32 keys have ten hot ones: with three, a cloud's largest dK entry is a sum over so few keys' queries that the
    worst of 257 clouds sits at 1e-5 for any float32 evaluation."""
    return sorted(set([0, 31, nk - 1] + [32 * t + (5 * t + 3) % 32 for t in range(nk // 32)] + [(5 * j + 2) % nk for j in range(8)]))


def one_hot(rng, b, m, nk):
    """Hot key j is K[hot_j] = 8 (2 e_j - w) with e_j a coordinate axis of its own and w the sum of those axes; every other key is
    -8 w plus a quarter of a benign key.  Query i is 11 (e_a + mu_i e_b) plus a tenth of a benign query, a and b the hot keys i and
    i + 1 (cyclic): its logit is +11 (1 - mu_i) at a, -11 (1 - mu_i) at b and -11 (1 + mu_i) elsewhere.  mu_i falls from 0.97 (a leads b
    by 0.66 nats) to 0 (a leads everything by 22 nats: P == 1 to an ulp or two of float32, dS cancels) as 0.97 (1 - (i / (m - 1))^4):
    most queries are mild, so a cloud's largest gradient entries are not themselves the remains of a cancellation.  Saturation needs a
    lead of 17 nats + ln nk, so max |s2| cannot be small here (about 40); the logits are single large products, not sums of 64, which
    keeps the rounding of s2 at an ulp."""
    q, k, v, do = benign(rng, b, m, nk)
    hot = np.asarray(hot_keys(nk))
    nh = hot.size
    assert nh <= D
    E = np.zeros((nh, D), F32)
    E[np.arange(nh), (7 * np.arange(nh) + 3) % D] = 1.0                 # 7 is coprime to 64: nh different axes
    w = E.sum(0)
    k = k * F32(0.25) - F32(8.0) * w
    k[:, hot] = F32(8.0) * (2.0 * E - w)
    i = np.arange(m)
    mu = (0.97 * (1.0 - (i / max(m - 1.0, 1.0)) ** 4))[:, None].astype(F32)
    q = (E[i % nh] + mu * E[(i + 1) % nh])[None] * F32(11.0) + q * (F32(0.1) * (1 - w))         # the noise keeps off the hot axes
    return q.astype(F32), k.astype(F32), v, do


def equal_keys(rng, b, m, nk):
    q, k, v, do = benign(rng, b, m, nk)
    k[:] = k[:, :1]
    return q, k, v, do


def zero_q(rng, b, m, nk):
    q, k, v, do = benign(rng, b, m, nk)
    q[:] = 0.0
    return q, k, v, do


def k_offset(rng, b, m, nk, target):
    """benign, then K += t_c w_c with one random direction w_c per cloud and t_c found by bisection so that the cloud's
    max |s2| (scale 1 / 8) is `target`."""
    q, k, v, do = benign(rng, b, m, nk)
    w = rng.standard_normal((b, 1, D))
    s0 = np.matmul(_f64(q), _t(_f64(k))) * (0.125 * LOG2E)
    s1 = np.matmul(_f64(q), _t(w)) * (0.125 * LOG2E)
    for c in range(b):
        lo, hi = 0.0, 1e4
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if np.abs(s0[c] + mid * s1[c]).max() < target:
                lo = mid
            else:
                hi = mid
        k[c] += (hi * w[c]).astype(F32)
    return q, k, v, do


def big_logits(rng, b, m, nk, mult):
    q = rng.standard_normal((b, m, D)).astype(F32) * F32(mult)
    k = rng.standard_normal((b, nk, D)).astype(F32) * F32(mult)
    return (q, k) + _vdo(rng, b, m, nk)


BUILDERS = {
    "benign": benign, "ascending": ascending, "descending": descending, "one_hot": one_hot, "equal_keys": equal_keys, "zero_q": zero_q,
    "k_offset70": lambda rng, b, m, nk: k_offset(rng, b, m, nk, 70.0), "k_offset280": lambda rng, b, m, nk: k_offset(rng, b, m, nk, 280.0),
    "big_logits4.5": lambda rng, b, m, nk: big_logits(rng, b, m, nk, 4.5), "big_logits8": lambda rng, b, m, nk: big_logits(rng, b, m, nk, 8.0),
}
WELL = ["benign", "ascending", "descending", "one_hot", "equal_keys", "zero_q"]          # held to 1e-5
ILL = ["k_offset70", "k_offset280", "big_logits4.5", "big_logits8"]                       # held to the float32 restatement


def build(kind, b, m, nk):
    """the inputs of `kind` at a shape, from a seed that depends on both."""
    seed = 100003 * sorted(BUILDERS).index(kind) + 1009 * b + 31 * m + nk
    return BUILDERS[kind](np.random.default_rng(seed), b, m, nk)
