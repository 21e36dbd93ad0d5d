"""Float64 oracle of the trainer's backward and training-mode kernels, for tests only (csrc/train_ops.hip, dispu_act_bias_grad of
csrc/train_gemm.hip), and the helpers the GPU tests of those kernels share.

Plain numpy with explicit indices and strides, written from the forward ops the kernels differentiate (Common/ops.py, tf_util.py,
math_grad._MinOrMaxGrad, tf.train.AdamOptimizer) and not from the kernels: neighbour indices are ARGUMENTS, so a reference is exact
for whatever indices it is given and no autograd graph is needed -- which is what lets the GPU tests use shapes above the kernels'
grid caps.  Inputs are float32 arrays, widened to float64 before any arithmetic; the copy / mask / fill / ordered-sum references stay
in float32 because the kernels are held to them bit for bit.  tests/test_train_ops_oracle.py holds the float64 formulas to autograd of
oracle/train_oracle.py (max_even, gather, batch_norm, repulsion, adam_step) and torch.softmax at 1e-12.

  act_bias_grad        dZ = dY * (act ? Y > 0 : 1) (float32, exact) and its float64 column sums
  max_k / max_k_grad   maximum over the neighbour axis (float32, exact) / its gradient shared evenly by tied maxima
  edge_feature_grad    scatter of d[F_i | F_j - F_i] back to F
  ps_group(_grad)      [xyz_j - xyz_i | xyz_j | feat_j] (float32, exact) / its scatter to xyz and feat
  point_matmul_grad    both gradients of out[i, c, t] = sum_s X2[i, s, c] wv[i, s, t]
  softmax_rows_grad    mul * P * (dP - rowsum(dP * P))
  bn_train(_grad)      contrib batch_norm in training mode: statistics, moving averages, output / dX, dgamma, dbeta
  repulsion_grad       loss_oracle.repulsion_value_grad
  adam                 one tf.train.AdamOptimizer update of p, m, v
  fill_rows            out[b, j] = val[b] * mul in float32
  splitk_finish        act(((P0 + P1) + ...) + bias) in float32, in that order
  f32_sum_orders       what summing terms in float32 costs, ascending and shuffled (the atomic hub cases)
"""
import ctypes as C

import numpy as np

F32 = np.float32
SENT = -12345.0                 # guard value around and between output columns
INVALID = 1                     # hipErrorInvalidValue


def _f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------ formulas ----
def act_bias_grad(dY, Y, act):
    """dY, Y [rows, n] float32 -> (dZ float32 [rows, n] = dY where Y > 0 (all of dY without act), float64 column sums of dZ [n])."""
    dY = np.asarray(dY, F32)
    dZ = np.where(np.asarray(Y, F32) > 0, dY, F32(0)) if act else dY.copy()
    return dZ, dZ.astype(np.float64).sum(0)


def max_k(X):
    """X [rows, ns, c] -> [rows, c], same dtype."""
    return np.asarray(X).max(1)


def max_k_grad(X, g):
    """X [rows, ns, c], g [rows, c] -> dX float64 [rows, ns, c]: g / (number of entries equal to the maximum) at each of them."""
    X = _f64(X)
    ind = X == X.max(1, keepdims=True)
    return ind * (_f64(g) / ind.sum(1))[:, None, :]


def edge_feature_grad(dE, idx, c):
    """E[b, i, s] = [F_i | F_j - F_i], j = idx[b, i, s]:  dE [B, n, k, 2c], idx [B, n, k] (cloud-local) -> dF float64 [B, n, c] with
    dF_i = sum_s (dE[i, s, :c] - dE[i, s, c:]) and dF_j += dE[i, s, c:] for every pair."""
    dE, idx = _f64(dE), np.asarray(idx, np.int64)
    B, n, k = idx.shape
    assert dE.shape == (B, n, k, 2 * c) and idx.min() >= 0 and idx.max() < n
    dF = (dE[..., :c] - dE[..., c:]).sum(2)
    np.add.at(dF, (np.broadcast_to(np.arange(B)[:, None, None], idx.shape), idx), dE[..., c:])
    return dF


def ps_group(xyz, feat, idx):
    """xyz [B, n, 3], feat [B, n, cf], idx [B, n, k] -> gf float32 [B, n, k, 6 + cf] (one float32 subtraction, copies otherwise)."""
    xyz, feat, idx = np.asarray(xyz, F32), np.asarray(feat, F32), np.asarray(idx, np.int64)
    bi = np.arange(xyz.shape[0])[:, None, None]
    gx = xyz[bi, idx]
    return np.concatenate([gx - xyz[:, :, None, :], gx, feat[bi, idx]], -1)


def ps_group_grad(dgf, idx, cf):
    """dgf [B, n, k, 6 + cf] -> (dxyz float64 [B, n, 3], dfeat float64 [B, n, cf])."""
    dgf, idx = _f64(dgf), np.asarray(idx, np.int64)
    B, n, k = idx.shape
    assert dgf.shape == (B, n, k, 6 + cf)
    bi = np.broadcast_to(np.arange(B)[:, None, None], idx.shape)
    dxyz = -dgf[..., 0:3].sum(2)
    np.add.at(dxyz, (bi, idx), dgf[..., 0:3] + dgf[..., 3:6])
    dfeat = np.zeros((B, n, cf))
    np.add.at(dfeat, (bi, idx), dgf[..., 6:])
    return dxyz, dfeat


def point_matmul_grad(X2, wv, dout):
    """out[i, c * T + t] = sum_s X2[i, s, c] wv[i, s, t]:  X2 [rows, k, c], wv [rows, k, T], dout [rows, c * T] ->
    (dX2[i, s, c] = sum_t dout[i, c, t] wv[i, s, t],  dwv[i, s, t] = sum_c X2[i, s, c] dout[i, c, t]), float64."""
    X2, wv = _f64(X2), _f64(wv)
    do = _f64(dout).reshape(X2.shape[0], X2.shape[2], wv.shape[2])
    return np.matmul(wv, do.transpose(0, 2, 1)), np.matmul(X2, do)


def softmax_rows_grad(P, dP, mul):
    """S -> P = softmax(mul * S):  dS = mul * P * (dP - sum_j dP_j P_j), rows of P [rows, n]."""
    P, dP = _f64(P), _f64(dP)
    return mul * P * (dP - (dP * P).sum(-1, keepdims=True))


def bn_train(X, gamma, beta, eps, decay, act, moving_mean=None, moving_var=None):
    """X [rows, c] -> dict(mean, var (biased), istd, pre (gamma * xhat + beta), y (relu(pre) with act), moving_mean, moving_var): the
    moving averages are decay * moving + (1 - decay) * batch with the Bessel-corrected variance (the biased one for a single row)."""
    X, gamma, beta = _f64(X), _f64(gamma), _f64(beta)
    rows = X.shape[0]
    mean = X.mean(0)
    var = ((X - mean) ** 2).mean(0)
    istd = 1.0 / np.sqrt(var + eps)
    pre = (X - mean) * istd * gamma + beta
    out = dict(mean=mean, var=var, istd=istd, pre=pre, y=np.maximum(pre, 0.0) if act else pre, moving_mean=None, moving_var=None)
    if moving_mean is not None:
        out["moving_mean"] = decay * _f64(moving_mean) + (1.0 - decay) * mean
    if moving_var is not None:
        out["moving_var"] = decay * _f64(moving_var) + (1.0 - decay) * var * (rows / (rows - 1.0) if rows > 1 else 1.0)
    return out


def bn_train_grad(X, keep, dY, gamma, eps):
    """keep [rows, c] bool: where the gradient passes the ReLU (all True without one).  dz = dY * keep;
    dbeta = sum dz, dgamma = sum dz xhat, dX = gamma istd (dz - mean dz - xhat mean(dz xhat)) -> (dX, dgamma, dbeta), float64."""
    X, gamma = _f64(X), _f64(gamma)
    mean = X.mean(0)
    istd = 1.0 / np.sqrt(((X - mean) ** 2).mean(0) + eps)
    xh = (X - mean) * istd
    dz = _f64(dY) * keep
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    m = X.shape[0]
    return gamma * istd * (dz - dbeta / m - xh * (dgamma / m)), dgamma, dbeta


def repulsion_grad(pred, idx, h, scale):
    import loss_oracle as LO
    return LO.repulsion_value_grad(pred, idx, h, scale)[1]


def adam(p, g, m, v, lr_t, beta1, beta2, eps, gscale):
    """-> (p, m, v) after one update with the gradient g * gscale, float64."""
    p, m, v = _f64(p), _f64(m), _f64(v)
    gg = _f64(g) * gscale
    m = beta1 * m + (1.0 - beta1) * gg
    v = beta2 * v + (1.0 - beta2) * gg * gg
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def fill_rows(val, mul, n):
    """val [b] float32 -> out float32 [b, n] = val[b] * mul, one float32 product."""
    return np.repeat((np.asarray(val, F32) * F32(mul))[:, None], n, axis=1)


def splitk_finish(parts, bias, act):
    """parts: list of float32 [rows, n] -> float32 max?(((P0 + P1) + ...) + bias), every addition rounded to float32 in that order."""
    t = np.asarray(parts[0], F32).copy()
    for q in parts[1:]:
        t = t + np.asarray(q, F32)
    if bias is not None:
        t = t + np.asarray(bias, F32)[None, :]
    return np.maximum(t, F32(0)) if act else t


def f32_sum_orders(terms, seed=0):
    """terms [m, ...]: the sum over axis 0 accumulated in float32 one term at a time, in ascending and in a shuffled order ->
    (worst |float32 sum - float64 sum| of either order, largest |float64 sum|).  What an atomic sum into one address may cost."""
    terms = np.asarray(terms, F32)
    ref = terms.astype(np.float64).sum(0)
    worst = 0.0
    for order in (np.arange(terms.shape[0]), np.random.default_rng(seed).permutation(terms.shape[0])):
        worst = max(worst, float(np.abs(np.cumsum(terms[order], axis=0, dtype=F32)[-1].astype(np.float64) - ref).max()))
    return worst, float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------- test inputs ----
def relu_like(rng, shape, neg_zero_rows=None):
    """a ReLU output: max(normal, 0), so half its entries are exact +0.0; rows [a, b) hold -0.0 (never `> 0` either)."""
    Y = np.maximum(rng.standard_normal(shape), 0).astype(F32)
    if neg_zero_rows is not None and Y.shape[0]:
        Y[neg_zero_rows[0]:neg_zero_rows[1]] = F32(-0.0)
    return Y


def knn_like(rng, B, n, k, kind="random"):
    """cloud-local neighbour lists [B, n, k] int32: `random`, `hub` (every neighbour of cloud 0 is its point 0, random elsewhere) or
    `self` (every point is its own only neighbour)."""
    idx = rng.integers(0, n, (B, n, k)).astype(np.int32)
    if kind == "hub":
        idx[0] = 0
    elif kind == "self":
        idx[:] = np.arange(n, dtype=np.int32)[None, :, None]
    return idx


def with_ties(X, ns):
    """X [rows * ns, ld] -> copy with, where the columns exist: column 0 all ns entries equal (an all-tie column), column 1 zero in
    every entry of row-group 5 % rows (an ns-way tie at zero), column 2 negative with the maximum -0.5 in slots 0 and ns - 1."""
    X = X.copy()
    rows = X.shape[0] // ns
    v = X.reshape(rows, ns, -1)
    v[:, :, 0] = v[:, :1, 0]
    if v.shape[2] > 1:
        v[5 % rows, :, 1] = 0.0
    if v.shape[2] > 2:
        v[:, :, 2] = -np.abs(v[:, :, 2]) - 1.0
        v[:, 0, 2] = v[:, ns - 1, 2] = -0.5
    return X


# ------------------------------------------------------------------------------- device helpers of the GPU tests ----
_KEEP = []     # device tensors created inline in a launch's argument list must outlive the launch


def release():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del _KEEP[:]


def dv(a, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if dtype is not None:
        t = t.to(dtype)
    _KEEP.append(t)
    return t


def p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(0)


def N_(t):
    return t.detach().cpu().numpy()


def close(a, ref, rel, what=""):
    """max |a - ref| <= rel * max |ref|, printed before it is asserted."""
    ref = np.asarray(ref, np.float64)
    assert np.shape(a) == ref.shape, "%s: shape %s vs %s" % (what, np.shape(a), ref.shape)
    scale = max(np.abs(ref).max(), 1e-30) if ref.size else 1e-30
    err = np.abs(np.asarray(a, np.float64) - ref).max() if ref.size else 0.0
    print("[measured] %s: max err %.3e of scale %.3e = %.2e (bound %.0e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e > %.0e)" % (what, err, scale, err / scale, rel)
    return err / scale


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Guarded(object):
    """a device float buffer of `n` elements with `g` guard elements of SENT on either side; `fill` goes into the body.  g is a
    multiple of 4, so the body starts 16-byte aligned."""

    def __init__(self, dev, n, fill=SENT, g=64):
        import torch
        self.n, self.g = n, g
        self.t = torch.full((n + 2 * g,), SENT, dtype=torch.float32, device=dev)
        if isinstance(fill, np.ndarray):
            self.t[g:g + n] = torch.from_numpy(np.ascontiguousarray(fill, F32).reshape(-1)).to(dev)
        else:
            self.t[g:g + n] = fill
        _KEEP.append(self.t)

    def ptr(self, off=0):
        return p(self.t, self.g + off)

    def body(self):
        return N_(self.t[self.g:self.g + self.n])

    def guards_intact(self):
        a = N_(self.t)
        return bool((a[:self.g] == F32(SENT)).all() and (a[self.g + self.n:] == F32(SENT)).all())


class Strided(object):
    """a guarded device matrix [rows, ld] of SENT whose columns [off, off + c) hold `data` (SENT when None): an operand or an output as
    a kernel sees it through (pointer + off, stride ld).  After a launch, `data()` is the window and `rest_untouched()` says that the
    guards and every column outside the window still hold what they held."""

    def __init__(self, dev, rows, c, ld=None, off=0, data=None):
        ld = c + off if ld is None else ld
        assert ld >= off + c
        self.rows, self.c, self.ld, self.off = rows, c, ld, off
        self.host = np.full((rows, ld), SENT, F32)
        if data is not None:
            self.host[:, off:off + c] = np.asarray(data, F32).reshape(rows, c)
        self.G = Guarded(dev, rows * ld, fill=self.host)

    def ptr(self):
        return self.G.ptr(self.off)

    def full(self):
        return self.G.body().reshape(self.rows, self.ld)

    def data(self):
        return self.full()[:, self.off:self.off + self.c]

    def rest_untouched(self):
        want = self.host.copy()
        got = self.full().copy()
        want[:, self.off:self.off + self.c] = 0
        got[:, self.off:self.off + self.c] = 0
        return self.G.guards_intact() and same_bits(got, want)

    def untouched(self):
        return self.G.guards_intact() and same_bits(self.full(), self.host)
