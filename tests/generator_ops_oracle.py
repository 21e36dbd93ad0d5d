"""Reference of the generator's forward glue kernels, for tests only (csrc/mlp_misc.hip, csrc/attention.hip, csrc/modules.hip and the
entry points of csrc/mlp_chain.hip).

Plain numpy with explicit indices and strides, written from the reference ops the kernels implement (Common/ops.py as restated in
oracle/generator.py, Common/pointnet_util.py / gcn_lib as restated in oracle/modules.py) and not from the kernels: neighbour indices
are ARGUMENTS (cloud-local, [B, n, k]), so a reference is exact for whatever indices it is given.  Inputs are float32.  Where a kernel's
arithmetic is a definite sequence of IEEE float32 operations the reference stays in float32 and is meant to be matched bit for bit;
otherwise it widens to float64 and comes with the magnitude its error bound is stated in.  The pinned fmaf chain is
oracle.generator.linear / matmul_nn (real fmaf in C); the single fused multiply-adds needed here (dup_grid's two grid terms, the fused
form scale_add may take) are fma32 below, which is exactly rounded (round-to-odd in float64, then one rounding to float32), not a
float64 product-sum rounded twice.  tests/test_generator_ops_oracle.py holds every helper to oracle/generator.py and oracle/modules.py.

  linear_mode1          R + sigmoid(z) - 0.5 in float64 of a float32 pre-activation z (dispu_linear_small_n mode 1, the chains' mode 1)
  dup_grid_input/_grid  duplicate_up's copy-major [tile(feat) | grid] rows / the chain continued from H = feat . W[:Kf] (float32, exact)
  ps_prep               G + xyz.(Wc + Wr) + b and A = xyz.Wc in float64, with the magnitudes of their bounds
  gather_sub_relu       max(G[j] - A[i], 0) (float32, exact)
  skip_max              max over neighbours of [xyz_j - xyz_i | xyz_j | feat_j] (float32, exact)
  weight_net            relu((dxyz.Ww + bw) * scale + shift) in float64, with the magnitude of its bound
  point_matmul          out[i, c, t] = chain_s X2[i, s, c] wv[i, s, t] (float32, exact)
  attention(_project)   softmax(scale * Q K^T) V (then relu(. W + b)) in float64
  mlp_chain             the four-layer head as oracle.generator.linear calls (float32, exact) -> (Y1, pre-activation of the head)
  pool_nsample          the six pooling modes: float32 in s order (0, 1, 2, 4, 5), float64 with sum |x| (3)
  group_center, idw_weights, edge_feature   float32, exact
  l2_normalize_rows     float64
  scale_add             the float32 results a compiler may produce: unfused and fused
  row_mean_max          float32 max, float64 mean
"""
import numpy as np

from oracle import generator as OG

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)          # 2^-23


def _f64(a):
    return np.asarray(a, np.float64)


def _bi(idx):
    return np.arange(idx.shape[0]).reshape((-1,) + (1,) * (idx.ndim - 1))


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly rounded: the float32 product is exact in float64; its float64 sum with c is made
    round-to-odd with the exact residual of the addition (two-sum), and a round-to-odd float64 rounds to float32 once, correctly."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                  # s + err = p + c exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)                    # inexact and even: one ulp towards the residual makes it odd
    return s.astype(F32)


# ------------------------------------------------------------------------------------------- csrc/mlp_misc.hip ----
def linear_mode1(z, R):
    """Common/ops.py:1106-1108 with `fine = coarse + offset`: R + sigmoid(z) - 0.5, float64, z the float32 pre-activation."""
    z = _f64(z)
    return _f64(R) + 1.0 / (1.0 + np.exp(-z)) - 0.5


def dup_grid_input(feat, grid):
    """Common/ops.py:1161-1185: feat [B, n, Kf], grid [up, 2] -> [B, up * n, Kf + 2]; row r * n + i = [feat[i] | grid[r]] (copy-major)."""
    feat, grid = np.asarray(feat, F32), np.asarray(grid, F32)
    B, n, kf = feat.shape
    up = grid.shape[0]
    out = np.empty((B, up * n, kf + 2), F32)
    for b in range(B):
        for r in range(up):
            out[b, r * n:(r + 1) * n, :kf] = feat[b]
            out[b, r * n:(r + 1) * n, kf:] = grid[r]
    return out


def dup_grid(H, Wg, bias, grid):
    """the 1x1 conv over dup_grid_input's rows continued from H = chain_{k < Kf} feat . W[:Kf]:  H [B, n, co], Wg [2, co] (the two grid
    rows of W) -> relu(fmaf(g_r1, Wg[1], fmaf(g_r0, Wg[0], H[i])) + bias) at row r * n + i, float32."""
    H, Wg, bias, grid = np.asarray(H, F32), np.asarray(Wg, F32), np.asarray(bias, F32), np.asarray(grid, F32)
    B, n, co = H.shape
    up = grid.shape[0]
    out = np.empty((B, up * n, co), F32)
    for r in range(up):
        acc = fma32(grid[r, 1], Wg[1], fma32(grid[r, 0], Wg[0], H))
        out[:, r * n:(r + 1) * n] = np.maximum(acc + bias, F32(0))
    return out


def ps_prep(Gf, xyz, W0, bias):
    """PointShuffle2's conv0 over [xyz_j - xyz_i | xyz_j | feat_j] split by linearity: conv0(i, j) = relu(G[j] - A[i]) with
    G = feat . W0[6:] + xyz . (Wc + Wr) + b, A = xyz . Wc, Wc = W0[0:3], Wr = W0[3:6].  Gf [rows, co] = feat . W0[6:] (float32),
    xyz [rows, 3] -> (G, A, magG, magA) float64; magG = |Gf| + sum |x| |Wc + Wr| + |b| and magA = sum |x| |Wc| are what the
    rounding errors of a float32 evaluation scale with."""
    Gf, x, W0, bias = _f64(Gf), _f64(xyz), _f64(W0), _f64(bias)
    Wc, Ws = W0[0:3], W0[0:3] + W0[3:6]
    G = Gf + x @ Ws + bias
    A = x @ Wc
    return G, A, np.abs(Gf) + np.abs(x) @ np.abs(Ws) + np.abs(bias), np.abs(x) @ np.abs(Wc)


def gather_sub_relu(G, A, idx):
    """G, A [B, n, c] float32, idx [B, n, k] -> X1 [B, n, k, c] = max(G[idx[i, s]] - A[i], 0), one float32 subtraction."""
    G, A, idx = np.asarray(G, F32), np.asarray(A, F32), np.asarray(idx, np.int64)
    return np.maximum(G[_bi(idx), idx] - A[:, :, None, :], F32(0))


def skip_max(xyz, feat, idx):
    """Common/ops.py:1049: max over the k neighbours of [xyz_j - xyz_i | xyz_j | feat_j] -> [B, n, 6 + cf] float32."""
    xyz, feat, idx = np.asarray(xyz, F32), np.asarray(feat, F32), np.asarray(idx, np.int64)
    B, n, k = idx.shape
    out = np.full((B, n, 6 + feat.shape[2]), -np.inf, F32)
    for b in range(B):
        for s in range(k):
            j = idx[b, :, s]
            out[b, :, 0:3] = np.maximum(out[b, :, 0:3], xyz[b, j] - xyz[b])
            out[b, :, 3:6] = np.maximum(out[b, :, 3:6], xyz[b, j])
            out[b, :, 6:] = np.maximum(out[b, :, 6:], feat[b, j])
    return out


def weight_net(xyz, idx, Ww, bw, scale, shift):
    """weight_net_hidden (Common/ops.py:181-191) with inference batch norm folded to scale / shift:
    relu(((xyz_j - xyz_i) . Ww + bw) * scale + shift) -> (w [B, n, k, t_n] float64, mag = (sum |dxyz| |Ww| + |bw|) * |scale| and |shift|)."""
    xyz, idx = np.asarray(xyz, F32), np.asarray(idx, np.int64)
    d = _f64(xyz[_bi(idx), idx] - xyz[:, :, None, :])               # the one float32 subtraction is exact to the kernel's
    Ww, bw, scale, shift = _f64(Ww), _f64(bw), _f64(scale), _f64(shift)
    pre = (d @ Ww + bw) * scale + shift
    mag = (np.abs(d) @ np.abs(Ww) + np.abs(bw)) * np.abs(scale)
    return np.maximum(pre, 0.0), mag, np.abs(shift)


def point_matmul(X2, wv):
    """Common/ops.py:1066-1067: X2 [rows, k, c], wv [rows, k, t] -> [rows, c * t], out[i, c, t] = chain_s X2[i, s, c] wv[i, s, t]."""
    X2, wv = np.asarray(X2, F32), np.asarray(wv, F32)
    out = OG.matmul_nn(np.ascontiguousarray(X2.transpose(0, 2, 1)), wv)
    return out.reshape(X2.shape[0], -1)


# ------------------------------------------------------------------------------------------ csrc/attention.hip ----
def attention(Q, K, V, scale):
    """Common/ops.py:326-339: Q [b, m, d], K, V [b, nk, d] -> softmax(scale * Q K^T) V, float64."""
    Q, K, V = _f64(Q), _f64(K), _f64(V)
    s = np.einsum("bqd,bkd->bqk", Q, K) * float(scale)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    return np.einsum("bqk,bkd->bqd", p / p.sum(-1, keepdims=True), V)


def attention_project(Q, K, V, scale, W, bias):
    """... followed by conv_back_project (ops.py:341-343): relu(. W + bias), float64."""
    return np.maximum(attention(Q, K, V, scale) @ _f64(W) + _f64(bias), 0.0)


# ------------------------------------------------------------------------------------------ csrc/mlp_chain.hip ----
def mlp_chain(X, W1, b1, W2, b2, W3, b3, W4, b4):
    """three ReLU layers and the 3-wide head as the pinned chain -> (Y1 [rows, N1], z [rows, 3] pre-activation), float32."""
    y1 = OG.linear(X, W1, b1, relu=True)
    y = OG.linear(y1, W2, b2, relu=True)
    y = OG.linear(y, W3, b3, relu=True)
    return y1, OG.linear(y, W4, b4, relu=False)


# -------------------------------------------------------------------------------------------- csrc/modules.hip ----
def pool_nsample(X, mode, gxyz=None):
    """Common/pointnet_util.py:121-140 over the nsample axis of X [rows, ns, c]: 0 max | 1 avg | 2 "min" = max(-x), never negated back |
    3 weighted_avg with w_s = exp(-5 |gxyz_s|) / sum_s | 4 [max | avg] | 5 sum.  Sums run in s order in float32 and the average divides
    by float32(ns).  Mode 3 is float64 and returns (value, sum_s |x|)."""
    X = np.asarray(X, F32)
    rows, ns, c = X.shape
    if mode == 3:
        g = _f64(gxyz)
        e = np.exp(-5.0 * np.sqrt((g * g).sum(-1)))                  # [rows, ns]
        w = e / e.sum(1, keepdims=True)
        return (_f64(X) * w[:, :, None]).sum(1), np.abs(_f64(X)).sum(1)
    acc = np.zeros((rows, c), F32)
    for s in range(ns):
        acc = acc + X[:, s]
    avg = acc / F32(ns)
    if mode == 0:
        return X.max(1)
    if mode == 1:
        return avg
    if mode == 2:
        return (-X).max(1)
    if mode == 4:
        return np.concatenate([X.max(1), avg], -1)
    if mode == 5:
        return acc
    raise ValueError(mode)


def group_center(grouped, center):
    """pointnet_util.py:43: grouped [rows, ns, c] - center [rows, c], float32."""
    return np.asarray(grouped, F32) - np.asarray(center, F32)[:, None, :]


def idw_weights(dist):
    """pointnet_util.py:204-208: dist [rows, 3] -> (1 / max(d, 1e-10)) / ((i0 + i1) + i2), float32."""
    inv = F32(1.0) / np.maximum(np.asarray(dist, F32), F32(1e-10))
    norm = (inv[:, 0:1] + inv[:, 1:2]) + inv[:, 2:3]
    return inv / norm


def l2_normalize_rows(X):
    """tf.nn.l2_normalize(x, -1): x / sqrt(max(sum x^2, 1e-12)), float64."""
    X = _f64(X)
    return X / np.sqrt(np.maximum((X * X).sum(-1, keepdims=True), 1e-12))


def scale_add(x, alpha, y):
    """x * alpha + y in float32 -> (two roundings, one rounding): a compiler may contract the pair or not."""
    x, y, alpha = np.asarray(x, F32), np.asarray(y, F32), F32(alpha)
    return x * alpha + y, fma32(x, alpha, y)


def edge_feature(F, idx):
    """tf_util.get_edge_feature: F [B, n, c], idx [B, n, k] -> [B, n, k, 2c] = [F_i | F_j - F_i], float32."""
    F, idx = np.asarray(F, F32), np.asarray(idx, np.int64)
    nbr = F[_bi(idx), idx]
    central = np.broadcast_to(F[:, :, None, :], nbr.shape)
    return np.concatenate([central, nbr - central], -1)


def row_mean_max(x):
    """x [b, n] -> (mean float64, max float32, mean |x| float64)."""
    x = np.asarray(x, F32)
    return _f64(x).mean(1), x.max(1), np.abs(_f64(x)).mean(1)
