"""tests/generator_ops_oracle.py held to the existing oracle (oracle/generator.py, oracle/modules.py) at one tiny shape: composed, the
helpers must give OG.point_shuffle2's pieces, OG.duplicate_up's first layer and the matching lines of oracle/modules.py.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generator_ops_oracle as GO  # noqa: E402
from generator_ops_oracle import EPS32, F32  # noqa: E402

from oracle import generator as OG  # noqa: E402
from oracle import modules as OM  # noqa: E402
from oracle import oracle as O  # noqa: E402

B, N, K = 2, 24, 16
PS = "refine/PointShuffle/"


@pytest.fixture(scope="module")
def P():
    return OG.init_params(7, bias_scale=0.05, bn_random=True)


@pytest.fixture(scope="module")
def ps(P):
    """the tensors OG.point_shuffle2 forms on the way, from its own primitives."""
    rng = np.random.default_rng(11)
    xyz = rng.uniform(-1, 1, (B, N, 3)).astype(F32)
    feat = rng.standard_normal((B, N, 128)).astype(F32)
    idx = O.knn_batch(xyz, xyz, K).astype(np.int64)
    g_xyz = OG.gather(xyz, idx)
    c_xyz = g_xyz - xyz[:, :, None, :]
    gf = np.concatenate([c_xyz, g_xyz, OG.gather(feat, idx)], -1)
    h0 = OG.linear(gf, P[PS + "conv0/weights"], P[PS + "conv0/biases"], relu=True)
    h = OG.linear(h0, P[PS + "conv1/weights"], P[PS + "conv1/biases"], relu=True)
    scale, shift = OG.bn_scale_shift(P, PS + "weight_net/wconv0/bn/")
    w = OG.linear(c_xyz, P[PS + "weight_net/wconv0/weights"], P[PS + "weight_net/wconv0/biases"])
    w = np.maximum(w * scale + shift, F32(0.0))
    hp = OG.matmul_nn(np.ascontiguousarray(h.transpose(0, 1, 3, 2)), w)
    return dict(xyz=xyz, feat=feat, idx=idx, gf=gf, h0=h0, h=h, w=w, hp=hp, scale=scale, shift=shift)


def test_fma32_is_one_rounding():
    """against exact rational arithmetic, on random operands and on sums that sit on a float32 rounding boundary in float64."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(400).astype(F32)
    b = rng.standard_normal(400).astype(F32)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-9, 3, 400)).astype(F32)
    # a * b = 1 + 2^-23 + 2^-46 (a = b = 1 + 2^-23 has a * b = 1 + 2^-22 + 2^-46); c = 2^-24 - 2^-22 ... ties broken by the tail only
    a[:4] = F32(1 + 2.0 ** -23)
    b[:4] = F32(1 + 2.0 ** -23)
    c[:4] = [F32(2.0 ** -24), F32(-2.0 ** -24), F32(3 * 2.0 ** -24), F32(2.0 ** 30)]
    got = GO.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F32(float(exact))                                       # within one float32 ulp of the answer; pick the nearest of 3
        cand = [np.nextafter(lo, F32(-np.inf)), lo, np.nextafter(lo, F32(np.inf))]
        dist = [abs(Fraction(float(v)) - exact) for v in cand]
        best = min(dist)
        winners = [v for v, d in zip(cand, dist) if d == best]
        if len(winners) > 1:                                         # an exact tie: to even
            winners = [v for v in winners if (np.asarray(v, F32).view(np.uint32) & 1) == 0]
        assert got[i] == winners[0], (i, got[i], winners)


def test_ps_prep_gather_sub_relu_is_conv0(P, ps):
    """relu(G[j] - A[i]) = relu(conv0([xyz_j - xyz_i | xyz_j | feat_j])) up to reassociation.  Both sides are float32 sums of the same
    134 products and a bias in different orders; each is off the exact value by a few rounding errors of sum |gf_k| |W0_k| + |b|, so the
    bound is 8 eps32 of that magnitude, per (point, neighbour, channel)."""
    W0, b0 = P[PS + "conv0/weights"], P[PS + "conv0/biases"]
    rows = B * N
    Gf = OG.linear(ps["feat"], W0[6:], None)
    G, A, _, _ = GO.ps_prep(Gf.reshape(rows, -1), ps["xyz"].reshape(rows, 3), W0, b0)
    X1 = GO.gather_sub_relu(G.astype(F32).reshape(B, N, -1), A.astype(F32).reshape(B, N, -1), ps["idx"])
    mag = np.abs(ps["gf"].astype(np.float64)) @ np.abs(W0.astype(np.float64)) + np.abs(b0.astype(np.float64))
    err = np.abs(X1.astype(np.float64) - ps["h0"])
    print("[measured] conv0 split: worst err / magnitude = %.2e (bound %.2e)" % ((err / mag).max(), 8 * EPS32))
    assert X1.shape == ps["h0"].shape and (err <= 8 * EPS32 * mag).all()
    assert (X1 > 0).any() and (X1 == 0).any()


def test_skip_max_is_gf_max(ps):
    assert np.array_equal(GO.skip_max(ps["xyz"], ps["feat"], ps["idx"]), ps["gf"].max(axis=2))


def test_weight_net(P, ps):
    w, mag, sh = GO.weight_net(ps["xyz"], ps["idx"], P[PS + "weight_net/wconv0/weights"], P[PS + "weight_net/wconv0/biases"],
                               ps["scale"], ps["shift"])
    assert w.shape == ps["w"].shape and np.abs(w - ps["w"]).max() <= 1e-6
    assert mag.shape == w.shape and (mag >= 0).all() and sh.shape == (16,)


def test_point_matmul_is_hp(ps):
    rows = B * N
    got = GO.point_matmul(ps["h"].reshape(rows, K, 128), ps["w"].reshape(rows, K, 16))
    assert np.array_equal(got, ps["hp"].reshape(rows, 128 * 16))


def test_dup_grid_is_duplicate_up_first_layer(P):
    rng = np.random.default_rng(3)
    feat = rng.standard_normal((B, N, 480)).astype(F32)
    W, b = P["generator/upshuffle_0/conv1/weights"], P["generator/upshuffle_0/conv1/biases"]
    grid = OG.gen_grid(OG.UP_RATIO)
    # OG.duplicate_up's first linear, on its own concat
    net = np.tile(feat, (1, OG.UP_RATIO, 1))
    g = np.repeat(grid[None, :, None, :], N, axis=2).reshape(1, OG.UP_RATIO * N, 2)
    want = OG.linear(np.concatenate([net, np.broadcast_to(g, (B, OG.UP_RATIO * N, 2))], -1), W, b, relu=True)
    assert np.array_equal(GO.dup_grid_input(feat, grid), np.concatenate([net, np.broadcast_to(g, (B, OG.UP_RATIO * N, 2))], -1))
    got = GO.dup_grid(OG.linear(feat, W[:480], None), W[480:], b, grid)
    assert np.array_equal(got, want)
    assert np.array_equal(OG.linear(got, P["generator/upshuffle_0/conv2/weights"], P["generator/upshuffle_0/conv2/biases"], relu=True),
                          OG.duplicate_up(P, feat))


def test_attention_is_non_local_cell(P):
    rng = np.random.default_rng(5)
    feature = rng.standard_normal((B, 4 * N, 128)).astype(F32)
    s = PS + "PointShuffle/"
    kv = OG.linear(feature, P[s + "conv_kv/weights"], P[s + "conv_kv/biases"])
    q = OG.linear(feature, P[s + "conv_query/weights"], P[s + "conv_query/biases"])
    kk, vv = kv[..., :64], kv[..., 64:]
    att = OG.matmul_nt(q, kk) / F32(8.0)
    att = att - att.max(-1, keepdims=True)
    e = np.exp(att.astype(np.float64))
    want = OG.matmul_nn((e / e.sum(-1, keepdims=True)).astype(F32), vv)
    assert np.abs(GO.attention(q, kk, vv, 0.125) - want).max() <= 1e-6
    Wb, bb = P[s + "conv_back_project/weights"], P[s + "conv_back_project/biases"]
    assert np.abs(GO.attention_project(q, kk, vv, 0.125, Wb, bb) - OG.non_local_cell(P, s, feature)).max() <= 1e-6


def test_mlp_chain_is_coordinate_regressor(P):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((B, N, 256)).astype(F32)
    s = "refine/fine_coordinate_regressor/"
    Wa, ba = P[PS + "aggregation/weights"], P[PS + "aggregation/biases"]
    y1, z = GO.mlp_chain(x, Wa, ba, *[P[s + "fc_layer%d/%s" % (i, t)] for i in range(3) for t in ("weights", "biases")])
    agg = OG.linear(x, Wa, ba, relu=True)
    assert np.array_equal(y1, agg)
    assert np.array_equal(z, OG.coordinate_regressor(P, s, agg, is_off=False))
    R = rng.standard_normal(z.shape).astype(F32)
    assert np.abs(GO.linear_mode1(z, R) - (R + OG.coordinate_regressor(P, s, agg, is_off=True).astype(np.float64))).max() <= 1e-6


def test_pooling_idw_l2_match_modules_oracle():
    rng = np.random.default_rng(8)
    rows, ns, c = 10, 5, 7
    x = rng.standard_normal((2, rows, ns, c)).astype(F32)
    gx = (rng.standard_normal((2, rows, ns, 3)) * 0.1).astype(F32)
    flat, gflat = x.reshape(-1, ns, c), gx.reshape(-1, ns, 3)
    assert np.array_equal(GO.pool_nsample(flat, 0), OM.pool(x, "max").reshape(-1, c))
    assert np.array_equal(GO.pool_nsample(flat, 2), OM.pool(x, "min").reshape(-1, c))
    # the float32 running sum against oracle/modules.py's float64 sum: ns roundings of at most sum |x|
    tol = ns * EPS32 * np.abs(flat).sum(1) / ns
    assert (np.abs(GO.pool_nsample(flat, 1) - OM.pool(x, "avg").reshape(-1, c)) <= tol).all()
    ma = OM.pool(x, "max_and_avg").reshape(-1, 2 * c)
    got = GO.pool_nsample(flat, 4)
    assert np.array_equal(got[:, :c], ma[:, :c]) and (np.abs(got[:, c:] - ma[:, c:]) <= tol).all()
    assert (np.abs(GO.pool_nsample(flat, 5) - flat.astype(np.float64).sum(1)) <= tol * ns).all()
    v3, mag = GO.pool_nsample(flat, 3, gflat)
    assert np.abs(v3 - OM.pool(x, "weighted_avg", gx).reshape(-1, c)).max() <= 1e-6 and mag.shape == v3.shape
    assert np.array_equal(GO.group_center(flat, flat[:, 0]), flat - flat[:, :1])
    # pointnet_fp_module's lines (oracle/modules.py), on distances with zeros
    dist = np.abs(rng.standard_normal((2, 9, 3))).astype(F32)
    dist[0, 0, 1] = 0.0
    dist[1, 2] = 0.0
    inv = F32(1.0) / np.maximum(dist, F32(1e-10))
    norm = (inv[..., 0:1] + inv[..., 1:2]) + inv[..., 2:3]
    got = GO.idw_weights(dist.reshape(-1, 3))
    assert np.array_equal(got, (inv / norm).reshape(-1, 3))
    # three zeros: 1e10 / fl(3e10), a third to the rounding of 3e10 (which float32 does not hold)
    assert (got[9 + 2] == got[9 + 2, 0]).all() and abs(float(got[9 + 2, 0]) - 1.0 / 3.0) <= EPS32 / 3
    # graphsage_conv_layer's lines
    out = rng.standard_normal((2, 9, 8)).astype(F32)
    out[0, 3] = 0.0
    ss = np.zeros(out.shape[:-1], F32)
    for ch in range(out.shape[-1]):
        ss = ss + out[..., ch] * out[..., ch]
    want = out * (F32(1.0) / np.sqrt(np.maximum(ss, F32(1e-12))))[..., None]
    got = GO.l2_normalize_rows(out.reshape(-1, 8)).reshape(out.shape)
    assert (np.abs(got - want) <= 4 * EPS32 * np.abs(got)).all() and (got[0, 3] == 0).all()


def test_edge_feature_scale_add_row_mean_max():
    rng = np.random.default_rng(9)
    F = rng.standard_normal((B, N, 5)).astype(F32)
    idx = rng.integers(0, N, (B, N, 3))
    nbr = OG.gather(F, idx)
    central = np.broadcast_to(F[:, :, None, :], nbr.shape)
    assert np.array_equal(GO.edge_feature(F, idx), np.concatenate([central, nbr - central], -1))      # oracle/modules.py:edge_conv_layer
    x, y = rng.standard_normal(100).astype(F32), rng.standard_normal(100).astype(F32)
    un, fu = GO.scale_add(x, 1.25, y)
    exact = x.astype(np.float64) * 1.25 + y
    assert np.array_equal(un, x * F32(1.25) + y) and (np.abs(fu - exact) <= 0.5 * EPS32 * np.abs(exact) * (1 + EPS32)).all()
    m = rng.standard_normal((3, 17)).astype(F32)
    mean, mx, mabs = GO.row_mean_max(m)
    assert np.allclose(mean, m.astype(np.float64).sum(1) / 17, rtol=1e-15) and np.array_equal(mx, m.max(1)) and (mabs > 0).all()
    assert math.isclose(EPS32, 2.0 ** -23)
