"""CPU tests of tests/train_ops_oracle.py: the explicit-index float64 formulas the GPU tests of the trainer's backward kernels rest on
(tests/test_train_ops_gpu.py) are held to float64 autograd of the forward ops of oracle/train_oracle.py (max_even, gather,
batch_norm, repulsion, adam_step) and torch.softmax at 1e-12 relative, the float32 references to hand-built cases, and the atomic hub
shapes of the GPU tests to what a float32 sum of their terms costs in either order (below 2.5e-6 of the scale, a quarter of the 1e-5
bound).  No kernel runs here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_oracle as TO  # noqa: E402

from oracle import oracle as O  # noqa: E402
from oracle import train_oracle as T  # noqa: E402

F64 = torch.float64
F32 = np.float32


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    assert np.shape(a) == ref.shape
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("rows,n,act", [(7, 5, 1), (300, 24, 1), (64, 130, 0)])
def test_act_bias_grad_matches_autograd(rows, n, act):
    rng = np.random.default_rng(rows)
    Z = rng.standard_normal((rows, n)).astype(F32)                  # the pre-activation; Y = relu(Z + b)
    g = rng.standard_normal((rows, n)).astype(F32)
    zt = torch.tensor(Z, dtype=F64, requires_grad=True)
    bt = torch.zeros(n, dtype=F64, requires_grad=True)
    yt = torch.relu(zt + bt) if act else zt + bt
    yt.backward(torch.tensor(g, dtype=F64))
    dZ, db = TO.act_bias_grad(g, yt.detach().numpy().astype(F32), act)
    assert dZ.dtype == F32 and np.array_equal(dZ, zt.grad.numpy().astype(F32))
    assert rel(db, bt.grad.numpy()) <= 1e-12


def test_act_bias_grad_zero_is_not_positive():
    dY = np.array([[1, 2, 3, 4]], F32)
    Y = np.array([[0.0, -0.0, 1e-30, -1.0]], F32)
    dZ, db = TO.act_bias_grad(dY, Y, 1)
    assert dZ.tolist() == [[0, 0, 3, 0]] and db.tolist() == [0, 0, 3, 0]
    assert TO.act_bias_grad(dY, Y, 0)[0].tolist() == dY.tolist()


@pytest.mark.parametrize("rows,ns,c", [(30, 16, 24), (7, 1, 3), (50, 20, 5)])
def test_max_k_grad_matches_autograd(rows, ns, c):
    rng = np.random.default_rng(ns)
    X = TO.with_ties(rng.standard_normal((rows * ns, c)).astype(F32), ns).reshape(rows, ns, c)
    g = rng.standard_normal((rows, c)).astype(F32)
    xt = torch.tensor(X, dtype=F64, requires_grad=True)
    yt = T.max_even(xt, 1)
    yt.backward(torch.tensor(g, dtype=F64))
    assert np.array_equal(TO.max_k(X), yt.detach().numpy().astype(F32))
    assert rel(TO.max_k_grad(X, g), xt.grad.numpy()) <= 1e-12
    if ns > 1:                                                      # the ties are there: all ns share column 0, two share column 2
        d = TO.max_k_grad(X, np.ones((rows, c), F32))
        assert np.allclose(d[:, :, 0], 1.0 / ns) and np.allclose(d[:, 0, 2], 0.5) and np.allclose(d[:, ns - 1, 2], 0.5)


@pytest.mark.parametrize("B,n,k,c,kind", [(2, 64, 16, 24, "random"), (3, 36, 1, 5, "hub"), (1, 100, 20, 48, "self")])
def test_edge_feature_grad_matches_autograd(B, n, k, c, kind):
    rng = np.random.default_rng(n + k)
    idx = TO.knn_like(rng, B, n, k, kind)
    dE = rng.standard_normal((B, n, k, 2 * c)).astype(F32)
    Ft = torch.zeros((B, n, c), dtype=F64, requires_grad=True)
    nbr = T.gather(Ft, torch.tensor(idx.astype(np.int64)))
    cen = Ft[:, :, None, :].expand_as(nbr)
    torch.cat([cen, nbr - cen], -1).backward(torch.tensor(dE, dtype=F64))
    assert rel(TO.edge_feature_grad(dE, idx, c), Ft.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("B,n,k,cf,kind", [(2, 64, 16, 128, "random"), (3, 50, 1, 1, "hub"), (2, 30, 4, 0, "random")])
def test_ps_group_matches_autograd(B, n, k, cf, kind):
    rng = np.random.default_rng(n + cf)
    idx = TO.knn_like(rng, B, n, k, kind)
    xyz = rng.standard_normal((B, n, 3)).astype(F32)
    feat = rng.standard_normal((B, n, cf)).astype(F32)
    g = rng.standard_normal((B, n, k, 6 + cf)).astype(F32)
    xt = torch.tensor(xyz, dtype=F64, requires_grad=True)
    ft = torch.tensor(feat, dtype=F64, requires_grad=True)
    it = torch.tensor(idx.astype(np.int64))
    gx = T.gather(xt, it)
    ref = torch.cat([gx - xt[:, :, None, :], gx, T.gather(ft, it)], -1)
    ref.backward(torch.tensor(g, dtype=F64))
    gf = TO.ps_group(xyz, feat, idx)
    assert gf.dtype == F32 and rel(gf, ref.detach().numpy()) <= 1e-6          # one float32 subtraction away from float64
    assert np.array_equal(gf[..., 3:], ref.detach().numpy()[..., 3:].astype(F32))
    dxyz, dfeat = TO.ps_group_grad(g, idx, cf)
    assert rel(dxyz, xt.grad.numpy()) <= 1e-12
    if cf:
        assert rel(dfeat, ft.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("rows,k,c,t", [(5, 16, 128, 16), (3, 4, 7, 2)])
def test_point_matmul_grad_matches_autograd(rows, k, c, t):
    rng = np.random.default_rng(rows)
    X2, wv = rng.standard_normal((rows, k, c)).astype(F32), rng.standard_normal((rows, k, t)).astype(F32)
    do = rng.standard_normal((rows, c * t)).astype(F32)
    xt, wt = torch.tensor(X2, dtype=F64, requires_grad=True), torch.tensor(wv, dtype=F64, requires_grad=True)
    (xt.transpose(1, 2) @ wt).reshape(rows, c * t).backward(torch.tensor(do, dtype=F64))
    dX2, dwv = TO.point_matmul_grad(X2, wv, do)
    assert rel(dX2, xt.grad.numpy()) <= 1e-12 and rel(dwv, wt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("rows,n,mul", [(5, 65, 0.125), (2, 1000, 1.0), (3, 1, 0.125)])
def test_softmax_rows_grad_matches_autograd(rows, n, mul):
    rng = np.random.default_rng(n)
    S = rng.standard_normal((rows, n)) * 4
    g = rng.standard_normal((rows, n))
    st = torch.tensor(S, dtype=F64, requires_grad=True)
    P = torch.softmax(st * mul, -1)
    P.backward(torch.tensor(g, dtype=F64))
    got = TO.softmax_rows_grad(P.detach().numpy(), g, mul)
    if n == 1:
        assert np.abs(got).max() <= 1e-15 and not st.grad.numpy().any()
    else:
        assert rel(got, st.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("rows,c,act", [(2, 1, 0), (300, 16, 1), (1025, 64, 1)])
def test_bn_train_matches_autograd(rows, c, act):
    rng = np.random.default_rng(rows)
    X = (rng.standard_normal((rows, c)) * rng.uniform(0.5, 2, c) + rng.standard_normal(c)).astype(F32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(F32), (rng.standard_normal(c) * 0.1).astype(F32)
    mm0, mv0 = rng.standard_normal(c).astype(F32), rng.uniform(0.5, 1.5, c).astype(F32)
    g = rng.standard_normal((rows, c)).astype(F32)
    Pt = {"s/gamma": torch.tensor(gamma, dtype=F64, requires_grad=True), "s/beta": torch.tensor(beta, dtype=F64, requires_grad=True),
          "s/moving_mean": torch.tensor(mm0, dtype=F64), "s/moving_variance": torch.tensor(mv0, dtype=F64)}
    xt = torch.tensor(X, dtype=F64, requires_grad=True)
    state = {}
    yt = T.batch_norm(Pt, "s/", xt, True, state)
    if act:
        yt = torch.relu(yt)
    yt.backward(torch.tensor(g, dtype=F64))
    f = TO.bn_train(X, gamma, beta, 1e-3, T.BN_DECAY, act, mm0, mv0)
    assert rel(f["y"], yt.detach().numpy()) <= 1e-12
    assert rel(f["moving_mean"], state["moving_mean"].numpy()) <= 1e-12
    assert rel(f["moving_var"], state["moving_variance"].numpy()) <= 1e-12
    dx, dga, dbe = TO.bn_train_grad(X, f["y"] > 0 if act else np.ones((rows, c), bool), g, gamma, 1e-3)
    assert rel(dx, xt.grad.numpy()) <= 1e-11                        # the two subtracted means cancel a few digits
    assert rel(dga, Pt["s/gamma"].grad.numpy()) <= 1e-12 and rel(dbe, Pt["s/beta"].grad.numpy()) <= 1e-12


def test_bn_train_single_row_and_constant_column():
    f = TO.bn_train(np.array([[3.0, -1.0]], F32), [2.0, 2.0], [0.5, -0.5], 1e-3, 0.95, 1, [1.0, 1.0], [1.0, 1.0])
    assert not f["var"].any() and f["y"].tolist() == [[0.5, 0.0]]
    assert np.allclose(f["moving_var"], 0.95) and np.allclose(f["moving_mean"], [0.95 + 0.15, 0.95 - 0.05])
    X = np.stack([np.full(10, 3.0), np.arange(10.0)], 1).astype(F32)
    f = TO.bn_train(X, [1.0, 1.0], [0.25, 0.0], 1e-3, 0.95, 0)
    assert f["var"][0] == 0.0 and (f["y"][:, 0] == 0.25).all() and f["moving_mean"] is None and f["moving_var"] is None


@pytest.mark.parametrize("B,M,ns", [(3, 100, 20), (2, 1024, 20), (17, 64, 5)])
def test_repulsion_grad_matches_autograd(B, M, ns):
    import loss_oracle as LO
    _, pred = LO.jittered_pair(B, M, M, seed=M)
    if M < 1024:
        pred = (pred * (M / 1024.0) ** 0.5).astype(F32)
    idx, _ = O.query_ball_point(0.07, ns, pred, pred)
    pt = torch.tensor(pred, dtype=F64, requires_grad=True)
    T.repulsion(pt, nsample=ns).backward()
    assert np.abs(pt.grad.numpy()).max() > 0
    assert rel(TO.repulsion_grad(pred, idx, 0.001, 1.0 / (B * M * 4)), pt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("n,gscale", [(1, 1.0), (255, 0.5), (5000, 0.5)])
def test_adam_matches_the_oracle(n, gscale):
    rng = np.random.default_rng(n)
    p0, g = rng.standard_normal(n), rng.standard_normal(n)
    g[::7] = 0.0
    state, ref = {}, {"w": p0}
    p_, m, v = p0, np.zeros(n), np.zeros(n)
    for t in range(1, 4):
        ref = T.adam_step(ref, {"w": g * gscale}, state, 1e-3)
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        p_, m, v = TO.adam(p_, g, m, v, lr_t, 0.9, 0.999, 1e-8, gscale)
    assert rel(p_ - p0, ref["w"] - p0) <= 1e-12 and rel(m, state["m"]["w"]) <= 1e-12 and rel(v, state["v"]["w"]) <= 1e-12


def test_adam_zero_gradient_divides_by_eps():
    p_, m, v = TO.adam([1.0], [0.0], [2e-8], [0.0], 1e-3, 0.9, 0.999, 1e-8, 1.0)
    assert v[0] == 0.0 and np.isclose(m[0], 1.8e-8) and np.isclose(p_[0], 1.0 - 1e-3 * 1.8, rtol=1e-12)


def test_fill_rows_and_splitk_finish_by_hand():
    out = TO.fill_rows(np.array([3.0, 0.1], F32), 1.0 / 1024, 4)
    assert out.dtype == F32 and out.shape == (2, 4) and (out[1] == F32(0.1) * F32(1.0 / 1024)).all() and (out[0] == F32(3.0 / 1024)).all()
    # float32 addition is not associative: (1e8 + 1) - 1e8 = 0 in the documented order, 1 if the last two were added first
    parts = [np.array([[1e8, 1.0, -2.0, 0.5]], F32), np.array([[1.0, 1.0, 1.0, 0.25]], F32), np.array([[-1e8, 1.0, 0.5, 0.25]], F32)]
    assert TO.splitk_finish(parts, None, 0).tolist() == [[0.0, 3.0, -0.5, 1.0]]
    assert TO.splitk_finish(parts, np.array([0.0, -4.0, 0.0, 0.0], F32), 1).tolist() == [[0.0, 0.0, 0.0, 1.0]]
    assert TO.splitk_finish(parts[:1], None, 0).tolist() == parts[0].tolist()


# the hub shapes of tests/test_train_ops_gpu.py (EF_CASES / PG_CASES with kind "hub"): n * k atomic terms land on one address, twice
# as many on the hub's xyz (the offset and the position of a neighbour both flow to it)
@pytest.mark.parametrize("terms", [100 * 16, 64 * 16, 2 * 100 * 16])
def test_hub_sums_stay_a_quarter_under_the_bound(terms):
    rng = np.random.default_rng(terms)
    worst, scale = TO.f32_sum_orders(rng.standard_normal((terms, 48)).astype(F32))
    print("float32 sum of %d terms: %.2e of the scale" % (terms, worst / scale))
    assert worst <= 2.5e-6 * scale
    assert TO.f32_sum_orders(np.array([[1e8], [1.0], [-1e8]], F32))[0] == 1.0          # the helper does see a lost term


def test_input_builders():
    rng = np.random.default_rng(0)
    Y = TO.relu_like(rng, (100, 8), (10, 20))
    assert (Y >= 0).all() and 0.3 < (Y[20:] == 0).mean() < 0.7 and np.signbit(Y[10:20]).all() and not np.signbit(Y[20:]).any()
    assert (TO.knn_like(rng, 2, 9, 3, "hub")[0] == 0).all() and TO.knn_like(rng, 2, 9, 3, "hub")[1].any()
    assert (TO.knn_like(rng, 2, 9, 3, "self")[1, 4] == 4).all()
