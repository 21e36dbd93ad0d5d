"""GPU parity of the training step (DisPU/model.py:68-87,158-178 counterpart) against oracle/train_oracle.py, the
float64 torch-autograd restatement of the reference's TF1 graph.  Tolerances: training-mode forward 1e-5 (the
north_star bound for fp32); every backward kernel alone 1e-5 against float64 autograd of its forward op.
End to end the loss is only piecewise smooth (ReLU masks, max-pool arg-max, Chamfer arg-min, repulsion top-k): an
fp32 forward picks a different branch than the float64 oracle at a handful of near-ties, which changes the
gradient of the affected ROWS by O(1) while everything else agrees to ~1e-6.  The end-to-end checks are therefore
row-wise and robust: median row error <= 1e-5 and <= 1 % of rows off by more than 1e-3 for the activation
gradients, relative L2 <= 3e-3 (and max <= 2e-2 of the largest entry) for the parameter gradients -- a wrong or
missing term moves these by orders of magnitude more (the reference's own gradient tests use 1e-4 on single ops,
tf_grouping_op_test.py:23-25).
The kernels between the generator's output and its first gradient (Chamfer value / gradient, fused repulsion, pu_loss_finalize,
transpose_batched, sigmoid_offset, dup_sum_grad, add3) have their own tests against float64 in tests/test_train_loss_gpu.py.
The "kernels" section below visits each backward kernel at one small shape; tests/test_train_ops_gpu.py runs the same kernels on every
path of their launch code (grid caps, float4 / scalar switches, strides, ties, exact zeros, NULL outputs, refusals) against the
explicit-index float64 formulas of tests/train_ops_oracle.py, and tests/test_train_fused_gpu.py the fused PointShuffle2 backward kernels
at the trainer's own shapes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_checks as K  # noqa: E402

from oracle import generator as OG  # noqa: E402
from oracle import train_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64


def N(t):
    return t.detach().cpu().numpy()


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


def close(a, ref, rel, what=""):
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(np.asarray(a, np.float64) - ref).max()
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------- kernels ----
@pytest.mark.parametrize("batch,M,K,N,ldx,ldz,acc", [(1, 1000, 48, 24, 120, 120, 1), (1, 5000, 134, 128, 134, 128, 1),
                                                      (1, 4096, 2048, 256, 2048, 256, 0), (3, 1024, 1024, 64, 1024, 64, 0),
                                                      (1, 777, 3, 16, 134, 16, 1), (1, 64, 2, 256, 2, 256, 1), (1, 1, 5, 7, 5, 7, 0),
                                                      # narrow outputs (N <= 64, K <= 256, M >= 4096): the wave-per-tile kernel
                                                      (1, 32768, 96, 24, 168, 120, 1), (1, 8192, 72, 24, 120, 24, 0), (1, 4100, 240, 48, 480, 48, 1),
                                                      (1, 20000, 3, 16, 134, 16, 1), (1, 4096, 256, 64, 256, 64, 0)])
def test_linear_tn(dev, L, batch, M, K, N, ldx, ldz, acc):
    rng = np.random.default_rng(M + K)
    X = rng.standard_normal((batch, M, ldx)).astype(np.float32)
    Z = rng.standard_normal((batch, M, ldz)).astype(np.float32)
    out0 = rng.standard_normal((batch, K, N)).astype(np.float32)
    ref = np.einsum("zmk,zmn->zkn", X[:, :, :K].astype(np.float64), Z[:, :, :N].astype(np.float64)) + (out0 if acc else 0)
    x, z, o = dv(X, dev), dv(Z, dev), dv(out0, dev)
    db0 = rng.standard_normal(N).astype(np.float32)
    db = dv(db0, dev)
    need = L.lib().dispu_linear_tn_scratch_floats(batch, M, K, N)
    sc = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_linear_tn(batch, M, K, N, p(x), ldx, M * ldx, p(z), ldz, M * ldz, p(o), N, K * N, acc, p(db), p(sc),
                                    sc.numel(), L.stream_ptr(dev)), "linear_tn")
    close(N_(o), ref, 2e-5 if M > 2000 else 1e-5, "linear_tn")
    close(N_(db), db0 + Z[:, :, :N].astype(np.float64).sum((0, 1)), 2e-5, "linear_tn bias row")
    if not acc:     # without a bias request a single split writes the result directly
        o2 = torch.empty((batch, K, N), dtype=torch.float32, device=dev)
        L.check(L.lib().dispu_linear_tn(batch, M, K, N, p(x), ldx, M * ldx, p(z), ldz, M * ldz, p(o2), N, K * N, 0, None, p(sc),
                                        sc.numel(), L.stream_ptr(dev)), "linear_tn")
        assert torch.equal(o2, o)


def N_(t):
    return t.detach().cpu().numpy()


def test_act_bias_grad(dev, L):
    rng = np.random.default_rng(3)
    rows, n, ld = 3001, 24, 120
    dY = rng.standard_normal((rows, ld)).astype(np.float32)
    Y = rng.standard_normal((rows, ld)).astype(np.float32)
    db0 = rng.standard_normal(n).astype(np.float32)
    dy, y, db = dv(dY, dev), dv(Y, dev), dv(db0, dev)
    sc = torch.empty(L.lib().dispu_act_bias_grad_scratch_floats(rows, n), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_act_bias_grad(rows, n, p(dy, 48), ld, p(y, 48), ld, 1, p(dy, 48), ld, p(db), 1, p(sc), sc.numel(),
                                        L.stream_ptr(dev)), "act_bias_grad")
    ref = dY.copy()
    ref[:, 48:72] = dY[:, 48:72] * (Y[:, 48:72] > 0)
    assert np.array_equal(N_(dy), ref)
    close(N_(db), db0 + ref[:, 48:72].astype(np.float64).sum(0), 1e-5, "db")


def test_max_k_and_grad(dev, L):
    rng = np.random.default_rng(4)
    rows, ns, c, ld = 300, 16, 96, 120
    X = rng.standard_normal((rows * ns, ld)).astype(np.float32)
    X[:, 72:96] = np.repeat(X[::ns, 72:96], ns, axis=0)            # the `central` columns: all ns entries tie
    X[5 * ns:6 * ns, 3] = 0.0                                     # a 16-way tie at zero
    x = dv(X, dev)
    y = torch.empty((rows, c), dtype=torch.float32, device=dev)
    st = L.stream_ptr(dev)
    L.check(L.lib().dispu_max_k(rows, ns, c, p(x), ld, p(y), c, st), "max_k")
    assert np.array_equal(N_(y), X.reshape(rows, ns, ld)[:, :, :c].max(1))
    g = rng.standard_normal((rows, c)).astype(np.float32)
    dx = torch.zeros((rows * ns, ld), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_max_k_grad(rows, ns, c, p(x), ld, p(y), c, p(dv(g, dev)), c, p(dx), ld, 0, st), "max_k_grad")
    xt = torch.tensor(X.reshape(rows, ns, ld)[:, :, :c], dtype=F64, requires_grad=True)
    T.max_even(xt, 1).backward(torch.tensor(g, dtype=F64))
    close(N_(dx).reshape(rows, ns, ld)[:, :, :c], xt.grad.numpy(), 1e-6, "max_k_grad")
    assert not N_(dx)[:, c:].any()
    # the variant that also clears `tail` columns behind the pooled ones (and nothing past them)
    dx2 = torch.full((rows * ns, ld), 7.0, dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_max_k_grad_tail(rows, ns, c, 20, p(x), ld, p(y), c, p(dv(g, dev)), c, p(dx2), ld, st), "max_k_grad_tail")
    assert torch.equal(dx2[:, :c], dx[:, :c]) and not bool(dx2[:, c:c + 20].any()) and bool((dx2[:, c + 20:] == 7.0).all())


def test_edge_feature_grad(dev, L):
    rng = np.random.default_rng(5)
    B, n, k, c = 2, 64, 16, 24
    idx = rng.integers(0, n, (B * n, k + 1)).astype(np.int32)
    dE = rng.standard_normal((B * n * k, 2 * c + 8)).astype(np.float32)
    dF = torch.zeros((B * n, c), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_edge_feature_grad(B * n, n, k, c, p(dv(dE, dev), 8), 2 * c + 8, p(dv(idx, dev, torch.int32)), k + 1, 1,
                                            p(dF), c, L.stream_ptr(dev)), "edge_feature_grad")
    Ft = torch.zeros((B, n, c), dtype=F64, requires_grad=True)
    it = torch.tensor(idx[:, 1:].reshape(B, n, k).astype(np.int64))
    nbr = T.gather(Ft, it)
    cen = Ft[:, :, None, :].expand_as(nbr)
    E = torch.cat([cen, nbr - cen], -1)
    E.backward(torch.tensor(dE[:, 8:].reshape(B, n, k, 2 * c), dtype=F64))
    close(N_(dF).reshape(B, n, c), Ft.grad.numpy(), 1e-5, "edge_feature_grad")


def test_ps_group_and_grad(dev, L):
    rng = np.random.default_rng(6)
    B, n, k, cf = 2, 128, 16, 128
    xyz = rng.standard_normal((B, n, 3)).astype(np.float32)
    feat = rng.standard_normal((B, n, cf)).astype(np.float32)
    idx = rng.integers(0, n, (B, n, k)).astype(np.int32)
    gf = torch.empty((B * n * k, 6 + cf), dtype=torch.float32, device=dev)
    st = L.stream_ptr(dev)
    di = dv(idx, dev, torch.int32)
    L.check(L.lib().dispu_ps_group(B * n, n, k, cf, p(di), p(dv(xyz, dev)), p(dv(feat, dev)), cf, p(gf), 6 + cf, st), "ps_group")
    xt = torch.tensor(xyz, dtype=F64, requires_grad=True)
    ft = torch.tensor(feat, dtype=F64, requires_grad=True)
    it = torch.tensor(idx.astype(np.int64))
    gx = T.gather(xt, it)
    ref = torch.cat([gx - xt[:, :, None, :], gx, T.gather(ft, it)], -1)
    assert np.array_equal(N_(gf).reshape(B, n, k, 6 + cf), ref.detach().numpy().astype(np.float32))
    g = rng.standard_normal((B * n * k, 6 + cf)).astype(np.float32)
    ref.backward(torch.tensor(g.reshape(B, n, k, 6 + cf), dtype=F64))
    dxyz = torch.zeros((B * n, 3), dtype=torch.float32, device=dev)
    dfeat = torch.zeros((B * n, cf), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_ps_group_grad(B * n, n, k, cf, p(di), p(dv(g, dev)), 6 + cf, p(dxyz), p(dfeat), cf, st), "ps_group_grad")
    close(N_(dxyz).reshape(B, n, 3), xt.grad.numpy(), 1e-5, "dxyz")
    close(N_(dfeat).reshape(B, n, cf), ft.grad.numpy(), 1e-5, "dfeat")


def test_point_matmul_grad(dev, L):
    rng = np.random.default_rng(7)
    rows, k, c, t = 37, 16, 128, 16
    X2 = rng.standard_normal((rows * k, c)).astype(np.float32)
    wv = rng.standard_normal((rows * k, t)).astype(np.float32)
    do = rng.standard_normal((rows, c * t)).astype(np.float32)
    dX2 = torch.empty((rows * k, c), dtype=torch.float32, device=dev)
    dwv = torch.empty((rows * k, t), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_ps_point_matmul_grad(rows, k, c, t, p(dv(X2, dev)), c, p(dv(wv, dev)), p(dv(do, dev)), c * t, p(dX2), c,
                                               p(dwv), L.stream_ptr(dev)), "point_matmul_grad")
    xt = torch.tensor(X2.reshape(rows, k, c), dtype=F64, requires_grad=True)
    wt = torch.tensor(wv.reshape(rows, k, t), dtype=F64, requires_grad=True)
    (xt.transpose(1, 2) @ wt).reshape(rows, c * t).backward(torch.tensor(do, dtype=F64))
    close(N_(dX2).reshape(rows, k, c), xt.grad.numpy(), 1e-5, "dX2")
    close(N_(dwv).reshape(rows, k, t), wt.grad.numpy(), 1e-5, "dwv")


def test_softmax_grad(dev, L):
    rng = np.random.default_rng(8)
    rows, n = 50, 1024
    S = rng.standard_normal((rows, n)).astype(np.float32) * 4
    g = rng.standard_normal((rows, n)).astype(np.float32)
    st_ = torch.tensor(S, dtype=F64, requires_grad=True)
    Pm = torch.softmax(st_ * 0.125, -1)
    Pm.backward(torch.tensor(g, dtype=F64))
    dP = dv(g, dev)
    L.check(L.lib().dispu_softmax_rows_grad(rows, n, 0.125, p(dv(Pm.detach().numpy(), dev)), n, p(dP), n, L.stream_ptr(dev)), "softmax_grad")
    close(N_(dP), st_.grad.numpy(), 1e-5, "softmax_grad")


def test_bn_train_and_grad(dev, L):
    rng = np.random.default_rng(9)
    rows, c = 40000, 16
    X = (rng.standard_normal((rows, c)) * rng.uniform(0.5, 2, c) + rng.standard_normal(c)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = (rng.standard_normal(c) * 0.1).astype(np.float32)
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)
    g = rng.standard_normal((rows, c)).astype(np.float32)
    st = L.stream_ptr(dev)
    x, y = dv(X, dev), torch.empty((rows, c), dtype=torch.float32, device=dev)
    stats = torch.empty(3 * c, dtype=torch.float32, device=dev)
    mm, mv = dv(mm0, dev), dv(mv0, dev)
    nb = L.lib().dispu_bn_scratch_bytes(rows, c)
    sc = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    ga, be = dv(gamma, dev), dv(beta, dev)
    L.check(L.lib().dispu_bn_train(rows, c, p(x), c, p(ga), p(be), 1e-3, 0.95, 1, p(y), c, p(stats), p(mm), p(mv), p(sc), nb, st), "bn_train")
    Pt = {"s/gamma": torch.tensor(gamma, dtype=F64, requires_grad=True), "s/beta": torch.tensor(beta, dtype=F64, requires_grad=True),
          "s/moving_mean": torch.tensor(mm0, dtype=F64), "s/moving_variance": torch.tensor(mv0, dtype=F64)}
    xt = torch.tensor(X, dtype=F64, requires_grad=True)
    state = {}
    yt = torch.relu(T.batch_norm(Pt, "s/", xt, True, state))
    close(N_(y), yt.detach().numpy(), 1e-5, "bn forward")
    close(N_(mm), state["moving_mean"].numpy(), 1e-6, "moving_mean")
    close(N_(mv), state["moving_variance"].numpy(), 1e-6, "moving_variance")
    yt.backward(torch.tensor(g, dtype=F64))
    dx = torch.empty((rows, c), dtype=torch.float32, device=dev)
    dga, dbe = torch.zeros(c, dtype=torch.float32, device=dev), torch.zeros(c, dtype=torch.float32, device=dev)
    sums = torch.empty(2 * c, dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_bn_train_grad(rows, c, p(x), c, p(y), c, p(dv(g, dev)), c, p(stats), p(ga), 1, p(dx), c, p(dga), p(dbe),
                                        p(sums), p(sc), nb, st), "bn_train_grad")
    close(N_(dx), xt.grad.numpy(), 2e-5, "bn dx")
    close(N_(dga), Pt["s/gamma"].grad.numpy(), 1e-5, "dgamma")
    close(N_(dbe), Pt["s/beta"].grad.numpy(), 1e-5, "dbeta")


def test_repulsion_grad(dev, L):
    from dispu_amd import synth
    from oracle import oracle as O
    _, gt = synth.patch_with_gt(2, 256, 1024, seed=3)
    pred = gt.astype(np.float32)
    idx, _ = O.query_ball_point(0.07, 20, pred, pred)
    pt = torch.tensor(pred, dtype=F64, requires_grad=True)
    T.repulsion(pt).backward()
    dpred = torch.zeros((2 * 1024, 3), dtype=torch.float32, device=dev)
    L.check(L.lib().dispu_repulsion_grad(2 * 1024, 1024, 20, 0.001, 1.0 / (2 * 1024 * 4), p(dv(pred, dev)), p(dv(idx, dev, torch.int32)),
                                         p(dpred), L.stream_ptr(dev)), "repulsion_grad")
    assert np.abs(pt.grad.numpy()).max() > 0
    close(N_(dpred).reshape(2, 1024, 3), pt.grad.numpy(), 1e-4, "repulsion_grad")


def test_adam(dev, L):
    rng = np.random.default_rng(10)
    n = 5000
    p0, g0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    P = {"w": p0}
    state = {}
    pt, gt_, m, v = dv(p0, dev), dv(g0 * 2, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ref = P
    for t in range(1, 4):
        ref = T.adam_step(ref, {"w": g0.astype(np.float64)}, state, 1e-3)
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        L.check(L.lib().dispu_adam(n, p(pt), p(gt_), p(m), p(v), lr_t, 0.9, 0.999, 1e-8, 0.5, L.stream_ptr(dev)), "adam")
    close(N_(pt) - p0, ref["w"] - p0, 1e-4, "adam update")


# ------------------------------------------------------------------------------------------- end to end ----
@pytest.fixture(scope="module")
def step(dev):
    """the step at (2, 256) on synth seed 5, radii (1.0, 1.3): one oracle evaluation and one fresh Trainer (tests/train_step_checks.py,
    which holds the checks below for every shape; tests/test_train_shapes_gpu.py runs them where train.py takes another path)"""
    return K.run_step(dev, 2, 256, 5)


def test_training_forward(step):
    K.check_training_forward(step, 2, 256)


def test_forward_intermediates(step):
    K.check_intermediates(step, 2, 256)


def test_loss_terms(step):
    K.check_loss_terms(step, 2, 256)


def test_activation_gradients_rowwise(step):
    K.check_activation_gradients_rowwise(step, 2, 256)


def test_gradients(step):
    K.check_gradients(step, 2, 256)


def test_train_step_matches_oracle_adam(step, dev):
    """a fresh Trainer.train_step == oracle loss_and_grads + adam_step (first step, t = 1)."""
    K.check_train_step_matches_oracle_adam(step, 2, 256, dev)


def test_loss_decreases(dev):
    """ten steps on one fixed batch reduce pu_loss (sanity of signs / scaling end to end)."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=1234)
    x, gt = synth.patch_with_gt(4, 256, 1024, seed=9)
    tr = Trainer(params=P, device=dev)
    xs, gs, rs = dv(x, dev), dv(gt, dev), torch.ones(4, device=dev)
    losses = [float(tr.train_step(xs, gs, rs)["pu_loss"]) for _ in range(10)]
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.7 * losses[0], losses


@pytest.mark.parametrize("dtype,B", [("f32", 4), ("bf16", 4), ("f32", 3), ("f32", 8)])
def test_weight_gradients_on_second_stream(dev, dtype, B):
    """The dW products of a step run on a second HIP stream next to the dX chain (schedule.py:StepSchedule.fork_point / side_stream / join).  Same kernels, same
    operands: the gradients equal the single-stream step's up to the order-free fp32 atomics of the scatter gradients
    (max_k / group / nn_distance, like the reference's) -- 1e-5 of each tensor's largest entry, run to run as well."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=1234, bias_scale=0.05)
    x, gt = synth.patch_with_gt(B, 256, 1024, seed=11)
    xs, gs, rs = dv(x, dev), dv(gt, dev), torch.ones(B, device=dev)

    def passes(overlap):
        tr = Trainer(params=P, device=dev, dtype=dtype)
        tr.overlap_dw = overlap
        out = []
        for _ in range(5):                       # same parameters every pass: no Adam in between
            tr.zero_grad()
            tr.forward(xs)
            tr.loss_backward(gs, rs)
            tr.backward()
            torch.cuda.synchronize()
            out.append({k: v.clone() for k, v in tr.G.items()})
        return tr, out

    tr_o, g_o = passes(True)
    tr_s, g_s = passes(False)
    assert tr_o.sched.side_streams and not tr_s.sched.side_streams
    # bf16 products: an fp32 ulp of atomics noise upstream can flip an operand's bf16 rounding (2^-9 relative) downstream
    tol = 1e-5 if dtype == "f32" else 1e-3
    for k in g_o[0]:
        scale = float(g_s[0][k].abs().max()) + 1e-12
        for a in (g_o[0], g_o[1], g_o[2], g_o[3], g_o[4], g_s[1], g_s[4]):
            assert float((a[k] - g_s[0][k]).abs().max()) <= tol * scale + 2e-6, k     # + rounding noise of gradients that are 0


def test_repulsion_term_equals_loss_utils(step, dev):
    """Trainer's repulsion term and loss_utils.get_repulsion_loss use the same ball-query arithmetic (CONTRACT, the
    nvcc form of tf_grouping_g.cu:3-36) -> the same value on the same cloud (loss_utils.py:271-298)."""
    from dispu_amd import loss_utils
    tr = step["tr"]
    fine = tr._ws[(2, 256)]["fine"]
    want = float(loss_utils.get_repulsion_loss(fine.clone()))
    got = float(step["t"]["repulsion_loss"])
    assert abs(got - tr.opts.repulsion_w * want) <= 1e-7 * max(1.0, abs(want)), (got, want)


def test_train_step_refuses_bad_targets(dev):
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    tr = Trainer(params=OG.init_params(seed=3), device=dev)
    x, gt = synth.patch_with_gt(2, 256, 1024, seed=9)
    tx, tg, r = dv(x, dev), dv(gt, dev), torch.ones(2, device=dev)
    with pytest.raises(ValueError):
        tr.train_step(tx, torch.cat([tg, tg], dim=1), r)            # more than 4N ground-truth points
    with pytest.raises(ValueError):
        tr.train_step(tx, tg[:1], r)                                # batch mismatch
    with pytest.raises(ValueError):
        tr.train_step(tx, tg.cpu(), r)                              # host tensor
    with pytest.raises(TypeError):
        tr.train_step(tx, tg.double(), r)
    with pytest.raises(ValueError):
        tr.train_step(tx, tg, torch.ones(3, device=dev))


def test_generator_is_training_routes_to_training_forward(step, dev):
    """Generator(opts, is_training=True)(inputs) (DisPU/generator.py:22-31, DisPU/model.py:68) = the training-mode forward:
    BatchNorm on batch statistics, moving averages updated; same values as Trainer.forward on the same variables."""
    from dispu_amd.generator import Generator
    gen = Generator(is_training=True, params=step["P"], device=dev)
    c, f = gen(dv(step["x"], dev))
    close(N_(c), step["ref"]["coarse"], 1e-5, "coarse")
    close(N_(f), step["ref"]["fine"], 1e-5, "fine")
    close(N_(gen.trainer.moving_mean), step["ref"]["bn"]["moving_mean"], 1e-5, "moving_mean")
    # and it differs from the inference graph exactly by the BatchNorm statistics
    ci, fi = Generator(is_training=False, params=step["P"], device=dev)(dv(step["x"], dev))
    assert np.array_equal(N_(ci), N_(c)) or np.abs(N_(ci) - N_(c)).max() < 1e-5      # coarse does not depend on BN
    assert np.abs(N_(fi) - N_(f)).max() > 0


def test_conv2d_training_mode_batch_norm(dev):
    """tf_util.conv2d(bn=True, is_training=True): contrib batch_norm on batch statistics + moving-average update
    (Common/tf_util.py:512-531, decay bn_decay)."""
    from dispu_amd import tf_util
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 50, 8, 12)).astype(np.float32)
    P = {"s/weights": (rng.standard_normal((12, 20)) * 0.3).astype(np.float32), "s/biases": rng.standard_normal(20).astype(np.float32) * 0.1,
         "s/bn/gamma": (1 + 0.1 * rng.standard_normal(20)).astype(np.float32), "s/bn/beta": (0.1 * rng.standard_normal(20)).astype(np.float32),
         "s/bn/moving_mean": np.zeros(20, np.float32), "s/bn/moving_variance": np.ones(20, np.float32)}
    y = N_(tf_util.conv2d(dv(x, dev), 20, (1, 1), "s", P, bn=True, is_training=True, bn_decay=0.9))
    z = x.reshape(-1, 12).astype(np.float64) @ P["s/weights"].astype(np.float64) + P["s/biases"]
    mu, var = z.mean(0), z.var(0)
    want = np.maximum((z - mu) / np.sqrt(var + 1e-3) * P["s/bn/gamma"] + P["s/bn/beta"], 0).reshape(2, 50, 8, 20)
    assert np.abs(y - want).max() <= 2e-5
    n = z.shape[0]
    assert np.abs(N_(P["s/bn/moving_mean"]) - 0.1 * mu).max() <= 1e-5
    assert np.abs(N_(P["s/bn/moving_variance"]) - (0.9 + 0.1 * var * n / (n - 1))).max() <= 1e-5   # fused BN: unbiased variance in the average
    # inference afterwards folds the UPDATED moving statistics
    y2 = N_(tf_util.conv2d(dv(x, dev), 20, (1, 1), "s", P, bn=True, is_training=False))
    mm, mv = N_(P["s/bn/moving_mean"]).astype(np.float64), N_(P["s/bn/moving_variance"]).astype(np.float64)
    want2 = np.maximum((z - mm) / np.sqrt(mv + 1e-3) * P["s/bn/gamma"] + P["s/bn/beta"], 0).reshape(2, 50, 8, 20)
    assert np.abs(y2 - want2).max() <= 2e-5


@pytest.mark.parametrize("dtype,B,n", [pytest.param("f32", 4, 256, id="f32"), pytest.param("bf16", 4, 256, id="bf16"),
                                       ("f32", 2, 40), ("bf16", 2, 40), ("f32", 1, 512), ("bf16", 1, 512)])
def test_taped_steps_equal_eager_steps(dev, dtype, B, n, monkeypatch):
    """train_step_taped re-issues the eager step's launch sequence from a recorded tape (dis-pu_amd/_lib.py:Tape): same kernels, same
    streams, same order -> the same gradients, loss terms, moving statistics and parameters as train_step from the same state (up to
    the float atomics), step after step with new inputs, across an epoch boundary that changes weight_fine (new tape).
    (2, 40): 160-row clouds under the 64-row tiles, after_conv without split-K; (1, 512): the forward without the fused stem."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=22, bias_scale=0.05, bn_random=True)
    batches = [synth.patch_with_gt(B, n, 4 * n, seed=40 + i) for i in range(4)]
    rs = torch.ones(B, device=dev)
    e = Trainer(params=P, device=dev, dtype=dtype)
    g = Trainer(params=P, device=dev, dtype=dtype)
    e.epoch = g.epoch = 20
    gtol = 2e-5 if dtype == "f32" else 2e-3
    for i, (x, gt) in enumerate(batches):
        if i == 2:
            e.epoch = g.epoch = 21
        for name in ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var"):
            getattr(g, name).copy_(getattr(e, name))
        g.adam_t, g.global_step = e.adam_t, e.global_step
        xs, gs = dv(x, dev), dv(gt, dev)
        te = e.train_step(xs, gs, rs)
        tg = g.train_step_taped(xs, gs, rs)
        torch.cuda.synchronize()
        floor = 4e-7 * float(e.flat_g.abs().max())
        for k in e.G:
            scale = float(e.G[k].abs().max()) + 1e-12
            assert float((g.G[k] - e.G[k]).abs().max()) <= gtol * scale + floor + 2e-6, (i, k)
        assert np.allclose(N(g.moving_mean), N(e.moving_mean), rtol=1e-5, atol=1e-6) and np.allclose(N(g.moving_var), N(e.moving_var), rtol=1e-5, atol=1e-6)
        for k in te:
            a, b = float(te[k]), float(tg[k])
            assert abs(a - b) <= (1e-5 if dtype == "f32" else 1e-2) * max(1.0, abs(a)), (i, k, a, b)
        diff = N((g.flat_p - e.flat_p).abs())
        assert diff.max() <= 2.5e-3 and np.quantile(diff, 0.99) <= (2e-5 if dtype == "f32" else 1e-3)
    if (B, n) == (4, 256):
        assert len(g._tapes) == 2 and all(len(t["tape"]) > 150 for t in g._tapes.values())
    else:
        # 150 belongs to the 256 path.  Elsewhere: a tape holds exactly the launches ONE eager pass makes through the library (counted
        # by a recording proxy around _lib.tape_lib()), plus the stream / event operations the schedule puts between them
        rec = K.recording(monkeypatch)
        e.zero_grad()
        e.forward(xs)
        e.loss_backward(gs, rs)
        e.backward()
        torch.cuda.synchronize()
        want = len(rec.launches())
        held = [sum(1 for c in t["tape"].calls if c[2] not in ("event_record", "stream_wait_event")) for t in g._tapes.values()]
        assert want > 50 and held == [want, want], (held, want)
    assert g.global_step == 4 and g.adam_t == 4


def test_tapes_are_dropped_when_their_buffers_move(dev):
    """A launch tape / captured graph holds raw device pointers.  A later, larger batch that grows a scratch buffer, or
    load_params (checkpoint restore) re-allocating the flat parameter / gradient buffers, must invalidate every recording: the
    next taped step at the old shape records afresh and still equals the eager step (round-4 advisor finding)."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=23, bias_scale=0.05, bn_random=True)
    e = Trainer(params=P, device=dev)
    g = Trainer(params=P, device=dev)

    def both(B, seed):
        x, gt = synth.patch_with_gt(B, 256, 1024, seed=seed)
        rs = torch.ones(B, device=dev)
        for name in ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var"):
            getattr(g, name).copy_(getattr(e, name))
        g.adam_t, g.global_step = e.adam_t, e.global_step
        te = e.train_step(dv(x, dev), dv(gt, dev), rs)
        tg = g.train_step_taped(dv(x, dev), dv(gt, dev), rs)
        torch.cuda.synchronize()
        floor = 4e-7 * float(e.flat_g.abs().max())
        for k in e.G:
            scale = float(e.G[k].abs().max()) + 1e-12
            assert float((g.G[k] - e.G[k]).abs().max()) <= 2e-5 * scale + floor + 2e-6, (B, seed, k)
        for k in te:
            assert abs(float(te[k]) - float(tg[k])) <= 1e-5 * max(1.0, abs(float(te[k]))), (B, seed, k)

    both(2, 60)
    small_tape = next(iter(g._tapes.values()))["tape"]
    ptrs_before = {k: v.data_ptr() for k, v in g._scratch.items()}
    both(16, 61)                                   # larger shape: scratch buffers grow -> the B = 2 tape must not survive
    grew = any(g._scratch[k].data_ptr() != p for k, p in ptrs_before.items())
    if grew:
        assert all(t["tape"] is not small_tape for t in g._tapes.values())
    both(2, 62)                                    # replays (or re-records) at the small shape: still the eager step
    g.load_params(e.params())                      # checkpoint restore path: flat buffers re-allocated
    assert not g._tapes and not g._ws
    g.adam_t = e.adam_t
    both(2, 63)


def test_forward_refuses_shapes_the_fused_kernels_cannot_take(dev):
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    tr = Trainer(params=OG.init_params(seed=3), device=dev)
    with pytest.raises(ValueError, match="multiple of 64"):
        tr.forward(dv(synth.patches(1, 250, seed=1), dev))           # 4 * 250 rows: not a multiple of 64
    with pytest.raises(ValueError, match="4096"):
        tr.forward(dv(synth.patches(1, 2048, seed=1), dev))          # 8192-point clouds: beyond the LDS graph inversion
    with pytest.raises(ValueError):
        tr.forward(dv(synth.patches(4, 16, seed=1), dev))            # fewer points than neighbours
    with pytest.raises(ValueError, match="32-point"):
        tr.forward(dv(synth.patches(4, 20, seed=1), dev))            # 320 rows pass the 64-row rule; 80-point clouds are not whole 32-point tiles
    # a refusal leaves nothing half-built behind: the same Trainer then runs a legal step exactly like a fresh one
    assert not tr._ws
    x, gt = synth.patch_with_gt(2, 24, 96, seed=2)
    xs, gs, rs = dv(x, dev), dv(gt, dev), torch.ones(2, device=dev)
    terms = []
    for t in (tr, Trainer(params=OG.init_params(seed=3), device=dev)):
        t.zero_grad()
        t.forward(xs)
        terms.append({k: float(v) for k, v in t.loss_backward(gs, rs).items()})
        t.backward()
        torch.cuda.synchronize()
    for k, a in terms[1].items():
        assert np.isfinite(a) and abs(terms[0][k] - a) <= 1e-5 * max(1.0, abs(a)), (k, terms[0][k], a)


def test_second_backward_on_one_forward(dev):
    """backward() masks / accumulates into buffers that forward() zero-fills; running it twice on one forward (new loss
    weights, new targets) must give the second loss's gradients, not the sum with stale ones."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=8, bias_scale=0.05)
    x, gt = synth.patch_with_gt(2, 256, 1024, seed=4)
    xs, gs, rs = dv(x, dev), dv(gt, dev), torch.ones(2, device=dev)
    tr = Trainer(params=P, device=dev)
    tr.zero_grad()
    tr.forward(xs)
    tr.loss_backward(gs, rs)
    tr.backward()
    torch.cuda.synchronize()
    first = tr.flat_g.clone()
    tr.zero_grad()
    tr.loss_backward(gs, rs)
    tr.backward()                                                    # no forward in between
    torch.cuda.synchronize()
    scale = float(first.abs().max())
    assert float((tr.flat_g - first).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_flash_attention_step_equals_materialised_attention_step(dev, dtype):
    """round 4: the non-local cell through dispu_attention_fwd_lse / dispu_attention_bwd (no [B, M, M] tensor) gives the step the
    SAME forward values and gradients as round 3's matmul -> softmax -> matmul path and its five backward products."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=77, bias_scale=0.05, bn_random=True)
    B = 4
    x, gt = synth.patch_with_gt(B, 256, 1024, seed=13)
    xs, gs, rs = dv(x, dev), dv(gt, dev), torch.ones(B, device=dev)
    res = {}
    for flash in (True, False):
        tr = Trainer(params=P, device=dev, dtype=dtype)
        tr.flash_attn = flash
        tr.zero_grad()
        c, f = tr.forward(xs)
        ws = tr._ws[(B, 256)]
        assert (ws["S"] is None) == flash
        terms = tr.loss_backward(gs, rs)
        tr.backward()
        torch.cuda.synchronize()
        res[flash] = dict(fine=f.clone(), nl=ws["nl"].clone(), att=ws["att"].clone(), dq=ws["dq"].clone(), dkv=ws["dkv"].clone(),
                          g={k: v.clone() for k, v in tr.G.items()}, loss=float(terms["pu_loss"]))
    a, b = res[True], res[False]
    tol = 2e-5 if dtype == "f32" else 5e-3
    for k in ("att", "nl", "fine", "dq", "dkv"):
        scale = float(b[k].abs().max()) + 1e-12
        assert float((a[k] - b[k]).abs().max()) <= tol * scale, k
    assert abs(a["loss"] - b["loss"]) <= tol * abs(b["loss"])
    gtol = 1e-4 if dtype == "f32" else 2e-2
    for k in a["g"]:
        scale = float(b["g"][k].abs().max()) + 1e-12
        assert float((a["g"][k] - b["g"][k]).abs().max()) <= gtol * scale + 2e-6, k
