"""CPU checks of the EMD term (DisPU/model.py:77): tests/emd_oracle.py against the project's C oracle and against a float64 torch
autograd restatement of `sum sqrt(d2) match / radius / M`; the option defaults, the train tool's flags, the C boundary's new
names and the scratch formula the header states; the log line and the meter-table reduction with the term's column.

Bounds: values 1e-5 relative, gradients 1e-5 of max |reference| against the fp32 C oracle; 1e-8 against the float64 autograd."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emd_oracle as EO  # noqa: E402

from oracle import oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CASES = [(2, 128, 128), (2, 300, 200), (2, 200, 300), (3, 1, 5)]


def clouds(b, n, m):
    from dispu_amd import synth
    if min(n, m) < 8:
        rng = np.random.default_rng(n * 1000 + m)
        return rng.random((b, n, 3), dtype=F32), rng.random((b, m, 3), dtype=F32)
    return synth.patches(b, n, seed=n), synth.patches(b, m, seed=m + 1)


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("b,n,m", CASES)
def test_oracle_against_the_c_oracle(b, n, m):
    x1, x2 = clouds(b, n, m)
    match = O.approx_match(x1, x2)
    cost, g1 = EO.match_cost(x1, x2, match), EO.match_cost_grad1(x1, x2, match)
    co, (o1, _) = O.match_cost(x1, x2, match), O.match_cost_grad(x1, x2, match)
    worst = float(np.abs(co / cost - 1.0).max())
    print("[measured] emd oracle vs C oracle (%d, %d, %d): cost rel %.2e, grad1 %.2e of max" % (b, n, m, worst, rel(o1, g1)))
    assert cost.min() > 0 and worst <= 1e-5
    assert rel(o1, g1) <= 1e-5


@pytest.mark.parametrize("b,n,m", CASES)
def test_oracle_against_float64_autograd(b, n, m):
    """value and gradient of emd_w * wf * mean_b(sum sqrt(d2) match / radius / M) with the plan held constant."""
    x1, x2 = clouds(b, n, m)
    match = O.approx_match(x1, x2)
    radius = np.linspace(0.5, 2.0, b)
    emd_w, wf = 10.0, 0.1
    res = EO.emd_value_grad(x1, x2, match, radius, emd_w, wf)
    p1 = torch.from_numpy(x1.astype(np.float64)).requires_grad_(True)
    p2 = torch.from_numpy(x2.astype(np.float64))
    d2 = ((p1[:, :, None, :] - p2[:, None, :, :]) ** 2).sum(-1)                      # [b, n, m]
    cost = (d2.sqrt() * torch.from_numpy(match.astype(np.float64)).transpose(1, 2)).sum((1, 2))
    value = emd_w * (cost / torch.from_numpy(radius) / float(m)).mean()
    (g,) = torch.autograd.grad(wf * value, p1)
    assert abs(res["value"] - float(value.detach())) <= 1e-8 * abs(float(value.detach()))
    assert rel(res["grad"], g.numpy()) <= 1e-8
    assert np.allclose(res["grad"], EO.grad_scale(radius, b, m, emd_w, wf)[:, None, None] * res["grad1"], rtol=0, atol=0)
    # radius None is radius 1
    assert EO.emd_value(res["cost"], None, m) == EO.emd_value(res["cost"], np.ones(b), m)


def test_coincident_points_take_the_clamp():
    """pred[0] == gt[1] exactly: that pair adds nothing to the gradient (0 / sqrt(1e-20)) and nothing to the cost; no NaN."""
    x1 = np.array([[[0.25, -0.5, 0.125], [1.0, 0.0, 0.0]]], F32)
    x2 = np.array([[[0.0, 0.0, 0.0], [0.25, -0.5, 0.125]]], F32)
    match = np.array([[[0.25, 0.5], [0.75, 0.5]]], F32)                               # [b, m, n]
    g = EO.match_cost_grad1(x1, x2, match)
    assert np.isfinite(g).all()
    d = x1[0, 0].astype(np.float64) - x2[0, 0]
    assert np.allclose(g[0, 0], 0.25 * d / np.linalg.norm(d), rtol=1e-12)            # only the pair (k = 0, l = 0)
    assert np.isclose(EO.match_cost(x1, x2, match)[0],
                      0.25 * np.linalg.norm(d) + 0.5 * 1.0 + 0.5 * np.linalg.norm(x1[0, 1].astype(np.float64) - x2[0, 1]), rtol=1e-12)


def test_finalize_arithmetic():
    import loss_oracle as LO
    rng = np.random.default_rng(5)
    rep, upart, cost, radius = rng.uniform(0, 4e-3, 64), rng.uniform(0, 0.5, 40), rng.uniform(20, 60, 3), np.array([0.5, 1.0, 2.0])
    for wf in (0.01, 1.0):
        t = EO.pu_loss_terms_e(0.02, 0.03, rep, 64, wf, 0.5, upart, 10.0, cost, radius, 1024, 10.0)
        base = LO.pu_loss_terms(0.02, 0.03, rep, 64, wf, 0.5)
        e = 10.0 * np.mean(cost / radius / 1024.0)
        u = 10.0 * upart.mean()
        assert np.allclose(t[:3], base[:3], rtol=0, atol=0) and t[4] == wf
        assert np.isclose(t[6], e, rtol=1e-15) and np.isclose(t[5], u, rtol=1e-15)
        assert np.isclose(t[3], base[3] + wf * e + u, rtol=1e-14)                    # inside the weight_fine parenthesis
        off = EO.pu_loss_terms_e(0.02, 0.03, None, 0, wf, 0.5, None, 10.0, cost, radius, 1024, 0.0)
        assert np.allclose(off[:5], LO.pu_loss_terms(0.02, 0.03, None, 0, wf, 0.5), rtol=1e-15) and off[5] == 0.0 and off[6] == 0.0
        # the fp32 restatement follows the float64 terms to fp32 rounding
        assert abs(float(EO.pu_loss_f32(t[0], t[1], t[6], t[2], t[5], wf)) - t[3]) <= 4 * 2.0 ** -24 * t[3]
        assert abs(float(EO.pu_loss_f32(t[0], t[1], t[6], t[2], None, wf)) - (t[3] - t[5])) <= 4 * 2.0 ** -24 * t[3]


# ------------------------------------------------------------------------------- the surface that did not exist ----
def test_train_opts_defaults():
    from dispu_amd.train import TrainOpts
    assert TrainOpts.use_emd is False and TrainOpts.emd_w == 10.0
    assert TrainOpts.use_uniform is False and TrainOpts.use_repulse is True


def test_train_tool_parses_the_emd_flags():
    spec = importlib.util.spec_from_file_location("train_tool", os.path.join(ROOT, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args([])
    assert a.use_emd is False and a.emd_w == 10.0
    a = tool.parse_args(["--use_emd", "true", "--emd_w", "2.5"])
    assert a.use_emd is True and a.emd_w == 2.5
    tool.refuse_unsupported(a)
    with pytest.raises(SystemExit):
        tool.parse_args(["--use_emd", "yes"])


def test_new_entries_are_bound():
    from dispu_amd import _lib
    for name in ("dispu_approx_match_levels_ws", "dispu_emd_loss_grad_scratch_bytes", "dispu_emd_loss_grad", "dispu_pu_loss_finalize_e"):
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["dispu_emd_loss_grad"][1]) == 14 and len(_lib.SIGNATURES["dispu_pu_loss_finalize_e"][1]) == 16
    assert len(_lib.SIGNATURES["dispu_approx_match_levels_ws"][1]) == 9


def header_scratch_bytes(b, n, m):
    """the formula include/dispu_hip.h states for dispu_emd_loss_grad_scratch_bytes."""
    rb, ch = -(-n // 256), 128
    while ch > 32 and rb * -(-m // ch) * b < 1024:
        ch //= 2
    nc = -(-m // ch)
    return 4 * b * (nc * n * 3 + rb * nc)


def test_scratch_bytes_is_the_header_formula():
    from dispu_amd import _lib
    lib = _lib.lib()
    assert header_scratch_bytes(2, 300, 200) == 4 * 2 * (7 * 300 * 3 + 2 * 7)          # 32-partner tiles at this size
    for b, n, m in ((2, 300, 200), (1, 1024, 1024), (8, 1024, 1024), (32, 1024, 1024), (64, 1024, 1024), (3, 1, 5), (1, 1025, 1023)):
        assert lib.dispu_emd_loss_grad_scratch_bytes(b, n, m) == header_scratch_bytes(b, n, m), (b, n, m)
    assert lib.dispu_emd_loss_grad_scratch_bytes(0, 300, 200) == 0 and lib.dispu_emd_loss_grad_scratch_bytes(2, 0, 200) == 0


def test_log_line_and_meter_reduction_carry_the_column():
    from dispu_amd import train
    plain = train.format_log_line(7, 1.5, 0.25, 12.0, 0.125, 3.0, 90.0)
    assert train.format_log_line(7, 1.5, 0.25, 12.0, 0.125, 3.0, 90.0, None) == plain
    assert train.format_log_line(7, 1.5, 0.25, 12.0, 0.125, 3.0, 90.0, 0.5) == plain + "  dis_fine_emd=0.500000000"
    r0 = [[1, 2, 3, 4, 5, 10], [2, 3, 9, 5, 1, 20]]
    r1 = [[3, 4, 1, 6, 7, 30], [4, 5, 2, 7, 8, 40]]
    got = train.reduce_meter_tables(np.array([np.ravel(r0), np.ravel(r1)], F32), 2, width=6)
    assert got == [2.5, 3.5, 6.0, 5.5, 7.5, 25.0]                  # means over ranks and steps; max over ranks for columns 2 and 4
    assert train.reduce_meter_tables(np.zeros((2, 0), F32), 0, width=6) == [0.0] * 6
    five = train.reduce_meter_tables(np.array([np.ravel(r0)[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]]], F32), 2)
    assert five == [1.5, 2.5, 6.0, 4.5, 3.0]
