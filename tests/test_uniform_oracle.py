"""CPU tests of tests/uniform_oracle.py: the explicit-index float64 formulas the GPU tests of the uniform term rest on
(tests/test_uniform_loss_gpu.py) are held to a float64 torch-autograd restatement of the reference's own graph
(Common/loss_utils.py:238-267: group_point, the distance matrix, top_k(-D, 2), sqrt(abs(. + 1e-8)), the moments), with seeds and slots
from the project's ball-query oracle; the host quantities and the refusal rules of dis-pu_amd/loss_utils.py are checked for a
1024-point cloud.  No kernel runs here.

Bound 1e-8 (relative, value and gradient): the restatement's expanded distance matrix |a|^2 - 2ab + |b|^2 and the oracle's
differences differ by a few ulps of 1 (~1e-15) in D; at D = 0 (a padded slot) that is ~5e-12 in u = sqrt(D + 1e-8) = 1e-4; everything
else is the same arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_oracle as LO  # noqa: E402
import uniform_oracle as UO  # noqa: E402

from oracle import oracle as O  # noqa: E402

F64 = torch.float64
CASES = [(1, 40, [0.05, 0.2]), (3, 100, [0.03, 0.05, 0.12]), (2, 333, [0.01, 0.02, 0.04, 0.1]), (2, 1024, UO.DEFAULT_PERCENTAGES)]


def rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def seeds_and_slots(pcd, percentages, radius=1.0):
    lv = UO.host_levels(pcd.shape[1], percentages, radius)
    seeds = O.farthest_point_sample(lv["npoint"], pcd)
    new_xyz = O.gather_point(pcd, seeds)
    slots, cnts = [], []
    for r, ns in zip(lv["r"], lv["ns"]):
        idx, cnt = O.query_ball_point(r, ns, pcd, new_xyz)
        slots.append(idx)
        cnts.append(cnt)
    return lv, seeds, slots, cnts


def reference_graph(pcd64, slots, percentages, radius, expanded):
    """get_uniform_loss (loss_utils.py:238-267) in float64 torch on given slots; `expanded`: the distance matrix as
    r_A - 2 A B^T + r_B^T (tf_grouping.py:61-66), else from differences (tf_grouping.py:132-134)."""
    B, N, _ = pcd64.shape
    loss = []
    for p, idx in zip(percentages, slots):
        nsample = int(N * p)
        disk_area = np.pi * (radius ** 2) * p / nsample
        expect_len = torch.sqrt(torch.tensor(disk_area, dtype=F64))
        ii = torch.as_tensor(np.asarray(idx, np.int64))
        grouped = pcd64[torch.arange(B)[:, None, None], ii]                 # group_point [B, npoint, nsample, 3]
        grouped = torch.cat(torch.unbind(grouped, dim=1), dim=0)            # concat(unstack(axis=1), axis=0)
        if expanded:
            r = (grouped * grouped).sum(2, keepdim=True)
            D = r - 2 * grouped @ grouped.transpose(1, 2) + r.transpose(1, 2)
        else:
            D = ((grouped[:, None, :, :] - grouped[:, :, None, :]) ** 2).sum(-1)
        var, _ = torch.topk(-D, 2, dim=-1)
        uniform_dis = -var[:, :, 1:]
        uniform_dis = torch.sqrt(torch.abs(uniform_dis + 1e-8))
        uniform_dis = uniform_dis.mean(-1)
        uniform_dis = (uniform_dis - expect_len) ** 2 / (expect_len + 1e-8)
        mean = uniform_dis.reshape(-1).mean()
        loss.append(mean * np.power(p * 100, 2))
    return sum(loss) / len(percentages)


@pytest.mark.parametrize("expanded", [True, False])
@pytest.mark.parametrize("B,N,percentages", CASES)
def test_oracle_matches_the_reference_graph(B, N, percentages, expanded):
    _, pcd = LO.jittered_pair(B, N, N, seed=N + B)
    lv, seeds, slots, cnts = seeds_and_slots(pcd, percentages)
    assert all((c >= 1).all() for c in cnts)
    assert any((c < ns).any() for c, ns in zip(cnts, lv["ns"])) or N == 40, "no padded ball in this case"
    res = UO.uniform_value_grad(pcd, slots, percentages)
    x = torch.tensor(pcd, dtype=F64, requires_grad=True)
    v = reference_graph(x, slots, percentages, 1.0, expanded)
    v.backward()
    want = float(v.detach())
    print("[measured] uniform oracle (%d, %d, L=%d, expanded=%s): value %.6e, rel %.2e, grad rel %.2e" %
          (B, N, len(percentages), expanded, want, abs(res["value"] - want) / abs(want), rel(res["grad"], x.grad.numpy())))
    assert want > 0 and np.abs(x.grad.numpy()).max() > 0
    assert abs(res["value"] - want) <= 1e-8 * abs(want)
    assert rel(res["grad"], x.grad.numpy()) <= 1e-8
    assert abs(res["partial"].mean() - res["value"]) <= 1e-15 * abs(want)


def test_scale_multiplies_the_gradient_only():
    _, pcd = LO.jittered_pair(2, 333, 333, seed=5)
    _, _, slots, _ = seeds_and_slots(pcd, [0.01, 0.04])
    a = UO.uniform_value_grad(pcd, slots, [0.01, 0.04])
    b = UO.uniform_value_grad(pcd, slots, [0.01, 0.04], scale=2.5)
    assert a["value"] == b["value"] and rel(b["grad"], 2.5 * a["grad"]) <= 1e-15


def test_near_tie_report():
    """three collinear points -a, 0, +a: the middle one's two partners tie exactly (gap 0), the outer ones' do not."""
    pcd = np.array([[[-0.25, 0, 0], [0, 0, 0], [0.25, 0, 0]]], np.float32)
    slots = [np.array([[[0, 1, 2]]], np.int32)]
    res = UO.uniform_value_grad(pcd, slots, [1.0])
    assert res["gap"][0][0, 0].tolist() == [0.75, 0.0, 0.75]
    assert res["partner"][0][0, 0].tolist() == [1, 0, 1]                        # the lowest slot wins the tie
    assert UO.near_tie_rows(res, slots, (1, 3)).tolist() == [[True, True, True]]
    # a padded ball: slots repeat point 0; each slot's partner is a copy of itself, no other point -> gap inf, no gradient
    res = UO.uniform_value_grad(pcd, [np.array([[[0, 0, 0]]], np.int32)], [1.0])
    assert np.isinf(res["gap"][0]).all() and not res["grad"].any()
    assert np.allclose(res["u"][0], 1e-4, rtol=1e-12)


def test_host_quantities_at_1024():
    """loss_utils.py:239-251 for the default percentages at N = 1024, in Python double arithmetic."""
    from dispu_amd import loss_utils as LU
    lv = LU.uniform_levels(1024)
    assert lv["npoint"] == 51 and lv["ns"] == [4, 6, 8, 10, 12]
    ps = UO.DEFAULT_PERCENTAGES
    assert lv["r"] == [np.sqrt(p * 1.0) for p in ps]
    assert lv["e"] == [float(np.sqrt(np.pi * 1.0 * p / k)) for p, k in zip(ps, lv["ns"])]
    assert lv["w"] == [pow(p * 100, 2) for p in ps]
    ref = UO.host_levels(1024)
    assert all(lv[k] == ref[k] for k in ("npoint", "ns", "r", "e", "w"))
    lv = LU.uniform_levels(1000, [0.0105, 0.02], radius=2.0)
    assert lv["npoint"] == 50 and lv["ns"] == [10, 20]
    assert lv["r"] == [np.sqrt(0.0105 * 2.0), np.sqrt(0.02 * 2.0)] and lv["e"][0] == float(np.sqrt(np.pi * 4.0 * 0.0105 / 10))
    t = LU.UniformTables(2, 1024, scale=3.0)
    assert t.nlevels == 5 and t.npoint == 51 and list(t.ns) == [4, 6, 8, 10, 12] and t.slots == 40
    lev = np.array(list(t.levels), np.float64).reshape(5, 4)
    assert np.array_equal(lev[:, 0], np.float32(ref["r"])) and np.array_equal(lev[:, 1], np.float32(ref["e"]))
    assert np.array_equal(lev[:, 2], np.float32([w / k for w, k in zip(ref["w"], ref["ns"])]))
    assert np.array_equal(lev[:, 3], np.float32([3.0 * w / k / (5 * 2 * 51) for w, k in zip(ref["w"], ref["ns"])]))


def test_refusals():
    """where the reference's own graph fails (a sample of zero seeds, top_k(., 2) of one slot) and the kernel's limits."""
    from dispu_amd import loss_utils as LU
    with pytest.raises(ValueError, match="positive npoint"):
        LU.uniform_levels(19, [0.2])
    for n in (64, 256, 499):
        with pytest.raises(ValueError, match="at least k columns"):
            LU.uniform_levels(n)
    assert LU.uniform_levels(500)["ns"] == [2, 3, 4, 5, 6] and LU.uniform_min_points() == 500
    assert LU.uniform_min_points([0.05, 0.2]) == 40
    with pytest.raises(ValueError, match="slots per ball"):
        LU.uniform_levels(1024, [0.07])                                         # 71 slots: more than a wave holds
    with pytest.raises(ValueError, match="percentages"):
        LU.uniform_levels(1024, [])
    with pytest.raises(ValueError, match="percentages"):
        LU.uniform_levels(1024, [0.01] * 9)
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        LU.get_uniform_loss(torch.zeros(1, 1024, 3))
