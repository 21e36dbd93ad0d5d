#!/usr/bin/env python3
"""The uniform term of the training loss (loss_utils.get_uniform_loss, Common/loss_utils.py:238-267) two ways on one cloud batch:

    fused     farthest point sampling + ONE dispu_uniform_loss_grad launch (value partials and gradient; csrc/uniform_loss.hip)
    composed  the reference's graph on this package's ops: per level query_ball_point, group_point, pairwise differences, torch.sort,
              the moments; the gradient through autograd (group_point's registered gradient)

    python tools/uniform_bench.py --batch 8 --mode fused --iters 50
    rocprofv3 --kernel-trace --stats -d out -- python tools/uniform_bench.py --batch 8 --mode composed --iters 50

Prints one JSON line: the value and the mean wall time per value + gradient evaluation (HIP events around the loop).  Kernel times
and launch counts come from the rocprofv3 run of each mode on its own; farthest point sampling is the same launch in both modes."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def composed_uniform_loss(pcd, percentages=(0.004, 0.006, 0.008, 0.010, 0.012), radius=1.0, seeds=None):
    """get_uniform_loss composed from the existing ops; differentiable w.r.t. pcd.  Distances from coordinate differences
    (tf_grouping.py:132-134), the nearest OTHER slot by a stable sort (the earlier slot first on ties, as tf.nn.top_k)."""
    from dispu_amd import loss_utils
    from dispu_amd.tf_grouping import group_point, query_ball_point
    from dispu_amd.tf_sampling import farthest_point_sample, gather_point
    b, n, _ = pcd.shape
    lv = loss_utils.uniform_levels(n, percentages, radius)
    if seeds is None:
        seeds = farthest_point_sample(lv["npoint"], pcd.detach())
    new_xyz = gather_point(pcd.detach(), seeds)
    loss = 0.0
    for ns, r, e, w in zip(lv["ns"], lv["r"], lv["e"], lv["w"]):
        idx, _ = query_ball_point(r, ns, pcd.detach(), new_xyz)
        grouped = group_point(pcd, idx)                                             # [b, npoint, ns, 3]
        diff = grouped[:, :, :, None, :] - grouped[:, :, None, :, :]
        d = (diff * diff).sum(-1)
        d = d + torch.diag(torch.full((ns,), float("inf"), device=pcd.device))      # a slot is not its own partner
        dmin = torch.sort(d, dim=-1, stable=True)[0][..., 0]
        u = torch.sqrt(dmin + 1e-8)
        loss = loss + ((u - e) ** 2 / (e + 1e-8)).mean() * w
    return loss / len(lv["ns"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    a = ap.parse_args()
    import numpy as np
    from dispu_amd import loss_utils, synth
    dev = torch.device("cuda:0")
    _, gt = synth.patch_with_gt(a.batch, max(16, a.points // 4), a.points, seed=5000)
    rng = np.random.default_rng(1)
    pcd = torch.from_numpy((gt + rng.normal(0, 0.02, gt.shape)).astype(np.float32)).to(dev).requires_grad_(True)
    fn = loss_utils.get_uniform_loss if a.mode == "fused" else composed_uniform_loss

    def once():
        v = fn(pcd)
        (g,) = torch.autograd.grad(v, pcd)
        return v, g
    value = float(fn(pcd))
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"metric": "uniform term, value + gradient", "mode": a.mode, "batch": a.batch, "points": a.points, "iters": a.iters,
                      "ms_per_eval": e0.elapsed_time(e1) / a.iters, "value": value}))


if __name__ == "__main__":
    main()
