#!/usr/bin/env python3
"""The EMD term of the training loss (emd_w * earth_mover(fine, gt, radius), DisPU/model.py:77) two ways on one batch of clouds, value
and gradient w.r.t. the prediction, through the C ABI on preallocated buffers (no allocation, no host work between the launches):

    fused     dispu_approx_match_levels_ws (21 launches) + dispu_emd_loss_grad (2 launches: tiles, combine); no [B, M, M] match
    composed  dispu_approx_match_ws (22) + dispu_match_cost_ws (2) + dispu_match_cost_grad_ws (3) + one scale-and-add into dpred

    python tools/emd_loss_bench.py                       # (8, 1024), (32, 1024), (64, 1024)
    python tools/emd_loss_bench.py --batches 8 --iters 100 --rounds 7

Timing: HIP events around `iters` back-to-back evaluations, after a warm-up, `rounds` times per path with the order of the two paths
alternating from round to round (fused first in even rounds, composed first in odd ones): the spread of a path over its rounds is
printed beside its median, and the two orders are reported apart.  The parts are timed the same way on their own: the auction
(levels_ws), the fused launches (emd_loss_grad alone, on the scratch the auction left), and what they replace: approx_match_ws
minus the auction (= the assembly), match_cost_ws, match_cost_grad_ws, the scale-and-add.  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per evaluation


def stats(v):
    s = sorted(v)
    return {"min": round(s[0], 2), "median": round(s[len(s) // 2], 2), "max": round(s[-1], 2)}


def bench_shape(B, M, iters, rounds, emd_w=10.0, wf=1.0):
    import numpy as np
    from dispu_amd import _lib, synth
    dev = torch.device("cuda:0")
    L, st, A = _lib.lib(), _lib.stream_ptr(dev), _lib.ARITH_CONTRACT
    _, gt = synth.patch_with_gt(B, max(16, M // 4), M, seed=5000)
    rng = np.random.default_rng(1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    pred, gtd = f32(gt + rng.normal(0, 0.02, gt.shape)), f32(gt)
    radius = f32(rng.uniform(0.5, 2.0, B))
    coef = emd_w * wf / (B * M)
    E = lambda n: torch.empty((max(int(n), 1),), dtype=torch.float32, device=dev)
    nt, ns = L.dispu_approx_match_scratch_bytes(B, M, M), L.dispu_emd_loss_grad_scratch_bytes(B, M, M)
    temp, temp2, sc = E(nt // 4 + 1), E(nt // 4 + 1), E(ns // 4)
    match, g1, g2 = E(B * M * M), E(B * M * 3).view(B, M, 3), E(B * M * 3)
    msc, gsc = E(L.dispu_match_cost_scratch_bytes(B, M, M) // 4), E(L.dispu_match_cost_grad_scratch_bytes(B, M, M) // 4)
    cost_f, cost_c = E(B), E(B)
    dp_f, dp_c = torch.zeros((B, M, 3), device=dev), torch.zeros((B, M, 3), device=dev)
    scale = (coef / radius).view(B, 1, 1)
    ck = _lib.check

    def levels():
        ck(L.dispu_approx_match_levels_ws(B, M, M, p(pred), p(gtd), p(temp), nt, A, st), "levels_ws")

    def fused_tail():
        ck(L.dispu_emd_loss_grad(B, M, M, p(pred), p(gtd), p(temp), p(radius), coef, p(cost_f), p(dp_f), p(sc), ns, A, st), "emd_loss_grad")

    def am_full():
        ck(L.dispu_approx_match_ws(B, M, M, p(pred), p(gtd), p(match), p(temp2), nt, A, st), "approx_match_ws")

    def mcost():
        ck(L.dispu_match_cost_ws(B, M, M, p(pred), p(gtd), p(match), p(cost_c), p(msc), A, st), "match_cost_ws")

    def mgrad():
        ck(L.dispu_match_cost_grad_ws(B, M, M, p(pred), p(gtd), p(match), p(g1), p(g2), p(gsc), A, st), "match_cost_grad_ws")

    def scale_add():
        dp_c.addcmul_(g1, scale)

    def fused():
        levels()
        fused_tail()

    def composed():
        am_full()
        mcost()
        mgrad()
        scale_add()

    # the two paths compute the same thing (one evaluation each from zero)
    fused()
    composed()
    torch.cuda.synchronize()
    dv = float((cost_f / cost_c - 1).abs().max())
    dg = float((dp_f - dp_c).abs().max() / dp_c.abs().max())
    dp_f.zero_()
    dp_c.zero_()
    res = {"fused": {"first": [], "second": []}, "composed": {"first": [], "second": []}}
    for r in range(rounds):
        order = (("fused", fused), ("composed", composed)) if r % 2 == 0 else (("composed", composed), ("fused", fused))
        for pos, (name, fn) in zip(("first", "second"), order):
            res[name][pos].append(timed(fn, iters))
    parts = {k: stats([timed(fn, iters) for _ in range(3)]) for k, fn in
             (("levels_ws", levels), ("emd_loss_grad", fused_tail), ("approx_match_ws", am_full), ("match_cost_ws", mcost),
              ("match_cost_grad_ws", mgrad), ("scale_add", scale_add))}
    replaced = parts["approx_match_ws"]["median"] - parts["levels_ws"]["median"] + parts["match_cost_ws"]["median"] + \
        parts["match_cost_grad_ws"]["median"] + parts["scale_add"]["median"]
    out = {"metric": "EMD term, value + gradient w.r.t. the prediction", "unit": "us per evaluation (HIP events)", "batch": B, "points": M,
           "iters": iters, "rounds": rounds,
           "fused": stats(res["fused"]["first"] + res["fused"]["second"]), "composed": stats(res["composed"]["first"] + res["composed"]["second"]),
           "fused_run_first": stats(res["fused"]["first"]), "fused_run_second": stats(res["fused"]["second"]),
           "composed_run_first": stats(res["composed"]["first"]), "composed_run_second": stats(res["composed"]["second"]),
           "parts": parts, "fused_launches_alone": parts["emd_loss_grad"]["median"], "launches_they_replace": round(replaced, 2),
           "match_bytes_not_written": 4 * B * M * M, "cost_rel_diff": dv, "grad_diff_of_max": dg}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds per path; the order of the two paths alternates (use an even number)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    for B in a.batches:
        print(json.dumps(bench_shape(B, a.points, a.iters, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
