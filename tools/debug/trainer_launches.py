#!/usr/bin/env python3
"""Launch signatures of a training step: what a change to train.py must leave alone.

    trainer_launches.py --out FILE        run every case on cuda:0 and write its signatures (one process, one tree)
    trainer_launches.py --compare A B     per-case call counts of two such files and whether they are equal (exit 1 if not)

The signature of one pass (zero_grad, forward, loss_backward, backward) is the launch tape taken over it (_lib.tape_begin / tape_end):
every C launch in order with its converted arguments, plus every event record and stream wait of the step's schedule, with each
pointer-typed argument (buffers, streams, events) replaced by the ordinal of its first appearance in that pass.  Equal signatures
mean the same launches on the same buffers, streams and events in the same order.  Each case is recorded twice on one fresh Trainer:
cold (workspace, scratch and streams are made on the way) and warm.  The tape does not see Trainer._bucket_point (eager data-parallel
ordering: tests/test_distributed_gpu.py).  The script touches only attributes every version of the Trainer has, so the same file runs
in a checkout of an older commit; compare the two outputs with --compare.

The use_uniform case runs at (1, 128), not (4, 64): the uniform term refuses clouds of fewer than 500 fine points."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generator_launches import compare  # noqa: E402

FULL = ("zero_grad", "forward", "loss_backward", "backward")
SHAPES = ((2, 24, 2), (2, 40, 1), (4, 64, 4), (1, 128, 1), (1, 512, 4), (68, 64, 1))     # tests/train_step_checks.py:SHAPE_CASES without (1, 1024)


def cases():
    """(name, dtype, (B, N, seed), Trainer attributes, TrainOpts attributes, the calls of the warm pass)"""
    out = [("f32 (8, 256)", "f32", (8, 256, 5), {}, {}, FULL)]
    out += [("f32 (%d, %d)" % (B, N), "f32", (B, N, s), {}, {}, FULL) for B, N, s in SHAPES]
    out += [("bf16 (8, 256)", "bf16", (8, 256, 5), {}, {}, FULL), ("bf16 (2, 40)", "bf16", (2, 40, 1), {}, {}, FULL)]
    for attrs in ({"overlap_dw": False}, {"group_reduce": False}, {"dw_streams": 1}, {"dw_streams": 3}, {"flash_attn": False},
                  {"fused_local_bwd": True}):
        out.append(("f32 (4, 64) %s" % ", ".join("%s=%s" % kv for kv in attrs.items()), "f32", (4, 64, 4), attrs, {}, FULL))
    out.append(("f32 (4, 64) use_repulse=False", "f32", (4, 64, 4), {}, {"use_repulse": False}, FULL))
    out.append(("f32 (1, 128) use_uniform=True", "f32", (1, 128, 1), {}, {"use_uniform": True}, FULL))
    out.append(("f32 (4, 64) use_emd=True", "f32", (4, 64, 4), {}, {"use_emd": True}, FULL))
    out.append(("f32 (4, 64) second loss_backward + backward on one forward", "f32", (4, 64, 4), {}, {}, ("loss_backward", "backward")))
    out.append(("f32 (4, 64) backward without loss_backward", "f32", (4, 64, 4), {}, {}, ("zero_grad", "forward", "backward")))
    out.append(("bf16 (8, 256) bf16_stream=False", "bf16", (8, 256, 5), {"bf16_stream": False}, {}, FULL))
    # corners of the dense-product dispatch (products.py): every product bf16 at a small shape; rm = 192, no multiple of 128, so the
    # ladder's fall-throughs run; the batched products and the batch-B TN of the gemm attention path in bf16 mode; TN without grouping / side streams
    for shape, attrs in (((4, 64, 4), {"bf16_min_macs": 0.0}), ((2, 24, 2), {"bf16_min_macs": 0.0}), ((4, 64, 4), {"flash_attn": False}),
                         ((4, 64, 4), {"group_reduce": False}), ((4, 64, 4), {"overlap_dw": False})):
        out.append(("bf16 (%d, %d) %s" % (shape[0], shape[1], ", ".join("%s=%s" % kv for kv in attrs.items())), "bf16", shape, attrs, {}, FULL))
    return out


def signature(tape):
    ids, sig = {}, []
    for _, args, name in tape.calls:
        sig.append([name] + [("p%d" % ids.setdefault(a.value, len(ids)) if a.value else "null") if isinstance(a, ctypes.c_void_p) else a.value
                             for a in args])
    return sig


def run(out):
    import numpy as np
    import torch
    from dispu_amd import _lib, synth
    from dispu_amd.params import init_params
    from dispu_amd.train import Trainer, TrainOpts
    dev = torch.device("cuda:0")
    P = init_params(1234)
    res = {}
    for name, dtype, (B, N, seed), attrs, oattrs, warm in cases():
        opts = TrainOpts()
        for k, v in oattrs.items():
            setattr(opts, k, v)
        tr = Trainer(opts, params=P, device=dev, dtype=dtype)
        for k, v in attrs.items():
            setattr(tr, k, v)
        x, gt = synth.patch_with_gt(B, N, 4 * N, seed=seed)
        x, gt = torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)
        radius = torch.from_numpy(np.linspace(1.0, 1.3, B).astype(np.float32)).to(dev)
        res[name] = {}
        for temp, calls in (("cold", FULL if "loss_backward" in warm else warm), ("warm", warm)):
            _lib.tape_begin()
            try:
                for c in calls:
                    getattr(tr, c)(*{"forward": (x,), "loss_backward": (gt, radius)}.get(c, ()))
            finally:
                tape = _lib.tape_end()
            torch.cuda.synchronize()
            res[name][temp] = signature(tape)
        print("%-60s cold %3d calls, warm %3d" % (name, len(res[name]["cold"]), len(res[name]["warm"])), flush=True)
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out or "trainer_launches.json")
