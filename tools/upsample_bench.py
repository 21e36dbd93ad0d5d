#!/usr/bin/env python3
"""Whole-cloud upsampling of clouds of different sizes: upsample_ragged over 64 seeded clouds of 1024 - 2048 points (sizes uniform),
a loop of upsample_cloud over the same clouds, and upsample_clouds over 64 equal 2048-point clouds.  Per-cloud wall time of the
whole call (host packing and the copy back included) after a warm-up, the device synchronised before the clock is read; the
median of --reps runs.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dispu_amd  # noqa: E402,F401
from dispu_amd import upsample as U  # noqa: E402
from dispu_amd.generator import Generator  # noqa: E402
from oracle import generator as OG  # noqa: E402


def clouds(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        g = rng.standard_normal((n, 3))
        out.append((g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, 3)).astype(np.float32))
    return out


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true", help="leave out the upsample_cloud loop (the slow one)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = Generator(params=OG.init_params(seed=1), device=dev)
    C = a.clouds
    sizes = [int(s) for s in np.random.default_rng(0).integers(1024, 2049, C)]
    mixed = clouds(sizes, 1)
    equal = np.stack(clouds([2048] * C, 2))
    res = dict(clouds=C, sizes_min=min(sizes), sizes_max=max(sizes), sizes_sum=sum(sizes))
    res["ragged_ms_per_cloud"] = timed(lambda: U.upsample_ragged(gen, mixed), a.reps) / C * 1e3
    res["equal_2048_ms_per_cloud"] = timed(lambda: U.upsample_clouds(gen, equal).cpu(), a.reps) / C * 1e3
    if not a.skip_loop:
        res["loop_ms_per_cloud"] = timed(lambda: [U.upsample_cloud(gen, pc) for pc in mixed], 1) / C * 1e3
        res["loop_over_ragged"] = res["loop_ms_per_cloud"] / res["ragged_ms_per_cloud"]
    res["ragged_over_equal"] = res["ragged_ms_per_cloud"] / res["equal_2048_ms_per_cloud"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
