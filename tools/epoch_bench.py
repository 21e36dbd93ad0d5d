#!/usr/bin/env python3
"""What the data path costs per training step (one GPU, fp32 step, one process): after warm-up, alternate windows of
  (a) train_step on a fixed batch                      -- the bare step
  (b) dataset.Fetcher.next_batch + train_step          -- host draws (the reference's numpy sequence), per-batch uploads
  (c) dataset.DeviceFetcher.next_batch + train_step    -- one dispu_sample_batch launch per batch
  (d) train.train_one_epoch over the DeviceFetcher     -- the loop as fit runs it: (c) + the two logged Hausdorff terms and the
                                                          device-side accumulation of the epoch means, one read-back per epoch
at 8 and 32 patches per batch on a seeded synthetic dataset of 2048 patches (1024 points each, 256 sub-sampled).  A window is
--steps steps (>= 200) timed with the host clock around a final device synchronise; fetchers are reset where their epoch ends
(inside the window: that cost belongs to the loop).  Also times bare DeviceFetcher.next_batch calls back to back.

At 8 patches it also compares the two meter paths of the epoch loop, on the same trainer, fetcher and batches, eager and taped:
  (e) train.train_one_epoch            -- fit's path: train._hausdorff_terms after every step (two nn_distance launches, four row
                                          reductions, torch glue) + stack / add into the epoch's accumulator
  (f) train.fill_meter_table + reduce  -- fit_parallel's path: ONE dispu_step_meters launch per step into a device table, one
                                          read-back and a host reduction per epoch
(--meters-only: just this comparison.)

Prints one JSON line and writes it to --out (default profiles/epoch_bench.json).
--sampler-only: just the bare next_batch calls (for a kernel trace of the sampler alone)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_patches(n, points, seed):
    from dispu_amd import synth
    rng = np.random.default_rng(seed)
    return np.stack([synth.normalize(synth.cap_patch(rng, points))[0].astype(np.float32) for _ in range(n)])


class Looping(object):
    """next() over a fetcher, resetting it where the reference's epoch ends (int(len / B) - 1 batches)."""

    def __init__(self, fetcher, batch):
        self.f, self.per_epoch, self.used = fetcher, int(len(fetcher) / batch) - 1, 0

    def next(self):
        if self.used == self.per_epoch:
            self.f.reset()
            self.used = 0
        self.used += 1
        return self.f.next_batch()


def window(dev, steps, body):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        body()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps


def epochs_window(dev, steps, trainer, fetcher, loop, batch):
    """whole epochs of train.train_one_epoch (+ the reset fit makes after each) until at least `steps` steps ran -> ms per step"""
    from dispu_amd import train
    fetcher.reset()
    loop.used = 0
    done = 0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    while done < steps:
        done += train.train_one_epoch(trainer, fetcher, batch)[-1]
        fetcher.reset()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / done


def meter_epochs_window(dev, steps, trainer, fetcher, batch, step_fn):
    """whole epochs as train.fit_parallel runs them at world 1 (fill_meter_table, the table's read-back, the host reduction, the
    reset) until at least `steps` steps ran -> ms per step"""
    from dispu_amd import train
    fetcher.reset()
    n = train.steps_per_epoch(len(fetcher), batch)
    table = torch.zeros(n * 5 + 2, dtype=torch.float32, device=dev)
    step = trainer.train_step if step_fn == "eager" else trainer.train_step_taped
    done = 0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    while done < steps:
        train.fill_meter_table(trainer, fetcher, table, n, step)
        train.reduce_meter_tables(table.view(1, -1).cpu().numpy()[:, :n * 5], n)
        fetcher.reset()
        done += n
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / done


def old_epochs_window(dev, steps, trainer, fetcher, batch, step_fn):
    from dispu_amd import train
    fetcher.reset()
    done = 0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    while done < steps:
        done += train.train_one_epoch(trainer, fetcher, batch, step_fn)[-1]
        fetcher.reset()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / done


def meters_row(dev, a, gt, P, B=8):
    """(e) against (f), eager and taped, alternating windows"""
    from dispu_amd import dataset
    from dispu_amd.params import init_params
    from dispu_amd.train import Trainer
    fetch = dataset.DeviceFetcher(gt, gt, B, patch_num_point=P, device=dev, seed=1)
    tr = Trainer(params=init_params(1234), device=dev)
    paths = {"e_hausdorff_terms": old_epochs_window, "f_step_meters": meter_epochs_window}
    times = {(k, fn): [] for fn in ("eager", "taped") for k in paths}
    for (k, fn) in times:
        paths[k](dev, a.warmup, tr, fetch, B, fn)
    for _ in range(a.windows):
        for (k, fn), v in times.items():
            v.append(paths[k](dev, a.steps, tr, fetch, B, fn))
    fetch.check_status()
    row = {"batch": B}
    for fn in ("eager", "taped"):
        row[fn] = {k: summary(times[(k, fn)]) for k in paths}
        row[fn]["f_minus_e_ms"] = row[fn]["f_step_meters"]["median_ms"] - row[fn]["e_hausdorff_terms"]["median_ms"]
        row[fn]["f_faster_in_every_window"] = bool(max(times[("f_step_meters", fn)]) < min(times[("e_hausdorff_terms", fn)]))
    return row


def summary(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "windows": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per window (at least 200)")
    ap.add_argument("--windows", type=int, default=3, help="windows per variant and batch size")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--patches", type=int, default=2048)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_bench.json"))
    ap.add_argument("--sampler-only", action="store_true")
    ap.add_argument("--meters-only", action="store_true", help="only the meter-path comparison at 8 patches")
    a = ap.parse_args()
    if a.steps < 200 and not a.sampler_only:
        sys.exit("--steps must be at least 200")
    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    from dispu_amd import dataset
    from dispu_amd.params import init_params
    from dispu_amd.train import Trainer

    dev = torch.device("cuda:0")
    P, G = 256, 1024
    gt = synthetic_patches(a.patches, G, seed=2024)
    res = {"bench": "epoch_bench", "device": torch.cuda.get_device_name(0), "patches": a.patches, "points": [P, G], "steps_per_window": a.steps,
           "dtype": "f32", "batch": {}}
    if not a.sampler_only:
        res["meters"] = meters_row(dev, a, gt, P)
    for B in ([] if a.meters_only else a.batches):
        dfetch = dataset.DeviceFetcher(gt, gt, B, patch_num_point=P, device=dev, seed=1)
        dloop = Looping(dfetch, B)
        # bare sampler calls, back to back (launch + kernel; the queue never drains)
        for _ in range(10):
            dloop.next()
        n_bare = 200
        bare_us = window(dev, n_bare, dloop.next) * 1e3
        row = {"sampler_call_us": bare_us,
               # one batch: the G-point rows read once (the sub-sample re-reads P points of a row just read), input + gt + radius written
               "sampler_bytes_read": B * G * 12 + B * 4, "sampler_bytes_written": B * (P + G) * 12 + B * 4}
        res["batch"][str(B)] = row
        if a.sampler_only:
            continue
        np.random.seed(1)
        hloop = Looping(dataset.Fetcher(gt, gt, B, patch_num_point=P, device=dev), B)
        tr = Trainer(params=init_params(1234), device=dev)
        fixed = dloop.next()

        variants = {"a_step_fixed_batch": lambda: tr.train_step(*fixed),
                    "b_host_fetcher_plus_step": lambda: tr.train_step(*hloop.next()),
                    "c_device_fetcher_plus_step": lambda: tr.train_step(*dloop.next())}
        for body in variants.values():
            for _ in range(a.warmup):
                body()
        epochs_window(dev, a.warmup, tr, dfetch, dloop, B)
        times = {k: [] for k in list(variants) + ["d_train_one_epoch"]}
        for _ in range(a.windows):
            for k, body in variants.items():                 # alternate: drift hits every variant alike
                times[k].append(window(dev, a.steps, body))
            times["d_train_one_epoch"].append(epochs_window(dev, a.steps, tr, dfetch, dloop, B))
        dfetch.check_status()
        for k, v in times.items():
            row[k] = summary(v)
        med = {k: row[k]["median_ms"] for k in variants}
        row["c_minus_a_ms"] = med["c_device_fetcher_plus_step"] - med["a_step_fixed_batch"]
        row["d_minus_a_ms"] = row["d_train_one_epoch"]["median_ms"] - med["a_step_fixed_batch"]
        row["b_minus_a_ms"] = med["b_host_fetcher_plus_step"] - med["a_step_fixed_batch"]
        row["spread_a_ms"] = row["a_step_fixed_batch"]["max_ms"] - row["a_step_fixed_batch"]["min_ms"]
        row["c_faster_than_b"] = bool(max(times["c_device_fetcher_plus_step"]) < min(times["b_host_fetcher_plus_step"]))
        del tr
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
