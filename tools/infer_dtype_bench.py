#!/usr/bin/env python3
"""Does Generator(dtype="bf16") pay?  One process, 32 patches of 256 points (bench.py's step), three generators on the same weights
and inputs: strict fp32, the exploratory split_bf16 switch, and dtype="bf16" (F' stored as bf16 by the local cell, after_conv on the
bf16 matrix pipe from the pre-packed weight).

Each mode is set up the way bench.py sets up its step: return_views, two eager steps, the forward captured into a hipGraph, settle
replays, then 40 steps of replay against 40 eager steps and the faster one kept.  The timed loops (--loops, at least five, --steps steps
each) are bracketed by device events and INTERLEAVED: loop i visits the modes in order, loop i + 1 in reverse, a few untimed steps in
front of each (the previous mode's working set leaves the caches).  One eager pass per mode with Generator.profile and branches = False
(every launch alone on the device) gives the after_conv and ps_local launch times by HIP events (the minimum of --profile-passes).

Pass condition (reported, exit status 1 if it fails): the bf16 step's median is below the f32 AND the split_bf16 medians by more than
the larger of the min-max spreads of the modes compared.  --parent-json: the JSON an `--only f32 --package-root <parent tree>` run of
this tool wrote; the f32 median of this run must agree with it within the same spread (the default path has not moved).

Accuracy record (not asserted): on synth.patch_with_gt(32, 256, 1024, seed=7) with biased weights and a folded BatchNorm,
max |fine_bf16 - fine_f32| and the Chamfer distance between the two outputs beside the f32 output's Chamfer distance to the ground
truth.  Released weights are not in the tree: this says nothing about trained models.

Writes one JSON (default profiles/infer_dtype_bench.json), stamped with build.source_hash()."""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, NPT, UP = 32, 256, 4
SETTLE = 100
MODES = ("f32", "split_bf16", "bf16")


def make_generator(mode, params, dev):
    from dispu_amd.generator import Generator
    gen = Generator(params=params, device=dev, dtype="bf16") if mode == "bf16" else Generator(params=params, device=dev)
    gen.split_bf16 = mode == "split_bf16"
    gen.return_views = True
    return gen


def setup_step(gen, x, torch):
    """bench.py's setup: capture, settle, keep the faster of graph replay and eager launches.  -> (step, launch description)"""
    import time
    gen(x)
    gen(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gen(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gen(x)
    for _ in range(SETTLE):
        graph.replay()
    torch.cuda.synchronize()

    def clock(fn, n=40):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n
    eager = lambda: gen(x)
    for _ in range(10):
        eager()
    t_graph, t_eager = clock(graph.replay), clock(eager)
    if t_eager < 0.995 * t_graph:
        return eager, "eager (%.4f vs hipgraph %.4f ms)" % (t_eager * 1e3, t_graph * 1e3), graph
    return graph.replay, "hipgraph (%.4f vs eager %.4f ms)" % (t_graph * 1e3, t_eager * 1e3), graph


def kernel_times(gen, x, torch, passes):
    """after_conv and ps_local of one eager pass, every launch alone on the device: min over `passes` of the HIP-event times (us)"""
    br = gen.branches
    gen.branches = False
    best = {}
    for p in range(passes + 1):                          # pass 0 warms the one-stream path up and is dropped
        gen.profile = []
        gen(x)
        torch.cuda.synchronize()
        for name, e0, e1 in gen.profile:
            key = None
            if name.startswith("ps_local"):
                key = "ps_local"
            elif "2048x256]" in name:
                key = "after_conv"
            if key:
                us = e0.elapsed_time(e1) * 1e3
                prev = best.get(key)
                best[key] = dict(name=name, us=us if prev is None else min(us, prev["us"]))
        if p == 0:
            best = {}
    gen.profile = None
    gen.branches = br
    return best


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=50, help="steps per timed loop")
    ap.add_argument("--loops", type=int, default=6, help="timed loops per mode (at least 5)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps in front of every timed loop")
    ap.add_argument("--profile-passes", type=int, default=5)
    ap.add_argument("--only", choices=MODES, default=None, help="time one mode only (the parent-tree run: --only f32)")
    ap.add_argument("--package-root", default=None, help="import dispu_amd from this tree instead of the tool's own")
    ap.add_argument("--parent-json", default=None, help="JSON of an --only f32 run on the parent commit's tree")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.loops < 5:
        sys.exit("--loops must be at least 5")
    root = os.path.abspath(a.package_root) if a.package_root else os.path.dirname(HERE)
    sys.path.insert(0, root)
    out = a.out or os.path.join(os.path.dirname(HERE), "profiles", "infer_dtype_bench.json")

    import numpy as np
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import synth
    from dispu_amd.params import init_params
    spec = importlib.util.spec_from_file_location("dispu_build", os.path.join(root, "dis-pu_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)

    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    modes = (a.only,) if a.only else MODES
    params = init_params(seed=1234)                               # bench.py's weights and inputs
    x = torch.from_numpy(synth.patches(B, NPT, seed=2000)).to(dev)
    gens, steps, launch = {}, {}, {}
    keep = []
    for m in modes:
        gens[m] = make_generator(m, params, dev)
        steps[m], launch[m], g = setup_step(gens[m], x, torch)
        keep.append(g)

    ms = {m: [] for m in modes}
    for loop in range(a.loops):
        for m in (modes if loop % 2 == 0 else modes[::-1]):
            for _ in range(a.warmup):
                steps[m]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                steps[m]()
            e1.record()
            torch.cuda.synchronize()
            ms[m].append(e0.elapsed_time(e1) / a.steps)

    rm = B * NPT * UP
    res = {"tool": "infer_dtype_bench", "source_hash": build.source_hash(), "tree": "other (--package-root)" if a.package_root else "own", "device": torch.cuda.get_device_name(dev),
           "patches": B, "points": NPT, "steps_per_loop": a.steps, "loops": a.loops, "modes": {}}
    for m in modes:
        v = sorted(ms[m])
        res["modes"][m] = dict(ms_per_step=float(np.median(v)), ms_min=v[0], ms_max=v[-1], ms_spread=v[-1] - v[0], ms_loops=ms[m], launch=launch[m],
                               kernels_us=kernel_times(gens[m], x, torch, a.profile_passes),
                               fprime_bytes=rm * 2048 * (2 if m == "bf16" else 4), fprime_storage="bf16" if m == "bf16" else "fp32")
    ok = True
    if not a.only:
        md = res["modes"]
        cond = {}
        for other in ("f32", "split_bf16"):
            margin = md[other]["ms_per_step"] - md["bf16"]["ms_per_step"]
            need = max(md[other]["ms_spread"], md["bf16"]["ms_spread"])
            cond["bf16_vs_" + other] = dict(margin_ms=margin, larger_spread_ms=need, passed=bool(margin > need))
            ok = ok and margin > need
        res["pass_condition"] = cond
        if a.parent_json:
            par = json.load(open(a.parent_json))
            pf = par["modes"]["f32"]
            diff = abs(md["f32"]["ms_per_step"] - pf["ms_per_step"])
            need = max(md["f32"]["ms_spread"], pf["ms_spread"])
            res["f32_vs_parent"] = dict(parent_ms_per_step=pf["ms_per_step"], parent_ms_min=pf["ms_min"], parent_ms_max=pf["ms_max"],
                                        parent_source_hash=par["source_hash"], diff_ms=diff, larger_spread_ms=need, passed=bool(diff <= need))
            ok = ok and diff <= need
        else:
            res["f32_vs_parent"] = "not measured"
        res["passed"] = bool(ok)

        # ---- accuracy record
        from dispu_amd import loss_utils
        from oracle import generator as OG
        P = OG.init_params(seed=1234, bias_scale=0.05, bn_random=True)
        xi, gt = synth.patch_with_gt(B, NPT, NPT * UP, seed=7)
        tx, tgt = torch.from_numpy(xi).to(dev), torch.from_numpy(gt).to(dev)
        fine = {}
        for m in ("f32", "bf16"):
            g = make_generator(m, P, dev)
            g.return_views = False
            fine[m] = g(tx)[1]
        torch.cuda.synchronize()
        res["accuracy"] = dict(
            inputs="synth.patch_with_gt(32, 256, 1024, seed=7), OG.init_params(seed=1234, bias_scale=0.05, bn_random=True)",
            max_abs_fine_bf16_minus_f32=float((fine["bf16"] - fine["f32"]).abs().max()),
            chamfer_bf16_to_f32=float(loss_utils.chamfer(fine["bf16"], fine["f32"])),
            chamfer_f32_to_gt=float(loss_utils.chamfer(fine["f32"], tgt)),
            chamfer_bf16_to_gt=float(loss_utils.chamfer(fine["bf16"], tgt)),
            note="random weights: released weights are not in the tree, no statement about trained models")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
