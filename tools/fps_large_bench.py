#!/usr/bin/env python3
"""Farthest point sampling above 24576 points: the streaming kernel (dispu_fps_ws, the yardstick) against the cell-skipping kernels
(dispu_fps_cells, csrc/fps_cells.hip) on seeded sphere clouds, in one process per shape.

Every shape is a step of its own: a fresh child process under its own time limit; the first step that fails or runs out of time ends
the run.  Times are device-event times of the whole call on an otherwise idle stream, after one warm-up call per path; the two paths
alternate inside the repeats; each figure is reported as [median, min, max] in ms.  The cell path is split into the pre-pass (the
call at m = 1: bounds, keys, sort, cells and a sampling kernel without rounds) and the rounds (the rest).  Indices must be equal.
Writes profiles/fps_large_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_M = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
# name -> (kind, args, time limit in seconds)
STEPS = [
    ("b1_n27648_m9216", ("pair", (1, 27648, 9216, 5), 120)),
    ("b1_n122880_m40960", ("pair", (1, 122880, 40960, 3), 240)),
    ("b8_n122880_m40960", ("pair", (8, 122880, 40960, 3), 240)),
    ("b1_n102400_m1200", ("pair", (1, 102400, 1200, 5), 120)),
    ("b1_n1228800_m8192", ("pair", (1, 1228800, 8192, 3), 300)),
    ("sweep_n30000", ("sweep", (30000, 5), 180)),
    ("sweep_n122880", ("sweep", (122880, 5), 240)),
    ("cells_b1_n1228800_m409600", ("cells", (1, 1228800, 409600, 3), 300)),
    ("cell_size_n122880_m40960", ("cellsize", (122880, 40960, (64, 128, 256, 512), 3), 240)),
    ("cell_size_n1228800_m65536", ("cellsize", (1228800, 65536, (512, 1024, 2048, 4096), 3), 300)),
    ("upsample_cloud_n102400", ("upsample", (102400, 2), 360)),
]


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def _sphere(b, n, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((b, n, 3), generator=g)
    x = x / x.norm(dim=2, keepdim=True) * torch.tensor([1.0, 0.8, 1.25])
    return x.to(torch.float32).contiguous().cuda()


class _Paths(object):
    """the two paths on one batch [b, n, 3], buffers allocated once"""

    def __init__(self, x, m, cell=0):
        import numpy as np
        import torch
        from dispu_amd import _lib
        self.L, self._lib, self.x, self.m, self.cell = _lib.lib(), _lib, x, m, cell
        b, n, _ = x.shape
        self.b, self.n = b, n
        dev = x.device
        self.st = _lib.stream_ptr(dev)
        self.out_s = torch.empty((b, m), dtype=torch.int32, device=dev)
        self.out_c = torch.empty((b, m), dtype=torch.int32, device=dev)
        nb = self.L.dispu_fps_scratch_bytes(b, n, m)
        self.temp = torch.empty((max(nb, 4) // 4,), dtype=torch.float32, device=dev)
        self.nb = nb
        self.off = (np.arange(b + 1, dtype=np.int64) * n).astype(np.int32)
        self.moff = {mm: (np.arange(b + 1, dtype=np.int64) * mm).astype(np.int32) for mm in (1, m)}
        self.d_off = torch.from_numpy(self.off).to(dev)
        self.d_moff = {mm: torch.from_numpy(v).to(dev) for mm, v in self.moff.items()}
        hp = lambda a: _lib.C.c_void_p(a.ctypes.data)
        self.hp = hp
        self.cb = self.L.dispu_fps_cells_scratch_bytes(b, hp(self.off), hp(self.moff[m]), 0)
        assert self.cb > 0
        self.scratch = torch.empty((self.cb,), dtype=torch.uint8, device=dev)
        self.status = torch.zeros((b,), dtype=torch.int32, device=dev)

    def stream(self):
        self._lib.check(self.L.dispu_fps_ws(self.b, self.n, self.m, self._lib.ptr(self.x), self._lib.ptr(self.temp), self.nb,
                                            self._lib.ptr(self.out_s), 1, self.st), "dispu_fps_ws")

    def cells(self, m=None):
        m = self.m if m is None else m
        self._lib.check(self.L.dispu_fps_cells(self.b, self._lib.ptr(self.d_off), self._lib.ptr(self.d_moff[m]), self.hp(self.off),
                                               self.hp(self.moff[m]), self._lib.ptr(self.x), self._lib.ptr(self.scratch), self.cb,
                                               self._lib.ptr(self.out_c), self._lib.ptr(self.status), 1, self.cell, self.st),
                        "dispu_fps_cells")

    def prepass(self):
        self.cells(1)


def _timed_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(fns, reps):
    """one warm-up call each, then `reps` rounds in which the functions alternate -> {name: [ms, ...]}"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_timed_ms(fn))
    return ts


def step_pair(b, n, m, reps):
    import torch
    p = _Paths(_sphere(b, n, 7), m)
    ts = _alternate(dict(stream=p.stream, cells=p.cells, prepass=p.prepass), reps)
    p.stream()
    p.cells()
    torch.cuda.synchronize()
    assert not bool(p.status.any())
    assert torch.equal(p.out_s, p.out_c), "the cell path's indices differ from dispu_fps_ws"
    s, c, pre = _stats(ts["stream"]), _stats(ts["cells"]), _stats(ts["prepass"])
    return dict(b=b, n=n, m=m, reps=reps, equal_indices=True, stream_ms=s, cells_ms=c, cells_prepass_ms=pre,
                cells_rounds_ms=round(c[0] - pre[0], 4), stream_us_per_round=round(s[0] * 1e3 / max(m - 1, 1), 3),
                cells_us_per_round=round((c[0] - pre[0]) * 1e3 / max(m - 1, 1), 3), speedup=round(s[0] / c[0], 3))


def step_sweep(n, reps):
    import torch
    x = _sphere(1, n, 9)
    rows = []
    for m in SWEEP_M:
        p = _Paths(x, m)
        ts = _alternate(dict(stream=p.stream, cells=p.cells), reps)
        torch.cuda.synchronize()
        assert torch.equal(p.out_s, p.out_c), "the cell path's indices differ from dispu_fps_ws"
        s, c = _stats(ts["stream"]), _stats(ts["cells"])
        # the cell path wins only where even its slowest repeat beats the streaming kernel's fastest
        rows.append(dict(m=m, stream_ms=s, cells_ms=c, cells_wins_beyond_spread=bool(c[2] < s[1])))
    return dict(n=n, reps=reps, equal_indices=True, rows=rows)


def step_cells(b, n, m, reps):
    import torch
    p = _Paths(_sphere(b, n, 7), m)
    ts = _alternate(dict(cells=p.cells, prepass=p.prepass), reps)
    torch.cuda.synchronize()
    assert not bool(p.status.any())
    c, pre = _stats(ts["cells"]), _stats(ts["prepass"])
    return dict(b=b, n=n, m=m, reps=reps, cells_ms=c, cells_prepass_ms=pre, cells_rounds_ms=round(c[0] - pre[0], 4),
                cells_us_per_round=round((c[0] - pre[0]) * 1e3 / (m - 1), 3), scratch_MB=round(p.cb / 2 ** 20, 1))


def step_cellsize(n, m, cells, reps):
    """the whole call at forced cell sizes (the first is the automatic one), alternating"""
    import torch
    x = _sphere(1, n, 7)
    ps = {c: _Paths(x, m, c) for c in cells}
    ts = _alternate({c: p.cells for c, p in ps.items()}, reps)
    torch.cuda.synchronize()
    for p in ps.values():
        assert torch.equal(p.out_c, ps[cells[0]].out_c)
    return dict(n=n, m=m, reps=reps, equal_indices=True, cells_ms_by_cell_size={str(c): _stats(t) for c, t in ts.items()})


def step_upsample(n, reps):
    """upsample_cloud's stages (dis-pu_amd/upsample.py:upsample_clouds, same calls in the same order) with the device synchronised
    between them; the result must equal upsample_cloud's"""
    import numpy as np
    import torch
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    from oracle import generator as OG
    dev = torch.device("cuda:0")
    gen = Generator(params=OG.init_params(seed=1), device=dev)
    cloud = _sphere(1, n, 11)
    k, ratio = 256, 4

    def staged():
        t = {}

        def lap(name, t0):
            torch.cuda.synchronize()
            t[name] = (time.perf_counter() - t0) * 1e3
            return time.perf_counter()
        t0 = time.perf_counter()
        cloud_n, c0, f0 = U.normalize_patches(cloud)
        t0 = lap("normalize", t0)
        seeds = U.farthest_point_sample(int(n / k * 3), cloud_n)
        t0 = lap("seed_fps", t0)
        pidx = U.knn_patch(cloud_n, U.gather_point(cloud_n, seeds), k)
        patches = U.gather_point(cloud_n, pidx.reshape(1, -1)).reshape(-1, k, 3)
        pn, pc_c, pc_f = U.normalize_patches(patches)
        t0 = lap("patches_knn_gather_normalize", t0)
        _, fine = U.generator_chain(gen, pn, ratio)
        t0 = lap("generator", t0)
        merged = U.denormalize_patches(U.denormalize_patches(fine, pc_c, pc_f).reshape(1, -1, 3), c0, f0)
        t0 = lap("denormalize", t0)
        sel = U.farthest_point_sample(n * ratio, merged)
        t0 = lap("final_fps", t0)
        res = U.gather_point(merged, sel)
        lap("gather", t0)
        return res, t, (int(merged.shape[1]), int(sel.shape[1]))

    staged()
    runs = [staged() for _ in range(reps)]
    want = U.upsample_cloud(gen, cloud[0])
    assert np.array_equal(runs[-1][0][0].cpu().numpy(), want)
    stages = {name: _stats([r[1][name] for r in runs]) for name in runs[0][1]}
    total = _stats([sum(r[1].values()) for r in runs])
    return dict(n=n, reps=reps, seed_fps_shape=[n, int(n / k * 3)], final_fps_shape=list(runs[0][2]), stages_ms=stages, total_ms=total,
                longest_stage=max(stages, key=lambda s: stages[s][0]))


KINDS = dict(cellsize=step_cellsize, pair=step_pair, sweep=step_sweep, cells=step_cells, upsample=step_upsample)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_large_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/fps_large_bench.py needs an MI355X"
        kind, args, _ = steps[a.step]
        print("RESULT " + json.dumps(KINDS[kind](*args)))
        return 0
    res = dict(metric="fps_large", unit="ms [median, min, max]", arith="contract",
               cloud="seeded ellipsoid surface (unit sphere scaled by 1, 0.8, 1.25)", steps={})
    rc = 0
    for name, (kind, args, limit) in STEPS:
        if a.only and name not in a.only:
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               timeout=limit)
            text = r.stdout.decode(errors="replace")
            line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                res["steps"][name] = dict(failed=True, returncode=r.returncode, tail=text[-2000:])
                rc = 1
            else:
                res["steps"][name] = json.loads(line[-1][7:])
        except subprocess.TimeoutExpired:
            res["steps"][name] = dict(failed=True, timeout_s=limit)
            rc = 1
        print(name, json.dumps(res["steps"][name]), flush=True)
        if rc:
            break                                        # nothing more on the device after a failure
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return rc


if __name__ == "__main__":
    sys.exit(main())
