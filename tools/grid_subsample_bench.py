#!/usr/bin/env python3
"""Grid-subsampling timings (HIP events, eager, warm-up then the median of `--reps`; run it in a fresh process): 2^20 and 2^22 samples
of a surface (a unit sphere, jittered along the normal like a scan), sampleDl bisected to about 8 points per voxel.  Per size: the whole
call on device tensors (points only; with 3 feature columns; with 3 feature and 1 label column), its two C steps alone (plan: bounds,
keys, sort, run heads with the two readbacks; emit: the serial-run reduce, and the label sort when there are labels), the sorter alone
on the same keys with the algorithmic bytes of its passes (12 B per element, read twice -- histogram and scatter -- and written once)
against the 8 TB/s of HBM, and as a yardstick the same keys through torch.sort(stable=True) plus index_add_ (not bit-exact: index_add_
adds with float atomics in any order).  Prints one JSON line; --out also writes it to a file.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dispu_amd  # noqa: E402,F401
from dispu_amd import _lib, grid_subsampling as G  # noqa: E402

HBM_PEAK = 8.0e12


def _ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def surface(n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.randn((n, 3), generator=g, device=dev, dtype=torch.float32)
    v = v / v.norm(dim=1, keepdim=True)
    return (v * (1.0 + 0.002 * torch.randn((n, 1), generator=g, device=dev, dtype=torch.float32))).contiguous()


def find_dl(p, per_voxel):
    lo, hi = 1e-4, 1.0
    for _ in range(14):
        mid = (lo * hi) ** 0.5
        if p.shape[0] / G.compute(p, sampleDl=mid).shape[0] < per_voxel:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 22])
    ap.add_argument("--per_voxel", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    out = {"metric": "grid_subsample", "unit": "ms", "reps": a.reps, "hbm_peak_TBps": HBM_PEAK / 1e12}
    for n in a.sizes:
        tag = "n%d" % n
        p = surface(n, dev)
        f = torch.rand((n, 3), device=dev, dtype=torch.float32)
        c = torch.randint(0, 13, (n, 1), device=dev, dtype=torch.int32)
        dl = find_dl(p, a.per_voxel)
        nbytes = L.dispu_grid_subsample_scratch_bytes(n, 3, 1)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        m, status, info = C.c_int(0), C.c_int(0), (C.c_double * 8)()

        def plan():
            _lib.check(L.dispu_grid_subsample_plan(n, _lib.ptr(p), dl, _lib.ptr(scratch), nbytes, C.byref(m), C.byref(status), info, st), "plan")
        plan()
        M = m.value
        passes = int(info[6])
        op = torch.empty((M, 3), dtype=torch.float32, device=dev)
        of = torch.empty((M, 3), dtype=torch.float32, device=dev)
        oc = torch.empty((M, 1), dtype=torch.int32, device=dev)

        def emit(fdim, ldim):
            _lib.check(L.dispu_grid_subsample_emit(n, M, fdim, ldim, _lib.ptr(p), _lib.ptr(f), _lib.ptr(c), _lib.ptr(scratch), nbytes,
                                                   _lib.ptr(op), _lib.ptr(of), _lib.ptr(oc), st), "emit")
        out[tag + "_dl"] = dl
        out[tag + "_voxels"] = M
        out[tag + "_points_per_voxel"] = n / M
        out[tag + "_grid"] = [int(info[3]), int(info[4]), int(info[5])]
        out[tag + "_sort_passes"] = passes
        out[tag + "_compute_points"] = _ms(lambda: G.compute(p, sampleDl=dl), a.reps)
        out[tag + "_compute_points_features3"] = _ms(lambda: G.compute(p, f, sampleDl=dl), a.reps)
        out[tag + "_compute_points_features3_labels1"] = _ms(lambda: G.compute(p, f, c, sampleDl=dl), a.reps)
        out[tag + "_plan_bounds_keys_sort_heads"] = _ms(plan, a.reps)
        out[tag + "_emit_points"] = _ms(lambda: emit(0, 0), a.reps)
        out[tag + "_emit_points_features3"] = _ms(lambda: emit(3, 0), a.reps)
        out[tag + "_emit_points_features3_labels1"] = _ms(lambda: emit(3, 1), a.reps)
        out[tag + "_label_sort_passes"] = (32 + max(M - 1, 0).bit_length() + 7) // 8
        # the same keys, made with torch's float32 operations from the grid the plan reports
        origin = torch.tensor([info[0], info[1], info[2]], dtype=torch.float32, device=dev)
        idx = torch.floor((p - origin) / torch.tensor(dl, dtype=torch.float32, device=dev)).to(torch.int64)
        keys = (idx[:, 0] + int(info[3]) * idx[:, 1] + int(info[3]) * int(info[4]) * idx[:, 2] - int(info[7])).contiguous()
        vals = torch.arange(n, dtype=torch.int32, device=dev)
        ko, vo = torch.empty_like(keys), torch.empty_like(vals)
        sbytes = L.dispu_radix_sort_scratch_bytes(n)
        ss = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        bits = int(keys.max().item()).bit_length()

        def sort():
            _lib.check(L.dispu_radix_sort_pairs(n, bits, _lib.ptr(keys), _lib.ptr(vals), _lib.ptr(ko), _lib.ptr(vo), _lib.ptr(ss), sbytes, st),
                       "sort")
        t_sort = _ms(sort, a.reps)
        sk, sv = torch.sort(keys, stable=True)
        out[tag + "_sorter_matches_torch_sort"] = bool(torch.equal(sk, ko) and torch.equal(sv.to(torch.int32), vo))
        out[tag + "_sort_alone"] = t_sort
        out[tag + "_sort_alone_passes"] = (bits + 7) // 8
        out[tag + "_sort_bytes_per_pass"] = 36 * n
        out[tag + "_sort_hbm_frac"] = 36.0 * n * ((bits + 7) // 8) / (t_sort * 1e-3) / HBM_PEAK
        out[tag + "_torch_sort_stable"] = _ms(lambda: torch.sort(keys, stable=True), a.reps)

        def yardstick():
            sk, sv = torch.sort(keys, stable=True)
            head = torch.ones_like(sk, dtype=torch.bool)
            head[1:] = sk[1:] != sk[:-1]
            vid = torch.cumsum(head, 0) - 1
            mm = int(vid[-1].item()) + 1
            sums = torch.zeros((mm, 3), dtype=torch.float32, device=dev).index_add_(0, vid, p[sv])
            cnt = torch.zeros(mm, dtype=torch.float32, device=dev).index_add_(0, vid, torch.ones(n, dtype=torch.float32, device=dev))
            return sums / cnt[:, None]
        out[tag + "_torch_sort_index_add_points"] = _ms(yardstick, a.reps)
        y = yardstick()
        out[tag + "_yardstick_max_abs_diff"] = float((y - G.compute(p, sampleDl=dl)).abs().max().item())
    line = json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
