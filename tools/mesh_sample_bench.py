#!/usr/bin/env python3
"""Mesh-sampler timings (HIP events, eager, warm-up then the median of `--reps`; run it in a fresh process): poisson_disk_cloud on one
mesh at 32768 -> 8192 and 8192 -> 2048 candidates -> points, and make_patches at 200 patches (4096 -> 1024 and -> 256), each with its
stages alone (surface samples, the two selections) and beside what a user could do before for the same job: the exact FPS of the same
m from the same candidates.  The b = 1 whole-cloud selection runs in ONE workgroup, i.e. on one CU, by design (the greedy order is
sequential per cloud); batching -- the 200 patch regions -- is what fills the part.  Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dispu_amd  # noqa: E402,F401
from dispu_amd import mesh as M, mesh_sample as S  # noqa: E402
from dispu_amd.tf_sampling import farthest_point_sample, gather_point  # noqa: E402
import mesh_oracle as MO  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mesh", default="fandisk", choices=("fandisk", "Icosahedron"))
    ap.add_argument("--patches", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    dev = torch.device("cuda:0")
    tmp = tempfile.TemporaryDirectory()
    golden = MO.extract_pugan(os.path.join(ROOT, "tests", "golden"), tmp.name)
    mesh = M.Mesh.from_off(os.path.join(golden, a.mesh + ".off"), dev)
    out = {"metric": "mesh_sample", "unit": "ms", "mesh": a.mesh, "faces": mesh.num_faces, "reps": a.reps}
    for m in (8192, 2048):
        n = 4 * m
        tag = "%d_to_%d" % (n, m)
        cand, _ = S.sample_surface(mesh, n, 0)
        c1 = cand.reshape(1, n, 3)
        r_hi = S.hex_radius(mesh.total_area, m)
        out["cloud_%s_total" % tag] = _ms(lambda: S.poisson_disk_cloud(mesh, m), a.reps)
        out["cloud_%s_sample_surface" % tag] = _ms(lambda: S.sample_surface(mesh, n, 0), a.reps)
        out["cloud_%s_select_12_steps" % tag] = _ms(lambda: S.poisson_disk_select(cand, m, r_hi), a.reps)
        out["cloud_%s_keep_one_radius" % tag] = _ms(lambda: S.poisson_disk_keep(cand, 0.85 * r_hi), a.reps)
        out["cloud_%s_exact_fps_same_candidates" % tag] = _ms(lambda: gather_point(c1, farthest_point_sample(m, c1)), a.reps)
        _, r, count = S.poisson_disk_select(cand, m, r_hi)
        out["cloud_%s_radius_over_r_hi" % tag] = float(r.item()) / r_hi
        out["cloud_%s_surplus" % tag] = int(count.item()) - m
    P, k = a.patches, 4096
    out["patches"] = P
    out["patches_make_patches_total"] = _ms(lambda: S.make_patches(mesh, P), a.reps)
    out["patches_regions_sample_fps_knn_sort"] = _ms(lambda: S.patch_regions(mesh, P, k), a.reps)
    dense, _, regions = S.patch_regions(mesh, P, k)
    D = dense.shape[0]
    cand = gather_point(dense.reshape(1, D, 3), regions.reshape(1, -1)).reshape(P, k, 3)
    area = mesh.total_area * k / D
    for num in (1024, 256):
        out["patches_select_4096_to_%d" % num] = _ms(lambda: S.poisson_disk_select(cand, num, S.hex_radius(area, num)), a.reps)
        out["patches_exact_fps_4096_to_%d" % num] = _ms(lambda: gather_point(cand, farthest_point_sample(num, cand)), a.reps)
        _, r, count = S.poisson_disk_select(cand, num, S.hex_radius(area, num))
        out["patches_4096_to_%d_max_surplus" % num] = int(count.max().item()) - num
    out["patches_sort_rows_%dx4096" % P] = _ms(lambda: S.sort_rows(regions), a.reps)
    print(json.dumps({k_: (round(x, 4) if isinstance(x, float) else x) for k_, x in out.items()}))


if __name__ == "__main__":
    main()
