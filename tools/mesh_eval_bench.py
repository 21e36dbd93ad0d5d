#!/usr/bin/env python3
"""Evaluator mesh-metric timings (HIP events, eager, median of `--reps`): P2F (dispu_point_to_mesh) at 8192 points on each
PU-GAN test mesh and at 32768 points on a subdivided sphere of 327680 faces, pruned and brute force; disk membership
(count + scan + fill, one scalar read back) and uniformity at 1000 seeds.  The float64 oracle of tests/mesh_oracle.py on
the first fixture gives the CPU time for comparison.  Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dispu_amd  # noqa: E402,F401
from dispu_amd import mesh as M, synth  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU oracle timing")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "mesh_eval", "unit": "ms"}
    tmp = tempfile.TemporaryDirectory()
    GOLDEN = MO.extract_pugan(os.path.join(ROOT, "tests", "golden"), tmp.name)
    for s in ("Icosahedron", "fandisk"):
        mesh = M.Mesh.from_off(os.path.join(GOLDEN, s + ".off"), dev)
        pts = np.loadtxt(os.path.join(GOLDEN, s + "_X4.xyz"))[:, :3].astype(np.float32)
        p = torch.from_numpy(pts).to(dev)
        out["p2f_8192_%s_%dF" % (s, mesh.num_faces)] = _ms(lambda: M.point_to_mesh(p, mesh), a.reps)
        out["p2f_8192_%s_brute" % s] = _ms(lambda: M.point_to_mesh(p, mesh, brute_force=True), a.reps)
        if s == "Icosahedron":
            fid, bary = M.sample_surface_seeds(mesh, 1000, seed=0)
            seeds = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
            _, proj, _ = M.point_to_mesh(p, mesh)
            radii = M.disk_radii(mesh)
            pct = np.asarray(M.DEFAULT_PERCENTAGES)
            out["membership_1000x2_8192"] = _ms(lambda: M.disk_members(seeds, proj, radii), a.reps)
            off, mem = M.disk_members(seeds, proj, radii)
            out["uniformity_1000x2_8192"] = _ms(lambda: M.uniformity(proj, off, mem, radii, pct), a.reps)
            out["mesh_metrics_total_8192"] = _ms(lambda: M.mesh_metrics(p, mesh), a.reps)
            if not a.no_cpu:
                t0 = time.perf_counter()
                MO.point_to_mesh(pts, mesh.verts, mesh.faces)
                out["cpu_oracle_p2f_8192_%s_ms" % s] = (time.perf_counter() - t0) * 1e3
                offn, memn = off.cpu().numpy(), mem.cpu().numpy()
                t0 = time.perf_counter()
                MO.analyze_uniform([memn[offn[k]:offn[k + 1]] for k in range(offn.shape[0] - 1)], radii, proj.cpu().numpy())
                out["cpu_oracle_uniformity_1000x2_ms"] = (time.perf_counter() - t0) * 1e3
    v, f = synth.icosphere(7, radius=0.8)
    mesh = M.Mesh(v, f, dev)
    rng = np.random.default_rng(0)
    g = rng.standard_normal((32768, 3))
    p = torch.from_numpy((g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.75, 0.85, (32768, 1))).astype(np.float32)).to(dev)
    out["p2f_32768_sphere_%dF" % mesh.num_faces] = _ms(lambda: M.point_to_mesh(p, mesh), a.reps)
    out["p2f_32768_sphere_brute"] = _ms(lambda: M.point_to_mesh(p, mesh, brute_force=True), max(2, a.reps // 3), warm=1)
    print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
