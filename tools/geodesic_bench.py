#!/usr/bin/env python3
"""Geodesic disk timings (HIP events, eager, median of `--reps`): exact geodesic membership (mesh.geodesic_disk_members: candidates,
window propagation, count + scan + fill, the host reads of the CSR sizes and the per-seed status included) at 1000 seeds x 2 radii
over the 8192 network outputs on each PU-GAN test mesh, and at 1000 seeds over 32768 points on a subdivided sphere of 327680 faces;
the Euclidean membership beside it; and the float64 oracle of tests/geodesic_oracle.py per seed for comparison.  Prints one JSON
line.  Not part of bench.py."""
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
import geodesic_oracle as GO  # noqa: E402
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
    ap.add_argument("--oracle-seeds", type=int, default=8, help="seeds the CPU oracle is timed on (0: skip)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "geodesic_disks", "unit": "ms"}
    tmp = tempfile.TemporaryDirectory()
    GOLDEN = MO.extract_pugan(os.path.join(ROOT, "tests", "golden"), tmp.name)
    for s in ("Icosahedron", "fandisk"):
        mesh = M.Mesh.from_off(os.path.join(GOLDEN, s + ".off"), dev)
        pts = torch.from_numpy(np.loadtxt(os.path.join(GOLDEN, s + "_X4.xyz"))[:, :3].astype(np.float32)).to(dev)
        _, proj, face = M.point_to_mesh(pts, mesh)
        fid, bary = M.sample_surface_seeds(mesh, 1000, seed=0)
        radii = M.disk_radii(mesh)
        seeds = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
        mesh.geodesic_tables()
        out["geodesic_1000x2_8192_%s_%dF" % (s, mesh.num_faces)] = _ms(lambda: M.geodesic_disk_members(mesh, fid, bary, proj, face, radii), a.reps)
        out["euclidean_1000x2_8192_%s" % s] = _ms(lambda: M.disk_members(seeds, proj, radii), a.reps)
        go, gm = M.geodesic_disk_members(mesh, fid, bary, proj, face, radii)
        eo, em = M.disk_members(seeds, proj, radii)
        out["members_geodesic_%s" % s] = int(go[-1].item())
        out["members_euclidean_%s" % s] = int(eo[-1].item())
        if a.oracle_seeds > 0:
            P, Fq = proj.cpu().numpy(), face.cpu().numpy()
            surf = GO.Surface(mesh.verts, mesh.faces)
            sp = mesh.surface_points(fid, bary)
            t0 = time.perf_counter()
            for i in range(a.oracle_seeds):
                near = np.nonzero(np.linalg.norm(P.astype(np.float64) - sp[i], axis=1) <= float(radii.max()) * 1.001)[0]
                GO.geodesic(mesh.verts, mesh.faces, fid[i], bary[i], P[near], Fq[near], float(radii.max()), surface=surf)
            out["cpu_oracle_per_seed_%s_ms" % s] = (time.perf_counter() - t0) * 1e3 / a.oracle_seeds
    v, f = synth.icosphere(7, radius=0.8)
    mesh = M.Mesh(v, f, dev)
    rng = np.random.default_rng(0)
    g = rng.standard_normal((32768, 3))
    p = torch.from_numpy((g / np.linalg.norm(g, axis=1, keepdims=True) * 0.8).astype(np.float32)).to(dev)
    _, proj, face = M.point_to_mesh(p, mesh)
    fid, bary = M.sample_surface_seeds(mesh, 1000, seed=0)
    radii = M.disk_radii(mesh)
    mesh.geodesic_tables()
    out["geodesic_1000x2_32768_sphere_%dF" % mesh.num_faces] = _ms(lambda: M.geodesic_disk_members(mesh, fid, bary, proj, face, radii),
                                                                  max(2, a.reps // 3), warm=1)
    print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
