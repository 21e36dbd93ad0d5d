#!/usr/bin/env python3
"""The surface reconstruction (dis-pu_amd/reconstruct.py, csrc/signed_distance.hip, csrc/reconstruct.hip), one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times around the WHOLE call (allocations, launches and read-backs
included) on an otherwise idle stream after one warm-up call, the compared functions alternating inside a round, reported as
[median, min, max] in ms.

c64_n8192: signed_distance alone on 64 sphere clouds of 8192 points, every cloud queried at itself moved off the surface, beside the
same value composed from what existed before: knn_cross, then torch gathers, the weights and the two sums in double.
c1_n*: one Poisson-disk cloud of the unit icosphere (poisson_cells.mesh_cloud) with its radial normals, voxel = twice the hexagonal
spacing, k = 8, support = 1.5, band = 1: reconstruct_surface whole, its split (grid stages, values, contouring: the events of its
`stages` argument) with the lattice and face counts, and signed_distance at the lattice's own positions beside the composed form.
The fused and the composed values are asserted to agree (to 1e-6 of the voxel: the composed sums add in another order) before anything is
timed.  Writes profiles/reconstruct_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, SUPPORT, BAND = 8, 1.5, 1

# name -> ((clouds, points per cloud, repeats), time limit in seconds)
STEPS = [
    ("c64_n8192", ((64, 8192, 5), 120)),
    ("c1_n102400", ((1, 102400, 5), 120)),
    ("c1_n409600", ((1, 409600, 5), 150)),
    ("c1_n1228800", ((1, 1228800, 3), 200)),
]


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def _timed_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _repeat(fns, reps):
    """one warm-up call each, then `reps` rounds in which the functions alternate -> {name: [median, min, max]}"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(_timed_ms(fn))
    return {name: _stats(t) for name, t in ts.items()}


def composed(queries, points, normals, k, support):
    """signed_distance from knn_cross and torch (lists in, lists out): the neighbours, then gathers, weights and sums in double"""
    import torch
    from dispu_amd.attributes import knn_cross
    idx, d2 = knn_cross(queries, points, k)
    out = []
    for q, p, n, i, d in zip(queries, points, normals, idx, d2):
        i = i.long()
        d = d.double()
        r2 = d / ((support * support) * d[:, k - 1:k])
        r = r2.clamp(0, 1).sqrt()
        w = torch.where(r2 < 1, (1 - r) ** 4 * (4 * r + 1), torch.zeros_like(r))
        g = ((q[:, None, :].double() - p[i].double()) * n[i].double()).sum(dim=2)
        s0 = w.sum(dim=1)
        out.append(torch.where(s0 != 0, (w * g).sum(dim=1) / s0, g[:, 0]).float())
    return out


def _agree(a, b, scale):
    import torch
    worst = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))
    assert worst <= 1e-6 * scale + 1e-9, "fused and composed signed distances differ by %g" % worst
    return worst


def step_batch(c, n, reps):
    import torch
    from dispu_amd.reconstruct import signed_distance
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn((c, n, 3), generator=g)
    x = (x / x.norm(dim=2, keepdim=True)).to(torch.float32).cuda()
    pts = [x[i].contiguous() for i in range(c)]
    qs = [(p * (1.0 + 0.05 * math.sin(i + 1.0))).contiguous() for i, p in enumerate(pts)]
    worst = _agree(signed_distance(qs, pts, pts, K, SUPPORT), composed(qs, pts, pts, K, SUPPORT), 1.0)
    ts = _repeat(dict(signed_distance=lambda: signed_distance(qs, pts, pts, K, SUPPORT),
                      composed_knn_cross_torch=lambda: composed(qs, pts, pts, K, SUPPORT)), reps)
    res = dict(clouds=c, n=n, queries=c * n, reps=reps, k=K, support=SUPPORT, largest_difference=worst)
    res.update({name + "_ms": t for name, t in ts.items()})
    return res


def step_cloud(n, reps):
    import torch
    from dispu_amd import mesh, poisson_cells, synth
    from dispu_amd.mesh_sample import hex_radius
    from dispu_amd.reconstruct import reconstruct_surface, signed_distance
    dev = torch.device("cuda:0")
    v, f = synth.icosphere(6)
    m = mesh.Mesh(v, f, dev)
    pts, _ = poisson_cells.mesh_cloud(m, n, oversample=4, seed=0)
    pts = pts.contiguous()
    nrm = (pts / pts.norm(dim=1, keepdim=True)).contiguous()
    voxel = 2.0 * float(hex_radius(m.total_area, n))
    stages = {}
    verts, faces = reconstruct_surface(pts, nrm, voxel, k=K, support=SUPPORT, band=BAND, stages=stages)
    pos = stages["positions"]
    worst = _agree([stages["values"]], composed([pos], [pts], [nrm], K, SUPPORT), voxel)
    split = {name: [] for name in ("grid_ms", "values_ms", "contour_ms")}

    def with_split():
        s = {}
        reconstruct_surface(pts, nrm, voxel, k=K, support=SUPPORT, band=BAND, stages=s)
        for name in split:
            split[name].append(s[name])
    with_split()                                               # warm-up of this form; its times are dropped
    for name in split:
        del split[name][:]
    ts = _repeat(dict(reconstruct_surface=lambda: reconstruct_surface(pts, nrm, voxel, k=K, support=SUPPORT, band=BAND),
                      reconstruct_surface_with_split=with_split,
                      signed_distance_at_lattice=lambda: signed_distance(pos, pts, nrm, K, SUPPORT),
                      composed_knn_cross_torch_at_lattice=lambda: composed([pos], [pts], [nrm], K, SUPPORT)), reps)
    for name in split:
        del split[name][0]                                     # _repeat's own warm-up call
    res = dict(clouds=1, n=n, reps=reps, k=K, support=SUPPORT, band=BAND, voxel=round(voxel, 6),
               occupied_voxels=stages["occupied"], active_voxels=stages["voxels"], lattice_vertices=stages["lattice"],
               mesh_vertices=int(verts.shape[0]), mesh_faces=int(faces.shape[0]), largest_difference=worst)
    res.update({name + "_ms": t for name, t in ts.items()})
    res.update({"split_" + name: _stats(t) for name, t in split.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        import dispu_amd  # noqa: F401
        assert torch.cuda.is_available(), "tools/reconstruct_bench.py needs an MI355X"
        (c, n, reps), _ = steps[a.step]
        print("RESULT " + json.dumps(step_batch(c, n, reps) if c > 1 else step_cloud(n, reps)))
        return 0
    res = dict(metric="surface_reconstruction", unit="ms [median, min, max], device events around the whole call", arith="plain",
               cloud="c64: seeded unit spheres; c1: Poisson-disk clouds of the level-6 icosphere, radial normals, voxel = 2 x hex spacing",
               steps={})
    rc = 0
    for name, (_, limit) in STEPS:
        if a.only and name not in a.only:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        text = r.stdout.decode(errors="replace")
        line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res["steps"][name] = dict(failed=True, returncode=r.returncode, tail=text[-2000:])
            rc = 1
        else:
            res["steps"][name] = json.loads(line[-1][7:])
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
