#!/usr/bin/env python3
"""Rigid registration (dis-pu_amd/registration.py, csrc/icp.hip) on seeded ellipsoid surfaces, one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times around the WHOLE call (allocations, launches and the status
read-back included) on an otherwise idle stream after one warm-up call, the sides alternating, reported as [median, min, max] in ms.

Per shape and mode (point to point, point to plane), at tolerance 0: icp at 10 iterations and at 0 (the evaluation every call ends
with), so the time per iteration is (t10 - t0) / 10; beside the same loop composed from what existed before: a float64 torch apply,
knn_cross(k = 1) with indices and distances, torch gathers, the normal equations as torch reductions in float64, torch.linalg.solve_ex
and the Rodrigues update, nothing read back inside the loop.  Before anything is timed the two are compared: after 10 iterations their
transforms must agree to 1e-6 (the two round the moved points in different orders, so a nearest point can differ at a near tie).  The
child prints its result once without the composed form and once with it, so a composed form that runs out of time still leaves the rest.
Writes profiles/icp_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attributes_bench import AXES, _ellipsoids, _repeat  # noqa: E402  (the same clouds, the same timing)

ITERATIONS = 10

# name -> ((pairs, source points per pair, target points per pair, repeats), time limit in seconds)
STEPS = [
    ("c64_q8192_m8192", ((64, 8192, 8192, 5), 300)),
    ("c1_q102400_m102400", ((1, 102400, 102400, 5), 240)),
    ("c1_q409600_m409600", ((1, 409600, 409600, 5), 300)),
    ("c1_q409600_m1228800", ((1, 409600, 1228800, 3), 360)),
]


def _motion(dev):
    """3 degrees about (0.3, -0.5, 0.8) and a shift of 0.01: inside the basin of both modes on these clouds"""
    import torch
    w = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    w = (w / w.norm() * (3.0 * 3.141592653589793 / 180.0)).tolist()
    K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.linalg.matrix_exp(K)
    M[:3, 3] = torch.tensor([0.005, -0.003, 0.002], dtype=torch.float64) * 2
    return M.to(dev)


def _skew(w):
    import torch
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def composed(sources, targets, normals, iterations):
    """the loop from knn_cross and torch, everything after the search in float64 -> the transforms [C, 4, 4] and the last rmse [C]"""
    import torch
    from dispu_amd import attributes as A
    dev = sources[0].device
    T = [torch.eye(4, dtype=torch.float64, device=dev) for _ in sources]
    rmse = [None] * len(sources)
    for it in range(iterations + 1):
        cur = [(s.double() @ t[:3, :3].T + t[:3, 3]).float() for s, t in zip(sources, T)]
        idx, _ = A.knn_cross(cur, targets, 1)
        for c, (x, tg, i) in enumerate(zip(cur, targets, idx)):
            j = i[:, 0].long()
            o = tg[0].double()
            p = x.double() - o
            d = p - (tg[j].double() - o)
            if normals is None:
                if it == iterations:
                    rmse[c] = (d * d).sum().div(len(x)).sqrt()
                    continue
                n = float(len(x))
                sp = p.sum(dim=0)
                Am = torch.zeros((6, 6), dtype=torch.float64, device=dev)
                Am[:3, :3] = (p * p).sum() * torch.eye(3, dtype=torch.float64, device=dev) - p.T @ p
                Am[:3, 3:] = _skew(sp)
                Am[3:, :3] = _skew(sp).T
                Am[3:, 3:] = n * torch.eye(3, dtype=torch.float64, device=dev)
                b = torch.cat([torch.linalg.cross(p, d).sum(dim=0), d.sum(dim=0)])
            else:
                nn = normals[c][j].double()
                r = (d * nn).sum(dim=1)
                if it == iterations:
                    rmse[c] = (r * r).sum().div(len(x)).sqrt()
                    continue
                J = torch.cat([torch.linalg.cross(p, nn), nn], dim=1)
                Am, b = J.T @ J, J.T @ r
            sol = torch.linalg.solve_ex(Am, -b)[0]
            R = torch.linalg.matrix_exp(_skew(sol[:3]))
            U = torch.eye(4, dtype=torch.float64, device=dev)
            U[:3, :3] = R
            U[:3, 3] = o + sol[3:] - R @ o
            T[c] = U @ T[c]
    return torch.stack(T), torch.stack(rmse)


def step(c, nq, m, reps):
    import torch
    from dispu_amd import registration as R
    targets = _ellipsoids(c, m, 7)
    M = _motion(targets[0].device)
    sources = R.apply_transform(_ellipsoids(c, nq, 11), M[None].expand(c, 4, 4))
    axes2 = torch.tensor(AXES, dtype=torch.float32, device=targets[0].device) ** 2
    normals = [torch.nn.functional.normalize(t / axes2, dim=1).contiguous() for t in targets]
    res = dict(pairs=c, q=nq, m=m, reps=reps, iterations=ITERATIONS, tolerance=0.0, composed="not measured")
    fns = {}
    for mode, nrm in (("point", None), ("plane", normals)):
        fns["icp_%s_%d" % (mode, ITERATIONS)] = lambda nrm=nrm: R.icp(sources, targets, nrm, iterations=ITERATIONS, tolerance=0.0)
        fns["icp_%s_0" % mode] = lambda nrm=nrm: R.icp(sources, targets, nrm, iterations=0, tolerance=0.0)

    def ratios():
        for mode in ("point", "plane"):
            t10, t0 = res["icp_%s_%d_ms" % (mode, ITERATIONS)][0], res["icp_%s_0_ms" % mode][0]
            res["icp_%s_ms_per_iteration" % mode] = round((t10 - t0) / ITERATIONS, 4)
            key = "composed_%s_%d_ms" % (mode, ITERATIONS)
            if key in res:
                c10, c0 = res[key][0], res["composed_%s_0_ms" % mode][0]
                res["composed_%s_ms_per_iteration" % mode] = round((c10 - c0) / ITERATIONS, 4)
                res["icp_over_composed_%s_whole_call" % mode] = round(t10 / c10, 3)
                res["icp_over_composed_%s_per_iteration" % mode] = round((t10 - t0) / (c10 - c0), 3)

    res.update({name + "_ms": t for name, t in _repeat(fns, reps).items()})
    ratios()
    print("RESULT " + json.dumps(res), flush=True)
    for mode, nrm in (("point", None), ("plane", normals)):
        ours = R.icp(sources, targets, nrm, iterations=ITERATIONS, tolerance=0.0)
        theirs, their_rmse = composed(sources, targets, nrm, ITERATIONS)
        gap = (ours.transform - theirs).abs().max().item()
        res["max_abs_transform_gap_to_composed_%s" % mode] = gap
        res["rmse_%s" % mode] = [ours.rmse.max().item(), their_rmse.max().item()]
        res["undone_motion_error_%s" % mode] = (ours.transform @ M - torch.eye(4, dtype=torch.float64, device=M.device)).abs().max().item()
        assert gap <= 1e-6, "icp and its composed form differ by %g in the transform (%s)" % (gap, mode)
        del ours, theirs
        fns["composed_%s_%d" % (mode, ITERATIONS)] = lambda nrm=nrm: composed(sources, targets, nrm, ITERATIONS)
        fns["composed_%s_0" % mode] = lambda nrm=nrm: composed(sources, targets, nrm, 0)
    res.update({name + "_ms": t for name, t in _repeat(fns, reps).items()})
    res["composed"] = "measured"
    ratios()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON lines")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/icp_bench.py needs an MI355X"
        step(*steps[a.step][0])
        return 0
    res = dict(metric="rigid_registration", unit="ms [median, min, max], device events around the whole call", arith="plain",
               cloud="seeded ellipsoid surfaces (unit sphere scaled by 1, 0.8, 1.25): the source another sample, turned by 3 degrees and "
                     "shifted by 0.01", steps={})
    rc = 0
    for name, (_, limit) in STEPS:
        if a.only and name not in a.only:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        text = r.stdout.decode(errors="replace")
        line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        got = json.loads(line[-1][7:]) if line else {}
        if r.returncode != 0:
            got.update(failed=True, returncode=r.returncode, tail=text[-2000:])
            rc = 1
        res["steps"][name] = got
        print(name, json.dumps(got), flush=True)
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
