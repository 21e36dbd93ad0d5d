#!/usr/bin/env python3
"""The MLS projection (dis-pu_amd/mls.py, csrc/mls_project.hip) on seeded ellipsoid surfaces, one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times around the WHOLE call (allocations, launches and the status
read-back included) on an otherwise idle stream after one warm-up call, the sides alternating, reported as [median, min, max] in ms.

Per shape, at k = 16 and support 1: mls_project at one and at three iterations, beside (a) knn_cross alone at the same k, the floor (the
fit adds no pass over memory to the search), and (b) the same step composed from what existed before: knn_cross with indices and
distances, torch gathers, the weights and moments in float64 and a batched torch.linalg.eigh.  Before anything is timed the composed
step and mls_project are compared: the share of coordinates that agree to 1e-5 of the cloud's size is recorded and must be 99 %.
The child prints its result once without (b) and once with it, so a composed form that runs out of time still leaves the rest.
Writes profiles/mls_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attributes_bench import _ellipsoids, _repeat  # noqa: E402  (the same clouds, the same timing)

K, SUPPORT = 16, 1.0

# name -> ((clouds, queries per cloud, references per cloud or 0 for the queries themselves, repeats), time limit in seconds)
STEPS = [
    ("self_c64_n8192", ((64, 8192, 0, 5), 240)),
    ("self_c1_n409600", ((1, 409600, 0, 5), 240)),
    ("cross_c1_q409600_m102400", ((1, 409600, 102400, 5), 240)),
    ("self_c1_n1228800", ((1, 1228800, 0, 3), 300)),
]


def composed(queries, refs, k, support):
    """one step from knn_cross and torch: weights, moments and the plane in float64, torch.linalg.eigh for the normal.  The stay rules
    are left out: on these clouds no neighbourhood is degenerate"""
    import torch
    from dispu_amd import attributes as A
    idx, d2 = A.knn_cross(queries, refs, k)
    out = []
    for q, r, i, d in zip(queries, refs, idx, d2):
        d = d.double()
        r2 = d / ((support * support) * d[:, -1:])
        rr = r2.sqrt()
        w = torch.where(r2 >= 1.0, torch.zeros_like(r2), (1.0 - rr) ** 4 * (4.0 * rr + 1.0))
        q64 = q.double()
        u = r[i.long()].double() - q64[:, None, :]
        s0 = w.sum(dim=1)
        c = (w[:, :, None] * u).sum(dim=1) / s0[:, None]
        cov = torch.einsum("nk,nki,nkj->nij", w, u, u) / s0[:, None, None] - c[:, :, None] * c[:, None, :]
        nrm = torch.linalg.eigh(cov)[1][:, :, 0]
        t = (c * nrm).sum(dim=1)
        out.append((q64 + t[:, None] * nrm).float())
    return out


def step(c, nq, m, reps):
    import torch
    from dispu_amd import attributes as A
    from dispu_amd import mls as M
    queries = _ellipsoids(c, nq, 11, jitter=0.002)
    refs = _ellipsoids(c, m, 7) if m else queries
    fns = dict(mls_project_1=lambda: M.mls_project(queries, refs, k=K, support=SUPPORT),
               mls_project_3=lambda: M.mls_project(queries, refs, k=K, support=SUPPORT, iterations=3),
               knn_cross=lambda: A.knn_cross(queries, refs, K))
    res = dict(clouds=c, q=nq, m=m or nq, self_projection=not m, reps=reps, k=K, support=SUPPORT, composed="not measured")
    res.update({name + "_ms": t for name, t in _repeat(fns, reps).items()})
    res["one_step_over_knn_cross"] = round(res["mls_project_1_ms"][0] / res["knn_cross_ms"][0], 3)
    print("RESULT " + json.dumps(res), flush=True)
    ours, theirs = M.mls_project(queries, refs, k=K, support=SUPPORT), composed(queries, refs, K, SUPPORT)
    close = [((a - b).abs() <= 1e-5).float().mean().item() for a, b in zip(ours, theirs)]
    res["share_of_coordinates_within_1e-5_of_composed"] = round(min(close), 6)
    assert min(close) >= 0.99, "mls_project and its composed form agree on only %g of the coordinates" % min(close)
    del ours, theirs
    fns["composed_knn_cross_eigh"] = lambda: composed(queries, refs, K, SUPPORT)
    res.update({name + "_ms": t for name, t in _repeat(fns, reps).items()})
    res["composed"] = "measured"
    res["one_step_over_knn_cross"] = round(res["mls_project_1_ms"][0] / res["knn_cross_ms"][0], 3)
    res["one_step_over_composed"] = round(res["mls_project_1_ms"][0] / res["composed_knn_cross_eigh_ms"][0], 3)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON lines")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mls_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/mls_bench.py needs an MI355X"
        step(*steps[a.step][0])
        return 0
    res = dict(metric="mls_projection", unit="ms [median, min, max], device events around the whole call", arith="plain",
               cloud="seeded ellipsoid surface (unit sphere scaled by 1, 0.8, 1.25); queries 0.002 off it", steps={})
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
