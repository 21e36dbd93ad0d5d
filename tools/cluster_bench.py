#!/usr/bin/env python3
"""Density clustering (dis-pu_amd/clusters.py, csrc/cluster.hip) on a seeded sphere surface with planted blobs, one fresh process per
shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times around the WHOLE call (allocations, launches and the one
read-back included) on an otherwise idle stream after one warm-up call, reported as [median, min, max] in ms; the functions of one
shape alternate inside every round.

Per shape and per (eps, min_points), eps = 2 x and 4 x the mean spacing sqrt(area / n), min_points = 1 and 10: dbscan and
keep_clusters(keep = 1), and next to them radius_neighbor_count with exact counts at the same radius -- ONE search pass over the same
cells, the floor of anything that has to look at every pair within eps -- and the ratio of the medians.  Also the number of link
launches that did work (read from the head of the scratch, include/dispu_hip.h), the clusters and noise points found, and how many
points keep_clusters(keep = 1) drops (the planted blobs are BLOBS * BLOB_POINTS of them; stray points of a sparse sphere the rest).
The last step is the candidate for a pathological link pass, scanner lines at a large eps: 64 parallel straight lines of 6400 points,
each one chain-shaped cluster, at eps = 8 x and 32 x the spacing along the line.

--trace STEP runs a few dbscan calls of one shape at eps = 4 x, min_points = 10 and nothing else: the command to put behind
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o prof --`;  --shares CSV reduces that run's kernel statistics to the
share of device time per kernel and stores it in the JSON.  Writes profiles/cluster_bench.json (or --out) and prints it as one line."""
import argparse
import csv
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOBS, BLOB_POINTS, BLOB_SIGMA, BLOB_RADIUS = 3, 500, 0.01, 1.6
EPS_FACTORS, MIN_POINTS = (2.0, 4.0), (1, 10)

LINES, LINE_GAP, LINE_EPS_FACTORS = 64, 40.0, (8.0, 32.0)         # the scanner-line cloud: lines, their distance in spacings, eps in spacings

# name -> ((cloud kind, clouds, points per cloud, repeats), time limit in seconds)
STEPS = [
    ("c64_n8192", (("sphere", 64, 8192, 5), 240)),
    ("c1_n102400", (("sphere", 1, 102400, 5), 240)),
    ("c1_n409600", (("sphere", 1, 409600, 3), 300)),
    ("c1_n1228800", (("sphere", 1, 1228800, 3), 420)),
    ("lines_n409600", (("lines", 1, 409600, 3), 300)),           # the candidate for a pathological link pass: long chains, large eps
]


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def spacing(n):
    """mean spacing of n points on the unit sphere: the side of a square of area 4 pi / n"""
    return math.sqrt(4.0 * math.pi / n)


def sphere_with_blobs(c, n, seed):
    """c clouds of n points: n - BLOBS * BLOB_POINTS on the unit sphere, then BLOBS Gaussian blobs of BLOB_POINTS points (sigma
    BLOB_SIGMA) at radius BLOB_RADIUS, far from the sphere and from each other; a list of [n, 3] tensors on the device, shuffled"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = n - BLOBS * BLOB_POINTS
    x = torch.randn((c, m, 3), generator=g)
    x = x / x.norm(dim=2, keepdim=True)
    centres = torch.tensor([[BLOB_RADIUS, 0.0, 0.0], [0.0, -BLOB_RADIUS, 0.0], [0.0, 0.0, BLOB_RADIUS]])[:BLOBS]
    b = centres[None, :, None, :] + BLOB_SIGMA * torch.randn((c, BLOBS, BLOB_POINTS, 3), generator=g)
    x = torch.cat([x, b.reshape(c, -1, 3)], dim=1).to(torch.float32)
    out = []
    for i in range(c):
        out.append(x[i][torch.randperm(n, generator=g)].contiguous().cuda())
    return out


def scanner_lines(c, n, seed):
    """c clouds of n points on LINES parallel straight lines at unit spacing along the line (jittered by 5 %), LINE_GAP spacings apart:
    every line is ONE chain-shaped cluster of n / LINES points as long as eps < LINE_GAP; shuffled"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    per = n // LINES
    t = torch.arange(per, dtype=torch.float64)[None, :, None] + 0.05 * torch.randn((LINES, per, 1), generator=g, dtype=torch.float64)
    y = LINE_GAP * torch.arange(LINES, dtype=torch.float64)[:, None, None].expand(LINES, per, 1)
    x = torch.cat([t, y, torch.zeros_like(t)], dim=2).reshape(-1, 3)
    x = (x / per).to(torch.float32)                              # a line has length 1
    return [x[torch.randperm(x.shape[0], generator=g)].contiguous().cuda() for _ in range(c)]


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


def launches_that_worked(clouds, eps, min_points):
    """(link launches, flatten launches) of one dbscan that did work, clusters of the batch: from the head of the scratch"""
    import torch
    from dispu_amd import clusters as M
    from dispu_amd.segments import Packed
    b = Packed(clouds, "cluster_bench", words=3)
    b.pack()
    scratch = M._cluster(b, float(eps), int(min_points))[4]
    head = scratch[:64].view(torch.int32).cpu().tolist()
    assert int(b.status.max()) == 0

    def worked(flags):                                           # launch 1 always works, launch j + 1 iff launch j ran short of a cap
        k = 1
        for f in flags[:3]:
            if not f:
                break
            k += 1
        return k
    return worked(head[0:4]), worked(head[4:8]), head[8]


def _cloud(kind, c, n):
    """-> (clouds, mean spacing, eps factors, what the result says about the cloud)"""
    if kind == "lines":
        return scanner_lines(c, n, 7), 1.0 / (n // LINES), LINE_EPS_FACTORS, dict(lines=LINES, line_gap_in_spacings=LINE_GAP)
    return sphere_with_blobs(c, n, 7), spacing(n - BLOBS * BLOB_POINTS), EPS_FACTORS, dict(blobs=BLOBS, blob_points=BLOB_POINTS)


def step(kind, c, n, reps):
    import torch
    from dispu_amd import clusters as M
    from dispu_amd import outliers
    clouds, h, factors, what = _cloud(kind, c, n)
    n = int(clouds[0].shape[0])
    res = dict(cloud=kind, clouds=c, n=n, reps=reps, mean_spacing=round(h, 8), cases={}, **what)
    for f in factors:
        eps = f * h
        counts = torch.cat(outliers.radius_neighbor_count(clouds, eps))
        for mp in MIN_POINTS:
            kept, labels = M.keep_clusters(clouds, eps, min_points=mp, keep=1, return_labels=True)
            dropped = [n - int(k.shape[0]) for k in kept]
            link, jump, nclusters = launches_that_worked(clouds, eps, mp)
            ts = _repeat(dict(radius_count_exact=lambda: outliers.radius_neighbor_count(clouds, eps),
                              dbscan=lambda: M.dbscan(clouds, eps, mp),
                              keep_clusters=lambda: M.keep_clusters(clouds, eps, min_points=mp, keep=1)), reps)
            case = dict(eps=round(eps, 8), eps_in_spacings=f, min_points=mp, mean_neighbors_within_eps=round(float(counts.double().mean()), 2),
                        clusters_in_batch=nclusters, noise_points=int(sum(int((l < 0).sum()) for l in labels)),
                        dropped_by_keep_1=[min(dropped), max(dropped)], link_launches_that_worked=link, flatten_launches_that_worked=jump)
            case.update({name + "_ms": t for name, t in ts.items()})
            for name in ("dbscan", "keep_clusters"):
                case[name + "_over_radius_count"] = round(ts[name][0] / ts["radius_count_exact"][0], 3)
            res["cases"]["eps%gx_mp%d" % (f, mp)] = case
    return res


def trace(kind, c, n, reps):
    """what the profiler run executes: dbscan alone at eps = 4 x, min_points = 10"""
    import torch
    from dispu_amd import clusters as M
    clouds, h, _, _ = _cloud(kind, c, n)
    eps = 4.0 * h
    for _ in range(reps + 1):
        M.dbscan(clouds, eps, 10)
    torch.cuda.synchronize()


def shares(path):
    """rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, ...) -> {kernel: percent of the device time}, largest first"""
    agg = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):                             # the bare function name: no namespaces, template or call arguments
            name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1]
            calls, t = agg.get(name, (0, 0.0))
            agg[name] = (calls + int(r["Calls"]), t + float(r["TotalDurationNs"]))
    rows = [(name, calls, t) for name, (calls, t) in agg.items()]
    total = sum(t for _, _, t in rows)
    rows.sort(key=lambda r: -r[2])
    return dict(total_device_ms=round(total / 1e6, 3),
                kernels={name: dict(calls=calls, percent=round(100.0 * t / total, 2)) for name, calls, t in rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--trace", help="run a few dbscan calls of this step and nothing else (for the profiler)")
    ap.add_argument("--shares", nargs=2, metavar=("STEP", "CSV"), help="store the kernel shares of a profiler run of --trace STEP in the JSON")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step or a.trace:
        import torch
        assert torch.cuda.is_available(), "tools/cluster_bench.py needs an MI355X"
        if a.trace:
            trace(*steps[a.trace][0])
            return 0
        print("RESULT " + json.dumps(step(*steps[a.step][0])))
        return 0
    if a.shares:
        with open(a.out) as fh:
            res = json.load(fh)
        res.setdefault("device_time_share", {})[a.shares[0]] = dict(case="dbscan at eps = 4 x the spacing, min_points = 10", **shares(a.shares[1]))
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return 0
    res = dict(metric="density_clustering", unit="ms [median, min, max], device events around the whole call", arith="plain",
               cloud="seeded unit sphere surface plus %d planted blobs of %d points" % (BLOBS, BLOB_POINTS), steps={})
    rc = 0
    for name, (args, limit) in STEPS:
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
