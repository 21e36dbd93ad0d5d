#!/usr/bin/env python3
"""The outlier filters (dis-pu_amd/outliers.py, csrc/outliers.hip) on seeded ellipsoid surfaces, one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times around the WHOLE call (allocations, launches and the one
read-back of the kept counts included) on an otherwise idle stream after one warm-up call, reported as [median, min, max] in ms.

Per shape: dispu_knn_mean_dist_segments at k = 16 beside dispu_pca_normals_segments at k = 17 on preallocated buffers (the mean
distance twice per round, before and after the normals: the first call of a round follows host-heavy torch work), and
knn_mean_distance beside estimate_normals likewise (the same search, the eigen-solve after it instead of 17 square roots: the mean
distance should not be the slower of the two); remove_statistical_outliers (k = 16, std_ratio = 2) beside the same
filter composed from what existed before -- estimate_normals(k + 1, return_neighbors=True), then torch gathers, sqrt, mean, std and
boolean indexing; radius_neighbor_count with exact counts and remove_radius_outliers at min_neighbors = 4, at a radius that gives about
16 neighbours, beside the composed form -- the neighbours at k = 5, the d2 of the fifth against r2.  The kept indices of each pair are
asserted equal before anything is timed.  Writes profiles/outliers_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, STD_RATIO, MIN_NEIGHBORS, ABOUT = 16, 2.0, 4, 16
AXES = (1.0, 0.8, 1.25)

# name -> ((clouds, points per cloud, repeats), time limit in seconds)
STEPS = [
    ("c64_n8192", ((64, 8192, 5), 180)),
    ("c1_n122880", ((1, 122880, 5), 180)),
    ("c1_n409600", ((1, 409600, 3), 240)),
    ("c1_n1228800", ((1, 1228800, 3), 300)),
]


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def _ellipsoids(c, n, seed):
    """c clouds of n points each on an ellipsoid surface (tools/normals_bench.py's), a list of [n, 3] tensors on the device"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((c, n, 3), generator=g)
    x = (x / x.norm(dim=2, keepdim=True) * torch.tensor(AXES)).to(torch.float32).cuda()
    return [x[i].contiguous() for i in range(c)]


def radius_for(n, about=ABOUT):
    """the radius of a disk that holds `about` of n points spread over the ellipsoid's surface (Knud Thomsen's area formula)"""
    a, b, c = AXES
    p = 1.6075
    area = 4.0 * math.pi * (((a * b) ** p + (a * c) ** p + (b * c) ** p) / 3.0) ** (1.0 / p)
    return math.sqrt(about * area / (math.pi * n))


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


def _d2(p, q):
    """fp32 d2 in the kernels' order, one rounding per operation (every torch operation is a kernel of its own: nothing is fused)"""
    d = q - p
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def composed_statistical(clouds, k, ratio):
    """the statistical filter from estimate_normals' neighbours and torch -> kept indices per cloud"""
    import torch
    from dispu_amd.normals import estimate_normals
    _, idx = estimate_normals(clouds, k=k + 1, return_neighbors=True)
    keep = []
    for p, i in zip(clouds, idx):
        d2 = _d2(p[:, None, :], p[i.long()])                                    # [n, k + 1], the point's own 0 included
        md = (d2.double().sqrt().sum(dim=1) / k).float().double()
        thr = md.mean() + ratio * md.std()
        keep.append(torch.nonzero(md <= thr).flatten())
    return keep


def composed_radius(clouds, radius, min_neighbors):
    """the radius filter at cap = min_neighbors from estimate_normals' neighbours: the (min_neighbors + 1)-th key lies within r2"""
    import numpy as np
    import torch
    from dispu_amd.normals import estimate_normals
    r = np.float32(radius)
    r2 = float(np.float32(r * r))
    _, idx = estimate_normals(clouds, k=max(min_neighbors + 1, 4), return_neighbors=True)
    keep = []
    for p, i in zip(clouds, idx):
        d2 = _d2(p, p[i[:, min_neighbors].long()])
        keep.append(torch.nonzero(d2 <= r2).flatten())
    return keep


def abi_calls(clouds, k):
    """the two C entries on the packed batch with every buffer allocated once: dispu_knn_mean_dist_segments at k and
    dispu_pca_normals_segments at k + 1 -- the same search with a different tail, nothing of the host path in the time"""
    import torch
    from dispu_amd import _lib
    from dispu_amd.segments import host_ptr, offsets
    L, p = _lib.lib(), _lib.ptr
    x = torch.cat(clouds).contiguous()
    dev, c, total = x.device, len(clouds), x.shape[0]
    off = offsets([t.shape[0] for t in clouds])
    hp = host_ptr(off)
    d_off = torch.from_numpy(off).to(dev)
    nb = max(L.dispu_knn_mean_dist_scratch_bytes(c, hp, k), L.dispu_pca_normals_scratch_bytes(c, hp, k + 1))
    assert nb > 0
    scratch = torch.empty((nb,), dtype=torch.uint8, device=dev)
    md = torch.empty((total,), dtype=torch.float32, device=dev)
    normal = torch.empty((total, 3), dtype=torch.float32, device=dev)
    status = torch.zeros((c,), dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    keep = (off, x, d_off, scratch, md, normal, status)

    def mean_dist(_keep=keep):
        _lib.check(L.dispu_knn_mean_dist_segments(c, p(d_off), hp, k, p(x), p(md), p(status), p(scratch), nb, st), "dispu_knn_mean_dist_segments")

    def normals(_keep=keep):
        _lib.check(L.dispu_pca_normals_segments(c, p(d_off), hp, k + 1, p(x), 0, p(None), p(normal), p(None), p(None), p(status), p(scratch),
                                                nb, st), "dispu_pca_normals_segments")
    return mean_dist, normals


def step(c, n, reps):
    import torch
    from dispu_amd import outliers as M
    from dispu_amd.normals import estimate_normals
    clouds = _ellipsoids(c, n, 7)
    radius = radius_for(n)
    _, s_idx = M.remove_statistical_outliers(clouds, k=K, std_ratio=STD_RATIO, return_index=True)
    _, r_idx = M.remove_radius_outliers(clouds, radius, min_neighbors=MIN_NEIGHBORS, return_index=True)
    for ours, theirs, what in ((s_idx, composed_statistical(clouds, K, STD_RATIO), "statistical"),
                               (r_idx, composed_radius(clouds, radius, MIN_NEIGHBORS), "radius")):
        for a, b in zip(ours, theirs):
            assert torch.equal(a, b), "the %s filter and its composed form keep different points" % what
    counts = torch.cat(M.radius_neighbor_count(clouds, radius))
    abi_mean_dist, abi_normals = abi_calls(clouds, K)
    ts = _repeat(dict(
        abi_mean_dist_k16=abi_mean_dist,
        abi_pca_normals_k17=abi_normals,
        abi_mean_dist_k16_after_normals=abi_mean_dist,
        knn_mean_distance=lambda: M.knn_mean_distance(clouds, k=K),
        estimate_normals_k17=lambda: estimate_normals(clouds, k=K + 1),
        remove_statistical=lambda: M.remove_statistical_outliers(clouds, k=K, std_ratio=STD_RATIO),
        composed_statistical=lambda: composed_statistical(clouds, K, STD_RATIO),
        radius_count_exact=lambda: M.radius_neighbor_count(clouds, radius),
        remove_radius=lambda: M.remove_radius_outliers(clouds, radius, min_neighbors=MIN_NEIGHBORS),
        composed_radius=lambda: composed_radius(clouds, radius, MIN_NEIGHBORS)), reps)
    total = c * n
    res = dict(clouds=c, n=n, reps=reps, k=K, std_ratio=STD_RATIO, radius=round(radius, 6), min_neighbors=MIN_NEIGHBORS,
               mean_neighbors_within_radius=round(float(counts.double().mean()), 2), equal_kept_indices=True,
               removed_statistical=total - sum(int(i.shape[0]) for i in s_idx), removed_radius=total - sum(int(i.shape[0]) for i in r_idx))
    res.update({name + "_ms": t for name, t in ts.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outliers_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/outliers_bench.py needs an MI355X"
        args, _ = steps[a.step]
        print("RESULT " + json.dumps(step(*args)))
        return 0
    res = dict(metric="outlier_filters", unit="ms [median, min, max], device events around the whole call", arith="plain",
               cloud="seeded ellipsoid surface (unit sphere scaled by 1, 0.8, 1.25)", steps={})
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
