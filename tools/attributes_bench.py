#!/usr/bin/env python3
"""The attribute transfer (dis-pu_amd/attributes.py, csrc/attributes.hip) on seeded ellipsoid surfaces, one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times around the WHOLE call (allocations, launches and the status
read-back included) on an otherwise idle stream after one warm-up call, the two sides alternating, reported as [median, min, max] in ms.

Per shape (q queries, m references, three feature columns, k = 3, inverse-distance weights): transfer_attributes beside the same result
composed from what existed before -- the brute-force three_nn (every query against every reference point) per cloud, then torch gathers
and the weights in float64.  The two are asserted equal to 1e-6 relative before anything is timed (the composed form adds in torch's
order, so not bit for bit).  Also dispu_knn_cross_segments alone on preallocated buffers (the search without the host path).
Writes profiles/attributes_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, F = 3, 3
AXES = (1.0, 0.8, 1.25)

# name -> ((clouds, queries per cloud, references per cloud, repeats), time limit in seconds)
STEPS = [
    ("c1_q8192_m2048", ((1, 8192, 2048, 7), 120)),
    ("c1_q409600_m102400", ((1, 409600, 102400, 5), 180)),
    ("c1_q1228800_m102400", ((1, 1228800, 102400, 3), 240)),
    ("c64_q8192_m2048", ((64, 8192, 2048, 5), 180)),
]


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def _ellipsoids(c, n, seed, jitter=0.0):
    """c clouds of n points each on an ellipsoid surface (tools/normals_bench.py's), a list of [n, 3] tensors on the device; jitter: the
    standard deviation of an offset from the surface (upsampled points do not lie on their input)"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((c, n, 3), generator=g)
    x = x / x.norm(dim=2, keepdim=True) * torch.tensor(AXES)
    if jitter:
        x = x + jitter * torch.randn((c, n, 3), generator=g)
    x = x.to(torch.float32).cuda()
    return [x[i].contiguous() for i in range(c)]


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


def composed(queries, refs, feats):
    """the transfer at k = 3 from three_nn (brute force, one call per cloud) and torch: weights 1 / max(d2, 1e-10) in float64"""
    from dispu_amd.tf_interpolate import three_nn
    out = []
    for q, r, f in zip(queries, refs, feats):
        d2, idx = three_nn(q.reshape(1, -1, 3), r.reshape(1, -1, 3))
        w = 1.0 / d2[0].double().clamp_min(1e-10)
        rows = f[idx[0].long()].double()                                        # [q, 3, F]
        out.append(((w[:, :, None] * rows).sum(dim=1) / w.sum(dim=1, keepdim=True)).float())
    return out


def abi_knn(queries, refs, k):
    """dispu_knn_cross_segments on the packed batch with every buffer allocated once: nothing of the host path in the time"""
    import torch
    from dispu_amd import _lib
    from dispu_amd.segments import host_ptr, offsets
    L, p = _lib.lib(), _lib.ptr
    q, r = torch.cat(queries).contiguous(), torch.cat(refs).contiguous()
    dev, c = q.device, len(queries)
    qoff, roff = offsets([t.shape[0] for t in queries]), offsets([t.shape[0] for t in refs])
    hq, hr = host_ptr(qoff), host_ptr(roff)
    d_qoff, d_roff = torch.from_numpy(qoff).to(dev), torch.from_numpy(roff).to(dev)
    nb = L.dispu_knn_cross_scratch_bytes(c, hq, hr)
    assert nb > 0
    scratch = torch.empty((nb,), dtype=torch.uint8, device=dev)
    idx = torch.empty((q.shape[0], k), dtype=torch.int32, device=dev)
    d2 = torch.empty((q.shape[0], k), dtype=torch.float32, device=dev)
    status = torch.zeros((c,), dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    keep = (qoff, roff, q, r, d_qoff, d_roff, scratch, idx, d2, status)

    def knn(_keep=keep):
        _lib.check(L.dispu_knn_cross_segments(c, p(d_qoff), hq, p(d_roff), hr, k, p(q), p(r), p(idx), p(d2), p(status), p(scratch), nb, st),
                   "dispu_knn_cross_segments")
    return knn


def step(c, nq, m, reps):
    import torch
    from dispu_amd import attributes as M
    refs = _ellipsoids(c, m, 7)
    queries = _ellipsoids(c, nq, 11, jitter=0.002)
    g = torch.Generator(device="cpu").manual_seed(3)
    feats = [t.contiguous() for t in torch.rand((c, m, F), generator=g).cuda()]
    ours, theirs = M.transfer_attributes(queries, refs, features=feats, k=K), composed(queries, refs, feats)
    worst = max(float(((a - b).abs() / b.abs().clamp_min(1e-3)).max()) for a, b in zip(ours, theirs))
    assert worst <= 1e-6, "transfer_attributes and its composed form differ by %g relative" % worst
    ts = _repeat(dict(
        transfer_attributes=lambda: M.transfer_attributes(queries, refs, features=feats, k=K),
        composed_three_nn=lambda: composed(queries, refs, feats),
        abi_knn_cross=abi_knn(queries, refs, K)), reps)
    res = dict(clouds=c, q=nq, m=m, reps=reps, k=K, F=F, mode="idw", worst_relative_difference=worst)
    res.update({name + "_ms": t for name, t in ts.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attributes_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/attributes_bench.py needs an MI355X"
        args, _ = steps[a.step]
        print("RESULT " + json.dumps(step(*args)))
        return 0
    res = dict(metric="attribute_transfer", unit="ms [median, min, max], device events around the whole call", arith="plain",
               cloud="seeded ellipsoid surface (unit sphere scaled by 1, 0.8, 1.25); queries 0.002 off it", steps={})
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
