#!/usr/bin/env python3
"""Consistent orientation (dispu_orient_consistent_segments, csrc/orient_consistent.hip) on the seeded ellipsoid surfaces of
tools/normals_bench.py, one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  The input is what the feature meets in use: the PCA normals of
dispu_pca_normals_segments with the canonical sign (orient_mode 0) and its neighbour lists, vote 0.  Times are device-event times of the
whole call on an otherwise idle stream after one warm-up call, [median, min, max] in ms over the repeats, for the two ways to end the
rounds: the device-side counter (the default; every launch of the ceil(log2 n) rounds is issued, the ones after the last live round
return at once) and one 4-byte read-back per round (DISPU_ORIENT_HOST_ROUNDS; the host waits once per round and stops issuing).  For
the read-back form the host's own wall time is given too, since the stream idles while the host waits.  The per-phase times and the
rounds come from one more call with profile_host (events around every phase, a wait after each: their sum leaves out the gaps).
dispu_pca_normals_segments with idx_out, alone, stands next to each row for scale: it is the call that makes this one's input.
There is no earlier GPU implementation to compare with and no threshold.  Writes profiles/orient_bench.json (or --out) and prints it
as one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> ((clouds, points per cloud, k, repeats), time limit in seconds)
STEPS = [
    ("c64_n8192_k16", ((64, 8192, 16, 5), 120)),
    ("c1_n409600_k16", ((1, 409600, 16, 5), 180)),
    ("c1_n1228800_k16", ((1, 1228800, 16, 3), 240)),
]
AXES = (1.0, 0.8, 1.25)
# what the library does by default, recorded beside the numbers that decided it ("Consistent orientation")
CHOICES = dict(
    termination="device-side counter (flags = 0): every launch of the ceil(log2 n_max) rounds is issued and returns at once after the "
                "last live round, the entry stays asynchronous; orient_host_readback_ms is the alternative behind DISPU_ORIENT_HOST_ROUNDS",
    contention="wave-level min / max / count when a wave's lanes share one address, else a load that skips an offer which cannot change "
               "the value; propose as a row pass (one offer per row to its own root) before the per-slot pass to the other root, dead "
               "rows skipped",
    replaced="one per-slot launch offering to both roots: 6.02 / 2.26 / 8.09 ms on c64_n8192 / c1_n409600 / c1_n1228800 (propose 5.50 / "
             "1.67 / 6.65 ms)")


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def _ellipsoids(c, n, seed):
    """c clouds of n points each on an ellipsoid surface, as tools/normals_bench.py makes them, packed [c * n, 3]"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((c, n, 3), generator=g)
    x = x / x.norm(dim=2, keepdim=True) * torch.tensor(AXES)
    return x.to(torch.float32).reshape(-1, 3).contiguous().cuda()


def _timed(fn):
    """-> (device-event ms, host wall ms) of one call, the stream drained before and after"""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def step(c, n, k, reps):
    import numpy as np
    import torch
    from dispu_amd import _lib
    from dispu_amd.segments import host_ptr, offsets
    L, p = _lib.lib(), _lib.ptr
    x = _ellipsoids(c, n, 7)
    dev, total = x.device, c * n
    st = _lib.stream_ptr(dev)
    off = offsets([n] * c)
    hp = host_ptr(off)
    d_off = torch.from_numpy(off).to(dev)
    nb, ob = L.dispu_pca_normals_scratch_bytes(c, hp, k), L.dispu_orient_consistent_scratch_bytes(c, hp, k)
    assert nb > 0 and ob > 0
    scratch = torch.empty((max(nb, ob),), dtype=torch.uint8, device=dev)
    normal = torch.empty((total, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((total, k), dtype=torch.int32, device=dev)
    status = torch.zeros((c,), dtype=torch.int32, device=dev)
    out = torch.empty((total, 3), dtype=torch.float32, device=dev)
    flip = torch.empty((total,), dtype=torch.uint8, device=dev)
    ncomp = torch.empty((c,), dtype=torch.int32, device=dev)
    prof = np.zeros(_lib.ORIENT_PROFILE_FLOATS, np.float32)

    def normals():
        _lib.check(L.dispu_pca_normals_segments(c, p(d_off), hp, k, p(x), 0, p(None), p(normal), p(None), p(idx), p(status), p(scratch), nb,
                                                st), "dispu_pca_normals_segments")

    def orient(flags=0, profile=None):
        _lib.check(L.dispu_orient_consistent_segments(c, p(d_off), hp, k, p(x), p(normal), p(idx), 0, flags, p(out), p(flip), p(None),
                                                      p(ncomp), p(status), p(scratch), ob,
                                                      _lib.C.c_void_p(profile.ctypes.data) if profile is not None else None, st),
                   "dispu_orient_consistent_segments")

    normals()
    torch.cuda.synchronize()
    t_nrm = [_timed(normals)[0] for _ in range(reps)]
    fns = dict(device_counter=lambda: orient(0), host_readback=lambda: orient(_lib.ORIENT_HOST_ROUNDS))
    flips = {}
    for name, fn in fns.items():                                # warm-up, and the two forms must agree
        fn()
        torch.cuda.synchronize()
        assert not bool(status.any())
        flips[name] = flip.clone()
    assert torch.equal(flips["device_counter"], flips["host_readback"])
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(_timed(fn))
    orient(0, prof)
    torch.cuda.synchronize()
    assert torch.equal(flip, flips["device_counter"])
    grad = x / (torch.tensor(AXES, device=dev) ** 2)            # the ellipsoid's outward direction
    outward = float(((out * grad).sum(dim=1) > 0).float().mean())
    dc = _stats([t[0] for t in ts["device_counter"]])
    return dict(clouds=c, n=n, k=k, reps=reps, pca_normals_with_idx_out_ms=_stats(t_nrm),
                orient_device_counter_ms=dc, orient_device_counter_host_wall_ms=_stats([t[1] for t in ts["device_counter"]]),
                orient_host_readback_ms=_stats([t[0] for t in ts["host_readback"]]),
                orient_host_readback_host_wall_ms=_stats([t[1] for t in ts["host_readback"]]),
                rounds_that_hooked=int(prof[0]), rounds_issued=int(prof[6]),
                phase_ms=dict(setup=round(float(prof[1]), 4), propose=round(float(prof[2]), 4), hook=round(float(prof[3]), 4),
                              compress=round(float(prof[4]), 4), finish=round(float(prof[5]), 4)),
                ns_per_point=round(dc[0] * 1e6 / total, 2), components=int(ncomp.sum()), outward_fraction=round(outward, 6),
                flipped_fraction=round(float(flip.float().mean()), 6), scratch_MB=round(ob / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/orient_bench.py needs an MI355X"
        print("RESULT " + json.dumps(step(*steps[a.step][0])))
        return 0
    res = dict(metric="orient_consistent", unit="ms [median, min, max]", vote="anchor",
               cloud="seeded ellipsoid surface (unit sphere scaled by 1, 0.8, 1.25)", input="PCA normals, orient_mode 0, with their lists",
               choices=CHOICES, steps={})
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
