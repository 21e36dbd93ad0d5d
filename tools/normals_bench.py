#!/usr/bin/env python3
"""Oriented normals (dispu_pca_normals_segments, csrc/normals.hip) on seeded ellipsoid surfaces, one fresh process per shape.

Every shape is a step of its own: a child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the
run (nothing more is started on the device).  Times are device-event times of the whole call on an otherwise idle stream after one
warm-up call, reported as [median, min, max] in ms over the repeats.  The search and the eigen-solve are ONE kernel, so kernel
boundaries give only two parts: the pre-pass (bounds, keys, sort, cells -- timed through dispu_fps_cells at m = 1, the same host step;
above 262144 points that entry cuts larger cells, the sort and the two passes before it are the same) and the rest (whole call minus
pre-pass: search + eigen-solve + stores).  The baseline steps run the existing dispu_knn_patch_segments as a self-search at k = 16,
alone, which is the floor of any alternative composed from existing kernels; the neighbour indices of the two must be equal.
Writes profiles/normals_bench.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (kind, (clouds, points per cloud, k, repeats), time limit in seconds)
STEPS = [
    ("c64_n8192_k16", ("normals", (64, 8192, 16, 5), 120)),
    ("c1_n8192_k16", ("normals", (1, 8192, 16, 5), 120)),
    ("c1_n122880_k16", ("normals", (1, 122880, 16, 5), 120)),
    ("c1_n409600_k16", ("normals", (1, 409600, 16, 3), 180)),
    ("c1_n1228800_k16", ("normals", (1, 1228800, 16, 3), 240)),
    ("c1_n409600_k32", ("normals", (1, 409600, 32, 3), 180)),
    ("baseline_c1_n8192_k16", ("baseline", (1, 8192, 16, 5), 120)),
    ("baseline_c1_n122880_k16", ("baseline", (1, 122880, 16, 3), 240)),
]


def _stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def _ellipsoids(c, n, seed):
    """c clouds of n points each on an ellipsoid surface, as dis-pu_amd/synth.py makes them, packed [c * n, 3]"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((c, n, 3), generator=g)
    x = x / x.norm(dim=2, keepdim=True) * torch.tensor([1.0, 0.8, 1.25])
    return x.to(torch.float32).reshape(-1, 3).contiguous().cuda()


def _timed_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


class _Calls(object):
    """the calls on one packed batch, buffers allocated once"""

    def __init__(self, c, n, k):
        import numpy as np
        import torch
        from dispu_amd import _lib
        from dispu_amd.segments import host_ptr, offsets
        self.L, self._lib, self.c, self.n, self.k = _lib.lib(), _lib, c, n, k
        self.x = _ellipsoids(c, n, 7)
        dev = self.x.device
        self.st = _lib.stream_ptr(dev)
        self.off = offsets([n] * c)
        self.moff = np.arange(c + 1, dtype=np.int32)
        self.d_off, self.d_moff = torch.from_numpy(self.off).to(dev), torch.from_numpy(self.moff).to(dev)
        self.hp = host_ptr
        self.nb = self.L.dispu_pca_normals_scratch_bytes(c, self.hp(self.off), k)
        self.cb = self.L.dispu_fps_cells_scratch_bytes(c, self.hp(self.off), self.hp(self.moff), 0)
        assert self.nb > 0 and self.cb > 0
        self.scratch = torch.empty((max(self.nb, self.cb),), dtype=torch.uint8, device=dev)
        self.normal = torch.empty((c * n, 3), dtype=torch.float32, device=dev)
        self.idx = torch.empty((c * n, k), dtype=torch.int32, device=dev)
        self.status = torch.zeros((c,), dtype=torch.int32, device=dev)
        self.fps_out = torch.empty((c,), dtype=torch.int32, device=dev)

    def normals(self, with_idx=False):
        p = self._lib.ptr
        self._lib.check(self.L.dispu_pca_normals_segments(self.c, p(self.d_off), self.hp(self.off), self.k, p(self.x), 0, p(None),
                                                          p(self.normal), p(None), p(self.idx if with_idx else None), p(self.status),
                                                          p(self.scratch), self.nb, self.st), "dispu_pca_normals_segments")

    def prepass(self):
        p = self._lib.ptr
        self._lib.check(self.L.dispu_fps_cells(self.c, p(self.d_off), p(self.d_moff), self.hp(self.off), self.hp(self.moff), p(self.x),
                                               p(self.scratch), self.cb, p(self.fps_out), p(self.status), 1, 0, self.st), "dispu_fps_cells")

    def baseline(self):
        p = self._lib.ptr
        self._lib.check(self.L.dispu_knn_patch_segments(self.c, p(self.d_off), p(self.d_off), self.hp(self.off), self.hp(self.off), self.k,
                                                        p(self.x), p(self.x), p(self.idx), self.st), "dispu_knn_patch_segments")


def _repeat(fns, reps):
    """one warm-up call each, then `reps` rounds in which the functions alternate -> {name: [ms, ...]}"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(_timed_ms(fn))
    return ts


def step_normals(c, n, k, reps):
    import torch
    q = _Calls(c, n, k)
    ts = _repeat(dict(call=q.normals, call_idx=lambda: q.normals(True), prepass=q.prepass), reps)
    torch.cuda.synchronize()
    assert not bool(q.status.any())
    length = q.normal.norm(dim=1)
    assert bool(((length - 1).abs() < 1e-5).all()), "a normal is not a unit vector"
    call, pre = _stats(ts["call"]), _stats(ts["prepass"])
    return dict(clouds=c, n=n, k=k, reps=reps, call_ms=call, call_with_idx_out_ms=_stats(ts["call_idx"]), prepass_ms=pre,
                search_and_eigen_ms=round(call[0] - pre[0], 4), ns_per_point=round(call[0] * 1e6 / (c * n), 2),
                scratch_MB=round(q.nb / 2 ** 20, 1))


def step_baseline(c, n, k, reps):
    import torch
    q = _Calls(c, n, k)
    q.normals(True)
    got = q.idx.clone()
    ts = _repeat(dict(knn=q.baseline), reps)
    torch.cuda.synchronize()
    assert torch.equal(got, q.idx), "dispu_pca_normals_segments' neighbours differ from dispu_knn_patch_segments'"
    t = _stats(ts["knn"])
    return dict(clouds=c, n=n, k=k, reps=reps, equal_indices=True, knn_patch_segments_self_search_ms=t,
                us_per_1e6_distances=round(t[0] * 1e3 / (c * n * n / 1e6), 4))


KINDS = dict(normals=step_normals, baseline=step_baseline)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="run this one step in this process and print its JSON line")
    ap.add_argument("--only", nargs="*", help="steps to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    a = ap.parse_args()
    steps = dict(STEPS)
    if a.step:
        import torch
        assert torch.cuda.is_available(), "tools/normals_bench.py needs an MI355X"
        kind, args, _ = steps[a.step]
        print("RESULT " + json.dumps(KINDS[kind](*args)))
        return 0
    res = dict(metric="pca_normals", unit="ms [median, min, max]", arith="plain",
               cloud="seeded ellipsoid surface (unit sphere scaled by 1, 0.8, 1.25)", steps={})
    rc = 0
    for name, (kind, args, limit) in STEPS:
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
