#!/usr/bin/env python3
"""Bring scans of one object into the frame of a target scan by ICP (dis-pu_amd/registration.py, csrc/icp.hip).

  register.py --target t.xyz --source a.xyz [b.xyz ...] --out_folder D [--method point|plane] [--max_distance d] [--iterations n]
              [--tolerance e] [--init M.txt] [--merge]

Every source goes against the target in ONE batched call.  --method plane estimates the target's normals (k = 16) and minimises the
point-to-plane residual; --init is a 4 x 4 text matrix applied to every source first.  Per source D gets <stem>_aligned.xyz (%.6f) and
<stem>_transform.txt (4 rows of %.17g: source coordinates -> target frame), and one log line is printed; --merge also writes
merged.xyz, the target followed by the aligned sources."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = ("out of iterations", "converged", "degenerate")


def _nonneg(allow_inf):
    def parse(text):
        v = float(text)
        if math.isnan(v) or v < 0 or (math.isinf(v) and not allow_inf):
            raise argparse.ArgumentTypeError("expected a number >= 0, got %r" % text)
        return v
    return parse


def _iterations(text):
    v = int(text)
    if not 0 <= v <= 128:
        raise argparse.ArgumentTypeError("expected an integer in 0 .. 128, got %r" % text)
    return v


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--target", required=True, help="the scan whose frame is kept (.xyz, the first three columns are read)")
    ap.add_argument("--source", required=True, nargs="+", help="the scans to move")
    ap.add_argument("--out_folder", required=True)
    ap.add_argument("--method", choices=("point", "plane"), default="point")
    ap.add_argument("--max_distance", type=_nonneg(True), default=float("inf"), help="leave out source points farther than this from the target")
    ap.add_argument("--iterations", type=_iterations, default=30)
    ap.add_argument("--tolerance", type=_nonneg(False), default=1e-6)
    ap.add_argument("--init", help="a 4 x 4 text matrix: the starting motion of every source")
    ap.add_argument("--merge", action="store_true", help="also write merged.xyz: the target followed by the aligned sources")
    a = ap.parse_args(argv)
    stems = [stem(p) for p in a.source]
    if len(set(stems)) != len(stems):
        ap.error("two sources share the file stem %r: their outputs would overwrite each other" % sorted(s for s in stems if stems.count(s) > 1)[0])
    return a


def stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def load_xyz(path):
    rows = np.loadtxt(path, ndmin=2, dtype=np.float64)
    if rows.shape[1] < 3 or rows.shape[0] < 1:
        raise SystemExit("%s: expected rows of at least three numbers" % path)
    return np.ascontiguousarray(rows[:, :3], np.float32)


def load_init(path):
    m = np.loadtxt(path, ndmin=2, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise SystemExit("%s: expected a finite 4 x 4 matrix" % path)
    return m


def main(argv=None):
    a = parse_args(argv)
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd.normals import estimate_normals
    from dispu_amd.registration import icp
    assert torch.cuda.is_available(), "tools/register.py needs a ROCm device"
    dev = torch.device("cuda")
    target = torch.from_numpy(load_xyz(a.target)).to(dev)
    sources = [torch.from_numpy(load_xyz(p)).to(dev) for p in a.source]
    C = len(sources)
    normals = [estimate_normals(target, k=16)] * C if a.method == "plane" else None
    init = None if a.init is None else [torch.from_numpy(load_init(a.init)).to(dev)] * C
    r = icp(sources, [target] * C, normals, init=init, max_distance=a.max_distance, iterations=a.iterations, tolerance=a.tolerance)
    os.makedirs(a.out_folder, exist_ok=True)
    T = r.transform.cpu().numpy()
    fitness, rmse, iters = r.fitness.cpu().numpy(), r.rmse.cpu().numpy(), r.iterations.cpu().numpy()
    flag = (r.converged.to(torch.int32) + 2 * r.degenerate.to(torch.int32)).cpu().numpy()
    aligned = [x.cpu().numpy() for x in r.aligned]
    for c, path in enumerate(a.source):
        s = stem(path)
        np.savetxt(os.path.join(a.out_folder, s + "_aligned.xyz"), aligned[c], fmt="%.6f")
        np.savetxt(os.path.join(a.out_folder, s + "_transform.txt"), T[c], fmt="%.17g")
        print("%s: fitness %.6f rmse %.6g iterations %d %s" % (s, fitness[c], rmse[c], iters[c], FLAGS[flag[c]]), flush=True)
    if a.merge:
        np.savetxt(os.path.join(a.out_folder, "merged.xyz"), np.concatenate([target.cpu().numpy()] + aligned), fmt="%.6f")
    return 0


if __name__ == "__main__":
    sys.exit(main())
