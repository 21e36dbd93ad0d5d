#!/usr/bin/env python3
"""Timings of the device-wide Poisson-disk tier (dis-pu_amd/poisson_cells.py; HIP events, eager, 2 warm-up calls then the median of
`--reps`; run it in a fresh process).  Candidates are uniform surface samples of one mesh in sample order (i.i.d., the order
shuffle_seed gives any input), n -> m = n / 3 like the merge of upsample_ragged (12 N -> 4 N):

  one keep (at the radius select ends on) and one select with 12 steps at 1 x 1228800 -> 409600, 1 x 122880 -> 40960 and
  64 x (24576 -> 8192), each beside fps_segments(path="auto") at the same shape; the same pair at 32768 -> 8192 and 49152 -> 12288
  beside the one-workgroup tier; the rounds per evaluation, the surplus, the nearest-neighbour-distance coefficient of variation of the
  FPS set and of the Poisson set of the same candidates; upsample_ragged of one 102400-point cloud with either merge.

Every call of the tier ends with a status read-back, so the event pair spans the whole call.  Writes one JSON object to --out
(profiles/poisson_cells_bench.json) and prints it on one line.  Not part of bench.py; no figure here is a gate."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dispu_amd  # noqa: E402,F401
from dispu_amd import mesh as M, mesh_sample as S, poisson_cells as PC, upsample as U  # noqa: E402
from dispu_amd.outliers import knn_mean_distance  # noqa: E402
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
    return round(float(np.median(ts)), 4)


def _nn_cv(points):
    """std / mean of the distance of every point to its nearest other point (float64 on the device)"""
    d = knn_mean_distance(points, k=1).double()
    return round(float((d.std(unbiased=False) / d.mean()).item()), 4)


def _shape(out, tag, mesh, b, n, m, reps, one_workgroup):
    cands = [S.sample_surface(mesh, n, seed)[0] for seed in range(b)]
    arg = cands[0] if b == 1 else cands
    r_hi = S.hex_radius(mesh.total_area, m)
    idx, r, count, rounds = PC.select(arg, m, r_hi, return_rounds=True)
    first = lambda v: v if b == 1 else v[0]
    r0 = float(first(r).item())
    out[tag + "_select_12_steps"] = _ms(lambda: PC.select(arg, m, r_hi), reps)
    out[tag + "_keep_one_radius"] = _ms(lambda: PC.keep(arg, r0), reps)
    out[tag + "_rounds_per_evaluation"] = rounds
    out[tag + "_keep_rounds"] = PC.keep(arg, r0, return_rounds=True)[2]
    out[tag + "_surplus"] = int(first(count).item()) - m
    out[tag + "_radius_over_r_hi"] = round(r0 / r_hi, 4)
    packed = torch.cat(cands)
    off, moff = U.segment_offsets([n] * b), U.segment_offsets([m] * b)
    out[tag + "_fps_segments_auto"] = _ms(lambda: U.fps_segments(packed, off, moff), reps)
    fps = U.fps_segments(packed, off, moff)
    out[tag + "_nn_cv_poisson"] = _nn_cv(cands[0][first(idx).long()])
    out[tag + "_nn_cv_fps"] = _nn_cv(cands[0][fps[:m].long()])
    if one_workgroup:
        out[tag + "_one_workgroup_select_12_steps"] = _ms(lambda: S.poisson_disk_select(cands[0], m, r_hi), reps)
        out[tag + "_one_workgroup_keep_one_radius"] = _ms(lambda: S.poisson_disk_keep(cands[0], r0), reps)
    print(tag, {k: v for k, v in out.items() if k.startswith(tag)}, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mesh", default="fandisk", choices=("fandisk", "Icosahedron"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_cells_bench.json"))
    ap.add_argument("--skip_large", action="store_true", help="leave out the 1228800-point shape and the 102400-point upsampling")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    dev = torch.device("cuda:0")
    tmp = tempfile.TemporaryDirectory()
    golden = MO.extract_pugan(os.path.join(ROOT, "tests", "golden"), tmp.name)
    mesh = M.Mesh.from_off(os.path.join(golden, a.mesh + ".off"), dev)
    out = {"metric": "poisson_cells", "unit": "ms", "mesh": a.mesh, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    shapes = [("1x32768_to_8192", 1, 32768, 8192, True), ("1x49152_to_12288", 1, 49152, 12288, True),
              ("64x24576_to_8192", 64, 24576, 8192, False), ("1x122880_to_40960", 1, 122880, 40960, False)]
    if not a.skip_large:
        shapes.append(("1x1228800_to_409600", 1, 1228800, 409600, False))
    for tag, b, n, m, one in shapes:
        _shape(out, tag, mesh, b, n, m, a.reps, one)
    if not a.skip_large:
        from dispu_amd.generator import Generator
        from oracle import generator as OG
        gen = Generator(params=OG.init_params(seed=3, bias_scale=0.05, bn_random=True), device=dev)
        cloud = S.sample_surface(mesh, 102400, 1)[0]
        for merge in ("fps", "poisson"):
            tag = "upsample_ragged_102400_merge_" + merge
            out[tag] = _ms(lambda: U.upsample_ragged(gen, [cloud], merge=merge), a.reps)
            outs, st = U.upsample_ragged(gen, [cloud], merge=merge, return_stages=True)
            out[tag + "_nn_cv"] = _nn_cv(torch.from_numpy(outs[0]).to(dev))
            if merge == "poisson":
                out[tag + "_surplus"] = int(st["merge_count"][0].item()) - outs[0].shape[0]
                out[tag + "_radius_over_r_hi"] = round(float(st["merge_r"][0].item()) / st["merge_r_hi"][0], 4)
            print(tag, out[tag], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
