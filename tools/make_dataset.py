#!/usr/bin/env python3
"""Make the data the other commands read, from triangle meshes (`*.off`) alone (dis-pu_amd/mesh_sample.py):

  make_dataset.py patches --mesh_dir DIR --out data/PUGAN_poisson_256_poisson_1024.h5
      the training file of tools/train.py: per mesh --patches_per_mesh Poisson-disk patches of --gt_num points and, over the same regions,
      of --in_num points, as the datasets `poisson_<gt_num>` / `poisson_<in_num>` [patches, points, 3] float32, un-normalised like the
      published file.  The mesh name of every patch goes, one per line, into <out minus .h5>_names.txt.
  make_dataset.py clouds --mesh_dir DIR --out_dir DIR --num 2048
      per mesh a Poisson-disk cloud of --num points as <stem>.xyz (the text format of tools/upsample.py's outputs): --num 2048 makes the
      inputs of tools/upsample.py, --num 8192 the ground truth of tools/evaluate.py.  --oversample x --num is at most 49152 candidates
      (the one-workgroup selection); --cells lifts that to 2^24: larger clouds go through dis-pu_amd/poisson_cells.py.

The reference's counterparts were made upstream with tools that are in neither tree, so the files are not the published ones: they
are reproducible from (meshes, --seed) and close the loop meshes -> train -> upsample -> evaluate with nothing downloaded.
Arguments are checked before the device is touched."""
import argparse
import os
import sys
from glob import glob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_PATCH_MAX_K = 4096        # dis-pu_amd/mesh_sample.py: candidates per patch (dispu_knn_patch, dispu_sort_rows_i32)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Poisson-disk training patches and test clouds from .off meshes.")
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("patches", help="the HDF5 training file of tools/train.py")
    p.add_argument("--mesh_dir", required=True, help="every *.off in it is used, in name order")
    p.add_argument("--out", default=os.path.join("data", "PUGAN_poisson_256_poisson_1024.h5"))
    p.add_argument("--patches_per_mesh", type=int, default=200)
    p.add_argument("--gt_num", type=int, default=1024)
    p.add_argument("--in_num", type=int, default=256)
    p.add_argument("--oversample", type=int, default=4, help="candidates per kept point")
    p.add_argument("--patch_fraction", type=float, default=0.05, help="share of the surface one patch region covers")
    p.add_argument("--seed", type=int, default=0)
    c = sub.add_parser("clouds", help="one Poisson-disk .xyz cloud per mesh")
    c.add_argument("--mesh_dir", required=True)
    c.add_argument("--out_dir", required=True)
    c.add_argument("--num", type=int, required=True, help="points per cloud (2048: upsampling inputs, 8192: ground truth)")
    c.add_argument("--oversample", type=int, default=4)
    c.add_argument("--cells", action="store_true",
                   help="allow more than %d candidates per cloud: above it the selection runs on the device-wide cell tier "
                        "(dis-pu_amd/poisson_cells.py), below it on the one-workgroup kernel as without this flag" % 49152)
    c.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def mesh_files(mesh_dir):
    """the *.off files of mesh_dir in name order; ValueError if the directory or the files are missing"""
    if not os.path.isdir(mesh_dir):
        raise ValueError("--mesh_dir %s: no such directory" % mesh_dir)
    files = sorted(glob(os.path.join(mesh_dir, "*.off")))
    if not files:
        raise ValueError("--mesh_dir %s: no *.off files" % mesh_dir)
    return files


def refuse_unsupported(a):
    """ValueError naming the first argument the command cannot honour; -> the mesh files."""
    sys.path.insert(0, ROOT)
    from dispu_amd import _lib           # constants only: neither torch nor the library is loaded
    if a.oversample < 1:
        raise ValueError("--oversample must be at least 1, got %d" % a.oversample)
    if a.command == "patches":
        if a.patches_per_mesh <= 0 or a.gt_num <= 0 or a.in_num <= 0:
            raise ValueError("--patches_per_mesh, --gt_num and --in_num must be positive")
        if a.in_num >= a.gt_num:
            raise ValueError("--in_num %d must be below --gt_num %d" % (a.in_num, a.gt_num))
        k = a.oversample * a.gt_num
        if k > KNN_PATCH_MAX_K:
            raise ValueError("--oversample %d x --gt_num %d = %d candidates per patch, at most %d" % (a.oversample, a.gt_num, k, KNN_PATCH_MAX_K))
        if not 0.0 < a.patch_fraction <= 1.0:
            raise ValueError("--patch_fraction must be in (0, 1], got %g" % a.patch_fraction)
        if not a.out.endswith((".h5", ".hdf5")):
            raise ValueError("--out %s: expected an .h5 file name" % a.out)
    else:
        if a.num <= 0:
            raise ValueError("--num must be positive, got %d" % a.num)
        if a.oversample * a.num > (1 << 24 if a.cells else _lib.POISSON_MAX_N):
            raise ValueError("--oversample %d x --num %d = %d candidates, at most %d per cloud%s"
                             % (a.oversample, a.num, a.oversample * a.num, 1 << 24 if a.cells else _lib.POISSON_MAX_N,
                                "" if a.cells else " (--cells lifts the limit: the device-wide cell tier)"))
    return mesh_files(a.mesh_dir)


def names_path(out):
    return os.path.splitext(out)[0] + "_names.txt"


def main(argv=None):
    a = parse_args(argv)
    try:
        files = refuse_unsupported(a)
    except ValueError as e:
        sys.exit(str(e))
    import numpy as np
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib, h5, mesh, mesh_sample, poisson_cells, upsample

    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    dev = torch.device("cuda:0")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    if a.command == "patches":
        inp, gt, names = [], [], []
        for f, stem in zip(files, stems):
            m = mesh.Mesh.from_off(f, dev)
            pi, pg = mesh_sample.make_patches(m, a.patches_per_mesh, gt_num=a.gt_num, in_num=a.in_num, oversample=a.oversample,
                                              patch_fraction=a.patch_fraction, seed=a.seed)
            inp.append(pi.cpu().numpy())
            gt.append(pg.cpu().numpy())
            names += [stem] * a.patches_per_mesh
            print("%s: %d patches" % (stem, a.patches_per_mesh))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        h5.write(a.out, {"poisson_%d" % a.in_num: np.concatenate(inp), "poisson_%d" % a.gt_num: np.concatenate(gt)})
        with open(names_path(a.out), "w") as fh:
            fh.write("".join(n + "\n" for n in names))
        print("%d patches of %d / %d points -> %s" % (len(names), a.in_num, a.gt_num, a.out))
    else:
        os.makedirs(a.out_dir, exist_ok=True)
        for f, stem in zip(files, stems):
            m = mesh.Mesh.from_off(f, dev)
            if a.oversample * a.num > _lib.POISSON_MAX_N:                # above the one-workgroup kernel: the device-wide cell tier
                pts, r = poisson_cells.mesh_cloud(m, a.num, oversample=a.oversample, seed=a.seed)
            else:
                pts, r = mesh_sample.poisson_disk_cloud(m, a.num, oversample=a.oversample, seed=a.seed)
            upsample.save_xyz(os.path.join(a.out_dir, stem + ".xyz"), pts.cpu().numpy())
            print("%s: %d points, radius %.6g" % (stem, a.num, r))


if __name__ == "__main__":
    main()
