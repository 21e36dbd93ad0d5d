#!/usr/bin/env python3
"""Command line of the reference's evaluate.py: CD / Hausdorff of --pred against --gt, plus P2F and uniformity where
--mesh DIR holds <name>.off (dis-pu_amd/evaluate.py:evaluate_dirs).  --disks geodesic decides disk membership by the exact
geodesic distance on the mesh, as the reference's CGAL tool does; the default, euclidean, by the straight-line distance.  Writes
evaluation.csv beside the predictions and prints its header and `avg` row."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dispu_amd  # noqa: E402,F401
from dispu_amd.evaluate import evaluate_dirs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred", required=True, help="directory of predicted .xyz")
    ap.add_argument("--gt", required=True, help="directory of ground-truth .xyz")
    ap.add_argument("--mesh", default=None, help="directory of ground-truth meshes <name>.off")
    ap.add_argument("--write-cgal-files", action="store_true", help="write the CGAL tool's three files beside each prediction")
    ap.add_argument("--use-cgal-files", action="store_true", help="read P2F and disks from existing CGAL tool files")
    ap.add_argument("--seed", type=int, default=0, help="seed of the 1000 disk centres")
    ap.add_argument("--disks", choices=("euclidean", "geodesic"), default="euclidean",
                    help="disk membership by straight-line (default) or exact geodesic distance (the CGAL tool's)")
    a = ap.parse_args()
    rows = evaluate_dirs(os.path.abspath(a.pred), os.path.abspath(a.gt), mesh_dir=a.mesh, write_cgal_files=a.write_cgal_files,
                         use_cgal_files=a.use_cgal_files, seed=a.seed, disks=a.disks)
    if not rows:
        sys.exit("no prediction matches a ground-truth file")
    lines = open(os.path.join(os.path.abspath(a.pred), "evaluation.csv")).read().strip().splitlines()
    print(lines[0])
    print(lines[-1])


if __name__ == "__main__":
    main()
