"""Evaluator: counterpart of /evaluate.py:33-41,153-162 of the reference (CD and Hausdorff between a predicted and a
ground-truth cloud, both normalised first with Common/ops.py:1954-1963).  The reference builds a TF graph around
tf_nndistance and runs one cloud pair per session call; here both clouds are normalised and matched on the device
(dispu_normalize_patches + dispu_nn_distance at (1, 8192, 8192)) and only four scalars travel to the host.

With a mesh (dis-pu_amd/mesh.py) the P2F and uniformity columns of evaluate.py:53-101,163-180 are added: the reference reads them
from the files of its CGAL tool (evaluation_code/evaluation.cpp); here they are computed on the device, with Euclidean disks (mode
"euclidean", the default) or with the CGAL tool's exact geodesic disks (mode "geodesic"), or read from existing CGAL files (mode
"cgal_files")."""
import csv
import os
from glob import glob

import numpy as np
import torch

from . import _lib
from . import mesh as M
from .tf_nndistance import nn_distance
from .upsample import normalize_patches


def evaluate_pair(pred, gt, mesh=None, seeds=1000, seed=0, percentages=M.DEFAULT_PERCENTAGES, disks="euclidean"):
    """pred [n,3], gt [m,3] device tensors or arrays -> {"CD": mean fwd + mean bwd, "hausdorff": max fwd + max bwd}.
    With mesh (a mesh.Mesh of the ground-truth surface) the dict also holds "p2f avg" / "p2f std" (P2F of the raw predicted
    points) and "uniform_<j>" per percentage, with "uniformity_mode": disks ("euclidean" or "geodesic", see mesh.py); seeds is a
    count drawn with `seed` or user-given (face_id, b0, b1, b2) rows (mesh.mesh_metrics)."""
    if disks not in M.DISK_MODES:
        raise ValueError("disks must be one of %s, got %r" % (M.DISK_MODES, disks))
    dev = pred.device if isinstance(pred, torch.Tensor) else torch.device("cuda:0")
    p = (pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pred[:, :3], np.float32)).to(dev))
    g = (gt if isinstance(gt, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(gt[:, :3], np.float32)).to(dev))
    pn = normalize_patches(p.reshape(1, -1, 3).contiguous())[0]
    gn = normalize_patches(g.reshape(1, -1, 3).contiguous())[0]
    fwd, _, bwd, _ = nn_distance(pn, gn)
    L = _lib.lib()
    out = torch.empty(4, dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(L.dispu_row_mean_max(1, fwd.shape[1], _lib.ptr(fwd), _lib.ptr(out), _lib.C.c_void_p(out.data_ptr() + 4), st), "row_mean_max")
    _lib.check(L.dispu_row_mean_max(1, bwd.shape[1], _lib.ptr(bwd), _lib.C.c_void_p(out.data_ptr() + 8),
                                    _lib.C.c_void_p(out.data_ptr() + 12), st), "row_mean_max")
    mf, xf, mb, xb = (float(v) for v in out.cpu())
    res = {"CD": mf + mb, "hausdorff": xf + xb, "cd_forward": mf, "cd_backward": mb}
    if mesh is not None:
        mm = M.mesh_metrics(p, mesh, seeds=seeds, seed=seed, percentages=percentages, disks=disks)
        res.update(_mesh_row(mm["p2f avg"], mm["p2f std"], mm["uniform"]))
        res["uniformity_mode"] = disks
    return res


def _mesh_row(m, s, uni):
    row = {"p2f avg": m, "p2f std": s}
    for j, u in enumerate(uni):
        row["uniform_%d" % j] = float(u)
    return row


def _from_cgal_files(pred_path, dev, percentages):
    """P2F and uniformity from the CGAL tool's files beside pred_path (evaluate.py:155-180): P2F from column 3 of
    `_point2mesh_distance.txt`, the disks of `_disk_idx.txt` over its projected points, N = its number of lines."""
    c = M.read_cgal_files(pred_path)
    if len(percentages) != c["radii"].shape[0]:
        raise ValueError("%s: %d radii but %d percentages" % (pred_path, c["radii"].shape[0], len(percentages)))
    dist = torch.from_numpy(c["dist"]).to(dev)
    proj = torch.from_numpy(c["proj"]).to(dev)
    off = torch.from_numpy(c["offsets"]).to(dev)
    mem = torch.from_numpy(c["members"]).to(dev)
    uni = M.uniformity(proj, off, mem, c["radii"], np.asarray(percentages, np.float64), N=proj.shape[0])
    m, s = M.mean_std(dist)
    return {"p2f avg": m, "p2f std": s, "uniform": uni, "dist": dist}


def evaluate_dirs(pred_dir, gt_dir, csv_name="evaluation.csv", mesh_dir=None, write_cgal_files=False, use_cgal_files=False,
                  seeds=1000, seed=0, percentages=M.DEFAULT_PERCENTAGES, disks="euclidean"):
    """evaluate.py:128-204: every gt/<name>.xyz against pred/<name>.xyz; writes the CSV next to the predictions and returns the
    rows plus the averages.  Without mesh_dir / use_cgal_files: the CD / hausdorff columns only, as before.
    mesh_dir: where mesh_dir/<name>.off exists the row gains "p2f avg", "p2f std", "uniform_<j>" (disks: "euclidean", the default,
    or "geodesic", the CGAL tool's membership) and the CSV has the reference's seven columns; write_cgal_files writes the CGAL
    tool's three files beside each such prediction, `_disk_idx.txt` with the disks of that mode.
    use_cgal_files: where the CGAL tool's files exist beside a prediction, P2F and the disks are read from them instead (the
    reference's route, geodesic disks included).  In the avg row P2F is over all files' distances concatenated (:200-204) and
    uniformity is the mean over files."""
    if disks not in M.DISK_MODES:
        raise ValueError("disks must be one of %s, got %r" % (M.DISK_MODES, disks))
    rows = []
    p2f_all, uni_all = [], []
    dev = torch.device("cuda:0")
    for gt_path in sorted(glob(os.path.join(gt_dir, "*.xyz"))):
        name = os.path.basename(gt_path)
        pred_path = os.path.join(pred_dir, name)
        if not os.path.isfile(pred_path):
            continue
        pred = np.loadtxt(pred_path)[:, :3]
        r = evaluate_pair(pred, np.loadtxt(gt_path)[:, :3])
        row = {"name": name, "CD": r["CD"], "hausdorff": r["hausdorff"]}
        mm = None
        mesh_path = os.path.join(mesh_dir, os.path.splitext(name)[0] + ".off") if mesh_dir else None
        if use_cgal_files and all(os.path.isfile(f) for f in M.cgal_paths(pred_path)):
            mm = _from_cgal_files(pred_path, dev, percentages)
            row["uniformity_mode"] = "cgal_files"
        elif mesh_path and os.path.isfile(mesh_path):
            p = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(dev)
            mm = M.mesh_metrics(p, M.Mesh.from_off(mesh_path, dev), seeds=seeds, seed=seed, percentages=percentages, disks=disks)
            row["uniformity_mode"] = disks
            if write_cgal_files:
                M.write_cgal_files(pred_path, p.cpu().numpy(), mm["dist"].cpu().numpy(), mm["proj"].cpu().numpy(), mm["radii"],
                                   mm["offsets"].cpu().numpy(), mm["members"].cpu().numpy())
        if mm is not None:
            row.update(_mesh_row(mm["p2f avg"], mm["p2f std"], mm["uniform"]))
            p2f_all.append(mm["dist"])
            uni_all.append(np.asarray(mm["uniform"], np.float64))
        rows.append(row)
    if rows:
        fields = ["name", "CD", "hausdorff"]
        avg = {"name": "avg", "CD": float(np.mean([r["CD"] for r in rows])), "hausdorff": float(np.mean([r["hausdorff"] for r in rows]))}
        if p2f_all:
            fields += ["p2f avg", "p2f std"] + ["uniform_%d" % j for j in range(len(percentages))]
            m, s = M.mean_std(torch.cat(p2f_all))
            avg.update(_mesh_row(m, s, np.mean(np.stack(uni_all), axis=0)))
        with open(os.path.join(pred_dir, csv_name), "w") as f:
            w = csv.DictWriter(f, fieldnames=fields, restval="-", extrasaction="ignore")
            w.writeheader()
            for r in rows + [avg]:
                w.writerow(r)
    return rows
