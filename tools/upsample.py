#!/usr/bin/env python3
"""Command line of the reference's test phase, `dis-pu.py --phase test` (DisPU/model.py:343-381): restore the latest checkpoint of
--log_dir, upsample every cloud matched by --test_data (default <data_dir>/test/*.xyz) and write <stem>_X<final_ratio>.xyz with
np.savetxt(fmt='%.6f') into --out_folder (default <data_dir>/test/output) -- the files tools/evaluate.py reads.

Clouds go through dis-pu_amd/upsample.py:upsample_ragged in groups of at most --max-points input points (a larger cloud is a group of
its own), so clouds of different sizes share launches; the outputs do not depend on the grouping.  Each output has final_ratio * n
points for its own n (the reference takes n from the first globbed file for all of them, model.py:356-359).  .xyz only: rows of
>= 3 numbers, read like pc_util.load (np.loadtxt, first three columns).

--merge poisson (default fps, the reference's exact farthest point sampling) thins the merged patches of every cloud to final_ratio * n
points by a Poisson-disk selection instead (dis-pu_amd/poisson_cells.py: greedy dart throwing in a random priority order seeded by
--merge_seed, the radius found by bisection): a blue-noise set of exactly as many points in about ten parallel rounds per radius where
FPS takes final_ratio * n dependent ones; no longer the reference's output, and reproducible from --merge_seed.

--grid_size G (off by default) first thins every cloud on the GPU to one barycentre per cube of edge G (dis-pu_amd/grid_subsampling.py,
the reference's cpp_subsampling): FPS seeds and 256-NN patches only mean "a patch of surface" at a roughly even density, which a raw
scan does not have.  The output then has final_ratio times the SUBSAMPLED count.

--normals pca (off by default) adds a unit normal to every output point, six columns x y z nx ny nz: the PCA of its --normals_k exact
nearest neighbours in the output cloud (dis-pu_amd/normals.py; the reference has no counterpart).  --orient picks the sign: none (the
largest component positive), centroid (outwards), viewpoint (towards --viewpoint X Y Z) or input (in agreement with the normal of the
nearest input point: every input file then needs six columns; with --grid_size the input normals are averaged per cube and
renormalised, and a cube whose normals cancel orients nothing).  --orient consistent makes the signs agree from point to point on any
shape, by propagation along the minimum spanning tree of the neighbour graph (normals.orient_consistent): alone, every connected piece
is turned so that its topmost point faces up (outwards on a closed surface); with --orient_prior centroid|viewpoint|input the normals
first take that hint and every piece then faces the way most of its points did.  The rules for --viewpoint and six-column inputs are
those of the prior.

--clean_input / --clean_output statistical|radius (both off by default) drop stray points on the GPU (dis-pu_amd/outliers.py; the
reference has no counterpart): statistical removes the points whose mean distance to their --outliers_k nearest neighbours exceeds the
cloud's mean + --outliers_std standard deviations of it, radius those with fewer than --outliers_min other points within
--outliers_radius.  Input cleaning runs first of all (before --grid_size; with --orient input the input normals follow the kept
points): one stray point shrinks its whole normalised patch.  Output cleaning runs on the upsampled cloud, before --normals.

--keep_clusters K --cluster_eps E (0 = off by default, K = 1 .. 32) keeps only the K largest density clusters of every input cloud on
the GPU (dis-pu_amd/clusters.py, exact DBSCAN; the reference has no counterpart): a floating blob, the turntable or a second object
passes both outlier filters and would be upsampled with the object.  A point is core with --cluster_min_points points within E, itself
included (1, the default: plain Euclidean cluster extraction); clusters below --cluster_min_size points are ignored.  It runs after
--clean_input and before --grid_size and --denoise_input; the run's log line reports the points dropped.

--attributes idw|nearest (off by default) carries per-point attributes (colour, intensity, labels) onto the output: every column beyond
the third of each input file is an attribute, and each output point takes the inverse-distance weighted mean over its --attributes_k
nearest points of the RAW input file (idw), or the row of the nearest one (nearest: labels stay labels), found by an exact search on
the GPU (dis-pu_amd/attributes.py; the reference has no counterpart).  The sources are the file's points before --clean_input and
--grid_size; the transfer runs after --clean_output and before --normals.  Output rows are x y z a1 .. aF [nx ny nz].  Not together
with --orient input, which reads columns 4-6 as normals.

--denoise_input T / --project_output T (both 0 = off by default, T = 1 .. 8 steps) move points onto a moving-least-squares surface on
the GPU (dis-pu_amd/mls.py; the reference has no counterpart): every point goes onto the plane fitted to its --mls_k nearest points of
the surface cloud, weighted out to --mls_support times the distance of the farthest of them.  --denoise_input projects every input
cloud onto its own surface, after --clean_input and --grid_size and before the generator (normals of --orient input stay with their
points).  --project_output projects the upsampled cloud onto the surface of the cloud that went into the generator, after
--clean_output and before --attributes and --normals."""
import argparse
import glob
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def output_name(path, final_ratio):
    """model.py:380: point_path.split('/')[-1][:-4] + '_X%d.xyz' % final_ratio."""
    return os.path.splitext(os.path.basename(path))[0] + "_X%d.xyz" % final_ratio


def refuse_unsupported(paths):
    """ValueError naming the first input that is not an .xyz file (pc_util.load's .ply / .pcd readers are not available)."""
    for p in paths:
        if os.path.splitext(p)[1].lower() != ".xyz":
            raise ValueError("%s: only .xyz point clouds are supported (rows of x y z [...]); convert .ply / .pcd files to .xyz first" % p)


def load_xyz(path):
    """pc_util.load(path)[:, :3] for an .xyz file: np.loadtxt as float32, the first three columns (files with normals work)."""
    pts = np.loadtxt(path, ndmin=2).astype(np.float32)
    if pts.shape[1] < 3:
        raise ValueError("%s: expected at least three columns, got %d" % (path, pts.shape[1]))
    return np.ascontiguousarray(pts[:, :3])


def load_xyz_normals(path):
    """(points [n, 3], normals [n, 3]) float32 of an .xyz file with rows x y z nx ny nz [...]; ValueError naming a file with fewer than
    six columns."""
    rows = np.loadtxt(path, ndmin=2).astype(np.float32)
    if rows.shape[1] < 6:
        raise ValueError("%s: --orient input needs six columns x y z nx ny nz, got %d" % (path, rows.shape[1]))
    return np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3:6])


def save_xyz_normals(path, points, normals):
    """rows x y z nx ny nz at %.6f"""
    np.savetxt(path, np.concatenate([np.asarray(points, np.float32), np.asarray(normals, np.float32)], axis=1), fmt="%.6f")


def load_xyz_attributes(path):
    """(points [n, 3], attributes [n, F]) float32 of an .xyz file with rows x y z a1 .. aF, F >= 1; ValueError naming a file with only
    three columns (or fewer)."""
    rows = np.loadtxt(path, ndmin=2).astype(np.float32)
    if rows.shape[1] < 4:
        raise ValueError("%s: --attributes needs at least one column beyond x y z, got %d columns" % (path, rows.shape[1]))
    return np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3:])


def save_xyz_columns(path, points, *more):
    """rows x y z and then every further block of columns, at %.6f"""
    np.savetxt(path, np.concatenate([np.asarray(points, np.float32)] + [np.asarray(m, np.float32) for m in more], axis=1), fmt="%.6f")


def group_by_budget(sizes, max_points):
    """Consecutive groups of indices into `sizes` (input order kept, no cloud split) whose point counts sum to at most max_points;
    a cloud above the budget forms a group of its own."""
    groups, cur, tot = [], [], 0
    for i, n in enumerate(sizes):
        if cur and tot + n > max_points:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n
    if cur:
        groups.append(cur)
    return groups


def positive_float(text):
    v = float(text)
    if not (math.isfinite(v) and v > 0.0):
        raise argparse.ArgumentTypeError("must be a finite number > 0, got %s" % text)
    return v


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Upsample point clouds with a trained generator (the reference's --phase test).")
    ap.add_argument("--log_dir", default="log", help="checkpoint directory (its `checkpoint` file names the latest model)")
    ap.add_argument("--data_dir", default="data", help="reads <data_dir>/test/*.xyz, writes <data_dir>/test/output")
    ap.add_argument("--test_data", default=None, help="glob of the input clouds (overrides <data_dir>/test/*.xyz)")
    ap.add_argument("--out_folder", default=None, help="output directory (overrides <data_dir>/test/output)")
    ap.add_argument("--final_ratio", type=int, choices=(4, 16), default=4, help="upsampling ratio: 4 (one generator pass) or 16 (two)")
    ap.add_argument("--patch_num_point", type=int, default=256, help="points per patch")
    ap.add_argument("--patch_num_ratio", type=int, default=3, help="patch seeds per patch_num_point input points")
    ap.add_argument("--max-points", dest="max_points", type=int, default=1 << 20,
                    help="input points per batch of clouds (bounds device memory and keeps packed offsets below 2^31)")
    ap.add_argument("--merge", choices=("fps", "poisson"), default="fps",
                    help="how the merged patches are thinned to final_ratio x N points: fps (the reference's exact farthest point sampling) "
                         "or poisson (a Poisson-disk selection of exactly as many points, dis-pu_amd/poisson_cells.py)")
    ap.add_argument("--merge_seed", type=int, default=0, help="--merge poisson: the seed of the greedy's random priority order")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32",
                    help="f32: the strict fp32 generator; bf16: after_conv as a bf16 product over F' stored as bf16 (Generator(dtype='bf16'))")
    ap.add_argument("--grid_size", type=positive_float, default=None,
                    help="off by default; G: grid-subsample every input cloud on the GPU first, one barycentre per cube of edge G "
                         "(for dense, uneven scans); the output has final_ratio x the subsampled count")
    ap.add_argument("--normals", choices=("none", "pca"), default="none",
                    help="pca: write six columns x y z nx ny nz, the normal from the PCA of the --normals_k nearest output points")
    ap.add_argument("--normals_k", type=int, default=16, help="neighbourhood size of --normals pca, 4 .. 32")
    ap.add_argument("--orient", choices=("none", "centroid", "viewpoint", "input", "consistent"), default="none",
                    help="sign of the normals: none (largest component positive), centroid (outwards), viewpoint (towards --viewpoint), "
                         "input (as the nearest input point's normal; the inputs need six columns), consistent (signs that agree from "
                         "point to point: propagation along the neighbour graph's minimum spanning tree)")
    ap.add_argument("--orient_prior", choices=("none", "centroid", "viewpoint", "input"), default="none",
                    help="with --orient consistent: orient by this hint first, then make the signs consistent and keep the direction "
                         "most points had")
    ap.add_argument("--viewpoint", type=float, nargs=3, metavar=("X", "Y", "Z"), default=None, help="the viewpoint of --orient viewpoint")
    ap.add_argument("--clean_input", choices=("none", "statistical", "radius"), default="none",
                    help="drop outliers from every input cloud first of all (before --grid_size)")
    ap.add_argument("--clean_output", choices=("none", "statistical", "radius"), default="none",
                    help="drop outliers from every upsampled cloud (before --normals)")
    ap.add_argument("--outliers_k", type=int, default=16, help="statistical: neighbours per point, 1 .. 31")
    ap.add_argument("--outliers_std", type=float, default=2.0, help="statistical: keep up to mean + this many standard deviations")
    ap.add_argument("--outliers_radius", type=positive_float, default=None, help="radius: the search radius (needed by `radius`)")
    ap.add_argument("--outliers_min", type=int, default=2, help="radius: keep points with at least this many others within the radius")
    ap.add_argument("--keep_clusters", type=int, default=0, metavar="K",
                    help="0: off; K = 1 .. 32: keep only the K largest density clusters of every input cloud (after --clean_input, "
                         "before --grid_size and --denoise_input); needs --cluster_eps")
    ap.add_argument("--cluster_eps", type=positive_float, default=None, help="--keep_clusters: the neighbourhood radius E")
    ap.add_argument("--cluster_min_points", type=int, default=1,
                    help="--keep_clusters: points within E, the point itself included, that make a core point (1: plain Euclidean clusters)")
    ap.add_argument("--cluster_min_size", type=int, default=1, help="--keep_clusters: ignore clusters of fewer points")
    ap.add_argument("--attributes", choices=("none", "idw", "nearest"), default="none",
                    help="carry every input column beyond x y z onto the output points: idw (inverse-distance weighted mean over the "
                         "--attributes_k nearest raw input points) or nearest (the nearest one's row; for labels); the output rows are "
                         "x y z a1 .. aF [nx ny nz]; not together with --orient input, which reads columns 4-6 as normals")
    ap.add_argument("--attributes_k", type=int, default=3, help="neighbours per output point of --attributes, 1 .. 32")
    ap.add_argument("--denoise_input", type=int, default=0, metavar="T",
                    help="0: off; T = 1 .. 8: project every input cloud onto its own moving-least-squares surface in T steps (after "
                         "--clean_input and --grid_size, before the generator)")
    ap.add_argument("--project_output", type=int, default=0, metavar="T",
                    help="0: off; T = 1 .. 8: project every upsampled cloud onto the moving-least-squares surface of the cloud that went "
                         "into the generator in T steps (after --clean_output, before --attributes and --normals)")
    ap.add_argument("--mls_k", type=int, default=16, help="neighbours per point of --denoise_input / --project_output, 4 .. 32")
    ap.add_argument("--mls_support", type=float, default=1.0,
                    help="the weights of --denoise_input / --project_output reach this many times the farthest neighbour's distance, 1 .. 4")
    ap.add_argument("--mesh", choices=("none", "off"), default="none",
                    help="off: also write <stem>_X<ratio>.off beside every cloud, the surface reconstructed from the written points and "
                         "their oriented normals (needs --normals pca, an --orient other than none, and --mesh_voxel)")
    ap.add_argument("--mesh_voxel", type=positive_float, default=None, help="--mesh: the lattice's edge H (no automatic choice)")
    ap.add_argument("--mesh_k", type=int, default=8, help="--mesh: neighbours per lattice vertex of the signed distance, 1 .. 32")
    ap.add_argument("--mesh_support", type=float, default=1.5,
                    help="--mesh: the weights reach this many times the farthest neighbour's distance, 1 .. 4")
    ap.add_argument("--mesh_band", type=int, default=1, help="--mesh: voxels followed around every occupied one, 1 .. 3")
    a = ap.parse_args(argv)
    if a.mesh != "none":
        if a.normals != "pca" or a.orient == "none":
            ap.error("--mesh needs oriented normals: --normals pca with an --orient other than none")
        if a.mesh_voxel is None:
            ap.error("--mesh needs --mesh_voxel H")
    if not 1 <= a.mesh_k <= 32:
        ap.error("--mesh_k must be in 1 .. 32, got %d" % a.mesh_k)
    if not 1.0 <= a.mesh_support <= 4.0:                                     # a NaN fails both comparisons
        ap.error("--mesh_support must be in 1 .. 4, got %s" % a.mesh_support)
    if not 1 <= a.mesh_band <= 3:
        ap.error("--mesh_band must be in 1 .. 3, got %d" % a.mesh_band)
    for name in ("denoise_input", "project_output"):
        if not 0 <= getattr(a, name) <= 8:
            ap.error("--%s must be in 0 .. 8, got %d" % (name, getattr(a, name)))
    if not 4 <= a.mls_k <= 32:
        ap.error("--mls_k must be in 4 .. 32, got %d" % a.mls_k)
    if not 1.0 <= a.mls_support <= 4.0:                                      # a NaN fails both comparisons
        ap.error("--mls_support must be in 1 .. 4, got %s" % a.mls_support)
    if "radius" in (a.clean_input, a.clean_output) and a.outliers_radius is None:
        ap.error("--clean_input / --clean_output radius need --outliers_radius R")
    if not 1 <= a.outliers_k <= 31:
        ap.error("--outliers_k must be in 1 .. 31, got %d" % a.outliers_k)
    if not math.isfinite(a.outliers_std):
        ap.error("--outliers_std must be finite")
    if a.outliers_min < 1:
        ap.error("--outliers_min must be >= 1, got %d" % a.outliers_min)
    if not 0 <= a.keep_clusters <= 32:
        ap.error("--keep_clusters must be in 0 .. 32, got %d" % a.keep_clusters)
    if a.keep_clusters > 0 and a.cluster_eps is None:
        ap.error("--keep_clusters K needs --cluster_eps E")
    if a.cluster_min_points < 1:
        ap.error("--cluster_min_points must be >= 1, got %d" % a.cluster_min_points)
    if a.cluster_min_size < 1:
        ap.error("--cluster_min_size must be >= 1, got %d" % a.cluster_min_size)
    if a.normals == "none" and (a.orient != "none" or a.viewpoint is not None):
        ap.error("--orient and --viewpoint need --normals pca")
    if not 4 <= a.normals_k <= 32:
        ap.error("--normals_k must be in 4 .. 32, got %d" % a.normals_k)
    if a.orient_prior != "none" and a.orient != "consistent":
        ap.error("--orient_prior needs --orient consistent")
    a.hint = a.orient_prior if a.orient == "consistent" else a.orient     # the pointwise rule: it decides what else is needed
    if (a.hint == "viewpoint") != (a.viewpoint is not None):
        ap.error("--orient viewpoint and --viewpoint X Y Z go together")
    if a.viewpoint is not None and not all(math.isfinite(v) for v in a.viewpoint):
        ap.error("--viewpoint must be finite")
    if not 1 <= a.attributes_k <= 32:
        ap.error("--attributes_k must be in 1 .. 32, got %d" % a.attributes_k)
    if a.attributes != "none" and a.hint == "input":
        ap.error("--attributes and --orient input do not go together: columns 4-6 would be both attributes and normals")
    return a


def remove_outliers(kind, arrays, a, dev):
    """the --clean_* step on a list of numpy clouds, in groups of at most --max-points -> (kept clouds, kept indices), numpy"""
    import torch
    from dispu_amd import outliers
    kept, index = [], []
    for group in group_by_budget([c.shape[0] for c in arrays], a.max_points):
        d = [torch.from_numpy(np.ascontiguousarray(arrays[i], np.float32)).to(dev) for i in group]
        if kind == "statistical":
            pts, idx = outliers.remove_statistical_outliers(d, k=a.outliers_k, std_ratio=a.outliers_std, return_index=True)
        else:
            pts, idx = outliers.remove_radius_outliers(d, a.outliers_radius, min_neighbors=a.outliers_min, return_index=True)
        kept += [t.cpu().numpy() for t in pts]
        index += [t.cpu().numpy() for t in idx]
    return kept, index


def keep_largest_clusters(arrays, a, dev):
    """the --keep_clusters step on a list of numpy clouds, in groups of at most --max-points -> (kept clouds, kept indices), numpy"""
    import torch
    from dispu_amd import clusters
    kept, index = [], []
    for group in group_by_budget([c.shape[0] for c in arrays], a.max_points):
        d = [torch.from_numpy(np.ascontiguousarray(arrays[i], np.float32)).to(dev) for i in group]
        pts, idx = clusters.keep_clusters(d, a.cluster_eps, min_points=a.cluster_min_points, keep=a.keep_clusters,
                                          min_size=a.cluster_min_size, return_index=True)
        kept += [t.cpu().numpy() for t in pts]
        index += [t.cpu().numpy() for t in idx]
    return kept, index


def transfer_attributes(preds, src_points, src_attrs, a, dev):
    """the --attributes step: numpy attributes [len(pred), F] for every cloud of `preds` from its raw input (points, attributes), in
    groups of at most --max-points output points; clouds of one group with different column counts go in separate calls"""
    import torch
    from dispu_amd import attributes
    out = [None] * len(preds)
    for group in group_by_budget([p.shape[0] for p in preds], a.max_points):
        for F in sorted({src_attrs[i].shape[1] for i in group}):
            same = [i for i in group if src_attrs[i].shape[1] == F]
            got = attributes.transfer_attributes([torch.from_numpy(np.ascontiguousarray(preds[i], np.float32)).to(dev) for i in same],
                                                 [torch.from_numpy(src_points[i]).to(dev) for i in same],
                                                 features=[torch.from_numpy(src_attrs[i]).to(dev) for i in same], k=a.attributes_k,
                                                 mode=a.attributes)
            for i, t in zip(same, got):
                out[i] = t.cpu().numpy()
    return out


def mls_project(points, surfaces, steps, a, dev):
    """the --denoise_input / --project_output step: every numpy cloud of `points` projected onto the surface of its cloud of `surfaces`
    in `steps` steps, in groups of at most --max-points points -> numpy clouds"""
    import torch
    from dispu_amd import mls
    out = [None] * len(points)
    for group in group_by_budget([p.shape[0] for p in points], a.max_points):
        got = mls.mls_project([torch.from_numpy(np.ascontiguousarray(points[i], np.float32)).to(dev) for i in group],
                              [torch.from_numpy(np.ascontiguousarray(surfaces[i], np.float32)).to(dev) for i in group],
                              k=a.mls_k, support=a.mls_support, iterations=steps)
        for i, t in zip(group, got):
            out[i] = t.cpu().numpy()
    return out


def stage(prefix, fn, *args, **kw):
    """fn(*args, **kw); a ValueError ends the run with `prefix` (the files concerned, the option) before its text"""
    try:
        return fn(*args, **kw)
    except ValueError as e:
        sys.exit("%s%s" % (prefix, e))


def load_inputs(a, paths):
    """-> (clouds, in_normals or None, (src_points, src_attrs) or None), numpy, one entry per path"""
    if a.hint == "input":
        clouds, in_normals = (list(t) for t in zip(*[load_xyz_normals(p) for p in paths]))
        return clouds, in_normals, None
    if a.attributes != "none":
        clouds, src_attrs = (list(t) for t in zip(*[load_xyz_attributes(p) for p in paths]))
        return clouds, None, (list(clouds), src_attrs)   # the raw file's points: --clean_input and --grid_size replace clouds[i], not these
    return [load_xyz(p) for p in paths], None, None


def prepare_inputs(a, paths, clouds, in_normals, dev):
    """--clean_input, --keep_clusters, --grid_size, then --denoise_input, in place on clouds (and on in_normals, which follow their
    points) -> (outliers removed per cloud, points dropped with the smaller clusters per cloud)"""
    import torch
    raw = [c.shape[0] for c in clouds]
    removed, dropped = [0] * len(clouds), [0] * len(clouds)
    if a.clean_input != "none":
        kept, index = stage("--clean_input: ", remove_outliers, a.clean_input, clouds, a, dev)
        for i, (k, ix) in enumerate(zip(kept, index)):
            if k.shape[0] < a.patch_num_point:
                sys.exit("%s: --clean_input %s leaves %d of %d points, fewer than --patch_num_point %d"
                         % (paths[i], a.clean_input, k.shape[0], raw[i], a.patch_num_point))
            removed[i] = raw[i] - k.shape[0]
            clouds[i] = k
            if in_normals is not None:
                in_normals[i] = np.ascontiguousarray(in_normals[i][ix])
    if a.keep_clusters > 0:
        kept, index = stage("--keep_clusters: ", keep_largest_clusters, clouds, a, dev)
        for i, (k, ix) in enumerate(zip(kept, index)):
            if k.shape[0] < a.patch_num_point:
                sys.exit("%s: --keep_clusters %d leaves %d of %d points, fewer than --patch_num_point %d"
                         % (paths[i], a.keep_clusters, k.shape[0], clouds[i].shape[0], a.patch_num_point))
            dropped[i] = clouds[i].shape[0] - k.shape[0]
            clouds[i] = k
            if in_normals is not None:
                in_normals[i] = np.ascontiguousarray(in_normals[i][ix])
    if a.grid_size is not None:
        from dispu_amd import grid_subsampling
        for i, c in enumerate(clouds):
            if in_normals is None:
                clouds[i] = stage("%s: " % paths[i], grid_subsampling.compute, c, sampleDl=a.grid_size)
            else:                                        # the normals ride through as features: the mean per cube, renormalised below
                pts, nrm = stage("%s: " % paths[i], grid_subsampling.compute, torch.from_numpy(c).to(dev),
                                 features=torch.from_numpy(in_normals[i]).to(dev), sampleDl=a.grid_size)
                length = nrm.norm(dim=1, keepdim=True)
                in_normals[i] = torch.where(length > 0, nrm / length, torch.zeros_like(nrm))      # a zero mean stays zero
                clouds[i] = pts.cpu().numpy()
    if a.denoise_input:
        clouds[:] = stage("--denoise_input: ", mls_project, clouds, clouds, a.denoise_input, a, dev)
    return removed, dropped


def orient_argument(a, group, clouds, in_normals, dev):
    """estimate_normals' orient for the clouds of one group"""
    import torch
    orient = None
    if a.hint == "centroid":
        orient = ("centroid",)
    elif a.hint == "viewpoint":
        orient = ("viewpoint", a.viewpoint)
    elif a.hint == "input":
        orient = ("reference", [torch.from_numpy(clouds[i]).to(dev) for i in group],
                  [torch.as_tensor(in_normals[i], device=dev).contiguous() for i in group])
    if a.orient == "consistent":
        orient = ("consistent",) if orient is None else ("consistent", orient)
    return orient


def process_group(a, gen, paths, group, clouds, in_normals, src, dev):
    """upsample, --clean_output, --attributes, --normals for one group -> (preds, attrs or None, normals or None, removed per cloud)"""
    import torch
    from dispu_amd.upsample import upsample_ragged
    names = ", ".join(paths[i] for i in group)
    preds = stage("%s: " % names, upsample_ragged, gen, [clouds[i] for i in group], a.patch_num_point, a.patch_num_ratio, a.final_ratio,
                  merge=a.merge, merge_seed=a.merge_seed)
    removed, attrs, normals = [0] * len(group), None, None
    if a.clean_output != "none":
        cleaned, _ = stage("%s: --clean_output: " % names, remove_outliers, a.clean_output, preds, a, dev)
        removed = [before.shape[0] - after.shape[0] for before, after in zip(preds, cleaned)]
        preds = cleaned
    if a.project_output:
        preds = stage("%s: --project_output: " % names, mls_project, preds, [clouds[i] for i in group], a.project_output, a, dev)
    if a.attributes != "none":
        attrs = stage("%s: --attributes: " % names, transfer_attributes, preds, [src[0][i] for i in group], [src[1][i] for i in group], a, dev)
    if a.normals == "pca":
        from dispu_amd.normals import estimate_normals
        dpred = [torch.from_numpy(p).to(dev) for p in preds]
        orient = orient_argument(a, group, clouds, in_normals, dev)
        normals = [t.cpu().numpy() for t in stage("%s: " % names, estimate_normals, dpred, k=a.normals_k, orient=orient)]
    return preds, attrs, normals, removed


def write_output(out, pred, attrs, normals):
    from dispu_amd.upsample import save_xyz
    if attrs is not None:
        save_xyz_columns(out, pred, attrs, *([normals] if normals is not None else []))
    elif normals is not None:
        save_xyz_normals(out, pred, normals)
    else:
        save_xyz(out, pred)


def write_mesh(xyz_path, a, dev):
    """the --mesh step: the surface of the cloud AS THE FILE HOLDS IT (x y z first, nx ny nz last, at the file's six decimals, so the
    mesh can be reproduced from the file alone) -> the path of the .off beside it, vertex and face counts"""
    import torch
    from dispu_amd import mesh, reconstruct
    rows = np.loadtxt(xyz_path, ndmin=2).astype(np.float32)
    pts, nrm = (torch.from_numpy(np.ascontiguousarray(rows[:, c])).to(dev) for c in (slice(0, 3), slice(-3, None)))
    verts, faces = reconstruct.reconstruct_surface(pts, nrm, a.mesh_voxel, k=a.mesh_k, support=a.mesh_support, band=a.mesh_band)
    off = os.path.splitext(xyz_path)[0] + ".off"
    mesh.save_off(off, verts, faces)
    return off, verts.shape[0], faces.shape[0]


def main(argv=None):
    a = parse_args(argv)
    if a.max_points <= 0:
        sys.exit("--max-points must be positive")
    pattern = a.test_data or os.path.join(a.data_dir, "test", "*.xyz")
    out_dir = a.out_folder or os.path.join(a.data_dir, "test", "output")
    paths = sorted(glob.glob(pattern))
    if not paths:
        sys.exit("no input matches %s" % pattern)
    stage("", refuse_unsupported, paths)
    clouds, in_normals, src = stage("", load_inputs, a, paths)

    sys.path.insert(0, ROOT)
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd.checkpoint import restore_generator

    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    dev = torch.device("cuda:0")
    epoch, gen = restore_generator(a.log_dir, device=dev, dtype=a.dtype)
    print("restored %s (epoch %d)" % (a.log_dir, epoch))
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    raw = [c.shape[0] for c in clouds]
    removed_in, dropped_in = prepare_inputs(a, paths, clouds, in_normals, dev)
    for group in group_by_budget([c.shape[0] for c in clouds], a.max_points):
        preds, attrs, normals, removed_out = process_group(a, gen, paths, group, clouds, in_normals, src, dev)
        for j, (i, pred) in enumerate(zip(group, preds)):
            out = os.path.join(out_dir, output_name(paths[i], a.final_ratio))
            write_output(out, pred, attrs[j] if attrs is not None else None, normals[j] if normals is not None else None)
            gone = ""
            if a.clean_input != "none" or a.clean_output != "none":
                gone = ", outliers removed: %d input, %d output" % (removed_in[i], removed_out[j])
            if a.keep_clusters > 0:
                gone += ", dropped with the smaller clusters: %d" % dropped_in[i]
            if a.grid_size is None:
                print("%s: %d -> %d points, %s%s" % (paths[i], clouds[i].shape[0], pred.shape[0], out, gone))
            else:
                print("%s: %d -> %d (grid %g) -> %d points, %s%s" % (paths[i], raw[i], clouds[i].shape[0], a.grid_size, pred.shape[0], out,
                                                                   gone))
            if a.mesh != "none":
                print("%s: %d vertices, %d faces" % stage("%s: --mesh: " % out, write_mesh, out, a, dev))
    print("%d clouds in %.2f s" % (len(paths), time.time() - t0))


if __name__ == "__main__":
    main()
