"""Whole-cloud upsampling (the reference's `Model.test()` data path, DisPU/model.py:306-381) on one MI355X:

    normalise cloud -> FPS seeds (N/256*3) -> 256-NN patches -> per-patch normalise -> generator (ALL patches in one
    batch; the reference feeds them one by one with batch size 1) -> de-normalise -> concat -> FPS to final_ratio*N.

Every stage is a kernel of libdispu_hip.so; the cloud crosses the host boundary once in and once out
(the reference crosses it ~2 x 24 times per 2048-point cloud plus the nanoflann hop inside every generator call)."""
import math

import numpy as np
import torch

from . import _lib
from .segments import host_ptr, offsets as segment_offsets, to_device
from .tf_sampling import farthest_point_sample, fps_ragged, gather_point


def knn_patch(cloud, queries, k):
    """pc_util.extract_knn_patch (:83-92): cloud[b,n,3], queries[b,m,3] -> idx[b,m,k] int32 (ascending distance)."""
    b, n, _ = cloud.shape
    m = queries.shape[1]
    idx = torch.empty((b, m, k), dtype=torch.int32, device=cloud.device)
    _lib.check(_lib.lib().dispu_knn_patch(b, n, m, k, _lib.ptr(cloud.contiguous()), _lib.ptr(queries.contiguous()), _lib.ptr(idx),
                                          _lib.stream_ptr(cloud.device)), "dispu_knn_patch")
    return idx


def normalize_patches(p):
    """pc_util.normalize_point_cloud (:147-161) per patch: -> (normalised [b,n,3], centroid [b,3], furthest [b])."""
    b, n, _ = p.shape
    out = torch.empty_like(p)
    c = torch.empty((b, 3), dtype=torch.float32, device=p.device)
    f = torch.empty((b,), dtype=torch.float32, device=p.device)
    _lib.check(_lib.lib().dispu_normalize_patches(b, n, _lib.ptr(p.contiguous()), _lib.ptr(out), _lib.ptr(c), _lib.ptr(f),
                                                  _lib.stream_ptr(p.device)), "dispu_normalize_patches")
    return out, c, f


def denormalize_patches(p, centroid, furthest):
    b, m, _ = p.shape
    out = torch.empty_like(p)
    _lib.check(_lib.lib().dispu_denormalize_patches(b, m, _lib.ptr(p.contiguous()), _lib.ptr(centroid), _lib.ptr(furthest),
                                                    _lib.ptr(out), _lib.stream_ptr(p.device)), "dispu_denormalize_patches")
    return out


def generator_chain(gen, patches, final_ratio=4, step_ratio=4):
    """Model.build_model_test (DisPU/model.py:114-118): G once, then round(final_ratio ** (1/step_ratio)) - 1 more times on
    its own output (final_ratio 16 -> two passes: 256 -> 1024 -> 4096 points per patch)."""
    coarse, fine = gen(patches)
    for _ in range(round(math.pow(final_ratio, 1.0 / step_ratio)) - 1):
        coarse, fine = gen(fine if not gen.return_views else fine.clone())   # views alias the reusable workspace
    return coarse, fine


def upsample_clouds(gen, clouds, patch_num_point=256, patch_num_ratio=3, final_ratio=4, return_stages=False):
    """A BATCH of equally sized clouds [C, N, 3] -> [C, final_ratio*N, 3] (device tensor).  Every stage of Model.test
    (model.py:343-381) already is a batched kernel, so C clouds cost the launches of one: the seed FPS and the final
    FPS - m - 1 dependent rounds on ONE CU per cloud, 17 ms for 24576 -> 8192 - run C clouds on C CUs at once, and the
    generator sees all C * seed_num patches in one batch.  Cloud c of the result is bit-identical to upsample_cloud(clouds[c])."""
    dev = gen.device
    cloud = torch.as_tensor(np.ascontiguousarray(clouds, np.float32) if not isinstance(clouds, torch.Tensor) else clouds,
                            dtype=torch.float32, device=dev)
    if cloud.dim() != 3 or cloud.shape[2] != 3:
        raise ValueError("upsample_clouds expects [C, N, 3]")
    C, n, _ = cloud.shape
    cloud_n, c0, f0 = normalize_patches(cloud)                                   # whole-cloud normalisation (model.py:364)
    seed_num = int(n / patch_num_point * patch_num_ratio)
    seeds = farthest_point_sample(seed_num, cloud_n)                             # model.py:323
    seed_xyz = gather_point(cloud_n, seeds)
    pidx = knn_patch(cloud_n, seed_xyz, patch_num_point)                         # pc_util.extract_knn_patch
    patches = gather_point(cloud_n, pidx.reshape(C, -1)).reshape(C * seed_num, patch_num_point, 3)
    pn, pc_c, pc_f = normalize_patches(patches)                                  # model.py:306-308
    coarse, fine = generator_chain(gen, pn, final_ratio)
    pred = denormalize_patches(fine, pc_c, pc_f)                                 # model.py:310
    merged = denormalize_patches(pred.reshape(C, -1, 3), c0, f0)                 # model.py:371-372
    out_num = int(n * final_ratio)
    sel = farthest_point_sample(out_num, merged)                                 # model.py:375
    result = gather_point(merged, sel)
    if return_stages:
        return result, dict(cloud_n=cloud_n, seeds=seeds, pidx=pidx, patches_n=pn, fine=fine, merged=merged, sel=sel)
    return result


# ---- ragged batches: clouds of different sizes packed into one [sum n_c, 3] array, segment c = points [off[c], off[c + 1]) -----------

def fps_segments(inp, off, moff, arith=_lib.ARITH_CONTRACT, path="auto", cell=0):
    """farthest_point_sample per segment: inp [sum n_c, 3] (device), off / moff host offsets of the points and of the samples ->
    idx [sum m_c] int32, local to each segment.  Segment c equals farthest_point_sample(m_c, cloud_c) bit for bit.
    path: "auto" (dispu_fps_segments_auto: the cell-skipping kernels where they are faster), "cells" (those kernels for every segment,
    cell = a forced cell size) or "stream" (dispu_fps_segments); the indices do not depend on it (tf_sampling.fps_ragged)."""
    return fps_ragged(inp, off, moff, arith, path, cell)


def knn_patch_segments(cloud, off, queries, qoff, k):
    """knn_patch per segment: cloud [sum n_c, 3], queries [sum m_c, 3] (device), host offsets -> idx [sum m_c, k] int32, local."""
    off, qoff = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(qoff, np.int32)
    idx = torch.empty((int(qoff[-1]), k), dtype=torch.int32, device=cloud.device)
    d_off, d_qoff = to_device(off, cloud.device), to_device(qoff, cloud.device)
    _lib.check(_lib.lib().dispu_knn_patch_segments(len(off) - 1, _lib.ptr(d_off), _lib.ptr(d_qoff), host_ptr(off), host_ptr(qoff), k,
                                                   _lib.ptr(cloud.contiguous()), _lib.ptr(queries.contiguous()), _lib.ptr(idx),
                                                   _lib.stream_ptr(cloud.device)), "dispu_knn_patch_segments")
    return idx


def normalize_segments(p, off):
    """normalize_patches over each whole segment: p [sum n_c, 3] -> (normalised [sum n_c, 3], centroid [C, 3], furthest [C])."""
    off = np.ascontiguousarray(off, np.int32)
    C = len(off) - 1
    out = torch.empty_like(p)
    c = torch.empty((C, 3), dtype=torch.float32, device=p.device)
    f = torch.empty((C,), dtype=torch.float32, device=p.device)
    d_off = to_device(off, p.device)
    _lib.check(_lib.lib().dispu_normalize_segments(C, _lib.ptr(d_off), host_ptr(off), _lib.ptr(p.contiguous()), _lib.ptr(out), _lib.ptr(c),
                                                   _lib.ptr(f), _lib.stream_ptr(p.device)), "dispu_normalize_segments")
    return out, c, f


def _gather_rows(points, idx):
    """points [n, 3], idx [r] int32 global rows -> [r, 3] (dispu_gather_point at b = 1)."""
    return gather_point(points.reshape(1, -1, 3), idx.reshape(1, -1)).reshape(-1, 3)


def upsample_ragged(gen, clouds, patch_num_point=256, patch_num_ratio=3, final_ratio=4, return_stages=False, merge="fps", merge_seed=0):
    """Clouds of ANY sizes (a sequence of [n_c, 3] numpy arrays or device tensors) -> a list of [final_ratio * n_c, 3] float32 numpy
    arrays in input order, each bit-identical to upsample_cloud(gen, clouds[c]) (model.py:343-381 per cloud).  The clouds are packed
    into one [sum n_c, 3] array; whole-cloud normalisation, both FPS stages and the patch k-NN run as ONE launch (sequence) over all
    segments, and all patches of all clouds go through one generator batch.  With return_stages also a dict of the packed device
    stages and their host offsets: cloud_n / off, seeds / seed_off (= rows of pidx, patches_n and fine), merged / merged_off,
    sel / out_off.
    merge: how the merged patch points of a cloud are thinned to final_ratio * n_c.  "fps" (the default) is the reference's exact FPS,
    out_nums dependent rounds.  "poisson" replaces that one stage by poisson_cells.select(merged segments, out_nums,
    poisson_cells.spacing_r_hi(inputs, final_ratio), shuffle_seed=merge_seed): a blue-noise set of exactly as many points in about ten
    parallel rounds per radius, no longer the reference's output; the rows keep the merged cloud's order, and the stages gain
    merge_r (the radius per cloud), merge_count (the points kept at it) and merge_r_hi (the start of the bisection)."""
    if merge not in ("fps", "poisson"):
        raise ValueError("merge must be 'fps' or 'poisson', got %r" % (merge,))
    clouds = list(clouds)
    if not clouds:
        raise ValueError("upsample_ragged needs at least one cloud")
    for i, c in enumerate(clouds):
        shape = tuple(c.shape) if hasattr(c, "shape") else np.shape(c)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("cloud %d: expected an [n, 3] array, got shape %s" % (i, shape))
        if shape[0] < patch_num_point:
            raise ValueError("cloud %d has %d points, fewer than patch_num_point = %d" % (i, shape[0], patch_num_point))
        if int(shape[0] / patch_num_point * patch_num_ratio) < 1:
            raise ValueError("cloud %d: %d points give no patch seed at patch_num_ratio = %g" % (i, shape[0], patch_num_ratio))
    dev = gen.device
    sizes = [int(c.shape[0]) for c in clouds]
    seed_nums = [int(n / patch_num_point * patch_num_ratio) for n in sizes]    # model.py:318, evaluated as upsample_clouds does
    out_nums = [int(n * final_ratio) for n in sizes]                            # model.py:359
    per_patch = patch_num_point * gen.up_ratio ** round(math.pow(final_ratio, 1.0 / 4))          # generator_chain's output rows
    off, soff, ooff = segment_offsets(sizes), segment_offsets(seed_nums), segment_offsets(out_nums)
    moff = segment_offsets([s * per_patch for s in seed_nums])                  # cloud c's patches: its merged segment
    if all(not isinstance(c, torch.Tensor) for c in clouds):
        cloud = torch.from_numpy(np.concatenate([np.asarray(c, np.float32) for c in clouds])).to(dev)
    else:
        cloud = torch.cat([torch.as_tensor(c if isinstance(c, torch.Tensor) else np.ascontiguousarray(c, np.float32), dtype=torch.float32,
                                           device=dev) for c in clouds])
    cloud = cloud.contiguous()
    # the segment base of every seed row (local indices -> rows of the packed cloud) and the cloud of every patch
    sbase = to_device(np.repeat(off[:-1], seed_nums), dev)
    pcloud = to_device(np.repeat(np.arange(len(sizes)), seed_nums), dev)

    cloud_n, c0, f0 = normalize_segments(cloud, off)                            # model.py:364
    seeds = fps_segments(cloud_n, off, soff)                                     # model.py:323
    seed_xyz = _gather_rows(cloud_n, seeds + sbase)
    pidx = knn_patch_segments(cloud_n, off, seed_xyz, soff, patch_num_point)     # pc_util.extract_knn_patch
    patches = _gather_rows(cloud_n, (pidx + sbase[:, None]).reshape(-1)).reshape(-1, patch_num_point, 3)
    pn, pc_c, pc_f = normalize_patches(patches)                                  # model.py:306-308
    coarse, fine = generator_chain(gen, pn, final_ratio)
    pred = denormalize_patches(fine, pc_c, pc_f)                                 # model.py:310
    merged = denormalize_patches(pred, c0[pcloud].contiguous(), f0[pcloud].contiguous()).reshape(-1, 3)   # model.py:371-372
    extra = {}
    if merge == "fps":
        sel = fps_segments(merged, moff, ooff)                                   # model.py:375
    else:
        from . import poisson_cells
        r_hi = poisson_cells.spacing_r_hi([cloud[off[c]:off[c + 1]] for c in range(len(sizes))], final_ratio)
        idx, r, count = poisson_cells.select([merged[moff[c]:moff[c + 1]] for c in range(len(sizes))], out_nums, r_hi,
                                             shuffle_seed=merge_seed)
        sel = torch.cat(idx)
        extra = dict(merge_r=torch.stack(r), merge_count=torch.stack(count), merge_r_hi=r_hi)
    result = _gather_rows(merged, sel + to_device(np.repeat(moff[:-1], out_nums), dev)).cpu().numpy()
    outs = [result[ooff[c]:ooff[c + 1]] for c in range(len(sizes))]
    if return_stages:
        return outs, dict(cloud_n=cloud_n, off=off, seeds=seeds, seed_off=soff, pidx=pidx, patches_n=pn, fine=fine, merged=merged,
                          merged_off=moff, sel=sel, out_off=ooff, **extra)
    return outs


def upsample_cloud(gen, pc, patch_num_point=256, patch_num_ratio=3, final_ratio=4, return_stages=False):
    """pc: [N,3] float32 (numpy or device tensor) -> upsampled [final_ratio*N, 3] numpy array (model.py:343-381).
    `gen` is a dispu_amd.generator.Generator with up_ratio 4 (final_ratio 4: one generator pass, model.py:117-118)."""
    cloud = pc if isinstance(pc, torch.Tensor) else np.ascontiguousarray(pc, np.float32)
    res = upsample_clouds(gen, cloud.reshape(1, -1, 3), patch_num_point, patch_num_ratio, final_ratio, return_stages)
    if return_stages:
        return res[0][0].cpu().numpy(), res[1]
    return res[0].cpu().numpy()


def save_xyz(path, points):
    """np.savetxt(path, pred_pc, fmt='%.6f') (model.py:381)."""
    np.savetxt(path, points, fmt="%.6f")
