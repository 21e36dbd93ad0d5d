"""Meshes -> data: Poisson-disk (blue-noise) clouds and training patches sampled from triangle meshes on the device.

The reference ships neither its training file (`PUGAN_poisson_256_poisson_1024.h5`, downloaded) nor the tools that made its test clouds
(2048-point inputs, 8192-point ground truth): both were Poisson-disk sampled from meshes upstream.  This module makes them from `.off`
meshes: area-weighted surface samples (csrc/mesh_sample.hip), then a Poisson-disk selection of exactly m of them (greedy dart throwing
in sample order with the radius found by bisection, csrc/poisson_disk.hip).  With tools/make_dataset.py the loop
meshes -> train -> upsample -> evaluate closes with nothing downloaded.  There is no reference code to match: the semantics are pinned
by the sequential float64 / numpy restatement in tests/mesh_sample_oracle.py, reproduced bit for bit (include/dispu_hip.h states them).

torch is used for device memory only.  Patches are Euclidean k-NN regions (the reference's own `extract_knn_patch` notion of a patch,
Common/pc_util.py:83-92); geodesic regions are out of scope."""
import math

import numpy as np
import torch

from . import _lib
from ._util import f32, req
from .tf_sampling import farthest_point_sample, gather_point
from .upsample import knn_patch

MAX_N = _lib.POISSON_MAX_N
KNN_PATCH_MAX_K = 4096                 # dispu_knn_patch above 8192 points, dispu_sort_rows_i32


def _mesh_tables(mesh):
    """device copies of (verts f32 [V,3], faces i32 [F,3], cum f64 [F+1]) of a mesh.Mesh, made on first use and kept on it"""
    t = getattr(mesh, "_sample_tables", None)
    if t is None:
        t = tuple(torch.from_numpy(np.ascontiguousarray(a, dt)).to(mesh.device)
                  for a, dt in ((mesh.verts, np.float32), (mesh.faces, np.int32), (mesh.cum_areas, np.float64)))
        mesh._sample_tables = t
    return t


def sample_surface(mesh, count, seed=0, return_bary=False):
    """count points on the surface of `mesh` (a mesh.Mesh), faces drawn in proportion to their areas (zero-area faces never), uniform
    inside a face -> (points [count,3] f32, face [count] i32) on the mesh's device (+ bary [count,3] f64 with return_bary).  Sample i
    is a function of (mesh, seed, i) only: the first k samples of any call are the k-sample call (include/dispu_hip.h:
    dispu_mesh_sample)."""
    count = int(count)
    req(count > 0, "sample_surface: count must be positive, got %d" % count)
    req(count < 2 ** 31, "sample_surface: count must be below 2^31")
    verts, faces, cum = _mesh_tables(mesh)
    dev = mesh.device
    points = torch.empty((count, 3), dtype=torch.float32, device=dev)
    face = torch.empty(count, dtype=torch.int32, device=dev)
    bary = torch.empty((count, 3), dtype=torch.float64, device=dev) if return_bary else None
    _lib.check(_lib.lib().dispu_mesh_sample(verts.shape[0], faces.shape[0], _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(cum), count,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(points), _lib.ptr(face), _lib.ptr(bary),
                                            _lib.stream_ptr(dev)), "dispu_mesh_sample")
    return (points, face, bary) if return_bary else (points, face)


def _clouds(points, what):
    p = f32(points, "points")
    req(p.dim() in (2, 3) and p.shape[-1] == 3, "%s: points must be of shape (n,3) or (b,n,3)" % what)
    single = p.dim() == 2
    if single:
        p = p.reshape(1, -1, 3)
    b, n, _ = p.shape
    req(b > 0 and n > 0, "%s: points must not be empty" % what)
    req(n <= MAX_N, "%s: %d points per cloud, the one-workgroup kernel takes at most DISPU_POISSON_MAX_N = %d" % (what, n, MAX_N))
    return p, single, b, n


def _radii(r, b, dev, what):
    if isinstance(r, torch.Tensor):
        r = f32(r, what).reshape(-1)
        req(r.device == dev, "%s and points live on different devices" % what)
    else:
        r = torch.from_numpy(np.full(b, r, np.float32) if np.ndim(r) == 0 else np.array(r, np.float32).reshape(-1)).to(dev)
    req(r.shape[0] == b, "%s: one radius per cloud (%d), got %d" % (what, b, r.shape[0]))
    return r


def _raise_on_status(status, what):
    """read the per-cloud status words (a blocking device-to-host copy) and raise on the first cloud that has a bit set"""
    st = status.cpu().numpy()
    if st.any():
        c = int(np.nonzero(st)[0][0])
        bits = int(st[c])
        why = []
        if bits & 1:
            why.append("did not settle in DISPU_POISSON_MAX_ROUNDS = %d rounds (a conflict chain that long: points ordered along a "
                       "line?)" % _lib.POISSON_MAX_ROUNDS)
        if bits & 2:
            why.append("fewer than m indices were written")
        if bits & ~3:
            why.append("unknown status bits 0x%x" % (bits & ~3))
        raise RuntimeError("%s: cloud %d %s" % (what, c, "; ".join(why)))


def poisson_disk_keep(points, radius):
    """Greedy dart throwing in index order: points [n,3] or [b,n,3] device f32, radius a number or one per cloud ->
    (keep u8 [n] / [b,n], count i32 [] / [b]).  keep[i] iff no kept j < i lies strictly closer than the radius (fp32, include/dispu_hip.h:
    dispu_poisson_disk_keep); a radius <= 0 keeps everything.  Raises RuntimeError if a cloud does not settle (status).
    The C entry is asynchronous on the stream; this call is not: it ends by reading the status words back, which waits for the kernel."""
    p, single, b, n = _clouds(points, "poisson_disk_keep")
    dev = p.device
    r = _radii(radius, b, dev, "radius")
    keep = torch.empty((b, n), dtype=torch.uint8, device=dev)
    count = torch.empty(b, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = L.dispu_poisson_disk_scratch_bytes(b, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.dispu_poisson_disk_keep(b, n, _lib.ptr(p), _lib.ptr(r), _lib.ptr(keep), _lib.ptr(count), _lib.ptr(scratch), nbytes,
                                         _lib.ptr(status), _lib.stream_ptr(dev)), "dispu_poisson_disk_keep")
    _raise_on_status(status, "poisson_disk_keep")
    return (keep[0], count[0]) if single else (keep, count)


def poisson_disk_select(points, m, r_hi, steps=12):
    """Exactly m points per cloud: points [n,3] or [b,n,3] device f32, r_hi a number or one per cloud (the start of the bisection; any
    value is legal, hex_radius is the natural one) -> (idx i32 [m] / [b,m] ascending, r f32 [] / [b], count i32 [] / [b]): the first m
    points the greedy keeps at the radius r the bisection ends on, count >= m of them in all (dispu_poisson_disk_select).
    Like poisson_disk_keep the call ends by reading the status words back, so it is synchronous although the C entry is not."""
    p, single, b, n = _clouds(points, "poisson_disk_select")
    m, steps = int(m), int(steps)
    req(m > 0, "poisson_disk_select: m must be positive, got %d" % m)
    req(n >= m, "poisson_disk_select: cannot select %d of %d points" % (m, n))
    req(steps >= 0, "poisson_disk_select: steps must be >= 0")
    dev = p.device
    rh = _radii(r_hi, b, dev, "r_hi")
    idx = torch.empty((b, m), dtype=torch.int32, device=dev)
    r = torch.empty(b, dtype=torch.float32, device=dev)
    count = torch.empty(b, dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = L.dispu_poisson_disk_scratch_bytes(b, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.dispu_poisson_disk_select(b, n, m, steps, _lib.ptr(p), _lib.ptr(rh), _lib.ptr(idx), _lib.ptr(r), _lib.ptr(count),
                                           _lib.ptr(scratch), nbytes, _lib.ptr(status), _lib.stream_ptr(dev)), "dispu_poisson_disk_select")
    _raise_on_status(status, "poisson_disk_select")
    return (idx[0], r[0], count[0]) if single else (idx, r, count)


def sort_rows(idx):
    """idx [b,k] device i32 (contiguous), k <= 4096: every row ascending, in place (dispu_sort_rows_i32).  Returns idx."""
    req(isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2,
        "sort_rows: idx must be a contiguous [b,k] int32 tensor on a ROCm device")
    b, k = idx.shape
    req(0 < k <= _lib.SORT_ROWS_MAX_K, "sort_rows: k must be in [1, %d], got %d" % (_lib.SORT_ROWS_MAX_K, k))
    _lib.check(_lib.lib().dispu_sort_rows_i32(b, k, _lib.ptr(idx), _lib.stream_ptr(idx.device)), "dispu_sort_rows_i32")
    return idx


def hex_radius(area, m):
    """sqrt(2 area / (sqrt(3) m)): the spacing of m points on `area` in a hexagonal lattice -- the densest packing, hence an upper bound
    of the Poisson-disk radius that keeps m points, and the natural r_hi."""
    return math.sqrt(2.0 * float(area) / (math.sqrt(3.0) * int(m)))


def poisson_disk_cloud(mesh, m, oversample=4, seed=0, steps=12):
    """m Poisson-disk points on the whole mesh: sample_surface(mesh, oversample m) candidates, poisson_disk_select with
    r_hi = hex_radius(mesh.total_area, m) -> (points [m,3] device f32 in sample order, r: the radius as a Python float)."""
    m, oversample = int(m), int(oversample)
    req(m > 0 and oversample >= 1, "poisson_disk_cloud: m must be positive and oversample >= 1")
    req(oversample * m <= MAX_N, "poisson_disk_cloud: %d x %d candidates, at most DISPU_POISSON_MAX_N = %d" % (oversample, m, MAX_N))
    cand, _ = sample_surface(mesh, oversample * m, seed)
    idx, r, _ = poisson_disk_select(cand, m, hex_radius(mesh.total_area, m), steps)
    return gather_point(cand.reshape(1, -1, 3), idx.reshape(1, -1))[0], float(r.item())


def patch_regions(mesh, patches, k, patch_fraction=0.05, seed=0):
    """The candidate regions of make_patches: D = ceil(k / patch_fraction) dense surface samples, `patches` seeds among them by the exact
    FPS, the k nearest dense samples of every seed (Euclidean) in SAMPLE order (k-NN returns them by distance; greedy dart throwing in
    that order would grow every patch from its centre, the sample order is i.i.d.).
    -> (dense [D,3] f32, seeds [patches] i32, regions [patches,k] i32 ascending), on the device."""
    patches, k = int(patches), int(k)
    req(patches > 0, "make_patches: patches must be positive")
    req(0 < k <= KNN_PATCH_MAX_K, "make_patches: oversample x gt_num = %d candidates per patch, at most %d (dispu_knn_patch)" % (k, KNN_PATCH_MAX_K))
    req(0.0 < float(patch_fraction) <= 1.0, "make_patches: patch_fraction must be in (0, 1]")
    D = int(math.ceil(k / float(patch_fraction)))
    req(patches <= D, "make_patches: %d patches from %d dense samples" % (patches, D))
    dense, _ = sample_surface(mesh, D, seed)
    d1 = dense.reshape(1, D, 3)
    seeds = farthest_point_sample(patches, d1)
    regions = knn_patch(d1, gather_point(d1, seeds), k)[0].contiguous()
    return dense, seeds[0], sort_rows(regions)


def make_patches(mesh, patches, gt_num=1024, in_num=256, oversample=4, patch_fraction=0.05, seed=0, steps=12, return_details=False):
    """`patches` training patches of one mesh -> (poisson_<in_num> [P,in_num,3], poisson_<gt_num> [P,gt_num,3]) device f32, un-normalised
    like the published PUGAN_poisson_256_poisson_1024.h5 (dataset.Fetcher / DeviceFetcher normalise).  A patch is a Euclidean k-NN region
    of k = oversample gt_num of D = ceil(k / patch_fraction) dense surface samples around an FPS seed (patch_regions; the reference's own
    extract_knn_patch notion of a patch -- geodesic regions are out of scope), Poisson-disk selected twice, to gt_num and to in_num
    points.  The dense samples are uniform, so a region's area is total_area k / D and r_hi = hex_radius of it: nothing is read back.
    return_details adds a dict (dense, seeds, regions, idx_in, idx_gt, r_in, r_gt, count_in, count_gt) for tests."""
    gt_num, in_num, oversample = int(gt_num), int(in_num), int(oversample)
    req(gt_num > 0 and in_num > 0 and oversample >= 1, "make_patches: gt_num, in_num must be positive and oversample >= 1")
    req(in_num < gt_num, "make_patches: in_num %d must be below gt_num %d" % (in_num, gt_num))
    k = oversample * gt_num
    dense, seeds, regions = patch_regions(mesh, patches, k, patch_fraction, seed)
    D = dense.shape[0]
    cand = gather_point(dense.reshape(1, D, 3), regions.reshape(1, -1)).reshape(regions.shape[0], k, 3)    # the existing gather, one cloud
    area = mesh.total_area * k / D
    out, det = [], {"dense": dense, "seeds": seeds, "regions": regions}
    for name, num in (("in", in_num), ("gt", gt_num)):
        idx, r, count = poisson_disk_select(cand, num, hex_radius(area, num), steps)
        out.append(gather_point(cand, idx))
        det.update({"idx_" + name: idx, "r_" + name: r, "count_" + name: count})
    return (out[0], out[1], det) if return_details else (out[0], out[1])
