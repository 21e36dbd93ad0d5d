"""GPU tests of dispu_pca_normals_segments / dispu_amd.normals.estimate_normals (csrc/normals.hip) against tests/normals_oracle.py:
the neighbour indices bit for bit, the normals against float64 eigh of the same neighbourhoods, degenerate and refused input, the sign
rules, and tools/upsample.py --normals end to end.  Every cloud has at most 8193 points (a batch up to 65535 clouds of 1 to 3); an
oracle run is shared through lru_cache."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import normals_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue


def N(t):
    return t.detach().cpu().numpy()


def run_abi(dev, clouds, k, mode=0, orient=None, want_var=True, want_idx=True, off=None, scratch="ok", C_arg=None, scratch_buf=None):
    """the C entry on a packed batch, every output pre-filled with a sentinel -> (return code, normal, variation, idx, status).
    scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the zero-filled one"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    cloud = torch.from_numpy(np.concatenate(clouds).astype(np.float32)).to(dev)
    if off is None:
        off = np.zeros(len(clouds) + 1, np.int32)
        np.cumsum([len(c) for c in clouds], out=off[1:])
    off = np.ascontiguousarray(off, np.int32)
    nC = len(off) - 1 if C_arg is None else C_arg
    total = cloud.shape[0]
    hp = C.c_void_p(off.ctypes.data)
    nbytes = L.dispu_pca_normals_scratch_bytes(nC, hp, k)
    good = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=good[1:])
    full = L.dispu_pca_normals_scratch_bytes(len(clouds), C.c_void_p(good.ctypes.data), 16)       # what legal arguments need
    buf = torch.zeros((max(full, 16),), dtype=torch.uint8, device=dev)
    if scratch == "ok":
        sp, sb = _lib.ptr(buf), max(nbytes, full)
    elif scratch == "null":
        sp, sb = C.c_void_p(0), full
    else:                                                       # one byte short
        sp, sb = _lib.ptr(buf), full - 1
    if scratch_buf is not None:
        assert scratch in ("ok", "short"), "with scratch_buf only a right or a one-byte-short size can be asked for"
        sp, sb = scratch_buf.ptr(), scratch_buf.nbytes - (0 if scratch == "ok" else 1)
    normal = torch.full((total, 3), 7.0, dtype=torch.float32, device=dev)
    var = torch.full((total,), 7.0, dtype=torch.float32, device=dev) if want_var else None
    idx = torch.full((total, k), -7, dtype=torch.int32, device=dev) if want_idx else None
    status = torch.full((max(nC, 1) if nC <= 70000 else 1,), -7, dtype=torch.int32, device=dev)
    d_off = torch.from_numpy(off).to(dev)
    d_or = torch.from_numpy(np.ascontiguousarray(orient, np.float32)).to(dev) if orient is not None else None
    rc = L.dispu_pca_normals_segments(nC, _lib.ptr(d_off), hp, k, _lib.ptr(cloud), mode, _lib.ptr(d_or), _lib.ptr(normal), _lib.ptr(var),
                                      _lib.ptr(idx), _lib.ptr(status), sp, sb, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    if scratch_buf is not None:
        scratch_buf.inputs = dict(cloud=N(cloud), off=N(d_off))               # as the call left them
    return rc, N(normal), (N(var) if want_var else None), (N(idx) if want_idx else None), N(status)


@functools.lru_cache(maxsize=None)
def cloud(name):
    r = np.random.RandomState(0)
    if name == "sphere":
        return O.sphere(4097)
    if name == "ellipsoid":
        return O.far_ellipsoid(2049)
    if name == "plane":
        return O.noisy_plane(1500)
    if name == "lattice":
        return O.lattice(17)                                    # 4913 points, massive distance ties
    if name == "coincident":                                    # more duplicates than k, spread over the index range
        p = r.random_sample((1040, 3)).astype(np.float32)
        p[r.permutation(1040)[:40]] = np.float32([0.25, 0.5, 0.75])
        return p
    if name == "clusters":                                      # two clusters 100 apart and 5 isolated points midway
        a = (r.random_sample((2000, 3)) - 0.5).astype(np.float32)
        b = (r.random_sample((2000, 3)) - 0.5).astype(np.float32) + np.float32([100, 0, 0])
        mid = np.float32([50, 0, 0]) + (r.random_sample((5, 3)) - 0.5).astype(np.float32)
        return np.concatenate([a, mid, b])
    if name == "collinear":
        return (np.arange(200, dtype=np.float32)[:, None] * np.float32([[0.5, 0.25, -1.0]])).astype(np.float32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def neighbours32(name, n=None):
    """the oracle's neighbours at k = 32: the first k columns are the neighbours at k (rows of fewer than k points padded afresh)"""
    p = cloud(name) if n is None else cloud(name)[:n]
    return O.neighbors(p, 32)


def oracle_idx(name, k, n=None):
    idx = neighbours32(name, n)[:, :k]
    return np.ascontiguousarray(idx)


@functools.lru_cache(maxsize=None)
def oracle(name, k):
    return O.normals(cloud(name), k, idx=oracle_idx(name, k))


# ---- the search -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 16, 32])
def test_neighbours_at_every_size(dev, k):
    for n in sorted({1, 2, 3, k, k + 1, 63, 64, 65, 4097}):                     # 4097: 65 cells, so pruning is live
        rc, _, _, idx, status = run_abi(dev, [cloud("sphere")[:n]], k)
        assert rc == 0 and status[0] == 0
        assert np.array_equal(idx, oracle_idx("sphere", k, n)), (n, k)


def test_ragged_batch_equals_each_cloud_alone(dev):
    sizes = (1, 65, 4097, 3)
    clouds = [cloud("sphere")[:n] for n in sizes]
    rc, nrm, var, idx, status = run_abi(dev, clouds, 16)
    assert rc == 0 and not status.any()
    o = 0
    for n, c in zip(sizes, clouds):
        rc1, nrm1, var1, idx1, _ = run_abi(dev, [c], 16)
        assert rc1 == 0
        assert np.array_equal(idx[o:o + n], idx1) and np.array_equal(idx1, oracle_idx("sphere", 16, n))
        assert np.array_equal(nrm[o:o + n].view(np.uint32), nrm1.view(np.uint32)) and np.array_equal(var[o:o + n], var1)
        o += n


MANY = {257: (1, 63, 64, 65, 130), 65535: (1, 2, 3)}          # segments: sizes in a cycle


@pytest.mark.parametrize("nC", sorted(MANY))
def test_neighbours_with_many_segments(dev, nC):
    """9 and 16 segment bits above the 30 Morton bits of the pre-pass's keys: sorting passes 5 and 6, c << 30 with large c.  One packed
    call; the brute-force rule runs once per distinct cloud and is asserted for every repeat of it at its own offset."""
    cycle = MANY[nC]
    sizes = np.array(cycle)[np.arange(nC) % len(cycle)]
    distinct, lo = {}, 0
    for n in cycle:
        distinct[n] = cloud("sphere")[lo:lo + n]
        lo += n
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rc, _, _, idx, status = run_abi(dev, [distinct[n] for n in sizes], 4, off=off)
    assert rc == 0 and len(status) == nC and not status.any()
    for n in cycle:
        want = O.neighbors(distinct[n], 4)
        rows = off[:-1][sizes == n][:, None] + np.arange(n)[None, :]
        assert np.array_equal(idx[rows], np.broadcast_to(want[None], (rows.shape[0], n, 4))), n


@pytest.mark.parametrize("name", ["lattice", "coincident", "clusters"])
@pytest.mark.parametrize("k", [4, 16, 32])
def test_neighbours_with_ties_duplicates_and_far_cells(dev, name, k):
    """lattice: the lower index wins among equal distances; coincident: 40 equal points, more than k; clusters: the 5 points midway
    have all their neighbours in far cells, a search that stops at nearby cells fails"""
    rc, _, _, idx, status = run_abi(dev, [cloud(name)], k)
    assert rc == 0 and status[0] == 0
    want = oracle_idx(name, k)
    assert np.array_equal(idx, want), np.nonzero((idx != want).any(axis=1))[0][:10]


def test_agrees_with_knn_patch_segments(dev):
    import torch
    from dispu_amd import upsample as U
    p = torch.from_numpy(cloud("sphere")).to(dev)
    off = np.int32([0, 4097])
    ref = N(U.knn_patch_segments(p, off, p, off, 16))
    _, _, _, idx, _ = run_abi(dev, [cloud("sphere")], 16)
    assert np.array_equal(idx, ref)


# ---- the normals ------------------------------------------------------------------------------------------------------------------------

def check_against_eigh(nrm, var, ref, oriented=False):
    """the checks of one cloud; ref is the oracle's dict on the same neighbourhoods"""
    ok = ref["ok"]
    w, cov = ref["evals"], ref["cov"]
    n64 = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n64[ok], axis=1) - 1.0).max() <= 1e-6
    ray = np.einsum("ni,nij,nj->n", n64, cov, n64)
    assert (ray[ok] <= w[ok, 0] + 1e-6 * w[ok, 2]).all()
    gap = (w[:, 1] - w[:, 0]) / np.where(ok, w[:, 2], 1.0)
    sel = ok & (gap >= 1e-2)
    assert (~sel).sum() <= 0.01 * len(nrm), "the gap filter leaves out %d of %d points" % ((~sel).sum(), len(nrm))
    want = ref["normal"].astype(np.float64) if oriented else ref["evec"]
    sin_a = np.linalg.norm(np.cross(n64[sel], want[sel]), axis=1) / np.linalg.norm(n64[sel], axis=1) / np.linalg.norm(want[sel], axis=1)
    print("largest angle %.3g rad, smallest gap %.3g, largest variation error %.3g" % (
        sin_a.max(), gap[ok].min(), np.abs(var - ref["variation"]).max()))
    assert sin_a.max() <= 1e-5                                   # sin a = a to 1e-15 here
    if oriented:                                                # where the two largest components are 1e-5 apart the leading axis is decided
        top = np.sort(np.abs(want), axis=1)
        clear = sel & (top[:, 2] - top[:, 1] > 1e-5)
        assert ((n64[clear] * want[clear]).sum(axis=1) > 0).all()
    assert np.abs(var - ref["variation"]).max() <= 1e-6
    assert np.array_equal(nrm[~ok], np.zeros_like(nrm[~ok])) and (var[~ok] == -1).all()


@pytest.mark.parametrize("name", ["sphere", "ellipsoid", "plane"])
def test_normals_against_float64_eigh(dev, name):
    """ellipsoid: 1 cm of structure at coordinates of 1000 -- fp32 moments of raw coordinates would lose it all"""
    rc, nrm, var, idx, status = run_abi(dev, [cloud(name)], 16)
    assert rc == 0 and status[0] == 0
    ref = oracle(name, 16)
    assert np.array_equal(idx, ref["idx"])
    check_against_eigh(nrm, var, ref, oriented=True)            # mode 0 is an orientation too: the canonical sign


@pytest.mark.parametrize("k", [4, 32])
def test_normals_at_other_k(dev, k):
    rc, nrm, var, idx, _ = run_abi(dev, [cloud("ellipsoid")], k)
    ref = oracle("ellipsoid", k)
    assert rc == 0 and np.array_equal(idx, ref["idx"])
    ok = ref["ok"]
    n64 = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n64[ok], axis=1) - 1.0).max() <= 1e-6
    assert (np.einsum("ni,nij,nj->n", n64, ref["cov"], n64)[ok] <= ref["evals"][ok, 0] + 1e-6 * ref["evals"][ok, 2]).all()
    assert np.abs(var - ref["variation"]).max() <= 1e-6


def test_outputs_that_are_not_asked_for(dev):
    rc, nrm, var, idx, _ = run_abi(dev, [cloud("plane")], 16, want_var=False, want_idx=False)
    rc2, nrm2, _, _, _ = run_abi(dev, [cloud("plane")], 16)
    assert rc == 0 and rc2 == 0 and var is None and idx is None and np.array_equal(nrm.view(np.uint32), nrm2.view(np.uint32))


# ---- degenerate and refused input -------------------------------------------------------------------------------------------------------

def test_degenerate_segments(dev):
    two = np.float32([[0, 0, 0], [1, 2, 3]])
    same = np.tile(np.float32([[3, -1, 2]]), (100, 1))
    one = np.float32([[5, 5, 5]])
    line = cloud("collinear")
    rc, nrm, var, idx, status = run_abi(dev, [two, same, one, line], 8)
    assert rc == 0 and not status.any()
    assert not nrm[:103].any() and (var[:103] == -1).all()                      # n < 3 and all-coincident: zero normals, variation -1
    assert np.array_equal(idx[:2], np.int32([[0, 1] + [-1] * 6, [1, 0] + [-1] * 6]))
    assert np.array_equal(idx[2:102], np.tile(np.arange(8, dtype=np.int32), (100, 1)))          # equal distances: the lowest indices
    ref = O.normals(line, 8)
    assert np.array_equal(idx[103:], ref["idx"]) and ref["ok"].all()
    n64 = nrm[103:].astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1.0).max() <= 1e-6               # a collinear segment: unit vectors across the line
    assert (np.einsum("ni,nij,nj->n", n64, ref["cov"], n64) <= ref["evals"][:, 0] + 1e-6 * ref["evals"][:, 2]).all()
    assert np.abs(var[103:] - ref["variation"]).max() <= 1e-6


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_non_finite_segment_is_flagged_and_left_alone(dev, poison):
    import torch
    from dispu_amd.normals import estimate_normals
    a, b, c = cloud("sphere")[:300], cloud("plane")[:200].copy(), cloud("ellipsoid")[:129]
    b[77, 1] = poison
    rc, nrm, var, idx, status = run_abi(dev, [a, b, c], 16)
    assert rc == 0 and list(status) == [0, 1, 0]
    assert (nrm[300:500] == 7).all() and (var[300:500] == 7).all() and (idx[300:500] == -7).all()   # none of its outputs is written
    for lo, hi, p in [(0, 300, a), (500, 629, c)]:
        _, n1, v1, i1, _ = run_abi(dev, [p], 16)
        assert np.array_equal(nrm[lo:hi].view(np.uint32), n1.view(np.uint32)) and np.array_equal(var[lo:hi], v1)
        assert np.array_equal(idx[lo:hi], i1)
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):
        estimate_normals([torch.from_numpy(x).to(dev) for x in (a, b, c)])


# ---- orientation ------------------------------------------------------------------------------------------------------------------------

def leading_component_positive(nrm):
    nz = nrm.any(axis=1)
    a = np.argmax(np.abs(nrm), axis=1)                          # the first of equal maxima: ties to the lowest axis
    return (nrm[np.arange(len(nrm)), a][nz] > 0).all()


def test_mode_0_is_the_canonical_sign(dev):
    flat = cloud("plane").copy()
    flat[:, 2] = 2.0                                            # an exact plane: (0, 0, 1), never (0, 0, -1)
    _, nrm, var, _, _ = run_abi(dev, [flat, cloud("lattice")], 16)
    assert np.array_equal(nrm[:1500], np.tile(np.float32([0, 0, 1]), (1500, 1))) and not var[:1500].any()
    assert leading_component_positive(nrm[1500:]) and np.abs(np.linalg.norm(nrm[1500:].astype(np.float64), axis=1) - 1).max() <= 1e-6
    _, nrm, _, _, _ = run_abi(dev, [cloud("sphere")], 16)
    assert leading_component_positive(nrm)


def test_viewpoint_and_centroid(dev):
    import torch
    from dispu_amd.normals import estimate_normals
    sph, ell = cloud("sphere"), cloud("ellipsoid")
    pts = [torch.from_numpy(sph).to(dev), torch.from_numpy(ell).to(dev)]
    views = np.float32([[3, 0.5, -0.25], [1000, -500, 250]])                    # outside the sphere; the ellipsoid's centre
    got = [N(t) for t in estimate_normals(pts, orient=("viewpoint", views))]
    for p, v, g, name in zip((sph, ell), views, got, ("sphere", "ellipsoid")):
        ref = oracle(name, 16)
        d = v.astype(np.float64)[None] - p.astype(np.float64)
        dot_ref = (ref["normal"].astype(np.float64) * d).sum(axis=1) / np.linalg.norm(d, axis=1)
        sel = np.abs(dot_ref) > 1e-3
        assert sel.sum() > 0.9 * len(p) and ((g.astype(np.float64) * d).sum(axis=1)[sel] > 0).all()
        assert np.abs(np.abs(g) - np.abs(ref["normal"])).max() < 1e-5           # the same lines, whatever the sign
    one = N(estimate_normals(pts[0], orient=("viewpoint", [3, 0.5, -0.25])))     # one cloud, three numbers
    assert np.array_equal(one.view(np.uint32), got[0].view(np.uint32))
    out = [N(t) for t in estimate_normals(pts, orient=("centroid",))]
    for p, g, name in zip((sph, ell), out, ("sphere", "ellipsoid")):
        d = p.astype(np.float64) - p.astype(np.float64).mean(axis=0)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        sel = np.abs((oracle(name, 16)["normal"].astype(np.float64) * d).sum(axis=1)) > 1e-3
        assert sel.mean() > 0.99 and ((g.astype(np.float64) * d).sum(axis=1)[sel] > 0).all()      # outwards on a closed convex surface


def test_reference_orientation_reproduces_flips(dev):
    import torch
    from dispu_amd.normals import estimate_normals
    sph = cloud("sphere")
    flips = np.where(np.random.RandomState(5).random_sample(len(sph)) < 0.5, -1.0, 1.0).astype(np.float32)
    p = torch.from_numpy(sph).to(dev)
    ref_n = torch.from_numpy(sph * flips[:, None]).to(dev)                      # radial normals, half of them flipped
    got = N(estimate_normals(p, orient=("reference", p, ref_n)))
    radial = (got.astype(np.float64) * sph).sum(axis=1)
    assert (np.abs(radial) > 0.9).all() and np.array_equal(np.sign(radial), flips.astype(np.float64))
    lst = estimate_normals([p, p[:500]], orient=("reference", [p, p], [ref_n, ref_n]))            # lists: one pair per cloud
    assert np.array_equal(N(lst[0]).view(np.uint32), got.view(np.uint32))
    assert np.array_equal(np.sign((N(lst[1]).astype(np.float64) * sph[:500]).sum(axis=1)), flips[:500].astype(np.float64))


def test_two_calls_give_identical_bytes(dev):
    args = dict(k=16, mode=2, orient=np.float32([[0, 0, 5], [1000, -500, 250.5]]))
    a = run_abi(dev, [cloud("sphere"), cloud("ellipsoid")], **args)
    b = run_abi(dev, [cloud("sphere"), cloud("ellipsoid")], **args)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_python_entry_shapes_and_refusals(dev):
    import torch
    from dispu_amd.normals import estimate_normals
    p = torch.from_numpy(cloud("plane")).to(dev)
    nrm, var, idx = estimate_normals(p, k=8, return_variation=True, return_neighbors=True)
    assert nrm.shape == (1500, 3) and var.shape == (1500,) and idx.shape == (1500, 8) and idx.dtype == torch.int32
    assert np.array_equal(N(idx), oracle_idx("plane", 8))
    nrm2, idx2 = estimate_normals([p, p[:2]], k=8, return_neighbors=True)
    assert isinstance(nrm2, list) and np.array_equal(N(nrm2[0]), N(nrm)) and not N(nrm2[1]).any()
    assert np.array_equal(N(idx2[1]), np.int32([[0, 1] + [-1] * 6, [1, 0] + [-1] * 6]))
    for bad in (dict(k=3), dict(k=33), dict(k=16.0), dict(orient=("mst",)), dict(orient=("viewpoint", [0, 0])),
                dict(orient=("viewpoint", [0, 0, np.inf])), dict(orient=("reference", p[:5], p[:4])), dict(orient=("centroid", 1))):
        with pytest.raises(ValueError):
            estimate_normals(p, **bad)
    for bad in (p.double(), p[:, :2], p.reshape(1, -1, 3), p[:0], p.cpu()):
        with pytest.raises(ValueError):
            estimate_normals(bad)


# ---- the C ABI's refusals: nothing is touched -------------------------------------------------------------------------------------------

def untouched(res):
    _, nrm, var, idx, status = res
    return (nrm == 7).all() and (var == 7).all() and (idx == -7).all() and (status == -7).all()


def test_abi_refusals_touch_nothing(dev):
    p = [cloud("sphere")[:500], cloud("plane")[:300]]
    for kw in (dict(k=3), dict(k=33), dict(k=16, scratch="null"), dict(k=16, scratch="short"), dict(k=16, C_arg=65536),
               dict(k=16, off=np.int32([0, 500, 400])), dict(k=16, off=np.int32([0, 500, 500])), dict(k=16, off=np.int32([1, 500, 800])),
               dict(k=16, mode=3), dict(k=16, mode=1, orient=None)):
        res = run_abi(dev, p, **kw)
        assert res[0] == INVALID and untouched(res), kw
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    off = np.int32([0, 500, 800])
    hp = C.c_void_p(off.ctypes.data)
    assert L.dispu_pca_normals_scratch_bytes(2, hp, 16) > 0
    assert L.dispu_pca_normals_scratch_bytes(2, hp, 3) == 0 and L.dispu_pca_normals_scratch_bytes(2, hp, 33) == 0
    assert L.dispu_pca_normals_scratch_bytes(0, hp, 16) == 0 and L.dispu_pca_normals_scratch_bytes(65536, hp, 16) == 0
    big = np.int32([0, (1 << 24) + 1])
    assert L.dispu_pca_normals_scratch_bytes(1, C.c_void_p(big.ctypes.data), 16) == 0            # a segment above 2^24 points
    assert run_abi(dev, p, 16)[0] == 0                                                          # the same call, legal


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------

def test_upsample_tool_writes_oriented_normals(dev, tmp_path):
    from dispu_amd import checkpoint as CK
    from oracle import generator as OG
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    pc = O.sphere(2048, seed=9)
    np.savetxt(str(data / "test" / "ball.xyz"), np.concatenate([pc, pc], axis=1), fmt="%.6f")    # radial normals
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    runs = {"plain": [], "normals": ["--normals", "pca", "--orient", "input"],
            "grid": ["--normals", "pca", "--orient", "input", "--grid_size", "0.05", "--normals_k", "8"]}
    procs = {name: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for name, extra in runs.items()}
    for name, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    plain = open(str(tmp_path / "plain" / "ball_X4.xyz")).read().splitlines()
    rows = open(str(tmp_path / "normals" / "ball_X4.xyz")).read().splitlines()
    assert len(rows) == 4 * 2048 and len(plain) == 4 * 2048
    assert all(len(r.split(" ")) == 6 for r in rows)
    assert [" ".join(r.split(" ")[:3]) for r in rows] == plain                  # x y z byte-identical to a run without --normals
    nrm = np.array([[float(v) for v in r.split(" ")[3:]] for r in rows])
    # %.6f moves a component by at most 5e-7, the length of a unit vector by at most sqrt(3) * 5e-7 < 1e-6; fp32 storage adds 1e-7
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 2e-6
    # with --grid_size the input normals ride through the subsampler: four rows per barycentre, six columns, unit normals
    grid = np.loadtxt(str(tmp_path / "grid" / "ball_X4.xyz"), ndmin=2)
    assert grid.shape[1] == 6 and grid.shape[0] % 4 == 0 and 4 * 256 <= grid.shape[0] < 4 * 2048
    assert np.abs(np.linalg.norm(grid[:, 3:], axis=1) - 1.0).max() <= 2e-6
