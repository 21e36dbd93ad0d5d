"""GPU tests of dispu_amd.grid_subsampling.compute (csrc/grid_subsample.hip) against the sequential float32 numpy restatement
(tests/grid_subsample_oracle.py): points, features, classes and the row order, bit for bit.

One oracle run per (n, grid) with 5 feature and 2 label columns serves every (fdim, ldim): columns are summed and counted independently,
so the oracle of a column subset is the subset of the oracle's columns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grid_subsample_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
TILE = 2048
SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 20000)
# the cloud spans [-1.5, 2.5]^3 ("one": shifted to [0.5, 4.5]^3 so that a single cell holds it)
GRIDS = {"one": f32(1000.0),       # one voxel for the whole cloud: the zero-pass path and one serial run of n points
         "dense": f32(1.0),        # 64 voxels: ~300 points per voxel at n = 20000
         "fine": f32(0.05)}        # 80^3 = 512000 cells in range > 2^16: three passes
COLUMNS = ((0, 0), (1, 0), (3, 1), (5, 2), (0, 2))
LABELS = np.array([-2 ** 31, -3, 0, 2, 2 ** 31 - 1], np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_cloud(n, grid, dl=None):
    """points with negative coordinates, a fifth of them exactly on voxel faces of this grid, a tenth duplicated; features of mixed
    magnitude (the order of the adds shows); labels from five values including the int32 extremes, duplicates labelled differently"""
    dl = GRIDS[grid] if dl is None else f32(dl)
    rng = np.random.default_rng(n * 7 + len(grid))
    p = (rng.random((n, 3)) * 4 - 1.5).astype(f32)
    k = n // 5
    p[:k] = (np.round(p[:k] / dl) * dl).astype(f32) if grid != "one" else np.round(p[:k]).astype(f32)
    d = n // 10
    p[k:k + d] = p[rng.integers(0, n, d)]
    if grid == "one":
        p = np.clip(p + f32(2.0), f32(0.5), f32(4.5))
    f = (rng.standard_normal((n, 5)) * np.array([1, 1e-3, 1e3, 1, 30], f32)).astype(f32)
    c = LABELS[rng.integers(0, 5, (n, 2))]
    return np.ascontiguousarray(p), np.ascontiguousarray(f), np.ascontiguousarray(c), dl


_CASES = {}


def case(n, grid):
    if (n, grid) not in _CASES:
        p, f, c, dl = make_cloud(n, grid)
        _CASES[(n, grid)] = (p, f, c, dl) + O.compute(p, f, c, dl)
    return _CASES[(n, grid)]


def compute(*a, **k):
    import dispu_amd  # noqa: F401
    from dispu_amd import grid_subsampling as G
    return G.compute(*a, **k)


def test_the_cases_cover_what_they_claim():
    p, f, c, dl, op, of, oc = case(20000, "one")
    assert O.grid(p, dl)[1] == [1, 1, 1] and len(op) == 1
    p, f, c, dl, op, of, oc = case(20000, "dense")
    assert len(op) <= 125 and 20000 / len(op) > 150
    p, f, c, dl, op, of, oc = case(20000, "fine")
    N = O.grid(p, dl)[1]
    assert N[0] * N[1] * N[2] > 1 << 16 and N[0] * N[1] * N[2] <= 1 << 24
    k = O.keys(p, dl)
    assert (np.bincount(np.unique(k, return_inverse=True)[1]) > 1).any()          # duplicates share voxels even on the fine grid
    assert p.min() < 0


@pytest.mark.parametrize("fdim, ldim", COLUMNS)
@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("n", SIZES)
def test_compute_matches_the_oracle_bit_for_bit(dev, n, grid, fdim, ldim):
    p, f, c, dl, op, of, oc = case(n, grid)
    kw = {}
    if fdim:
        kw["features"] = np.ascontiguousarray(f[:, :fdim])
    if ldim:
        kw["classes"] = np.ascontiguousarray(c[:, :ldim])
    out = compute(p, sampleDl=dl, **kw)
    out = list(out) if isinstance(out, tuple) else [out]
    assert len(out) == 1 + (fdim > 0) + (ldim > 0)
    assert same_bits(out[0], op), "points (or the row order)"
    if fdim:
        assert same_bits(out[1], of[:, :fdim]), "features"
    if ldim:
        assert same_bits(out[-1], oc[:, :ldim]), "classes"


def edge_cloud(n, pattern):
    """unit cells, one point per sorted position j (shuffled on input): "one_cell" puts all of them into one cell (no sorting pass, the
    run heads come from the null-keys branch), "own_cell" each into its own (n runs of one), "straddle" gives the positions within 5 of
    a multiple of the sorter's tile one cell per multiple, so that a run starts in one tile and ends in the next (below TILE + 1 points:
    a run of several points at either end of the array)"""
    rng = np.random.default_rng(n * 3 + len(pattern))
    j = np.arange(n)
    if pattern == "one_cell":
        cell = np.zeros((n, 3), np.int64)
    elif pattern == "own_cell":
        cell = np.stack([j % 17, (j // 17) % 17, j // 289], axis=1)
    else:
        r = j % TILE
        x = np.where(r >= TILE - 5, (j // TILE + 1) * TILE, np.where(r < 5, j - r, j))
        cell = np.stack([x, 0 * x, 0 * x], axis=1)
    p = (cell + 0.5 + (rng.random((n, 3)) - 0.5) * 0.5).astype(f32)                # inside the cell, away from its faces
    order = rng.permutation(n)
    f = (rng.standard_normal((n, 2)) * np.array([1, 1e3], f32)).astype(f32)
    c = LABELS[rng.integers(0, 5, (n, 1))]
    return np.ascontiguousarray(p[order]), f, c, f32(1.0)


@pytest.mark.parametrize("pattern", ("one_cell", "own_cell", "straddle"))
@pytest.mark.parametrize("n", (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1))
def test_run_numbering_at_its_edges(dev, n, pattern):
    p, f, c, dl = edge_cloud(n, pattern)
    ks = np.sort(O.keys(p, dl))
    runs = 1 + int(np.count_nonzero(np.diff(ks)))
    if pattern == "one_cell":
        assert O.grid(p, dl)[1] == [1, 1, 1] and runs == 1
    elif pattern == "own_cell":
        assert runs == n
    else:
        assert all(ks[b - 1] == ks[b] and ks[b - 5] != ks[b - 6] for b in range(TILE, n, TILE))      # a run across every tile boundary
        assert n < 5 or (ks[0] == ks[4] and ks[n - 1] == ks[n - 2])                                  # and runs of several points at both ends
    op, of, oc = O.compute(p, f, c, dl)
    assert len(op) == runs
    pts, feats, cls = compute(p, f, c, sampleDl=dl)
    assert same_bits(pts, op), "points (or the row order)"
    assert same_bits(feats, of) and same_bits(cls, oc)


# ---- past the second trips: the sizes at which a loop runs again or a scan tier splits its work (tests/test_second_trips.py restates the
# thresholds from the sources), against the vectorised oracle, which tests/test_grid_subsample_oracle.py holds to O.compute ----------------
BIG = ((262145, "four"), (524289, "four"), (524289, "one"))


def four_dl(n):
    """about four points per voxel: the cloud fills 4^3"""
    return f32((256.0 / n) ** (1.0 / 3.0))


STRIDE = 1024 * 256                  # points per trip of the bounds kernel's stride loop (tests/test_second_trips.py)


def big_cloud(n, grid):
    """make_cloud with, on the "four" grid, the extremes that decide the grid moved into the later trips of the bounds kernel: the last
    point of the second trip (or the only one) lies a voxel and a half below the box on z and above it on x, and at 524289 points the
    one point of the third trip the same below on x and above on y.  A bounds pass that drops a trip, strides wrongly or loses the
    tail gets another origin and another N (tests/test_grid_subsample_oracle.py asserts that every prefix of whole trips does).  The
    "one" grid cannot be made to depend on its later points: every subset of a cloud inside one cell has that cell's grid."""
    p, f, c, dl = make_cloud(n, grid, four_dl(n) if grid == "four" else None)
    if grid == "four":
        below, above = f32(-1.5) - f32(1.5) * dl, f32(2.5) + f32(1.5) * dl
        j = min(n, 2 * STRIDE) - 1
        p[j, 2], p[j, 0] = below, above
        if n > 2 * STRIDE:
            p[n - 1, 0], p[n - 1, 1] = below, above
    return p, f, c, dl


def big_case(n, grid):
    if (n, grid, "big") not in _CASES:
        p, f, c, dl = big_cloud(n, grid)
        f, c = np.ascontiguousarray(f[:, :1]), np.ascontiguousarray(c[:, :1])
        _CASES[(n, grid, "big")] = (p, f, c, dl) + O.compute_fast(p, f, c, dl)
    return _CASES[(n, grid, "big")]


@pytest.mark.parametrize("n, grid", BIG)
def test_past_the_bounds_stride_and_one_scan_sum_per_thread(dev, n, grid):
    """262145 points: the bounds kernel's 1024 workgroups stride a second time, and the grid depends on what that trip sees
    (big_cloud); 524289: a third trip the grid depends on as well, and 257 tile sums in the scan of the run heads, in the
    voxel sort's table scan not yet (257 tiles), so the voxel sort, the label sort and the run numbering all run at that size; "one":
    the zero-pass path, run heads without keys, one serial run of 524289 points"""
    p, f, c, dl, op, of, oc = big_case(n, grid)
    if grid == "one":
        assert O.grid(p, dl)[1] == [1, 1, 1] and len(op) == 1 and O.passes(p, dl) == 0
    else:
        assert 3.0 < n / len(op) < 5.0 and O.passes(p, dl) == 3
    pts, feats, cls = compute(p, f, c, sampleDl=dl)
    assert same_bits(pts, op), "points (or the row order)"
    assert same_bits(feats, of) and same_bits(cls, oc)


# name: (dl, cells per axis, the axis that has points below the doubly rounded origin, sorting passes)
WIDE = {"two": (0.1, (31, 33, 29), 0, 2), "four": (0.7, (1000, 1025, 999), 2, 4), "five": (0.1, (8000, 8200, 8100), 1, 5),
        "six": (0.7, (65000, 66000, 32000), 2, 6), "seven": (0.1, (260000, 262000, 250000), 0, 7),
        "eight": (0.7, (1048000, 1048500, 1040000), 2, 8)}


def below_origin_min(dl):
    """(x0, origin): a minimum x0 whose origin floor(x0 (1 / dl)) dl, rounded twice, lies ABOVE it: points at x0 get cell -1"""
    inv = f32(1.0) / dl
    for j in range(1, 100000):
        x0 = np.nextafter(f32(-j) * dl, f32(-np.inf))
        origin = f32(np.floor(f32(x0 * inv))) * dl
        if origin > x0:
            return x0, origin
    raise AssertionError("no minimum below its rounded origin at dl = %r" % dl)


def wide_cloud(name, n=5000):
    """n points in 1500 occupied cells of a grid of up to 2^20 cells per axis (float32 still resolves a sixth of dl at its far end): the
    first and the last cell of every axis, 40 points exactly on voxel faces, 3 points below the rounded origin of one axis"""
    dl, cells, axis, _ = WIDE[name]
    dl = f32(dl)
    rng = np.random.default_rng(sum(cells))
    x0, o_axis = below_origin_min(dl)
    occupied = np.stack([rng.integers(0, cells[a], 1500) for a in range(3)], axis=1)
    occupied[0], occupied[1] = 0, np.array(cells) - 1
    cell = occupied[np.r_[0, 1, rng.integers(0, 1500, n - 2)]]
    frac = 0.1 + 0.8 * rng.random((n, 3))
    frac[np.arange(10, 50), rng.integers(0, 3, 40)] = 0.0                                     # on a face (as near as float32 comes to it)
    origin = np.zeros(3)
    origin[axis] = o_axis
    p = (origin[None, :] + (cell + frac) * np.float64(dl)).astype(f32)
    p[50] = p[0]                                                                   # one of them in the first cell of the other axes
    p[50:53, axis] = x0
    f = (rng.standard_normal((n, 2)) * np.array([1, 1e3], f32)).astype(f32)
    c = LABELS[rng.integers(0, 5, (n, 1))]
    return np.ascontiguousarray(p), f, c, dl


def plan_info(dev, p, dl):
    """(status, m, the 8 doubles dispu_grid_subsample_plan reports: origin, N, passes, key_min)"""
    import torch
    from dispu_amd import _lib
    L = _lib.lib()
    n = p.shape[0]
    tp = torch.from_numpy(p).to(dev)
    nbytes = L.dispu_grid_subsample_scratch_bytes(n, 0, 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    m, status, info = C.c_int(0), C.c_int(0), (C.c_double * 8)()
    _lib.check(L.dispu_grid_subsample_plan(n, _lib.ptr(tp), float(dl), _lib.ptr(scratch), nbytes, C.byref(m), C.byref(status), info,
                                           _lib.stream_ptr(dev)), "plan")
    return status.value, m.value, list(info)


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_grids_of_two_and_four_to_eight_passes(dev, name):
    """key ranges of 15 to 60 bits on 5000 points: the pass counts between the suite's 0, 1 and 3, products NX NY iz far above 2^32,
    and a negative key_min"""
    p, f, c, dl = wide_cloud(name)
    status, m, info = plan_info(dev, p, dl)
    op, of, oc = O.compute(p, f, c, dl)
    assert status == 0 and m == len(op) and int(info[6]) == WIDE[name][3] == O.passes(p, dl) and info[7] < 0
    pts, feats, cls = compute(p, f, c, sampleDl=dl)
    assert same_bits(pts, op), "points (or the row order)"
    assert same_bits(feats, of) and same_bits(cls, oc)


def test_one_dimensional_classes_and_empty_feature_columns(dev):
    p, f, c, dl, op, of, oc = case(TILE + 1, "dense")
    pts, feats, cls = compute(p, features=f[:, :0], classes=np.ascontiguousarray(c[:, 0]), sampleDl=dl)
    assert same_bits(pts, op) and feats.shape == (len(op), 0) and same_bits(cls, oc[:, :1])
    assert same_bits(compute(p, sampleDl=dl, method="voxelcenters"), op)           # the wrapper computes barycentres for both names


def test_forced_label_ties_and_negative_labels(dev):
    p = np.zeros((8, 3), f32) + f32(0.25)
    p[4:] += f32(1.0)
    c = np.array([[5, -7], [-1, -7], [5, 3], [-1, 3], [2 ** 31 - 1, 0], [-2 ** 31, 0], [9, 1], [9, 2]], np.int32)
    pts, cls = compute(p, classes=c, sampleDl=1.0)
    assert cls.tolist() == [[-1, -7], [9, 0]]
    assert same_bits(cls, O.compute(p, None, c, 1.0)[2])


def test_numpy_and_tensor_entries_give_the_same_bytes_twice(dev):
    import torch
    p, f, c, dl, op, of, oc = case(20000, "fine")
    a = compute(p, f, c, sampleDl=dl)
    tp, tf, tc = (torch.from_numpy(x).to(dev) for x in (p, f, c))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                                 # the tensor entry works on the current stream
        b = compute(tp, tf, tc, sampleDl=float(dl))
    side.synchronize()
    b2 = compute(tp, tf, tc, sampleDl=float(dl))
    assert all(isinstance(x, torch.Tensor) and x.device == tp.device for x in b)
    assert b[0].dtype == torch.float32 and b[1].dtype == torch.float32 and b[2].dtype == torch.int32
    for x, y, z, o in zip(a, b, b2, (op, of, oc)):
        assert same_bits(x, o) and same_bits(y.cpu().numpy(), o) and same_bits(z.cpu().numpy(), o)


@pytest.mark.parametrize("name", ("unit", "faces", "fine", "below_origin"))
def test_golden_clouds_of_the_reference(dev, golden_dir, name):
    g = np.load(os.path.join(golden_dir, "grid_subsample_ref.npz"))
    pts, feats, cls = compute(g[name + "_points"], g[name + "_features"], g[name + "_classes"], sampleDl=g[name + "_dl"])
    assert same_bits(pts, g[name + "_out_points"])
    assert same_bits(feats, g[name + "_out_features"])
    assert same_bits(cls, g[name + "_out_classes"])


def test_grid_parameters_are_the_oracles(dev):
    import torch
    from dispu_amd import _lib
    L = _lib.lib()
    for n, grid in ((20000, "fine"), (TILE - 1, "dense"), (20000, "one")):       # passes: 3, 1, 0
        p, f, c, dl, op, of, oc = case(n, grid)
        tp = torch.from_numpy(p).to(dev)
        nbytes = L.dispu_grid_subsample_scratch_bytes(n, 0, 0)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        m, status, info = C.c_int(0), C.c_int(0), (C.c_double * 8)()
        _lib.check(L.dispu_grid_subsample_plan(n, _lib.ptr(tp), float(dl), _lib.ptr(scratch), nbytes, C.byref(m), C.byref(status), info,
                                               _lib.stream_ptr(dev)), "plan")
        origin, N = O.grid(p, dl)
        assert status.value == 0 and m.value == len(op)
        assert [f32(info[i]) for i in range(3)] == origin.tolist() and [int(info[3 + i]) for i in range(3)] == N
        lo = [int(np.floor(f32(f32(p[:, a].min() - origin[a]) / dl))) for a in range(3)]      # 0, or -1 below a doubly rounded origin
        key_min = lo[0] + N[0] * lo[1] + N[0] * N[1] * lo[2]
        key_max = N[0] * N[1] * N[2] - 1
        assert int(info[7]) == key_min <= O.keys(p, dl).min() and int(info[6]) == ((key_max - key_min).bit_length() + 7) // 8


def test_refusals_leave_the_device_usable(dev):
    p, f, c, dl, op, of, oc = case(TILE + 1, "dense")
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[TILE, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            compute(q, f, c, sampleDl=dl)
    q = p.copy()
    q[:, 1] *= f32(0.25)
    q[:, 2] *= f32(0.25)                                  # x spans 4 / 1e-6 = 4e6 > 2^21 cells, y and z 1e6
    with pytest.raises(ValueError, match=r"the x axis .* 2\^21 cells .* larger sampleDl"):
        compute(q, sampleDl=1e-6)
    with pytest.raises(ValueError, match=r"the z axis .* larger sampleDl"):
        compute(np.ascontiguousarray(q[:, ::-1]), sampleDl=1e-6)
    with pytest.raises(ValueError, match=r"axis .* larger sampleDl"):
        compute(p, sampleDl=1e-30)
    out = compute(p, f, c, sampleDl=dl)
    assert same_bits(out[0], op) and same_bits(out[1], of) and same_bits(out[2], oc)


def test_upsample_tool_with_grid_size_end_to_end(dev, tmp_path):
    """tools/upsample.py --grid_size on an uneven .xyz scan with a restored checkpoint: the output is the upsampled SUBSAMPLED cloud,
    final_ratio x its count, and the printed line shows both counts"""
    import subprocess
    ROOT = os.path.dirname(HERE)
    sys.path.insert(0, ROOT)
    import dispu_amd  # noqa: F401
    from dispu_amd import checkpoint as CK, upsample as U
    from oracle import generator as OG
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    rng = np.random.default_rng(3)
    v = rng.standard_normal((6000, 3))
    v[:4000, 2] = np.abs(v[:4000, 2]) * 4                  # two thirds of the scan crowd around one pole
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    np.savetxt(str(data / "test" / "scan.xyz"), v, fmt="%.6f")
    pts = np.loadtxt(str(data / "test" / "scan.xyz"), ndmin=2).astype(f32)
    sub = compute(pts, sampleDl=0.15)
    assert 256 <= len(sub) < 3000
    _, gen = CK.restore_generator(str(log_dir), device=dev)
    want = str(tmp_path / "want.xyz")
    np.savetxt(want, U.upsample_cloud(gen, sub), fmt="%.6f")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data), "--grid_size", "0.15"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text
    got = data / "test" / "output" / "scan_X4.xyz"
    assert open(str(got), "rb").read() == open(want, "rb").read()
    assert np.loadtxt(str(got)).shape == (4 * len(sub), 3)
    assert "6000 -> %d (grid 0.15) -> %d points" % (len(sub), 4 * len(sub)) in text
