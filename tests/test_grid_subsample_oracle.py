"""CPU tests of grid subsampling: the numpy oracle (tests/grid_subsample_oracle.py) against outputs recorded from the reference's own
grid_subsampling (tests/golden/grid_subsample_ref.npz), the two rules the reference leaves open, and everything
dispu_amd.grid_subsampling.compute and tools/upsample.py --grid_size decide before a device is touched.

The golden file: four clouds (unit: 2000 points in [0,1]^3 at dl 0.25, tens of points per voxel; faces: negative coordinates, points
exactly on voxel faces, duplicates; fine: a thin slab at dl 0.013; below_origin: the doubly rounded origin lies above the minimum, so
some points get cell -1 on x), each with 3 feature columns and 1 label column that is a function of the voxel (no count ties).  The
outputs are those of the reference's function compiled with a small main, rows sorted by voxel key."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import grid_subsample_oracle as O  # noqa: E402

CLOUDS = ("unit", "faces", "fine", "below_origin")
f32 = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "grid_subsample_ref.npz"))


@pytest.mark.parametrize("name", CLOUDS)
def test_oracle_reproduces_the_reference_bit_for_bit(golden, name):
    g = {k: golden[name + "_" + k] for k in ("points", "features", "classes", "dl", "out_points", "out_features", "out_classes")}
    p, f, c = O.compute(g["points"], g["features"], g["classes"], g["dl"])
    assert same_bits(p, g["out_points"])
    assert same_bits(f, g["out_features"])
    assert same_bits(c, g["out_classes"])
    assert np.all(np.diff(np.unique(O.keys(g["points"], g["dl"]))) > 0) and len(p) == len(np.unique(O.keys(g["points"], g["dl"])))


def test_golden_covers_what_it_claims(golden):
    k = O.keys(golden["unit_points"], golden["unit_dl"])
    assert np.bincount(k - k.min()).max() >= 30                              # tens of points per voxel
    assert golden["faces_points"].min() < 0
    origin, N = O.grid(golden["below_origin_points"], golden["below_origin_dl"])
    assert origin[0] > golden["below_origin_points"][:, 0].min()             # the case the signed key exists for
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "grid_subsample_ref.npz")) < 256 * 1024


def test_label_tie_goes_to_the_smallest_signed_label():
    p = np.zeros((6, 3), f32) + f32(0.5)
    c = np.array([[3, 7], [-2, 7], [3, -9], [-2, 0], [5, 0], [5, -9]], np.int32)     # column 0: 3, -2, 5 twice each; column 1: 7, -9, 0
    _, _, out = O.compute(p, None, c, 1.0)
    assert out.tolist() == [[-2, -9]]
    c1 = np.array([4, 4, 1, 1, 1, 9], np.int32)                                      # no tie: the majority wins, not the smallest
    assert O.compute(p, None, c1, 1.0)[2].tolist() == [[1]]


def test_rows_come_in_ascending_key_order_and_sums_in_point_order():
    p = np.array([[2.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [2.25, 0.75, 0.25], [0.25, 0.25, 0.75]], f32)
    f = np.array([[1e8], [1.0], [2.0], [-1e8], [3.0]], f32)
    op, of, _ = O.compute(p, f, None, 1.0)
    assert O.keys(p, 1.0).tolist() == [2, 0, 3, 2, 0]
    assert op.tolist() == [[0.375, 0.375, 0.625], [2.375, 0.625, 0.375], [0.5, 1.5, 0.5]]
    assert of.tolist() == [[2.0], [0.0], [2.0]]
    big = np.array([[0.5, 0.5, 0.5]] * 3, f32)
    fo = np.array([[1.0], [1e8], [-1e8]], f32)                              # ((0 + 1) + 1e8) - 1e8 = 0 in float32: the order is the index order
    assert O.compute(big, fo, None, 1.0)[1].tolist() == [[0.0]]


def test_origin_and_grid_size_with_negative_coordinates():
    p = np.array([[-1.25, -0.1, 0.0], [0.3, 2.05, -0.74], [-0.6, 0.0, 0.26]], f32)
    origin, N = O.grid(p, 0.5)
    assert origin.tolist() == [-1.5, -0.5, -1.0]
    assert N == [4, 6, 3]
    assert O.keys(p, 0.5).tolist() == [0 + 4 * 0 + 24 * 2, 3 + 4 * 5 + 24 * 0, 1 + 4 * 1 + 24 * 2]
    dl = f32(0.1)
    origin, N = O.grid(p, dl)                                               # every step in float32
    inv = f32(1.0) / dl
    assert origin[0] == f32(np.floor(f32(f32(-1.25) * inv))) * dl
    assert N[0] == int(np.floor(f32(f32(f32(0.3) - origin[0]) / dl))) + 1 and N[1] == int(np.floor(f32(f32(f32(2.05) - origin[1]) / dl))) + 1


# ---- the vectorised oracle and the wide grids of tests/test_grid_subsample_gpu.py (imported for its case builders only) -----------------
def _same(a, b):
    return all((x is None and y is None) or same_bits(x, y) for x, y in zip(a, b))


def test_fast_oracle_equals_the_sequential_one_on_every_gpu_case():
    import test_grid_subsample_gpu as T
    for n in T.SIZES:
        for grid in sorted(T.GRIDS):
            p, f, c, dl = T.make_cloud(n, grid)
            assert _same(O.compute_fast(p, f, c, dl), O.compute(p, f, c, dl)), (n, grid)
    for n in (1, T.TILE + 1, 2 * T.TILE + 1):
        for pattern in ("one_cell", "own_cell", "straddle"):
            p, f, c, dl = T.edge_cloud(n, pattern)
            assert _same(O.compute_fast(p, f, c, dl), O.compute(p, f, c, dl)), (n, pattern)
    p, f, c, dl = T.make_cloud(T.TILE, "dense")
    assert _same(O.compute_fast(p, None, None, dl), O.compute(p, None, None, dl))
    assert _same(O.compute_fast(p, None, c[:, 0], dl), O.compute(p, None, c[:, 0], dl))
    # forced label ties, negative labels, a lone -0.0 and sums whose order shows
    p = np.zeros((8, 3), f32) + f32(0.25)
    p[4:] += f32(1.0)
    c = np.array([[5, -7], [-1, -7], [5, 3], [-1, 3], [2 ** 31 - 1, 0], [-2 ** 31, 0], [9, 1], [9, 2]], np.int32)
    assert O.compute_fast(p, None, c, 1.0)[2].tolist() == [[-1, -7], [9, 0]] and _same(O.compute_fast(p, None, c, 1.0), O.compute(p, None, c, 1.0))
    p6 = np.zeros((6, 3), f32) + f32(0.5)
    c6 = np.array([[3, 7], [-2, 7], [3, -9], [-2, 0], [5, 0], [5, -9]], np.int32)
    assert O.compute_fast(p6, None, c6, 1.0)[2].tolist() == [[-2, -9]]
    big = np.array([[0.5, 0.5, 0.5]] * 3 + [[1.5, 0.5, 0.5]], f32)
    fo = np.array([[1.0], [1e8], [-1e8], [-0.0]], f32)
    assert O.compute_fast(big, fo, None, 1.0)[1].tolist() == [[0.0], [0.0]] and _same(O.compute_fast(big, fo, None, 1.0), O.compute(big, fo, None, 1.0))
    assert _same(O.compute_fast(big[:3], fo[:3], None, 1.0), O.compute(big[:3], fo[:3], None, 1.0))      # the single-voxel branch


def test_the_wide_grids_have_the_passes_they_claim():
    import test_grid_subsample_gpu as T
    assert sorted(w[3] for w in T.WIDE.values()) == [2, 4, 5, 6, 7, 8]
    for name, (_, cells, axis, want) in T.WIDE.items():
        p, f, c, dl = T.wide_cloud(name)
        origin, N = O.grid(p, dl)
        assert O.passes(p, dl) == want, name
        below = np.floor((p[:, axis] - origin[axis]).astype(f32) / dl) == -1
        assert origin[axis] > p[:, axis].min() and below.sum() == 3 and O.keys(p, dl).min() < 0, name
        assert all(abs(N[a] - cells[a]) <= 2 for a in range(3)) and max(N) <= 1 << 20, (name, N)
        k = O.keys(p, dl)
        assert (np.bincount(np.unique(k, return_inverse=True)[1]) > 1).any()    # voxels of several points
        far = np.abs(p).max()
        assert np.nextafter(far, f32(np.inf)) - far <= dl / f32(6), name          # float32 still resolves dl at the far end
    p, f, c, dl = T.wide_cloud("eight")
    N = O.grid(p, dl)[1]
    assert N[0] * N[1] > 1 << 39 and N[0] * N[1] * N[2] > 1 << 59                  # NX NY iz far above 2^32
    for n, grid in T.BIG:                                                          # and what the large cases claim
        if grid == "four":
            assert 3.4 < n / (4.0 / float(T.four_dl(n))) ** 3 < 4.6


def test_the_large_grids_depend_on_every_trip_of_the_bounds_loop():
    """origin or N of the "four" cases changes when the points of the last trip are left out, and again without the last two"""
    import test_grid_subsample_gpu as T

    def grid(p, dl):
        origin, N = O.grid(p, dl)
        return origin.tolist(), N

    for n, name in T.BIG:
        p, f, c, dl = T.big_cloud(n, name)
        trips = -(-n // T.STRIDE)
        assert trips == (2 if n == T.STRIDE + 1 else 3)
        seen = [grid(p[:t * T.STRIDE], dl) for t in range(1, trips)] + [grid(p, dl)]
        if name == "one":
            assert all(g == ([0.0, 0.0, 0.0], [1, 1, 1]) for g in seen)            # one cell whatever is left out: nothing to plant
            continue
        for a, b in zip(seen, seen[1:]):
            assert a[0] != b[0] and a[1] != b[1], (n, a, b)                        # another origin AND another grid size per trip
        assert O.passes(p, dl) == 3


# ---- compute(): everything refused before the device is touched ------------------------------------------------------------------------
def _compute(*a, **k):
    import dispu_amd  # noqa: F401
    from dispu_amd import grid_subsampling as G
    return G.compute(*a, **k)


P = np.zeros((4, 3), f32)


@pytest.mark.parametrize("args, kwargs, match", [
    ((np.zeros((4, 2), f32),), {}, r"points.shape is not \(N, 3\)"),
    ((np.zeros((4, 3, 1), f32),), {}, r"points.shape is not \(N, 3\)"),
    ((np.zeros(12, f32),), {}, r"points.shape is not \(N, 3\)"),
    ((np.zeros((0, 3), f32),), {}, "must not be empty"),
    ((P,), {"features": np.zeros(4, f32)}, r"features.shape is not \(N, d\)"),
    ((P,), {"features": np.zeros((5, 2), f32)}, r"features.shape is not \(N, d\)"),
    ((P,), {"classes": np.zeros((4, 1, 1), np.int32)}, r"classes.shape is not \(N,\) or \(N, d\)"),
    ((P,), {"classes": np.zeros(3, np.int32)}, r"classes.shape is not \(N,\) or \(N, d\)"),
    ((P,), {"classes": np.zeros((5, 2), np.int32)}, r"classes.shape is not \(N,\) or \(N, d\)"),
    ((P,), {"sampleDl": 0.0}, "sampleDl"),
    ((P,), {"sampleDl": -0.1}, "sampleDl"),
    ((P,), {"sampleDl": float("nan")}, "sampleDl"),
    ((P,), {"sampleDl": float("inf")}, "sampleDl"),
    ((P,), {"sampleDl": 1e-60}, "sampleDl"),
    ((P,), {"sampleDl": 1e60}, "sampleDl"),
    ((P,), {"method": "centers"}, "Valid method names"),
])
def test_compute_refuses_before_the_device_is_touched(args, kwargs, match, monkeypatch):
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("the library was loaded for a call that must be refused first")
    monkeypatch.setattr(_lib, "lib", no_device)
    with pytest.raises(ValueError, match=match):
        _compute(*args, **kwargs)


def test_too_many_points_is_a_status_before_anything_is_touched():
    """n >= 2^31 is refused by the C entry itself, as a status value, with no pointer read (the library loads without a device)"""
    import ctypes as C
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib, grid_subsampling as G
    L = _lib.lib()
    m, status = C.c_int(-1), C.c_int(-1)
    assert L.dispu_grid_subsample_plan(1 << 31, None, 0.1, None, 0, C.byref(m), C.byref(status), None, None) == 0
    assert (m.value, status.value) == (0, _lib.GRID_TOO_MANY_POINTS)
    with pytest.raises(ValueError, match="2\\^31"):
        G._raise_on_status(status.value, 0.1, None)
    for st, word in ((_lib.GRID_NONFINITE, "NaN or infinite"), (_lib.GRID_AXIS_X, "the x axis"), (_lib.GRID_AXIS_Y, "the y axis"),
                     (_lib.GRID_AXIS_Z, "the z axis .* larger sampleDl")):
        with pytest.raises(ValueError, match=word):
            G._raise_on_status(st, 0.1, None)
    assert L.dispu_grid_subsample_scratch_bytes(1 << 31, 0, 0) == 0 and L.dispu_grid_subsample_scratch_bytes(0, 0, 0) == 0
    n = 5000                                              # keys, payload (two each), order, voxel ids, starts, table, scan sums, bounds
    assert 36 * n < L.dispu_grid_subsample_scratch_bytes(n, 3, 1) < 40 * n + (1 << 16)
    assert L.dispu_grid_subsample_scratch_bytes(n, 0, 0) == L.dispu_grid_subsample_scratch_bytes(n, 5, 2)


def test_compute_signature_mirrors_the_wrapper():
    import inspect
    import dispu_amd  # noqa: F401
    from dispu_amd import grid_subsampling as G
    sig = inspect.signature(G.compute)
    assert list(sig.parameters) == ["points", "features", "classes", "sampleDl", "method", "verbose"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, None, 0.1, "barycenters", 0]
    assert G.METHODS == ("barycenters", "voxelcenters")


def test_upsample_tool_lists_grid_size_and_it_is_off_by_default():
    tool = os.path.join(ROOT, "tools", "upsample.py")
    out = subprocess.run([sys.executable, tool, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    assert "--grid_size" in out
    import importlib.util
    spec = importlib.util.spec_from_file_location("upsample_tool_for_grid", tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args([]).grid_size is None
    assert mod.parse_args(["--grid_size", "0.02"]).grid_size == 0.02
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            mod.parse_args(["--grid_size", bad])
