"""tests/ops_rows_oracle.py held to the existing float32 oracle and the reference's golden vectors, its restated launch constants held
to the .hip sources, and its case tables held to what tests/test_ops_rows_gpu.py needs of them.  CPU only.

  * the float64 references equal oracle.oracle after rounding to float32 (forward) or within T * 2^-24 * S (gradients: the oracle
    sums T float32 terms in index order; nn_distance_grad, whose terms are formed with two roundings each, within
    (T + 1) * 2^-24 * S), and agree with tests/golden/ref_grouping.npz / ref_interpolate.npz;
  * every path of the row movers and of the grid-stride gradients that the GPU module claims to run is taken by a named case;
  * on every "exact data" gradient case the reference is a float32 number and no partial sum, in any order, can round: bit equality
    is then a fair demand on kernels that add with float atomics."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ops_rows_oracle as RO  # noqa: E402
from ops_rows_oracle import F32, F64, U  # noqa: E402

from oracle import oracle as O  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dis-pu_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def within_sum_bound(got32, ref):
    g, T, S = ref
    return bool((np.abs(got32.astype(F64) - g) <= T * U * S).all())


# --------------------------------------------------------------------------------------------- against the existing oracle ----
SMALL = [(1, 1, 1, 1), (2, 19, 5, 33), (3, 64, 12, 100), (2, 37, 130, 7)]        # b, n points, c, rows per cloud


@pytest.mark.parametrize("b,n,c,rows", SMALL)
def test_gather_references_equal_the_oracle(b, n, c, rows):
    rng = np.random.default_rng(rows)
    pts = rng.standard_normal((b, n, c)).astype(F32)
    idx = rng.integers(0, n, (b, rows, 3)).astype(np.int32)
    assert np.array_equal(RO.gather_rows(pts, idx).astype(F32), O.group_point(pts, idx))
    go = rng.standard_normal((b, rows, 3, c)).astype(F32)
    assert within_sum_bound(O.group_point_grad(pts, idx, go), RO.group_point_grad(idx, go, n))
    xyz, i2 = np.ascontiguousarray(pts[:, :, :1].repeat(3, 2)) + F32(1.5), np.ascontiguousarray(idx[:, :, 0])
    assert np.array_equal(RO.gather_rows(xyz, i2).astype(F32), O.gather_point(xyz, i2))
    og = rng.standard_normal((b, rows, 3)).astype(F32)
    assert within_sum_bound(O.gather_point_grad(xyz, i2, og), RO.gather_point_grad(i2, og, n))


@pytest.mark.parametrize("b,m,c,n", SMALL)
def test_interpolate_references_equal_the_oracle(b, m, c, n):
    rng = np.random.default_rng(n)
    pts = rng.standard_normal((b, m, c)).astype(F32)
    idx = rng.integers(0, m, (b, n, 3)).astype(np.int32)
    w = rng.random((b, n, 3)).astype(F32)
    replay = RO.three_interpolate_f32(pts, idx, w)
    assert replay.dtype == F32 and np.array_equal(replay, O.three_interpolate(pts, idx, w))
    # three products and two sums, each rounded once: within 3 * 2^-24 of the absolute terms' sum (first order, the sums' share)
    S = (np.abs(RO.gather_rows(pts, idx)) * w.astype(F64)[..., None]).sum(axis=2)
    assert (np.abs(replay - RO.three_interpolate(pts, idx, w)) <= 3 * U * S).all()
    go = rng.standard_normal((b, n, c)).astype(F32)
    # T - 1 rounded additions (the first lands on zero), and the T rounded products together add at most 2^-24 * S: T in all
    assert within_sum_bound(O.three_interpolate_grad(pts, idx, w, go), RO.three_interpolate_grad(idx, w, go, m))


@pytest.mark.parametrize("b,n,m", [(1, 1, 1), (2, 5, 1), (3, 40, 77), (2, 100, 30)])
def test_nn_distance_grad_reference_equals_the_oracle(b, n, m):
    rng = np.random.default_rng(n + m)
    x1, x2 = rng.standard_normal((b, n, 3)).astype(F32), rng.standard_normal((b, m, 3)).astype(F32)
    gd1, gd2 = rng.standard_normal((b, n)).astype(F32), rng.standard_normal((b, m)).astype(F32)
    i1, i2 = rng.integers(0, m, (b, n)).astype(np.int32), rng.integers(0, n, (b, m)).astype(np.int32)
    want = O.nn_distance_grad(x1, x2, gd1, i1, gd2, i2)
    # a term v = (2 * gd) * (from - to) is formed with two roundings, the difference and the product (2 * gd is exact): at most
    # 2 * 2^-24 * |v| each, 2 * 2^-24 * S per element; the in-order sum from zero adds T - 1 roundings: (T + 1) * 2^-24 * S.
    # T * 2^-24 * S is too small here: a point with a single term already carries both of that term's roundings.
    for got, (g, T, S) in zip(want, RO.nn_distance_grad(x1, x2, gd1, i1, gd2, i2)):
        assert (np.abs(got.astype(F64) - g) <= (T + 1) * U * S).all()
    # the true arg-mins: every xyz1 point carries its own term
    _, a1, _, a2 = O.nn_distance(x1, x2)
    (g1, T1, S1), (g2, T2, S2) = RO.nn_distance_grad(x1, x2, gd1, a1, gd2, a2)
    assert (T1 >= 1).all() and (T2 >= 1).all() and T1.sum() == T2.sum() == 3 * b * (n + m)


def test_references_equal_the_reference_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_grouping.npz"))
    assert np.array_equal(RO.gather_rows(z["points"], z["idx"]).astype(F32), z["out"])
    assert within_sum_bound(z["grad_points"], RO.group_point_grad(z["idx"], z["grad_out"], z["points"].shape[1]))
    z = np.load(os.path.join(golden_dir, "ref_interpolate.npz"))
    assert np.array_equal(RO.three_interpolate_f32(z["points"], z["idx"], z["weight"]), z["out"])
    assert within_sum_bound(z["grad_points"], RO.three_interpolate_grad(z["idx"], z["weight"], z["grad_out"], z["points"].shape[1]))


def test_term_counts_and_absolute_sums():
    idx = np.array([[[0, 0, 2], [2, 2, 2]]], np.int32)                       # [1, 2, 3] into 4 points
    go = np.array([[[[1, -2]], [[3, 4]], [[-5, 6]]], [[[7, 8]], [[-9, 10]], [[11, -12]]]], F32).reshape(1, 2, 3, 2)
    g, T, S = RO.group_point_grad(idx, go, 4)
    assert g[0].tolist() == [[4, 2], [0, 0], [4, 12], [0, 0]] and T[0].tolist() == [[2, 2], [0, 0], [4, 4], [0, 0]]
    assert S[0].tolist() == [[4, 6], [0, 0], [32, 36], [0, 0]]
    w = np.array([[[0.5, 0.25, 0.25]]], F32)
    g, T, S = RO.three_interpolate_grad(np.array([[[1, 1, 0]]], np.int32), w, np.array([[[-4.0]]], F32), 2)
    assert g.ravel().tolist() == [-1.0, -3.0] and T.ravel().tolist() == [1, 2] and S.ravel().tolist() == [1.0, 3.0]


# ----------------------------------------------------------------------------------------------- the restated launch constants ----
def test_restated_constants_are_the_sources():
    grouping, interp, sampling, nnd = src("grouping.hip"), src("interpolate.hip"), src("sampling.hip"), src("nndistance.hip")
    cap = lambda text: [int(v) for v in re.findall(r"if \(g > (\d+)\) g = \1;", text)]
    assert cap(grouping) == [RO.GRID_CAP["group_point_grad"]] and cap(interp) == [RO.GRID_CAP["three_interpolate_grad"]]
    assert cap(sampling) == [RO.GRID_CAP["gather_point_grad"]]
    for text, kernel in ((grouping, "group_point_grad_kernel"), (interp, "three_interpolate_grad_kernel"), (sampling, "gather_point_grad_kernel")):
        assert re.search(kernel + r", dim3\(grid_for\(total, %d\)\), dim3\(%d\)" % (RO.GRID_BS, RO.GRID_BS), text)
    launcher = grouping[grouping.index("int launch_gather_rows"):grouping.index("DISPU_EXPORT int dispu_group_point(")]
    assert [int(v) for v in re.findall(r"constexpr int R = (\d+);", launcher)] == [RO.XYZ_R, RO.ROWS_R["group_rows_kernel"]]
    entry = interp[interp.index("DISPU_EXPORT int dispu_three_interpolate("):interp.index("DISPU_EXPORT int dispu_three_interpolate_grad(")]
    assert [int(v) for v in re.findall(r"constexpr int R = (\d+);", entry)] == [RO.ROWS_R["three_interpolate_rows_kernel"]]
    for text in (launcher, entry):
        assert "(c % 4 == 0) && (((uintptr_t)points | (uintptr_t)out) % 16 == 0)" in text
        assert "while ((1 << tx_log2) < cv && tx_log2 < 6) ++tx_log2;" in text
    assert "base + 256u * R <= rows && ((uintptr_t)out % 16 == 0)" in grouping
    assert "dim3 grid((mx + 255) / 256, b, 2);" in nnd


def test_plans_at_known_shapes():
    p = RO.rows_plan("group_point", 4800, 134, 1600)
    assert (p["kernel"], p["vec"], p["tx_log2"], p["slots"], p["wg_rows"], p["workgroups"], p["column_trips"]) == ("group_rows_kernel", 1, 6, 4, 32, 150, 3)
    p = RO.rows_plan("three_interpolate", 600, 20, 300)
    assert (p["kernel"], p["vec"], p["tx_log2"], p["wg_rows"], p["workgroups"], p["partial_last"]) == ("three_interpolate_rows_kernel", 4, 3, 128, 5, True)
    assert RO.rows_plan("three_interpolate", 5, 3, 5)["kernel"] == "three_interpolate_rows_kernel"
    p = RO.rows_plan("gather_point", 2062, 3, 1031)
    assert (p["kernel"], p["full_passes"], p["tail_pass"], p["cloud_boundary_inside"]) == ("gather_xyz_kernel", 2, True, True)
    assert RO.grid_stride_plan("group_point_grad", 643200)["trips"] == 1          # the largest total of tests/test_ops_gpu.py
    assert RO.grid_stride_plan("group_point_grad", 4194304)["trips"] == 1 and RO.grid_stride_plan("group_point_grad", 4194305)["trips"] == 2
    assert RO.grid_stride_plan("gather_point_grad", 2097153)["trips"] == 2


# ------------------------------------------------------------------------------------------------------------- the case tables ----
def test_the_cases_cover_what_they_claim():
    hit = {}

    def mark(path, name):
        hit.setdefault(path, name)

    for name, k in RO.FORWARD_CASES.items():
        p = RO.forward_plan(name)
        rows = k.b * k.rpc
        if k.pattern != "random":
            mark((k.op, "pattern", k.pattern), name)
        if p["kernel"] == "gather_xyz_kernel":
            for what in ("full_passes", "tail_pass", "out_misaligned", "cloud_boundary_inside", "xcd_remap"):
                if p[what]:
                    mark(("gather_xyz_kernel", k.op, what), name)
            if p["cloud_boundary_inside"] and 1024 % k.rpc:
                mark(("gather_xyz_kernel", "boundary inside a pass, rows per cloud does not divide 1024"), name)
            mark(("gather_xyz_kernel", "rows", rows), name)
            continue
        key = (p["kernel"], "float4" if p["vec"] == 4 else "scalar")
        mark(key + ("lanes", p["lanes_class"]), name)
        mark(key + ("column trips", "one" if p["column_trips"] == 1 else "more"), name)
        mark(key + ("last workgroup", "partial" if p["partial_last"] else "full"), name)
        for what in ("cloud_boundary_inside", "xcd_remap"):
            if p[what]:
                mark(key + (what,), name)
        if p["cloud_boundary_inside"] and p["wg_rows"] % k.rpc:
            mark(key + ("boundary inside, rows per cloud does not divide the workgroup's rows",), name)
        if p["fallback"]:
            mark((p["kernel"], "fallback", p["fallback"]), name)
        for what, r in (("one row", 1), ("fewer rows than slots", p["slots"] - 1), ("one row short of a workgroup", p["wg_rows"] - 1),
                        ("one workgroup", p["wg_rows"]), ("one row over a workgroup", p["wg_rows"] + 1)):
            if rows == r:
                mark(key + (what,), name)
        if p["workgroups"] >= 3 and p["partial_last"]:
            mark(key + ("several workgroups, the last partial",), name)
        if p["column_trips"] > 1 and p["workgroups"] > 1:
            mark(key + ("more column trips beyond one workgroup",), name)
    for name, k in RO.GRAD_CASES.items():
        p = RO.grad_plan(name)
        if k.op == "nn_distance_grad":
            b, n, m = k.dims
            mark(("nn_distance_grad", "n < m" if n < m else "n > m" if n > m else "n == m"), name)
            for z, idle in ((0, "idle_workgroups_z0"), (1, "idle_workgroups_z1")):
                if p[idle]:
                    mark(("nn_distance_grad", "slice %d has a whole idle workgroup" % z), name)
            if k.pattern == "one" and min(n, m) > 1:
                mark(("nn_distance_grad", "all sources pull one target"), name)
        else:
            mark((k.op, "trips", p["trips"]), name)
            for what in ("at_cap", "one_over"):
                if p[what]:
                    mark((k.op, what), name)
            if k.data == "normal" and k.pattern == "random":
                assert p["trips"] == 1
                mark((k.op, "random data"), name)
        mark((k.op, "pattern", k.pattern, k.data), name)

    need = []
    for kernel in ("group_rows_kernel", "three_interpolate_rows_kernel"):
        for vec in ("float4", "scalar"):
            key = (kernel, vec)
            need += [key + ("lanes", c) for c in RO.LANES_CLASSES]
            need += [key + ("column trips", "one"), key + ("column trips", "more"), key + ("last workgroup", "full"),
                     key + ("last workgroup", "partial"), key + ("cloud_boundary_inside",), key + ("xcd_remap",),
                     key + ("boundary inside, rows per cloud does not divide the workgroup's rows",), key + ("one row",),
                     key + ("fewer rows than slots",), key + ("one row short of a workgroup",), key + ("one workgroup",),
                     key + ("one row over a workgroup",), key + ("several workgroups, the last partial",),
                     key + ("more column trips beyond one workgroup",)]
        need += [(kernel, "fallback", w) for w in ("points", "out", "both")]
    need += [("gather_xyz_kernel", op, what) for op in ("gather_point", "group_point") for what in ("full_passes", "tail_pass", "out_misaligned")]
    need += [("gather_xyz_kernel", "gather_point", "cloud_boundary_inside"), ("gather_xyz_kernel", "gather_point", "xcd_remap"),
             ("gather_xyz_kernel", "boundary inside a pass, rows per cloud does not divide 1024")]
    need += [("gather_xyz_kernel", "rows", r) for r in (1023, 1024, 1025)] + [("gather_xyz_kernel", "rows", 3 * m) for m in RO.XYZ_M]
    need += [(op, "pattern", pat) for op in ("group_point", "gather_point", "three_interpolate") for pat in ("one", "identity", "reversed")]
    for op in ("group_point_grad", "gather_point_grad", "three_interpolate_grad"):
        need += [(op, "trips", 1), (op, "trips", 2), (op, "at_cap"), (op, "one_over"), (op, "random data"), (op, "pattern", "perm", "normal"),
                 (op, "pattern", "random", "exact"), (op, "pattern", "one", "exact"), (op, "pattern", "half", "exact")]
    need += [("nn_distance_grad", w) for w in ("n < m", "n > m", "n == m", "slice 0 has a whole idle workgroup", "slice 1 has a whole idle workgroup",
                                               "all sources pull one target")]
    need += [("nn_distance_grad", "pattern", "random", "exact"), ("nn_distance_grad", "pattern", "one", "exact"),
             ("nn_distance_grad", "pattern", "random", "normal")]
    missing = [path for path in need if path not in hit]
    for path in need:
        if path in hit:
            print("%-110s %s" % (" / ".join(str(v) for v in path), hit[path]))
    assert not missing, "no case takes: %s" % missing
    for name in ("group-sparse", "gather-sparse", "interp-sparse"):              # the zero-fill test needs elements no index points at
        assert (RO.grad_reference(name)[1] == 0).mean() > 0.5
    # the one-point cases put thousands of atomics on one address, and n = 1 is among them
    for name in ("group-one-of-1", "gather-one-of-1", "interp-one-of-1"):
        g, T, S = RO.grad_reference(name)
        assert g.shape[1] == 1 and T.min() >= 4000


def test_forward_cases_stay_small():
    for name, k in RO.FORWARD_CASES.items():
        assert k.n <= 300 and k.b * k.rpc * k.c <= 1 << 20, name
        x = RO.forward_inputs(name)
        assert x["idx"].dtype == np.int32 and x["idx"].min() >= 0 and x["idx"].max() < k.n, name
    big = [name for name in RO.GRAD_CASES if RO.grad_inputs(name)[{"group_point_grad": "grad_out", "gather_point_grad": "out_g",
                                                                  "three_interpolate_grad": "grad_out", "nn_distance_grad": "xyz1"}[RO.GRAD_CASES[name].op]].size > 1 << 20]
    assert sorted(big) == sorted(["group-at-cap", "group-one-over-cap", "group-second-trip", "gather-at-cap", "gather-one-over-cap",
                                  "interp-at-cap", "interp-one-over-cap", "interp-second-trip"])


@pytest.mark.parametrize("name", [n for n, k in RO.GRAD_CASES.items() if k.data == "exact"])
def test_exact_data_cannot_round(name):
    k, x = RO.GRAD_CASES[name], RO.grad_inputs(name)
    whole = lambda a, grid=1.0: bool((np.asarray(a, F64) / grid == np.rint(np.asarray(a, F64) / grid)).all())
    if k.op == "nn_distance_grad":
        assert whole(x["xyz1"], 2.0 ** -6) and whole(x["xyz2"], 2.0 ** -6) and whole(x["grad_dist1"]) and whole(x["grad_dist2"])
        assert x["xyz1"].min() >= 0 and x["xyz1"].max() < 1 and x["xyz2"].min() >= 0 and x["xyz2"].max() < 1
        refs = RO.grad_reference(name)
    else:
        assert whole(x["out_g"] if k.op == "gather_point_grad" else x["grad_out"])
        if k.op == "three_interpolate_grad":
            assert np.array_equal(np.sort(x["weight"], axis=2), np.broadcast_to(np.array([0.25, 0.25, 0.5], F32), x["weight"].shape))
        refs = (RO.grad_reference(name),)
    for g, T, S in refs:
        assert RO.exact_in_any_order(g, S, RO.EXACT_GRID[k.op]), name
