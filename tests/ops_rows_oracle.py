"""Float64 references, a restatement of the launch arithmetic, and the case tables for the row movers and scatter gradients behind
tf_grouping / tf_sampling / tf_interpolate / tf_nndistance (tests/test_ops_rows_oracle.py on the CPU, tests/test_ops_rows_gpu.py on the
GPU).  Plain numpy: no torch, no GPU, nothing of oracle/oracle.py.

References.  gather_rows and three_interpolate are the forward ops in float64; three_interpolate_f32 is the float32 evaluation
(p0*w0 + p1*w1) + p2*w2 with every operation rounded, which is what the kernel computes.  Every gradient is a scatter-add of float64 terms
and returns (g, T, S) per output element: the sum, the number of terms that land on the element and the sum of their absolute values.
A float32 sum of T terms in ANY order differs from g by at most (T - 1) * 2^-24 * S to first order, and every rounding made while a term
itself is formed (the product g*w, or the difference and the product of nn_distance_grad) adds at most 2^-24 * |term|:
(T + 2) * 2^-24 * S bounds all of it (random_data_bound).

Dispatch.  rows_plan / grid_stride_plan / nn_grad_plan restate launch_gather_rows (csrc/grouping.hip), dispu_three_interpolate
(csrc/interpolate.hip), the three grid-stride gradients and dispu_nn_distance_grad (csrc/nndistance.hip) as arithmetic on the shape.  They
describe which path a case takes, for the coverage check; they are not a reference for values.

Cases.  FORWARD_CASES and GRAD_CASES map a name to a shape, an index pattern and a kind of data; forward_inputs / grad_inputs build the
arrays from the name alone (seeded by it) and forward_expected / grad_reference the results, computed once per process (the inputs of
the few gradient cases of tens of MB are rebuilt when asked for again, not kept)."""
import collections
import functools
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                      # unit roundoff of float32

# ------------------------------------------------------------------------------------------------------------------ references ----


def _f64(a):
    return np.asarray(a, F64)


def gather_rows(points, idx):
    """points [b, n, c], idx [b, ...] -> [b, ..., c] float64: out[i, j..., :] = points[i, idx[i, j...], :]  (group_point, gather_point)"""
    p, idx = _f64(points), np.asarray(idx)
    b = p.shape[0]
    assert idx.shape[0] == b and (idx.size == 0 or (idx.min() >= 0 and idx.max() < p.shape[1]))
    return p[np.arange(b).reshape((b,) + (1,) * (idx.ndim - 1)), idx]


def three_interpolate(points, idx, weight):
    """points [b, m, c], idx / weight [b, n, 3] -> [b, n, c] float64: the weighted sum of the three rows"""
    return (gather_rows(points, idx) * _f64(weight)[..., None]).sum(axis=2)


def three_interpolate_f32(points, idx, weight):
    """the same in float32, left to right, every product and sum rounded (numpy rounds each float32 operation)"""
    p = gather_rows(points, idx).astype(F32)
    w = np.asarray(weight, F32)[..., None]
    return (p[:, :, 0] * w[:, :, 0] + p[:, :, 1] * w[:, :, 1]) + p[:, :, 2] * w[:, :, 2]


def _scatter(keys, terms, shape):
    keys, terms = np.asarray(keys).ravel(), _f64(terms).ravel()
    size = int(np.prod(shape))
    assert keys.shape == terms.shape and (keys.size == 0 or (keys.min() >= 0 and keys.max() < size))
    g = np.bincount(keys, weights=terms, minlength=size).reshape(shape)
    T = np.bincount(keys, minlength=size).reshape(shape)
    S = np.bincount(keys, weights=np.abs(terms), minlength=size).reshape(shape)
    return g, T, S


def _row_keys(idx, n, c):
    """idx [b, ...] of rows into [b, n, c] -> element keys [rows, c] of the flat gradient"""
    idx = np.asarray(idx)
    b = idx.shape[0]
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < n)
    rows = (np.arange(b, dtype=np.int64).reshape((b,) + (1,) * (idx.ndim - 1)) * n + idx).reshape(-1)
    return rows[:, None] * c + np.arange(c, dtype=np.int64)


def group_point_grad(idx, grad_out, n):
    """idx [b, m, ns], grad_out [b, m, ns, c] -> (g, T, S) [b, n, c]: g[i, idx[i, j, k], :] += grad_out[i, j, k, :]"""
    c = grad_out.shape[-1]
    return _scatter(_row_keys(idx, n, c), grad_out, (idx.shape[0], n, c))


def gather_point_grad(idx, out_g, n):
    """idx [b, m], out_g [b, m, 3] -> (g, T, S) [b, n, 3]"""
    return _scatter(_row_keys(idx, n, 3), out_g, (idx.shape[0], n, 3))


def three_interpolate_grad(idx, weight, grad_out, m):
    """idx / weight [b, n, 3], grad_out [b, n, c] -> (g, T, S) [b, m, c]: g[i, idx[i, j, t], :] += grad_out[i, j, :] * weight[i, j, t]"""
    b, n, c = grad_out.shape
    keys = _row_keys(idx, m, c)                                            # [b * n * 3, c]
    terms = _f64(grad_out)[:, :, None, :] * _f64(weight)[..., None]       # [b, n, 3, c]; a product of two float32 is exact in float64
    return _scatter(keys, terms, (b, m, c))


def nn_distance_grad(xyz1, xyz2, grad_dist1, idx1, grad_dist2, idx2):
    """-> ((g1, T1, S1) [b, n, 3], (g2, T2, S2) [b, m, 3]).  Point j of the from-cloud with partner k = idx[j] adds
    v = 2 * grad_dist[j] * (from[j] - to[k]) to its own gradient and -v to the partner's, in both directions."""
    x1, x2 = _f64(xyz1), _f64(xyz2)
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]

    def direction(frm, to, gd, idx, nf, nt):
        v = 2.0 * _f64(gd)[..., None] * (frm - gather_rows(to, idx))
        own = np.broadcast_to(np.arange(nf), (b, nf))
        return _row_keys(own, nf, 3), _row_keys(idx, nt, 3), v

    own1, to2, v1 = direction(x1, x2, grad_dist1, idx1, n, m)
    own2, to1, v2 = direction(x2, x1, grad_dist2, idx2, m, n)
    r1 = _scatter(np.concatenate([own1.ravel(), to1.ravel()]), np.concatenate([v1.ravel(), -v2.ravel()]), (b, n, 3))
    r2 = _scatter(np.concatenate([own2.ravel(), to2.ravel()]), np.concatenate([v2.ravel(), -v1.ravel()]), (b, m, 3))
    return r1, r2


def random_data_bound(T, S):
    return (T + 2) * U * S


def exact_in_any_order(g, S, grid):
    """every term is a multiple of `grid` (the caller's data guarantees it) and the absolute terms of an element sum to less than 2^24
    grid units: then every partial sum, in any order, is an integer below 2^24 in those units, so float32 adds none of them inexactly."""
    units_g, units_S = _f64(g) / grid, _f64(S) / grid
    return bool((units_g == np.rint(units_g)).all() and (units_S == np.rint(units_S)).all() and (units_S < 2.0 ** 24).all()
                and np.array_equal(_f64(g).astype(F32).astype(F64), _f64(g)))


# -------------------------------------------------------------------------------------------------------------------- dispatch ----
ROW_KERNEL = {"group_point": "group_rows_kernel", "gather_point": "group_rows_kernel", "three_interpolate": "three_interpolate_rows_kernel"}
ROWS_R = {"group_rows_kernel": 8, "three_interpolate_rows_kernel": 4}       # rows per slot (constexpr int R of the two launchers)
XYZ_R = 4                                                                   # passes of 256 rows per gather_xyz_kernel workgroup
GRID_CAP = {"group_point_grad": 16384, "three_interpolate_grad": 16384, "gather_point_grad": 8192}   # grid_for of the op's file
GRID_BS = 256
LANES_CLASSES = ("1", "2", "3-4", "5-8", "9-16", "17-32", "33-64", ">64")    # vectors per row -> lanes per row 1 .. 64, and beyond


def _boundary_inside(rows, rpc, wg_rows):
    lo = np.arange(0, rows, wg_rows, dtype=np.int64)
    hi = np.minimum(lo + wg_rows, rows) - 1
    return bool((lo // rpc != hi // rpc).any())


def _xcd_remap(g):
    """xcd_block (csrc/common.h) re-orders the workgroup ids of a grid that is a multiple of 8; at 8 itself the order is unchanged"""
    return g % 8 == 0 and g > 8


def rows_plan(op, rows, c, rows_per_cloud, points_off=0, out_off=0):
    """What launch_gather_rows (group_point, gather_point) / dispu_three_interpolate launch for `rows` output rows of c floats.
    points_off / out_off: the offset of the pointer from a 16-byte boundary, in floats."""
    assert rows > 0 and rows_per_cloud > 0
    p_al, o_al = points_off % 4 == 0, out_off % 4 == 0
    if c == 3 and op != "three_interpolate":
        wg_rows = 256 * XYZ_R
        g = -(-rows // wg_rows)
        return dict(kernel="gather_xyz_kernel", R=XYZ_R, wg_rows=wg_rows, workgroups=g, xcd_remap=_xcd_remap(g),
                    full_passes=rows // wg_rows if o_al else 0, tail_pass=bool(rows % wg_rows) and o_al, out_misaligned=not o_al,
                    partial_last=bool(rows % wg_rows), cloud_boundary_inside=_boundary_inside(rows, rows_per_cloud, wg_rows))
    kernel = ROW_KERNEL[op]
    R = ROWS_R[kernel]
    vec4 = c % 4 == 0 and p_al and o_al
    cv = c // 4 if vec4 else c
    tx_log2 = 0
    while (1 << tx_log2) < cv and tx_log2 < 6:
        tx_log2 += 1
    slots = 256 >> tx_log2
    wg_rows = slots * R
    g = -(-rows // wg_rows)
    fallback = None
    if c % 4 == 0 and not vec4:
        fallback = "both" if not (p_al or o_al) else ("out" if p_al else "points")
    return dict(kernel=kernel, vec=4 if vec4 else 1, R=R, tx_log2=tx_log2, lanes_class=LANES_CLASSES[tx_log2 if cv <= 64 else 7],
                slots=slots, wg_rows=wg_rows, workgroups=g, partial_last=bool(rows % wg_rows), column_trips=-(-cv // (1 << tx_log2)),
                cloud_boundary_inside=_boundary_inside(rows, rows_per_cloud, wg_rows), xcd_remap=_xcd_remap(g), fallback=fallback)


def grid_stride_plan(op, total):
    """The grid-stride gradients: total = elements of grad_out (group_point_grad, three_interpolate_grad) or rows (gather_point_grad)."""
    cap = GRID_CAP[op]
    grid = max(1, min(-(-total // GRID_BS), cap))
    return dict(kernel=op + "_kernel", cap=cap, cap_total=cap * GRID_BS, grid=grid, trips=-(-total // (grid * GRID_BS)),
                at_cap=total == cap * GRID_BS, one_over=total == cap * GRID_BS + 1)


def nn_grad_plan(n, m):
    """dispu_nn_distance_grad launches max(n, m) lanes (rounded up to 256) for BOTH z-slices: slice 0 walks xyz1 (guard j >= n),
    slice 1 walks xyz2 (guard j >= m)."""
    lanes = -(-max(n, m) // 256) * 256
    return dict(workgroups=lanes // 256, idle_lanes_z0=lanes - n, idle_lanes_z1=lanes - m,
                idle_workgroups_z0=(lanes - n) // 256, idle_workgroups_z1=(lanes - m) // 256)


# ----------------------------------------------------------------------------------------------------------------------- cases ----
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_idx(rng, pattern, b, rows, n):
    """[b, rows] int32 indices into n points.  random: uniform; one: every row the same point; identity / reversed: row r -> r mod n /
    n - 1 - r mod n (a permutation where rows == n); perm: a random permutation per cloud (rows == n); half: every other row to one
    point, the rest uniform."""
    if pattern == "random":
        idx = rng.integers(0, n, (b, rows))
    elif pattern == "one":
        idx = np.full((b, rows), n // 2)
    elif pattern == "identity":
        idx = np.broadcast_to(np.arange(rows) % n, (b, rows))
    elif pattern == "reversed":
        idx = np.broadcast_to(n - 1 - np.arange(rows) % n, (b, rows))
    elif pattern == "perm":
        assert rows == n
        idx = np.stack([rng.permutation(n) for _ in range(b)]) if b else np.zeros((0, rows))
    elif pattern == "half":
        idx = rng.integers(0, n, (b, rows))
        idx[:, ::2] = n // 3
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(idx, np.int32)


def _exact_weights(rng, b, n):
    """[b, n, 3]: a rotation of (0.5, 0.25, 0.25) per row"""
    base = np.array([0.5, 0.25, 0.25], F32)
    return base[(np.arange(3) + rng.integers(0, 3, (b, n, 1))) % 3]


def _ints(rng, shape):
    return rng.integers(-8, 9, shape).astype(F32)


# forward cases: op, b, n (points per cloud), c, rpc (rows per cloud), ns (group_point: idx is [b, rpc / ns, ns]), pattern, offsets
Forward = collections.namedtuple("Forward", "op b n c rpc ns pattern points_off out_off")
VEC4_C = (4, 8, 16, 20, 64, 68, 256, 260)                 # c / 4 = 1, 2, 4, 5, 16, 17, 64, 65: one per lanes class
SCALAR_C = {"group_point": (1, 2, 7, 9, 31, 33, 67),     # class 3-4 exists for group_point only as the misaligned c = 4 (c = 3 is xyz)
            "three_interpolate": (1, 2, 3, 7, 9, 31, 33, 67)}
MISALIGNED_C = (4, 64, 260)
XYZ_M = (1, 1023, 1024, 1025, 4096 + 7)


class _Cases(collections.OrderedDict):
    """a case table: a name is given once"""

    def __setitem__(self, name, case):
        assert name not in self, "two cases are named %s" % name
        super().__setitem__(name, case)


def _forward_cases():
    cases = _Cases()
    for op in ("group_point", "three_interpolate"):
        for c in VEC4_C + SCALAR_C[op]:
            p = rows_plan(op, 1, c, 1)
            wg, slots = p["wg_rows"], p["slots"]
            xcd_rpc = -(-(15 * wg + 1) // 3)                                # three clouds over sixteen workgroups, the last partial
            for variant, b, rpc in (("one", 1, 1), ("few", 1, slots - 1), ("wg-1", 1, wg - 1), ("wg", 1, wg), ("wg+1", 1, wg + 1),
                                    ("multi", 3, wg + 7), ("xcd", 3, xcd_rpc)):
                cases["%s-c%d-%s" % (op, c, variant)] = Forward(op, b, 37, c, rpc, 1, "random", 0, 0)
        for c in MISALIGNED_C:
            wg = rows_plan(op, 1, c, 1, 1, 0)["wg_rows"]
            for what, po, oo in (("points", 1, 0), ("out", 0, 1), ("both", 1, 1)):
                cases["%s-c%d-misaligned-%s" % (op, c, what)] = Forward(op, 3, 37, c, wg + 7, 1, "random", po, oo)
        for c in (4, 7):
            for pattern in ("one", "identity", "reversed"):
                cases["%s-c%d-pattern-%s" % (op, c, pattern)] = Forward(op, 2, 300, c, 300, 4 if op == "group_point" else 1, pattern, 0, 0)
    for m in XYZ_M + (5200,):                                                # 5200: sixteen workgroups, the last partial
        cases["gather_point-b3-m%d" % m] = Forward("gather_point", 3, 300, 3, m, 1, "random", 0, 0)
    for m in (1023, 1024, 1025):
        cases["gather_point-b1-m%d" % m] = Forward("gather_point", 1, 300, 3, m, 1, "random", 0, 0)
    for m in (1024, 1025):
        cases["gather_point-b3-m%d-misaligned-out" % m] = Forward("gather_point", 3, 300, 3, m, 1, "random", 0, 1)
    for pattern in ("one", "identity", "reversed"):
        cases["gather_point-pattern-%s" % pattern] = Forward("gather_point", 2, 300, 3, 300, 1, pattern, 0, 0)
    cases["group_point-c3-one"] = Forward("group_point", 1, 37, 3, 1, 1, "random", 0, 0)
    cases["group_point-c3-multi"] = Forward("group_point", 3, 37, 3, 1025, 5, "random", 0, 0)
    cases["group_point-c3-misaligned-out"] = Forward("group_point", 3, 37, 3, 1025, 5, "random", 0, 1)
    return cases


FORWARD_CASES = _forward_cases()


def forward_plan(name):
    k = FORWARD_CASES[name]
    return rows_plan(k.op, k.b * k.rpc, k.c, k.rpc, k.points_off, k.out_off)


@functools.lru_cache(maxsize=None)
def forward_inputs(name):
    """-> dict(points [b, n, c], idx, weight or None); idx is [b, m, ns] (group_point), [b, m] (gather_point) or [b, n_out, 3]"""
    k, rng = FORWARD_CASES[name], _rng(name)
    points = rng.standard_normal((k.b, k.n, k.c)).astype(F32)
    if k.op == "three_interpolate":
        idx = make_idx(rng, k.pattern, k.b, k.rpc * 3, k.n).reshape(k.b, k.rpc, 3)
        return dict(points=points, idx=idx, weight=rng.random((k.b, k.rpc, 3)).astype(F32))
    idx = make_idx(rng, k.pattern, k.b, k.rpc, k.n)
    if k.op == "group_point":
        assert k.rpc % k.ns == 0
        idx = idx.reshape(k.b, k.rpc // k.ns, k.ns)
    return dict(points=points, idx=idx, weight=None)


@functools.lru_cache(maxsize=None)
def forward_expected(name):
    """float32, the bits the kernel must produce"""
    k, x = FORWARD_CASES[name], forward_inputs(name)
    if k.op == "three_interpolate":
        return three_interpolate_f32(x["points"], x["idx"], x["weight"])
    return gather_rows(x["points"], x["idx"]).astype(F32)


# gradient cases: op, dims, pattern, data ("exact": every term and partial sum representable; "normal": standard normal)
#   group_point_grad        dims = (b, n, c, m, ns)
#   gather_point_grad       dims = (b, n, m)
#   three_interpolate_grad  dims = (b, n, c, m): n rows interpolated from m points
#   nn_distance_grad        dims = (b, n, m)
Grad = collections.namedtuple("Grad", "op dims pattern data")
NN_SHAPES = ((1, 1), (1, 5), (5, 1), (200, 300), (300, 200), (255, 256), (256, 257), (257, 255), (1030, 7))


def _grad_cases():
    c = _Cases()
    G, P, I, D = "group_point_grad", "gather_point_grad", "three_interpolate_grad", "nn_distance_grad"
    cap_e, cap_r = GRID_CAP[G] * GRID_BS, GRID_CAP[P] * GRID_BS              # 4194304 elements, 2097152 rows
    assert cap_e + 1 == 5 * 397 * 2113
    c["group-perm"] = Grad(G, (2, 240, 5, 60, 4), "perm", "normal")
    c["group-uniform"] = Grad(G, (3, 50, 7, 40, 16), "random", "exact")
    c["group-one-of-1"] = Grad(G, (2, 1, 3, 500, 8), "one", "exact")           # n = 1: 4000 atomics on each address
    c["group-one-of-37"] = Grad(G, (2, 37, 4, 100, 8), "one", "exact")
    c["group-half"] = Grad(G, (2, 37, 9, 100, 8), "half", "exact")
    c["group-sparse"] = Grad(G, (2, 300, 9, 10, 8), "half", "exact")           # most points receive nothing
    c["group-normal"] = Grad(G, (3, 50, 12, 50, 16), "random", "normal")       # 16 terms per element on average
    c["group-at-cap"] = Grad(G, (1, 64, 128, 2048, 16), "random", "exact")
    c["group-one-over-cap"] = Grad(G, (1, 50, 5, 2113, 397), "random", "exact")
    c["group-second-trip"] = Grad(G, (2, 64, 128, 1100, 16), "random", "exact")
    c["gather-perm"] = Grad(P, (2, 300, 300), "perm", "normal")
    c["gather-uniform"] = Grad(P, (3, 50, 700), "random", "exact")
    c["gather-one-of-1"] = Grad(P, (2, 1, 4000), "one", "exact")
    c["gather-half"] = Grad(P, (2, 37, 1000), "half", "exact")
    c["gather-sparse"] = Grad(P, (2, 300, 100), "half", "exact")
    c["gather-normal"] = Grad(P, (3, 50, 800), "random", "normal")
    c["gather-at-cap"] = Grad(P, (1, 50, cap_r), "random", "exact")
    c["gather-one-over-cap"] = Grad(P, (1, 50, cap_r + 1), "random", "exact")  # also this kernel's second trip
    c["interp-perm"] = Grad(I, (2, 100, 5, 300), "perm", "normal")
    c["interp-uniform"] = Grad(I, (3, 200, 7, 50), "random", "exact")
    c["interp-one-of-1"] = Grad(I, (2, 1400, 3, 1), "one", "exact")
    c["interp-half"] = Grad(I, (2, 300, 9, 37), "half", "exact")
    c["interp-sparse"] = Grad(I, (2, 30, 9, 300), "half", "exact")
    c["interp-normal"] = Grad(I, (3, 160, 12, 30), "random", "normal")         # 3 * 160 / 30 = 16 terms per element
    c["interp-at-cap"] = Grad(I, (1, 32768, 128, 64), "random", "exact")
    c["interp-one-over-cap"] = Grad(I, (1, 838861, 5, 50), "random", "exact")
    c["interp-second-trip"] = Grad(I, (2, 17000, 128, 64), "random", "exact")
    for n, m in NN_SHAPES:
        for b in (1, 3):
            for pattern in ("random", "one"):
                c["nn-b%d-%dx%d-%s" % (b, n, m, pattern)] = Grad(D, (b, n, m), pattern, "exact")
    c["nn-normal-300x200"] = Grad(D, (3, 300, 200), "random", "normal")
    c["nn-normal-16x256"] = Grad(D, (3, 16, 256), "random", "normal")           # 1 + 16 terms on every xyz1 element
    return c


GRAD_CASES = _grad_cases()
EXACT_GRID = {"group_point_grad": 1.0, "gather_point_grad": 1.0, "three_interpolate_grad": 0.25, "nn_distance_grad": 2.0 ** -6}


def grad_plan(name):
    k = GRAD_CASES[name]
    if k.op == "group_point_grad":
        b, n, c, m, ns = k.dims
        return grid_stride_plan(k.op, b * m * ns * c)
    if k.op == "gather_point_grad":
        return grid_stride_plan(k.op, k.dims[0] * k.dims[2])
    if k.op == "three_interpolate_grad":
        b, n, c, m = k.dims
        return grid_stride_plan(k.op, b * n * c)
    return nn_grad_plan(k.dims[1], k.dims[2])


@functools.lru_cache(maxsize=2)                                              # the cap cases are tens of MB each: keep none for long
def grad_inputs(name):
    k, rng = GRAD_CASES[name], _rng(name)
    val = (lambda shape: _ints(rng, shape)) if k.data == "exact" else (lambda shape: rng.standard_normal(shape).astype(F32))
    if k.op == "group_point_grad":
        b, n, c, m, ns = k.dims
        return dict(n=n, idx=make_idx(rng, k.pattern, b, m * ns, n).reshape(b, m, ns), grad_out=val((b, m, ns, c)))
    if k.op == "gather_point_grad":
        b, n, m = k.dims
        return dict(n=n, idx=make_idx(rng, k.pattern, b, m, n), out_g=val((b, m, 3)))
    if k.op == "three_interpolate_grad":
        b, n, c, m = k.dims
        w = _exact_weights(rng, b, n) if k.data == "exact" else rng.random((b, n, 3)).astype(F32)
        return dict(m=m, idx=make_idx(rng, k.pattern, b, n * 3, m).reshape(b, n, 3), weight=w, grad_out=val((b, n, c)))
    b, n, m = k.dims
    if k.data == "exact":                                                    # coordinates on a 2^-6 grid in [0, 1)
        xyz1, xyz2 = (rng.integers(0, 64, (b, n, 3)) / 64.0).astype(F32), (rng.integers(0, 64, (b, m, 3)) / 64.0).astype(F32)
    else:
        xyz1, xyz2 = rng.standard_normal((b, n, 3)).astype(F32), rng.standard_normal((b, m, 3)).astype(F32)
    return dict(xyz1=xyz1, xyz2=xyz2, grad_dist1=val((b, n)), idx1=make_idx(rng, k.pattern, b, n, m), grad_dist2=val((b, m)),
                idx2=make_idx(rng, k.pattern, b, m, n))


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """(g, T, S), or for nn_distance_grad ((g1, T1, S1), (g2, T2, S2))"""
    k, x = GRAD_CASES[name], grad_inputs(name)
    if k.op == "group_point_grad":
        return group_point_grad(x["idx"], x["grad_out"], x["n"])
    if k.op == "gather_point_grad":
        return gather_point_grad(x["idx"], x["out_g"], x["n"])
    if k.op == "three_interpolate_grad":
        return three_interpolate_grad(x["idx"], x["weight"], x["grad_out"], x["m"])
    return nn_distance_grad(x["xyz1"], x["xyz2"], x["grad_dist1"], x["idx1"], x["grad_dist2"], x["idx2"])
