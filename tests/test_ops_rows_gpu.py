"""The row movers (group_point, gather_point, three_interpolate) and the scatter gradients (group_point_grad, gather_point_grad,
three_interpolate_grad, nn_distance_grad) alone, on every path their launchers can take (pytest -m gpu).  References, dispatch
restatement and case tables: tests/ops_rows_oracle.py; tests/test_ops_rows_oracle.py checks on the CPU that the tables reach the paths
named here and that the "exact data" cases cannot round.

  * forward: the bits of the float64 reference rounded to float32 (three_interpolate: of (p0*w0 + p1*w1) + p2*w2 with every
    operation rounded), through the Python shim and again through the C ABI into a sentinel-filled buffer whose pad must survive;
    misaligned `points` / `out` (views one float into a larger buffer) give the aligned call's bits;
  * gradients on exact data (small integers, weights of 0.5 / 0.25 / 0.25, coordinates on a 2^-6 grid): array_equal -- one lost, doubled
    or misplaced term shows, whatever order the float atomics take; a permutation is a re-ordering and bit-exact for any data;
  * gradients on standard-normal data: per element within (T + 2) * 2^-24 * S of the float64 sum, T and S being the element's term
    count and absolute-term sum (derived in ops_rows_oracle, not measured);
  * the zero fill: a sentinel-filled gradient buffer, called twice, equals the reference both times, untouched rows are +0.0, the pad
    keeps its sentinel, b = 0 touches nothing and an empty index set leaves zeros;
  * autograd through the shims equals the *_grad entries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ops_rows_oracle as RO  # noqa: E402
from ops_rows_oracle import F32, F64  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
PAD = 64                    # floats behind (and, for a misaligned view, in front of) a buffer that must keep the sentinel


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def ops(dev):
    import dispu_amd.tf_sampling as S
    import dispu_amd.tf_grouping as G
    import dispu_amd.tf_interpolate as I
    import dispu_amd.tf_nndistance as D
    from dispu_amd import _lib
    return dict(S=S, G=G, I=I, D=D, L=_lib.lib(), lib=_lib)


def placed(dev, a, off=0):
    """a copy of `a` on the device whose first element lies `off` floats behind a 16-byte boundary"""
    a = np.ascontiguousarray(a, F32)
    whole = torch.zeros(off + a.size + 4, dtype=torch.float32, device=dev)
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


class Guarded(object):
    """`size` floats at `off` floats behind a 16-byte boundary, filled with the sentinel like the floats around them"""

    def __init__(self, dev, size, off=0):
        self.whole = torch.full((4 + off + size + PAD,), SENTINEL, dtype=torch.float32, device=dev)
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.hi = 4 + off, 4 + off + size
        self.view = self.whole[self.lo:self.hi]

    def fill(self):
        self.whole.fill_(SENTINEL)

    def surroundings_intact(self):
        w = N(self.whole)
        return bool((w[:self.lo] == F32(SENTINEL)).all() and (w[self.hi:] == F32(SENTINEL)).all())

    def all_intact(self):
        return bool((N(self.whole) == F32(SENTINEL)).all())

    def get(self, shape):
        return N(self.view).reshape(shape)


def call_forward_raw(ops, dev, k, x, out, points):
    L, lib = ops["L"], ops["lib"]
    idx = T(x["idx"], dev)
    st = lib.stream_ptr(dev)
    if k.op == "group_point":
        rc = L.dispu_group_point(k.b, k.n, k.c, k.rpc // k.ns, k.ns, lib.ptr(points), lib.ptr(idx), lib.ptr(out), st)
    elif k.op == "gather_point":
        rc = L.dispu_gather_point(k.b, k.n, k.rpc, lib.ptr(points), lib.ptr(idx), lib.ptr(out), st)
    else:
        weight = T(x["weight"], dev)
        rc = L.dispu_three_interpolate(k.b, k.n, k.c, k.rpc, lib.ptr(points), lib.ptr(idx), lib.ptr(weight), lib.ptr(out), st)
    torch.cuda.synchronize()
    assert rc == 0, rc


def call_forward_shim(ops, dev, k, x):
    if k.op == "group_point":
        return ops["G"].group_point(T(x["points"], dev), T(x["idx"], dev))
    if k.op == "gather_point":
        return ops["S"].gather_point(T(x["points"], dev), T(x["idx"], dev))
    return ops["I"].three_interpolate(T(x["points"], dev), T(x["idx"], dev), T(x["weight"], dev))


# ------------------------------------------------------------------------------------------------------------ forward row movers ----
@pytest.mark.parametrize("name", list(RO.FORWARD_CASES))
def test_forward_rows_bit_exact(ops, dev, name):
    k, x, want = RO.FORWARD_CASES[name], RO.forward_inputs(name), RO.forward_expected(name)
    aligned = None
    if k.points_off == 0 and k.out_off == 0:
        aligned = N(call_forward_shim(ops, dev, k, x))
        assert same_bits(aligned, want), "through the shim"
    out = Guarded(dev, want.size, k.out_off)
    call_forward_raw(ops, dev, k, x, out.view, placed(dev, x["points"], k.points_off))
    assert same_bits(out.get(want.shape), want), "through the C ABI, points + %d floats, out + %d floats" % (k.points_off, k.out_off)
    assert out.surroundings_intact(), "the floats around the output changed"
    if aligned is None:                                   # a misaligned case: the aligned call of the same inputs gives the same bits
        assert same_bits(out.get(want.shape), N(call_forward_shim(ops, dev, k, x)))


def test_forward_empty_row_sets_touch_nothing(ops, dev):
    L, lib = ops["L"], ops["lib"]
    pts, idx, out = placed(dev, np.ones((2, 5, 8), F32)), torch.zeros(8, dtype=torch.int32, device=dev), Guarded(dev, 64)
    st = lib.stream_ptr(dev)
    for b, m, ns in ((0, 4, 2), (2, 0, 2), (2, 4, 0)):
        assert L.dispu_group_point(b, 5, 8, m, ns, lib.ptr(pts), lib.ptr(idx), lib.ptr(out.view), st) == 0
    for b, m in ((0, 4), (2, 0)):
        assert L.dispu_gather_point(b, 5, m, lib.ptr(pts), lib.ptr(idx), lib.ptr(out.view), st) == 0
        assert L.dispu_three_interpolate(b, 5, 8, m, lib.ptr(pts), lib.ptr(idx), lib.ptr(pts), lib.ptr(out.view), st) == 0
    torch.cuda.synchronize()
    assert out.all_intact()


# ------------------------------------------------------------------------------------------------------------- scatter gradients ----
def run_grad(ops, dev, name):
    """the gradient of a case through the reference-named *_grad entry of the shim -> numpy array (nn_distance_grad: a pair)"""
    k, x = RO.GRAD_CASES[name], RO.grad_inputs(name)
    if k.op == "group_point_grad":
        b, n, c, m, ns = k.dims
        return N(ops["G"].group_point_grad(torch.empty((b, n, c), device=dev), T(x["idx"], dev), T(x["grad_out"], dev)))
    if k.op == "gather_point_grad":
        b, n, m = k.dims
        return N(ops["S"].gather_point_grad(torch.empty((b, n, 3), device=dev), T(x["idx"], dev), T(x["out_g"], dev)))
    if k.op == "three_interpolate_grad":
        b, n, c, m = k.dims
        return N(ops["I"].three_interpolate_grad(torch.empty((b, m, c), device=dev), T(x["idx"], dev), T(x["weight"], dev), T(x["grad_out"], dev)))
    g1, g2 = ops["D"].nn_distance_grad(T(x["xyz1"], dev), T(x["xyz2"], dev), T(x["grad_dist1"], dev), T(x["idx1"], dev),
                                       T(x["grad_dist2"], dev), T(x["idx2"], dev))
    return N(g1), N(g2)


def pairs(name, got):
    """[(got, (g, T, S)), ...]: one pair, or nn_distance_grad's two"""
    ref = RO.grad_reference(name)
    return list(zip(got, ref)) if RO.GRAD_CASES[name].op == "nn_distance_grad" else [(got, ref)]


def mismatch(got, g):
    bad = np.argwhere(got.astype(F64) != g)
    return "%d of %d elements differ, first at %s: got %r, want %r" % (len(bad), g.size, tuple(bad[0]), got[tuple(bad[0])], g[tuple(bad[0])])


@pytest.mark.parametrize("name", [n for n, k in RO.GRAD_CASES.items() if k.data == "exact"])
def test_gradient_on_exact_data_is_the_reference(ops, dev, name):
    """no term and no partial sum can round (test_exact_data_cannot_round): every order of the atomics gives the float64 sum"""
    for got, (g, _, _) in pairs(name, run_grad(ops, dev, name)):
        assert got.dtype == F32 and got.shape == g.shape
        assert np.array_equal(got.astype(F64), g), mismatch(got, g)


@pytest.mark.parametrize("name", [n for n, k in RO.GRAD_CASES.items() if k.pattern == "perm"])
def test_gradient_of_a_permutation_is_a_reordering(ops, dev, name):
    """one term per element: nothing is summed, so standard-normal data comes back bit for bit (three_interpolate_grad: as the
    float32 product g * w, which the float64 product rounds to)"""
    got, (g, T_, _) = pairs(name, run_grad(ops, dev, name))[0]
    assert (T_ == 1).all() and same_bits(got, g.astype(F32)), mismatch(got, g.astype(F32).astype(F64))


@pytest.mark.parametrize("name", [n for n, k in RO.GRAD_CASES.items() if k.data == "normal" and k.pattern != "perm"])
def test_gradient_on_random_data_within_the_summation_bound(ops, dev, name):
    """(T + 2) * 2^-24 * S per element, derived in ops_rows_oracle.  [measured on an MI355X] the largest error / bound ratio is 0.13 - 0.22
    at 16 - 17 terms per element and 0.61 where an nn_distance_grad element has a single term (two roundings against a bound of three)."""
    for got, (g, T_, S) in pairs(name, run_grad(ops, dev, name)):
        err, bound = np.abs(got.astype(F64) - g), RO.random_data_bound(T_, S)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print("[measured] %s: mean terms per element %.1f, largest error / bound %.3f" % (name, T_.mean(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), "element %s: error %.3e, bound %.3e (T = %d)" % (worst, err[worst], bound[worst], T_[worst])


ZERO_FILL = ["group-sparse", "gather-sparse", "interp-sparse", "nn-b3-300x200-random", "nn-b3-1030x7-one"]


def raw_grad_call(ops, dev, name, bufs, b=None, empty=False):
    """the C entry of a case's op on guarded gradient buffers; b overrides the batch, empty asks for an empty index set (m = 0 / n = 0)"""
    L, lib = ops["L"], ops["lib"]
    k, x = RO.GRAD_CASES[name], RO.grad_inputs(name)
    st = lib.stream_ptr(dev)
    dv = {key: T(v, dev) for key, v in x.items() if isinstance(v, np.ndarray)}
    if k.op == "group_point_grad":
        bb, n, c, m, ns = k.dims
        rc = L.dispu_group_point_grad(bb if b is None else b, n, c, 0 if empty else m, ns, lib.ptr(dv["grad_out"]), lib.ptr(dv["idx"]), lib.ptr(bufs[0].view), st)
    elif k.op == "gather_point_grad":
        bb, n, m = k.dims
        rc = L.dispu_gather_point_grad(bb if b is None else b, n, 0 if empty else m, lib.ptr(dv["out_g"]), lib.ptr(dv["idx"]), lib.ptr(bufs[0].view), st)
    elif k.op == "three_interpolate_grad":
        bb, n, c, m = k.dims
        rc = L.dispu_three_interpolate_grad(bb if b is None else b, 0 if empty else n, c, m, lib.ptr(dv["grad_out"]), lib.ptr(dv["idx"]), lib.ptr(dv["weight"]),
                                            lib.ptr(bufs[0].view), st)
    else:
        bb, n, m = k.dims
        rc = L.dispu_nn_distance_grad(bb if b is None else b, n, lib.ptr(dv["xyz1"]), 0 if empty else m, lib.ptr(dv["xyz2"]), lib.ptr(dv["grad_dist1"]),
                                      lib.ptr(dv["idx1"]), lib.ptr(dv["grad_dist2"]), lib.ptr(dv["idx2"]), lib.ptr(bufs[0].view), lib.ptr(bufs[1].view), st)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", ZERO_FILL)
def test_gradient_entries_zero_fill_their_output(ops, dev, name):
    k = RO.GRAD_CASES[name]
    refs = pairs(name, [None, None] if k.op == "nn_distance_grad" else None)
    bufs = [Guarded(dev, g.size) for _, (g, _, _) in refs]
    untouched = 0
    for _ in range(2):                                                      # the second call starts from the first call's result
        assert raw_grad_call(ops, dev, name, bufs) == 0
        for buf, (_, (g, T_, _)) in zip(bufs, refs):
            got = buf.get(g.shape)
            assert np.array_equal(got.astype(F64), g), mismatch(got, g)
            assert (got[T_ == 0].view(np.uint32) == 0).all(), "an element no index points at is not +0.0"
            assert buf.surroundings_intact()
            untouched += int((T_ == 0).sum())
    assert untouched > 0 or k.op == "nn_distance_grad"                       # every nn_distance_grad point carries its own term
    for buf in bufs:
        buf.fill()
    assert raw_grad_call(ops, dev, name, bufs, b=0) == 0                     # an empty batch touches nothing
    assert all(buf.all_intact() for buf in bufs)
    rc = raw_grad_call(ops, dev, name, bufs, empty=True)
    if k.op == "nn_distance_grad":                                           # the entry admits no empty cloud: it refuses and writes nothing
        assert rc != 0 and all(buf.all_intact() for buf in bufs)
    else:                                                                    # no rows: the gradient is all +0.0
        assert rc == 0 and (bufs[0].get(refs[0][1][0].shape).view(np.uint32) == 0).all() and bufs[0].surroundings_intact()


def test_group_point_grad_without_samples_leaves_zeros(ops, dev):
    L, lib = ops["L"], ops["lib"]
    buf = Guarded(dev, 2 * 5 * 8)
    dummy = torch.zeros(8, dtype=torch.int32, device=dev)
    assert L.dispu_group_point_grad(2, 5, 8, 3, 0, lib.ptr(dummy), lib.ptr(dummy), lib.ptr(buf.view), lib.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert (buf.get((80,)).view(np.uint32) == 0).all() and buf.surroundings_intact()


# ---------------------------------------------------------------------------------------------------------------- autograd wiring ----
def expanded(dev, rng, shape):
    """small integers along the last axis, expanded (stride 0) over the others: a non-contiguous upstream gradient"""
    return T(rng.integers(1, 6, shape[-1]).astype(F32), dev).expand(*shape)


def test_autograd_is_the_grad_entry(ops, dev):
    """scatter-heavy exact-data cases: (out * w).sum() with an expanded w sends a stride-0 gradient into backward()"""
    rng = np.random.default_rng(0)
    x = RO.grad_inputs("group-half")
    b, n, c, m, ns = RO.GRAD_CASES["group-half"].dims
    pts = T(rng.integers(-8, 9, (b, n, c)).astype(F32), dev).requires_grad_(True)
    out = ops["G"].group_point(pts, T(x["idx"], dev))
    w = expanded(dev, rng, out.shape)
    assert not w.is_contiguous()
    (out * w).sum().backward()
    assert torch.equal(pts.grad, ops["G"].group_point_grad(pts.detach(), T(x["idx"], dev), w.contiguous()))

    x = RO.grad_inputs("gather-half")
    b, n, m = RO.GRAD_CASES["gather-half"].dims
    pts = T(rng.integers(-8, 9, (b, n, 3)).astype(F32), dev).requires_grad_(True)
    out = ops["S"].gather_point(pts, T(x["idx"], dev))
    w = expanded(dev, rng, out.shape)
    (out * w).sum().backward()
    assert torch.equal(pts.grad, ops["S"].gather_point_grad(pts.detach(), T(x["idx"], dev), w.contiguous()))

    x = RO.grad_inputs("interp-half")
    b, n, c, m = RO.GRAD_CASES["interp-half"].dims
    pts = T(rng.integers(-8, 9, (b, m, c)).astype(F32), dev).requires_grad_(True)
    out = ops["I"].three_interpolate(pts, T(x["idx"], dev), T(x["weight"], dev))
    w = expanded(dev, rng, out.shape)
    (out * w).sum().backward()
    assert torch.equal(pts.grad, ops["I"].three_interpolate_grad(pts.detach(), T(x["idx"], dev), T(x["weight"], dev), w.contiguous()))

    x = RO.grad_inputs("nn-b3-1030x7-random")                                 # 1030 sources on 7 targets; the shim finds the arg-mins itself
    t1, t2 = T(x["xyz1"], dev).requires_grad_(True), T(x["xyz2"], dev).requires_grad_(True)
    d1, i1, d2, i2 = ops["D"].nn_distance(t1, t2, arith=0)
    w1 = T(np.array([3.0], F32), dev).expand(*d1.shape)
    w2 = T(rng.integers(1, 6, (d2.shape[0], 1)).astype(F32), dev).expand(*d2.shape)
    ((d1 * w1).sum() + (d2 * w2).sum()).backward()
    g1, g2 = ops["D"].nn_distance_grad(t1.detach(), t2.detach(), w1.contiguous(), i1, w2.contiguous(), i2)
    assert torch.equal(t1.grad, g1) and torch.equal(t2.grad, g2)
    (r1, _, _), (r2, _, _) = RO.nn_distance_grad(x["xyz1"], x["xyz2"], N(w1), N(i1), N(w2), N(i2))
    assert np.array_equal(N(g1).astype(F64), r1) and np.array_equal(N(g2).astype(F64), r2)
