"""The trainer's backward and training-mode kernels, each ALONE through the C ABI against tests/train_ops_oracle.py (numpy float64 with
explicit indices, itself held to float64 autograd by tests/test_train_ops_oracle.py), on every path their launch code takes.

Entries under test (csrc/train_ops.hip, csrc/train_gemm.hip): dispu_act_bias_grad, dispu_max_k, dispu_max_k_grad(_tail),
dispu_edge_feature_grad, dispu_ps_group(_grad), dispu_ps_point_matmul_grad, dispu_softmax_rows_grad, dispu_bn_train(_grad),
dispu_repulsion_grad, dispu_adam, dispu_fill_rows, dispu_linear_splitk_finish.  tests/test_train_gpu.py visits each at one small shape;
here the shapes are chosen from the launch code: the float4 / scalar switch of the mask kernels, the 16384-workgroup cap of the
grid-stride kernels (a second trip above 4 194 304 elements) and the caps of the kernels that have their own, the column loop and the
rows_per_block switch of the column sums, the strided partial sums of batch norm, strides wider than the data on every operand,
pointer offsets, ties, exact and negative zeros, hub neighbours, accumulate on and off, NULL outputs, and every refusal.  The comment
next to a parameter list says which path a shape is for.  One capped loop is NOT entered: dispu_repulsion_grad's (below).

Every output sits between guards of a sentinel and, where it is strided, between columns of it (train_ops_oracle.Strided): a kernel
that writes one element outside its window fails the test.  No element is left out of any comparison: where a ReLU decision of the
float64 reference would sit within 1e-5 of zero the INPUT is nudged away on the host (bn_inputs).

Bounds (the project's own, none new): floats 1e-5 of the largest entry of the float64 reference; bn dx 2e-5, adam update 1e-4,
repulsion_grad 1e-4; max_k_grad 1e-6, moving statistics 1e-6; masks, copies, maxima, gathers, fills, sentinels and splitk_finish in
its documented order bit-exact.  Every float comparison prints its measured error next to its bound (pytest -s).

dispu_repulsion_grad above the grid cap needs 4.2 M points; its host reference (20 slots per point, sorted, in float64) takes minutes
and gigabytes, so that case is NOT included: the kernel's grid-stride loop is the same one-line idiom the other capped kernels share.

Measured on an MI355X (worst case of each group, relative as above; bound 1e-5 unless stated or exact):
  act_bias_grad             dZ bit-exact on every path; dbias 8.1e-7 (524288 x 5), 6.9e-7 at 600001 x 3, 1.3e-7 at 1000 x 256
  max_k                     bit-exact; max_k_grad 4.1e-8 accumulating (bound 1e-6), max_k_grad_tail 1.3e-9, tails and untouched columns exact
  edge_feature_grad         9.0e-7 (1600 atomic terms on a hub point), below 4e-7 at random neighbours
  ps_group                  bit-exact; ps_group_grad dxyz 7.4e-7, dfeat 1.4e-6 (both on the 5 x 100 hub case)
  ps_point_matmul_grad      dX2 2.0e-7, dwv 5.1e-7
  softmax_rows_grad         4.5e-7; the one-hot rows exactly zero
  bn_train                  mean 3.3e-8, var 4.7e-8, 1/std 4.4e-8, y 1.4e-7, moving statistics 6.2e-8 (bound 1e-6); every ReLU decision
                            equal to the float64 reference's
  bn_train_grad             dx 1.5e-7 (bound 2e-5; 70000 x 64, above the apply kernels' grid cap), dgamma 1.2e-7, dbeta 6.2e-8
  bn, mean 100 / std 0.01   y 9.6e-6 (the float32 mean of `stats` is 2.6e-6 off, 8e-5 standard deviations: this is what the stats layout
                            allows, see the test), moving_mean 2.0e-7, dx 1.6e-7, dgamma 6.0e-8
  repulsion_grad            1.1e-7 (bound 1e-4); the hand-built six-way tie exact
  adam, ten steps           update 7.3e-6 (bound 1e-4, 4 194 305 parameters), m 1.7e-7, v 7.2e-7
  fill_rows, splitk_finish  bit-exact"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_oracle as LO  # noqa: E402
import train_ops_oracle as TO  # noqa: E402
from train_ops_oracle import F32, INVALID, SENT, Guarded, Strided, N_, close, dv, p, same_bits  # noqa: E402

from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release():
    yield
    TO.release()


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


def run(L, dev, name, *args):
    """one entry of the C ABI on the current stream, synchronised -> its return code."""
    rc = getattr(L.lib(), name)(*(args + (L.stream_ptr(dev),)))
    torch.cuda.synchronize()
    return rc


def ok(L, dev, name, *args):
    L.check(run(L, dev, name, *args), name)


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


# ----------------------------------------------------------------------------------------- dispu_act_bias_grad ----
def abg(dev, L, rows, n, act, dz, dbias, acc, ld=(None, None, None), off=(0, 0, 0), seed=0, short=0, expect=0, scratch_buf=None):
    """one call and every check of it.  scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .floats,
    .guards_intact()) in place of the sentinel-filled one.  dz: "none" (NULL), "alias" (dZ = dY's own window) or "sep"; ld / off: stride and column offset
    of dY, Y, dZ (an offset of 1 under a stride that is a multiple of 4 is a pointer that is not 16-byte aligned); short: floats
    withheld from the scratch.  expect != 0: the call must be refused and write nothing."""
    rng = np.random.default_rng(1000 * seed + n)
    ld = [n + o if l is None else l for l, o in zip(ld, off)]
    dY = rng.standard_normal((rows, n)).astype(F32)
    Y = TO.relu_like(rng, (rows, n), (rows // 3, rows // 3 + max(1, rows // 8)))
    sdy, sy = Strided(dev, rows, n, ld[0], off[0], dY), Strided(dev, rows, n, ld[1], off[1], Y)
    sdz = sdy if dz == "alias" else Strided(dev, rows, n, ld[2], off[2]) if dz == "sep" else None
    db0 = rng.standard_normal(n).astype(F32)
    gdb = Guarded(dev, n, fill=db0) if dbias else None
    need = L.lib().dispu_act_bias_grad_scratch_floats(rows, n) if dbias else 0
    assert need > 0 or not dbias or rows == 0
    sc = Guarded(dev, max(need - short, 0))
    scn = sc.n
    if scratch_buf is not None:
        sc, scn = scratch_buf, scratch_buf.floats - short
    rc = run(L, dev, "dispu_act_bias_grad", rows, n, sdy.ptr(), ld[0], sy.ptr(), ld[1], act, sdz.ptr() if sdz else None,
             sdz.ld if sdz else 0, gdb.ptr() if dbias else None, acc, sc.ptr(), scn)
    assert rc == expect, "returned %d" % rc
    assert sy.untouched() and sc.guards_intact()
    what = "act_bias_grad %d x %d act %d dZ %s acc %d" % (rows, n, act, dz, acc)
    if expect:
        assert sdy.untouched() and (sdz is None or sdz.untouched()), what + ": a refused call wrote"
        assert gdb is None or (same_bits(gdb.body(), db0) and gdb.guards_intact())
        return
    refZ, refsum = TO.act_bias_grad(dY, Y, act)
    if dz != "alias":
        assert sdy.untouched(), what + ": dY changed"
    if sdz is not None:
        assert same_bits(sdz.data(), refZ), what + ": dZ differs from where(Y > 0, dY, 0)"
        assert sdz.rest_untouched(), what + ": wrote outside dZ's window"
    if dbias:
        assert gdb.guards_intact()
        if rows == 0:
            assert same_bits(gdb.body(), db0 if acc else np.zeros(n, F32))
        else:
            close(gdb.body().astype(np.float64) - (db0 if acc else 0.0), refsum, 1e-5, what + " dbias")      # of the largest column sum


ABG_MASK = [
    # dbias = NULL: the mask kernels.  (rows, n, dz, ld (dY, Y, dZ), off (dY, Y, dZ))
    (8192, 48, "alias", (48, 48, 48), (0, 0, 0)),          # float4 path, the trainer's own call (train.py: prep's mask), compact
    (8192, 48, "alias", (480, 48, 480), (0, 0, 0)),        # float4 path, in place in the 480-wide feature gradient
    (2048, 48, "sep", (480, 52, 56), (432, 4, 8)),         # float4 path, three strides, aligned column offsets
    (131072, 132, "alias", (132, 132, 132), (0, 0, 0)),    # float4 path, 4 325 376 quads: second trip of its grid-stride loop
    (1000, 46, "sep", (48, 48, 48), (0, 0, 0)),            # scalar path by n % 4 != 0
    (1000, 48, "sep", (50, 48, 52), (0, 0, 0)),            # scalar path by a stride with ld % 4 != 0 (dY)
    (1000, 48, "sep", (48, 48, 49), (0, 0, 0)),            # ... (dZ)
    (1000, 48, "sep", (52, 48, 48), (1, 0, 0)),            # scalar path by a pointer offset of one float on dY
    (1000, 48, "sep", (48, 52, 48), (0, 1, 0)),            # ... on Y
    (1000, 48, "sep", (48, 48, 52), (0, 0, 1)),            # ... on dZ
    (1000, 48, "alias", (52, 48, 52), (1, 0, 1)),          # ... in place
    (131072, 65, "sep", (65, 66, 67), (0, 0, 0)),          # scalar path, 8 519 680 elements: above its own cap of 32768 workgroups
    (1, 1, "sep", (1, 1, 1), (0, 0, 0)),
]


@pytest.mark.parametrize("case", ABG_MASK, ids=ids(ABG_MASK))
def test_act_bias_grad_mask_only(dev, L, case):
    rows, n, dz, ld, off = case
    abg(dev, L, rows, n, 1, dz, False, 0, ld, off, seed=1)


def test_act_bias_grad_mask_only_null_and_identity(dev, L):
    """dbias = NULL: dZ = NULL leaves every buffer untouched; act = 0 with dZ aliasing dY leaves it untouched; act = 0 with a SEPARATE
    dZ is the header's contract dZ = dY (a strided copy)."""
    for act in (0, 1):
        abg(dev, L, 1000, 48, act, "none", False, 0, (52, 48, 48), seed=2)
    abg(dev, L, 1000, 48, 0, "alias", False, 0, (52, 48, 52), seed=3)
    for n, ld in [(48, (48, 48, 56)), (46, (50, 46, 47)), (130, (130, 130, 132)), (5, (5, 5, 5))]:
        abg(dev, L, 3001, n, 0, "sep", False, 0, ld, seed=4)


ABG_N = [1, 24, 64, 65, 130, 256]          # one trip of the column loop, a full one, a second with one column, a third partial, four full
ABG_ROWS = [1, 3, 4, 255, 257, 524288, 524289, 600001]     # fewer rows than row lanes .. 2048 x 256, where rows_per_block is re-derived
ABG_MODES = [(1, "sep", 1), (0, "alias", 0), (1, "none", 0), (1, "alias", 1), (0, "sep", 1), (0, "none", 0)]      # (act, dz, accumulate)


@pytest.mark.parametrize("n", ABG_N)
def test_act_bias_grad_column_loop(dev, L, n):
    act, dz, acc = ABG_MODES[ABG_N.index(n) % 6]
    abg(dev, L, 1000, n, act, dz, True, acc, (n + 3, n, n + 5), seed=5)


@pytest.mark.parametrize("rows", ABG_ROWS)
def test_act_bias_grad_row_blocks(dev, L, rows):
    act, dz, acc = ABG_MODES[(ABG_ROWS.index(rows) + 3) % 6]
    n = 3 if rows == 600001 else 5
    abg(dev, L, rows, n, act, dz, True, acc, (n + 1, n, n + 2), seed=6)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dz", ["none", "alias", "sep"])
@pytest.mark.parametrize("acc", [0, 1])
def test_act_bias_grad_modes(dev, L, act, dz, acc):
    abg(dev, L, 257, 65, act, dz, True, acc, (70, 66, 70), (2, 1, 3), seed=7)


def test_act_bias_grad_edges_and_refusals(dev, L):
    abg(dev, L, 0, 24, 1, "sep", True, 0)                    # rows = 0: dbias zeroed ...
    abg(dev, L, 0, 24, 1, "sep", True, 1)                    # ... or left
    abg(dev, L, 0, 24, 1, "sep", False, 0)
    abg(dev, L, 3001, 24, 1, "sep", True, 1, short=1, expect=INVALID)        # scratch one float too small
    abg(dev, L, 600001, 3, 1, "sep", True, 1, short=1, expect=INVALID)
    lib, st = L.lib(), L.stream_ptr(dev)
    a, b, d = Strided(dev, 8, 4, data=np.ones((8, 4))), Strided(dev, 8, 4, data=np.ones((8, 4))), Guarded(dev, 4, fill=1.0)
    sc = Guarded(dev, 64)
    for rows, n, y in [(-1, 4, b.ptr()), (8, -1, b.ptr()), (8, 4, None)]:    # negative sizes; act without Y
        assert lib.dispu_act_bias_grad(rows, n, a.ptr(), 4, y, 4, 1, a.ptr(), 4, d.ptr(), 1, sc.ptr(), 64, st) == INVALID
    assert lib.dispu_act_bias_grad(8, 4, a.ptr(), 4, b.ptr(), 4, 1, a.ptr(), 4, d.ptr(), 1, None, 64, st) == INVALID
    for act, db in [(0, None), (1, None), (1, d.ptr())]:                     # dZ = dY's pointer under another stride: not "in place"
        assert lib.dispu_act_bias_grad(4, 2, a.ptr(), 4, b.ptr(), 4, act, a.ptr(), 8, db, 1, sc.ptr(), 64, st) == INVALID
    assert lib.dispu_act_bias_grad(8, 0, a.ptr(), 4, b.ptr(), 4, 1, a.ptr(), 4, d.ptr(), 1, sc.ptr(), 64, st) == 0    # n = 0: nothing to do
    torch.cuda.synchronize()
    assert a.untouched() and b.untouched() and same_bits(d.body(), np.ones(4, F32)) and d.guards_intact()
    assert lib.dispu_act_bias_grad_scratch_floats(0, 4) == 0 and lib.dispu_act_bias_grad_scratch_floats(4, -1) == 0


# ----------------------------------------------------------------- dispu_max_k, dispu_max_k_grad, dispu_max_k_grad_tail ----
MK_CASES = [
    # (rows, ns, c, ldx, ldo, lddy, lddx, accumulate, tail)
    (2048, 16, 96, 120, 480, 480, 128, 0, 24),     # the trainer's own call: width = 72 + C of the edge tensor into / out of a 480-wide buffer
    (257, 1, 1, 3, 2, 5, 4, 1, 0),                 # one neighbour, one channel: the maximum is the entry
    (1000, 2, 120, 121, 123, 122, 125, 1, 1),      # every stride different and odd
    (513, 20, 96, 100, 97, 99, 130, 0, 24),
    (300, 16, 120, 120, 120, 120, 120, 1, 0),      # compact
    (70000, 2, 64, 66, 65, 64, 67, 0, 1),          # 4 480 000 outputs (4 550 000 with the tail): second trip of the grid-stride loops
]


@pytest.mark.parametrize("case", MK_CASES, ids=ids(MK_CASES))
def test_max_k_and_its_gradients(dev, L, case):
    """ties in every case (train_ops_oracle.with_ties): column 0 is an all-tie (the `central` half of an edge feature), column 1 holds
    an ns-way tie at zero, column 2 two-way ties at a negative maximum."""
    rows, ns, c, ldx, ldo, lddy, lddx, acc, tail = case
    rng = np.random.default_rng(rows + ns)
    X = TO.with_ties(rng.standard_normal((rows * ns, c)).astype(F32), ns)
    X3 = X.reshape(rows, ns, c)
    sx = Strided(dev, rows * ns, c, ldx, 0, X)
    so = Strided(dev, rows, c, ldo, (ldo - c) // 2)
    ok(L, dev, "dispu_max_k", rows, ns, c, sx.ptr(), ldx, so.ptr(), ldo)
    assert same_bits(so.data(), TO.max_k(X3)) and so.rest_untouched() and sx.untouched()
    g = rng.standard_normal((rows, c)).astype(F32)
    sg = Strided(dev, rows, c, lddy, lddy - c, g)
    dX0 = rng.standard_normal((rows * ns, c)).astype(F32)
    sd = Strided(dev, rows * ns, c, lddx, (lddx - c) // 2, dX0)
    ok(L, dev, "dispu_max_k_grad", rows, ns, c, sx.ptr(), ldx, so.ptr(), ldo, sg.ptr(), lddy, sd.ptr(), lddx, acc)   # Y: the device's own
    grad = TO.max_k_grad(X3, g).reshape(rows * ns, c)
    what = "%d x %d x %d" % (rows, ns, c)
    close(sd.data(), grad + (dX0 if acc else 0.0), 1e-6, "max_k_grad %s accumulate %d" % (what, acc))
    assert sd.rest_untouched() and so.rest_untouched() and sg.untouched()
    if not acc:
        assert not sd.data()[grad == 0].any(), "entries below the maximum must be exactly zero"
    w = c + tail
    st_ = Strided(dev, rows * ns, w, w + 5, 2, np.full((rows * ns, w), 7.0, F32))
    ok(L, dev, "dispu_max_k_grad_tail", rows, ns, c, tail, sx.ptr(), ldx, so.ptr(), ldo, sg.ptr(), lddy, st_.ptr(), w + 5)
    got = st_.data()
    close(got[:, :c], grad, 1e-6, "max_k_grad_tail %s tail %d" % (what, tail))
    assert same_bits(got[:, c:], np.zeros((rows * ns, tail), F32)) and st_.rest_untouched()
    assert not got[:, :c][grad == 0].any()


# --------------------------------------------------------------------------------------- dispu_edge_feature_grad ----
EF_CASES = [
    # (B, n, k, c, ioff, ldi, lde, eoff, lddf, foff, kind)
    (2, 64, 16, 24, 1, 17, 56, 8, 24, 0, "random"),        # the shape of tests/test_train_gpu.py
    (8, 256, 16, 24, 1, 17, 120, 72, 480, 96, "random"),   # as the trainer passes it: dE + 72 of a 120-wide buffer, k + 1 lists, dF in 480
    (1, 36, 1, 5, 0, 3, 84, 72, 7, 1, "hub"),              # one neighbour, first column of a wider list
    (3, 100, 20, 48, 2, 25, 172, 72, 50, 2, "random"),     # lists that start two columns in
    (3, 100, 16, 24, 0, 18, 48, 0, 24, 0, "hub"),          # cloud 0: 1600 atomic terms per channel on point 0
    (3, 36, 20, 5, 2, 23, 13, 3, 5, 0, "self"),            # no point is anyone's neighbour but its own
    (342, 256, 1, 48, 1, 3, 96, 0, 48, 0, "random"),       # 4 202 496 outputs: second trip of the grid-stride loop
]


@pytest.mark.parametrize("case", EF_CASES, ids=ids(EF_CASES))
def test_edge_feature_grad(dev, L, case):
    """dF starts non-zero (the entry accumulates); the unused columns of the index lists hold other valid indices."""
    B, n, k, c, ioff, ldi, lde, eoff, lddf, foff, kind = case
    rng = np.random.default_rng(B * n + k)
    idx = TO.knn_like(rng, B, n, k, kind)
    lists = rng.integers(0, n, (B * n, ldi)).astype(np.int32)
    lists[:, ioff:ioff + k] = idx.reshape(B * n, k)
    dE = rng.standard_normal((B * n * k, 2 * c)).astype(F32)
    dF0 = rng.standard_normal((B * n, c)).astype(F32)
    se, sf = Strided(dev, B * n * k, 2 * c, lde, eoff, dE), Strided(dev, B * n, c, lddf, foff, dF0)
    ok(L, dev, "dispu_edge_feature_grad", B * n, n, k, c, se.ptr(), lde, p(dv(lists, dev)), ldi, ioff, sf.ptr(), lddf)
    ref = dF0 + TO.edge_feature_grad(dE.reshape(B, n, k, 2 * c), idx, c).reshape(B * n, c)
    close(sf.data(), ref, 1e-5, "edge_feature_grad %s" % (case,))
    assert sf.rest_untouched() and se.untouched()


# ----------------------------------------------------------------------------- dispu_ps_group, dispu_ps_group_grad ----
PG_CASES = [
    # (B, n, k, cf, ldf, ldg, kind)
    (2, 128, 16, 128, 128, 134, "random"),     # the shape of tests/test_train_gpu.py
    (3, 50, 1, 0, 4, 8, "random"),             # no features at all, one neighbour
    (2, 64, 16, 1, 3, 9, "hub"),               # cloud 0: 1024 atomic terms on point 0
    (8, 256, 16, 128, 130, 136, "random"),     # 2048 x 16 x 134 = 4 390 912 elements: second trip of both grid-stride loops
    (5, 100, 16, 128, 132, 134, "hub"),
]


@pytest.mark.parametrize("case", PG_CASES, ids=ids(PG_CASES))
def test_ps_group_and_grad(dev, L, case):
    B, n, k, cf, ldf, ldg, kind = case
    rng = np.random.default_rng(n + cf)
    rows, w = B * n, 6 + cf
    idx = TO.knn_like(rng, B, n, k, kind)
    xyz = rng.standard_normal((B, n, 3)).astype(F32)
    feat = rng.standard_normal((B, n, cf)).astype(F32)
    di, dx = dv(idx, dev), dv(xyz, dev)
    sfeat = Strided(dev, rows, cf, ldf, ldf - cf, feat)
    sg = Strided(dev, rows * k, w, ldg, ldg - w)
    ok(L, dev, "dispu_ps_group", rows, n, k, cf, p(di), p(dx), sfeat.ptr(), ldf, sg.ptr(), ldg)
    assert same_bits(sg.data(), TO.ps_group(xyz, feat, idx).reshape(rows * k, w)) and sg.rest_untouched() and sfeat.untouched()
    g = rng.standard_normal((rows * k, w)).astype(F32)
    dxyz0, dfeat0 = rng.standard_normal((rows, 3)).astype(F32), rng.standard_normal((rows, cf)).astype(F32)
    sdg = Strided(dev, rows * k, w, ldg, 0, g)
    gx = Guarded(dev, rows * 3, fill=dxyz0)
    sdf = Strided(dev, rows, cf, ldf + 1, 1, dfeat0)
    ok(L, dev, "dispu_ps_group_grad", rows, n, k, cf, p(di), sdg.ptr(), ldg, gx.ptr(), sdf.ptr(), ldf + 1)
    rx, rf = TO.ps_group_grad(g.reshape(B, n, k, w), idx, cf)
    close(gx.body().reshape(rows, 3), dxyz0 + rx.reshape(rows, 3), 1e-5, "ps_group_grad dxyz %s" % (case,))
    close(sdf.data(), dfeat0 + rf.reshape(rows, cf), 1e-5, "ps_group_grad dfeat %s" % (case,))
    assert gx.guards_intact() and sdf.rest_untouched() and sdg.untouched()


# ------------------------------------------------------------------------------------ dispu_ps_point_matmul_grad ----
@pytest.mark.parametrize("rows", [1, 37, 8192, 8200])       # 8192 workgroups at most: 8200 rows send eight of them round their loop again
def test_point_matmul_grad(dev, L, rows):
    rng = np.random.default_rng(rows)
    k, c, t = 16, 128, 16
    ldx2, lddx2, ldo = 130, 132, c * t + 4                   # every stride wider than the data
    X2 = rng.standard_normal((rows * k, c)).astype(F32)
    wv = rng.standard_normal((rows * k, t)).astype(F32)
    do = rng.standard_normal((rows, c * t)).astype(F32)
    sx, so = Strided(dev, rows * k, c, ldx2, 2, X2), Strided(dev, rows, c * t, ldo, 4, do)
    sd = Strided(dev, rows * k, c, lddx2, 1)
    gw = Guarded(dev, rows * k * t)
    ok(L, dev, "dispu_ps_point_matmul_grad", rows, k, c, t, sx.ptr(), ldx2, p(dv(wv, dev)), so.ptr(), ldo, sd.ptr(), lddx2, gw.ptr())
    rX, rW = TO.point_matmul_grad(X2.reshape(rows, k, c), wv.reshape(rows, k, t), do)
    close(sd.data(), rX.reshape(rows * k, c), 1e-5, "point_matmul_grad dX2, %d rows" % rows)
    close(gw.body().reshape(rows * k, t), rW.reshape(rows * k, t), 1e-5, "point_matmul_grad dwv, %d rows" % rows)
    assert sd.rest_untouched() and gw.guards_intact() and sx.untouched() and so.untouched()


# --------------------------------------------------------------------------------------- dispu_softmax_rows_grad ----
SM_CASES = [
    # (rows, n, ldp, lddp, mul)
    (1, 1, 1, 3, 0.125),               # a single probability of exactly 1: dS is exactly zero
    (2, 63, 64, 70, 1.0),              # one trip of the lane loop, last lane idle
    (5, 64, 64, 64, 0.125),            # exactly one trip; five rows: the second workgroup has one wave of work
    (5, 65, 66, 67, 1.0),              # a second trip for lane 0 only
    (2, 1000, 1001, 1003, 0.125),
    (5, 4096, 4100, 4096, 1.0),        # the attention's own row length at 4 x 1024 points
    (65537, 8, 9, 10, 0.125),          # one row more than 16384 workgroups x 4 waves: second trip of the row loop
]


@pytest.mark.parametrize("case", SM_CASES, ids=ids(SM_CASES))
def test_softmax_rows_grad(dev, L, case):
    rows, n, ldp, lddp, mul = case
    rng = np.random.default_rng(n)
    S = rng.standard_normal((rows, n)) * 4 * mul
    P = np.exp(S - S.max(-1, keepdims=True))
    P = (P / P.sum(-1, keepdims=True)).astype(F32)
    P[0] = 0.0
    P[0, n // 2] = 1.0                                       # a one-hot row: P exactly 1 and 0
    g = rng.standard_normal((rows, n)).astype(F32)
    sp, sd = Strided(dev, rows, n, ldp, ldp - n, P), Strided(dev, rows, n, lddp, lddp - n, g)
    ok(L, dev, "dispu_softmax_rows_grad", rows, n, mul, sp.ptr(), ldp, sd.ptr(), lddp)
    close(sd.data(), TO.softmax_rows_grad(P, g, mul), 1e-5, "softmax_rows_grad %s" % (case,))
    assert not sd.data()[0].any(), "the one-hot row's gradient must be exactly zero"
    assert sd.rest_untouched() and sp.untouched()


# ------------------------------------------------------------------------------ dispu_bn_train, dispu_bn_train_grad ----
EPS, DECAY = 1e-3, 0.95


def bn_inputs(rng, rows, c, special=None):
    """X [rows, c] with its own scale and shift per column; column 0 constant where there are two columns or more; `special`
    (mean, std) for column 1.  Where the float64 pre-activation gamma * xhat + beta comes within 2e-5 of its largest entry of zero the
    input is moved until it does not: an fp32 evaluation may then not take the other side of the ReLU."""
    X = (rng.standard_normal((rows, c)) * rng.uniform(0.5, 2, c) + rng.standard_normal(c)).astype(F32)
    if c >= 2:
        X[:, 0] = 3.0
    if special is not None:
        X[:, 1] = (special[0] + special[1] * rng.standard_normal(rows)).astype(F32)
    gamma = rng.uniform(0.5, 1.5, c).astype(F32)
    beta = ((0.02 + np.abs(rng.standard_normal(c) * 0.1)) * rng.choice([-1.0, 1.0], c)).astype(F32)
    for _ in range(20):
        pre = TO.bn_train(X, gamma, beta, EPS, DECAY, 0)["pre"]
        near = np.abs(pre) < 2e-5 * np.abs(pre).max()
        if not near.any():
            return X, gamma, beta
        X[near] += (np.abs(X[near]) * 1e-3 + 1e-3).astype(F32)
    raise AssertionError("could not move the inputs off the ReLU's edge")


def bn_scratch(dev, L, rows, c):
    nb = L.lib().dispu_bn_scratch_bytes(rows, c)
    assert nb > 0 and nb % 8 == 0
    return Guarded(dev, nb // 4), nb


def bn_both(dev, L, rows, c, ldx, ldy, lddy, lddx, act, alias, moving, dgb, special=None, what="", scratch_buf=None, seed=0):
    """bn_train, then bn_train_grad on its outputs.  scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(),
    .guards_intact()) in place of the sentinel-filled one; seed: other inputs of the same sizes"""
    rng = np.random.default_rng(rows + c + seed)
    X, gamma, beta = bn_inputs(rng, rows, c, special)
    mm0, mv0 = rng.standard_normal(c).astype(F32), rng.uniform(0.5, 1.5, c).astype(F32)
    f = TO.bn_train(X, gamma, beta, EPS, DECAY, act, mm0, mv0)
    sx = Strided(dev, rows, c, ldx, ldx - c, X)
    sy = sx if alias else Strided(dev, rows, c, ldy, (ldy - c) // 2)
    stats = Guarded(dev, 3 * c)
    gm, gv = (Guarded(dev, c, fill=mm0), Guarded(dev, c, fill=mv0)) if moving else (None, None)
    ga, be = dv(gamma, dev), dv(beta, dev)
    sc, nb = bn_scratch(dev, L, rows, c)
    if scratch_buf is not None:
        sc = scratch_buf
    ok(L, dev, "dispu_bn_train", rows, c, sx.ptr(), sx.ld, p(ga), p(be), EPS, DECAY, act, sy.ptr(), sy.ld, stats.ptr(),
       gm.ptr() if moving else None, gv.ptr() if moving else None, sc.ptr(), nb)
    what = "bn %d x %d act %d %s" % (rows, c, act, what)
    s = stats.body()
    close(s[:c], f["mean"], 1e-5, what + " mean")
    close(s[c:2 * c], f["var"], 1e-5, what + " var")
    close(s[2 * c:], f["istd"], 1e-5, what + " 1/std")
    if moving:
        close(gm.body(), f["moving_mean"], 1e-6, what + " moving_mean")
        close(gv.body(), f["moving_var"], 1e-6, what + " moving_var")
        assert gm.guards_intact() and gv.guards_intact()
    y = sy.data().copy()
    close(y, f["y"], 1e-5, what + " y")
    if act:
        assert np.array_equal(y > 0, f["pre"] > 0), what + ": a ReLU decision differs from the float64 reference"
    assert sy.rest_untouched() and stats.guards_intact() and sc.guards_intact() and (alias or sx.untouched())
    # the gradient: the mask is read from the DEVICE's own Y (checked above to take the reference's side everywhere)
    g = rng.standard_normal((rows, c)).astype(F32)
    sx2 = Strided(dev, rows, c, ldx, 0, X) if alias else sx
    sy2 = Strided(dev, rows, c, ldy, ldy - c, y)
    sg = Strided(dev, rows, c, lddy, (lddy - c) // 2, g)
    sd = Strided(dev, rows, c, lddx, lddx - c)
    dga0, dbe0 = rng.standard_normal(c).astype(F32), rng.standard_normal(c).astype(F32)
    gga, gbe = (Guarded(dev, c, fill=dga0), Guarded(dev, c, fill=dbe0)) if dgb else (None, None)
    sums = Guarded(dev, 2 * c)
    ok(L, dev, "dispu_bn_train_grad", rows, c, sx2.ptr(), ldx, sy2.ptr(), ldy, sg.ptr(), lddy, stats.ptr(), p(ga), act, sd.ptr(), lddx,
       gga.ptr() if dgb else None, gbe.ptr() if dgb else None, sums.ptr(), sc.ptr(), nb)
    rdx, rdga, rdbe = TO.bn_train_grad(X, f["pre"] > 0 if act else np.ones((rows, c), bool), g, gamma, EPS)
    close(sd.data(), rdx, 2e-5, what + " dx")
    close(sums.body()[:c], rdbe, 1e-5, what + " sum dz")
    close(sums.body()[c:], rdga, 1e-5, what + " sum dz xhat")
    if dgb:
        close(gga.body(), dga0 + rdga, 1e-5, what + " dgamma")
        close(gbe.body(), dbe0 + rdbe, 1e-5, what + " dbeta")
        assert gga.guards_intact() and gbe.guards_intact()
    assert sd.rest_untouched() and sums.guards_intact() and sc.guards_intact() and sx2.untouched() and sy2.untouched() and sg.untouched()


BN_CASES = [
    # (rows, c, ldx, ldy, lddy, lddx, act, Y aliases X, moving statistics, dgamma / dbeta)
    (1, 1, 1, 1, 1, 1, 1, 0, 1, 1),                # a single row: variance 0, no Bessel correction, dx = 0
    (2, 2, 3, 4, 5, 6, 0, 0, 1, 1),
    (1023, 4, 4, 4, 4, 4, 1, 1, 0, 1),             # one row short of a full block; no moving statistics
    (1025, 8, 10, 10, 9, 11, 0, 1, 1, 0),          # one row into a second block; in place in a wider buffer; dgamma = dbeta = NULL
    (65537, 16, 16, 16, 16, 16, 1, 1, 1, 1),       # 65 partials: lane 0 of the finalize kernels adds two; in place, as tf_util.py calls it
    (70000, 32, 40, 33, 32, 36, 1, 0, 1, 1),       # 69 partials, four different strides
    (40000, 64, 64, 66, 65, 64, 0, 0, 1, 1),       # the widest accepted: four rows per pass of a block
    (70000, 64, 66, 65, 67, 68, 1, 0, 1, 1),       # 4 480 000 elements: second trip of bn_apply's and bn_grad_apply's grid-stride loops
    (1048577, 2, 2, 3, 2, 2, 1, 0, 1, 1),          # above 1024 x 1024 rows bn_blocks re-derives rows_per_block (1025)
]


@pytest.mark.parametrize("case", BN_CASES, ids=ids(BN_CASES))
def test_bn_train_and_grad(dev, L, case):
    """column 0 is constant wherever there are two columns (variance exactly 0: the clamp, 1/sqrt(eps))."""
    bn_both(dev, L, *case)


def test_bn_train_and_grad_large_mean_small_spread(dev, L):
    """column 1 has mean 100 and standard deviation 0.01: x - mean cancels four digits.  The margin of `y` is thin by construction:
    `stats` holds the mean as a float32, off by up to half an ulp of 100 (3.8e-6), which is 1.2e-4 of a deviation with eps = 1e-3 and,
    times gamma, up to 4e-5 of the largest entry of y -- four times the bound.  With this seed the mean happens to round 2.6e-6 off
    and y lands at 9.6e-6: another seed, row count or summation order may well miss, and the stats layout (three floats per channel)
    leaves the forward no room to do better.  The gradient does not share the problem: it measures the offset (sum xhat) and removes
    it."""
    bn_both(dev, L, 4096, 4, 4, 4, 4, 4, 1, 0, 1, 1, special=(100.0, 0.01), what="(column 1: mean 100, std 0.01)")


def test_bn_refusals(dev, L):
    rows = 64
    x, y = Strided(dev, rows, 128, data=np.ones((rows, 128))), Strided(dev, rows, 128)
    stats, sums, mm = Guarded(dev, 3 * 128), Guarded(dev, 2 * 128), Guarded(dev, 128, fill=1.0)
    ga = dv(np.ones(128, F32), dev)
    sc = Guarded(dev, 4096)

    def fwd(rows_, c, scp, nbytes):
        return run(L, dev, "dispu_bn_train", rows_, c, x.ptr(), 128, p(ga), p(ga), EPS, DECAY, 1, y.ptr(), 128, stats.ptr(), mm.ptr(), mm.ptr(), scp, nbytes)

    def bwd(rows_, c, scp, nbytes, sm):
        return run(L, dev, "dispu_bn_train_grad", rows_, c, x.ptr(), 128, x.ptr(), 128, x.ptr(), 128, stats.ptr(), p(ga), 1, y.ptr(), 128,
                   mm.ptr(), mm.ptr(), sm, scp, nbytes)

    for c in (3, 24, 65, 128, 0, -1):                       # c must divide 256 and be at most 64
        assert fwd(rows, c, sc.ptr(), 4 * 4096) == INVALID and bwd(rows, c, sc.ptr(), 4 * 4096, sums.ptr()) == INVALID, c
    for r in (0, -1):
        assert fwd(r, 16, sc.ptr(), 4 * 4096) == INVALID and bwd(r, 16, sc.ptr(), 4 * 4096, sums.ptr()) == INVALID
    for r, c in [(rows, 16), (70000, 32), (1048577, 2)]:    # scratch one byte short, or missing: the gradient keeps three partial
        nb = L.lib().dispu_bn_scratch_bytes(r, c)           # sums per block and channel, the forward two of them
        assert 0 < nb <= 4 * 4096 * 16 and nb % 3 == 0
        assert fwd(r, c, sc.ptr(), nb // 3 * 2 - 1) == INVALID and bwd(r, c, sc.ptr(), nb - 1, sums.ptr()) == INVALID
        assert fwd(r, c, None, nb) == INVALID and bwd(r, c, None, nb, sums.ptr()) == INVALID
    assert bwd(rows, 16, sc.ptr(), 4 * 4096, None) == INVALID                                     # sums is not optional
    assert L.lib().dispu_bn_scratch_bytes(0, 16) == 0 and L.lib().dispu_bn_scratch_bytes(16, 0) == 0
    assert x.untouched() and y.untouched() and stats.guards_intact() and sums.guards_intact() and sc.guards_intact()
    assert same_bits(stats.body(), np.full(3 * 128, SENT, F32)) and same_bits(mm.body(), np.ones(128, F32)) and same_bits(sc.body(), np.full(4096, SENT, F32))


# ------------------------------------------------------------------------------------------ dispu_repulsion_grad ----
H, BALL = 0.001, 0.07


@pytest.mark.parametrize("B,M,ns", [(3, 100, 20), (2, 1024, 20), (17, 64, 5), (5, 333, 5)])      # 300 / 1088 / 1665 rows: none a multiple of 256
def test_repulsion_grad(dev, L, B, M, ns):
    _, pred = LO.jittered_pair(B, M, M, seed=M)
    if M < 1024:
        pred = (pred * (M / 1024.0) ** 0.5).astype(F32)        # the density of a 1024-point patch: the 0.07 balls are not all empty
    idx, _ = O.query_ball_point(BALL, ns, pred, pred)
    scale = 1.0 / (B * M * 4)
    ref = TO.repulsion_grad(pred, idx, H, scale)
    assert np.abs(ref).max() > 0
    d0 = (np.random.default_rng(M).standard_normal((B, M, 3)) * np.abs(ref).max()).astype(F32)     # dpred accumulates
    gd = Guarded(dev, B * M * 3, fill=d0)
    ok(L, dev, "dispu_repulsion_grad", B * M, M, ns, H, scale, p(dv(pred, dev)), p(dv(idx.astype(np.int32), dev)), gd.ptr())
    close(gd.body().reshape(B, M, 3), d0 + ref, 1e-4, "repulsion_grad %d x %d ns %d" % (B, M, ns))
    assert gd.guards_intact()


def test_repulsion_grad_by_hand(dev, L):
    """six different neighbours at exactly the same distance (+-0.01 along the axes) in slots 1..6 behind the point itself: slots 1..4
    carry 2 * scale * 0.01 each along their own axis, slots 5 and 6 nothing (tf.nn.top_k puts the lower index first among equals)."""
    M, ns, scale = 7, 20, 0.25
    pred = np.zeros((1, M, 3), F32)
    for k in range(6):
        pred[0, 1 + k, k // 2] = F32(0.01) * (1 if k % 2 == 0 else -1)
    idx = np.tile(np.arange(M, dtype=np.int32)[None, :, None], (1, 1, ns))
    idx[0, 0] = [0, 1, 2, 3, 4, 5, 6] + [1] * (ns - 7)
    e = 2 * scale * float(F32(0.01))
    want = np.zeros((M, 3))
    want[1, 0], want[2, 0], want[3, 1], want[4, 1] = -e, e, -e, e
    assert np.allclose(TO.repulsion_grad(pred, idx, H, scale)[0], want, rtol=1e-12, atol=1e-18)      # row 0: the four terms cancel in pairs
    gd = Guarded(dev, M * 3, fill=0.0)
    ok(L, dev, "dispu_repulsion_grad", M, M, ns, H, scale, p(dv(pred, dev)), p(dv(idx, dev)), gd.ptr())
    got = gd.body().reshape(M, 3)
    close(got, want, 1e-4, "repulsion_grad, six-way tie")
    assert not got[5:].any() and not got[0].any() and gd.guards_intact()


# ---------------------------------------------------------------------------------------------------- dispu_adam ----
@pytest.mark.parametrize("total,gscale", [(1, 1.0), (255, 0.5), (5000, 1.0), (4194305, 0.5)])     # one element past 16384 x 256
def test_adam(dev, L, total, gscale):
    """ten steps from non-zero moments; every fifth parameter has a gradient of exactly zero and v = 0, so its update is
    -lr_t m / eps (m is sized so that this is an update like the others).  The reference takes the float32 values of the scalar
    arguments, as the kernel receives them.  p is sized like the network's weights (0.05): the bound is on the UPDATE, and half an
    ulp of a parameter of size 5 per step would be 1e-4 of a ten-step update by itself."""
    rng = np.random.default_rng(total)
    p0, g = (rng.standard_normal(total) * 0.05).astype(F32), rng.standard_normal(total).astype(F32)     # p at the scale of the weights
    m0, v0 = (rng.standard_normal(total) * 0.1).astype(F32), rng.uniform(0.01, 1.0, total).astype(F32)
    g[::5], v0[::5] = 0.0, 0.0
    m0[::5] = (rng.standard_normal(m0[::5].shape) * 1e-8).astype(F32)
    b1, b2, eps = float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    gp, gm, gv = Guarded(dev, total, fill=p0), Guarded(dev, total, fill=m0), Guarded(dev, total, fill=v0)
    gg = Guarded(dev, total, fill=g)
    rp, rm, rv = p0, m0, v0
    for t in range(11, 21):
        lr_t = float(F32(1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        ok(L, dev, "dispu_adam", total, gp.ptr(), gg.ptr(), gm.ptr(), gv.ptr(), lr_t, b1, b2, eps, gscale)
        rp, rm, rv = TO.adam(rp, g, rm, rv, lr_t, b1, b2, eps, gscale)
    assert np.abs((rp - p0)[::5]).max() > 0                      # the zero-gradient parameters did move
    close(gp.body().astype(np.float64) - p0, rp - p0, 1e-4, "adam update, %d x 10 steps" % total)
    close(gm.body(), rm, 1e-5, "adam m")
    close(gv.body(), rv, 1e-5, "adam v")
    assert not gv.body()[::5].any()
    assert gp.guards_intact() and gm.guards_intact() and gv.guards_intact() and same_bits(gg.body(), g) and gg.guards_intact()


# ----------------------------------------------------------------------------------------------- dispu_fill_rows ----
@pytest.mark.parametrize("b,n", [(1, 1), (3, 100), (64, 1024), (5, 1000000)])      # 5 000 000 elements: second trip of the grid-stride loop
@pytest.mark.parametrize("mul", [1.0, 1.0 / 1024])
def test_fill_rows(dev, L, b, n, mul):
    val = np.random.default_rng(b).standard_normal(b).astype(F32)
    out = Guarded(dev, b * n)
    ok(L, dev, "dispu_fill_rows", b, n, p(dv(val, dev)), mul, out.ptr())
    assert same_bits(out.body().reshape(b, n), TO.fill_rows(val, mul, n)) and out.guards_intact()


# ------------------------------------------------------------------------------------ dispu_linear_splitk_finish ----
SK_CASES = [
    # (rows, n, nparts, bias, act, ldy, yoff, gap between the partials)
    (300, 4, 1, 0, 0, 4, 0, 0),
    (300, 24, 2, 1, 1, 28, 4, 0),
    (301, 256, 3, 1, 0, 256, 0, 8),
    (8192, 256, 4, 1, 1, 256, 0, 0),           # the trainer's own: after_conv at 8 patches
    (33, 8, 5, 0, 1, 16, 8, 4),
    (1000, 132, 6, 1, 1, 136, 0, 12),
    (7, 64, 7, 0, 0, 64, 0, 0),
    (513, 12, 8, 1, 1, 20, 4, 4),
    (65537, 256, 2, 1, 1, 256, 0, 0),          # 4 194 368 quads: second trip of the grid-stride loop
]


@pytest.mark.parametrize("case", SK_CASES, ids=ids(SK_CASES))
def test_splitk_finish(dev, L, case):
    """bit-exact against float32 numpy in the documented order ((P0 + P1) + ...) + bias, then max(., 0): the kernel only adds.  The
    partials differ in magnitude (x 4^s), so another association rounds differently."""
    rows, n, nparts, bias, act, ldy, yoff, gap = case
    rng = np.random.default_rng(rows + nparts)
    stride = rows * n + gap
    parts = (rng.standard_normal((nparts, stride)) * 4.0 ** np.arange(nparts)[:, None]).astype(F32)
    b = rng.standard_normal(n).astype(F32) if bias else None
    gp = Guarded(dev, nparts * stride, fill=parts)
    sy = Strided(dev, rows, n, ldy, yoff)
    ok(L, dev, "dispu_linear_splitk_finish", rows, n, nparts, gp.ptr(), stride, p(dv(b, dev)) if bias else None, act, sy.ptr(), ldy)
    ref = TO.splitk_finish([parts[s, :rows * n].reshape(rows, n) for s in range(nparts)], b, act)
    assert np.array_equal(sy.data(), ref), "splitk_finish differs from the ordered float32 sum in %d entries" % int((sy.data() != ref).sum())
    assert sy.rest_untouched() and same_bits(gp.body(), parts.reshape(-1)) and gp.guards_intact()


def test_splitk_finish_refusals(dev, L):
    rows, n = 16, 8
    gp = Guarded(dev, 9 * rows * n + 8, fill=1.0)
    sy = Strided(dev, rows, n, 12, 4)
    gb = Guarded(dev, n + 4, fill=1.0)

    def call(rows_=rows, n_=n, nparts=2, part=gp.ptr(), stride=rows * n, bias=gb.ptr(), y=sy.ptr(), ldy=12):
        return run(L, dev, "dispu_linear_splitk_finish", rows_, n_, nparts, part, stride, bias, 1, y, ldy)

    assert call(n_=6) == INVALID and call(n_=0) == INVALID and call(n_=-4) == INVALID and call(rows_=-1) == INVALID
    assert call(nparts=0) == INVALID and call(nparts=9) == INVALID
    assert call(ldy=13) == INVALID and call(ldy=14) == INVALID and call(stride=rows * n + 2) == INVALID
    assert call(part=None) == INVALID and call(y=None) == INVALID
    assert call(part=gp.ptr(1)) == INVALID and call(y=sy.G.ptr(5)) == INVALID and call(bias=gb.ptr(1)) == INVALID
    assert call(rows_=0) == 0
    assert sy.untouched() and gp.guards_intact() and gb.guards_intact()
    assert call() == 0 and call(bias=None, nparts=8) == 0 and not sy.untouched()       # the same arguments, valid, do write


# --------------------------------------------------------------------- sizes every other entry refuses or ignores ----
def test_refusals_and_noops_write_nothing(dev, L):
    """negative sizes, ns <= 0, c <= 0 and the unsupported (k, c, t_n) are refused; rows = 0 / total = 0 is a no-op; neither writes."""
    rng = np.random.default_rng(0)
    bufs = [Guarded(dev, 4096, fill=rng.standard_normal(4096).astype(F32)) for _ in range(5)]
    a, b, c, d, e = [g.ptr() for g in bufs]
    before = [g.body().copy() for g in bufs]
    idx = p(dv(np.zeros(4096, np.int32), dev))

    def r(name, *args):
        return run(L, dev, name, *args)

    for rows, ns, ch, want in [(-1, 4, 4, INVALID), (4, 0, 4, INVALID), (4, -1, 4, INVALID), (4, 4, 0, INVALID), (4, 4, -2, INVALID), (0, 4, 4, 0)]:
        assert r("dispu_max_k", rows, ns, ch, a, 4, b, 4) == want
        assert r("dispu_max_k_grad", rows, ns, ch, a, 4, b, 4, c, 4, d, 4, 0) == want
        assert r("dispu_max_k_grad_tail", rows, ns, ch, 2, a, 4, b, 4, c, 4, d, 8) == want
    assert r("dispu_max_k_grad_tail", 4, 4, 4, -1, a, 4, b, 4, c, 4, d, 8) == INVALID
    for rows, n, k, ch, want in [(-1, 4, 2, 4, INVALID), (4, 0, 2, 4, INVALID), (4, 4, 0, 4, INVALID), (4, 4, 2, 0, INVALID), (0, 4, 2, 4, 0)]:
        assert r("dispu_edge_feature_grad", rows, n, k, ch, a, 8, idx, 2, 0, b, 4) == want
    for rows, n, k, cf, want in [(-1, 4, 2, 4, INVALID), (4, 0, 2, 4, INVALID), (4, 4, 0, 4, INVALID), (4, 4, 2, -1, INVALID), (0, 4, 2, 4, 0)]:
        assert r("dispu_ps_group", rows, n, k, cf, idx, a, b, 4, c, 10) == want
        assert r("dispu_ps_group_grad", rows, n, k, cf, idx, c, 10, d, e, 4) == want
    for rows, k, ch, t, want in [(1, 15, 128, 16, INVALID), (1, 16, 64, 16, INVALID), (1, 16, 128, 8, INVALID), (1, 8, 128, 8, INVALID),
                                 (1, 16, 127, 16, INVALID), (-1, 16, 128, 16, INVALID), (0, 16, 128, 16, 0)]:
        assert r("dispu_ps_point_matmul_grad", rows, k, ch, t, a, 128, b, c, 2048, d, 128, e) == want
    for rows, n, want in [(-1, 8, INVALID), (4, 0, INVALID), (4, -1, INVALID), (0, 8, 0)]:
        assert r("dispu_softmax_rows_grad", rows, n, 0.125, a, 8, b, 8) == want
    for rows, n, ns, want in [(8, 8, 4, INVALID), (8, 8, 0, INVALID), (-1, 8, 20, INVALID), (8, 0, 20, INVALID), (0, 8, 20, 0)]:
        assert r("dispu_repulsion_grad", rows, n, ns, H, 1.0, a, idx, b) == want
    assert r("dispu_adam", -1, a, b, c, d, 1e-3, 0.9, 0.999, 1e-8, 1.0) == INVALID and r("dispu_adam", 0, a, b, c, d, 1e-3, 0.9, 0.999, 1e-8, 1.0) == 0
    for bb, n, want in [(-1, 4, INVALID), (4, -1, INVALID), (0, 4, 0), (4, 0, 0)]:
        assert r("dispu_fill_rows", bb, n, a, 1.0, b) == want
    for g, was in zip(bufs, before):
        assert same_bits(g.body(), was) and g.guards_intact()
