"""Every kernel the dense-layer dispatch can pick (csrc/linear.hip, csrc/linear_skinny.hip), at its edges, through the C ABI:
dispu_linear, dispu_linear_bn and dispu_linear_masked on each of the five block tiles (forced with dispu_debug_linear_tile) x
{interior DMA pipeline, interior transposed-B, edge, edge transposed-B} x every epilogue, the skinny kernel in its four unroll depths
x transb, and the N-tail split.  The case table is tests/linear_paths.py; tests/test_linear_plan.py proves on the CPU that it covers
every instantiation the dispatch can reach and that every case takes the path its group names.  Here each case's plan is asked again
with the real device pointers and must be the one the CPU saw.

Reference: the pinned ascending-k fmaf chain (oracle.generator.linear) with the epilogue replayed in numpy fp32 in the kernel's order
(bias, ReLU, + R1, + R2, mask), compared bit for bit.  The BatchNorm fold v * scale + shift may be contracted to an fma, so its cases
are held to float64 evaluated on the bit-exact chain + bias, within 2^-22 (|y sc| + |sh| + |R1| + |R2|) elementwise (four fp32
roundings).  Operand padding is NaN, outputs sit between sentinel columns and guard rows that must come back untouched.

[measured] BatchNorm fold, all 40 cases, 660 500 outputs: 660 500 equal the unfused fp32 evaluation (the library is built with
-ffp-contract=off: the fold is a multiply and an add), 577 326 of them also equal the fused (fma) one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_paths as LP

pytestmark = pytest.mark.gpu

BN_STATS = {"n": 0, "fused": 0, "unfused": 0, "cases": 0}


@pytest.fixture()
def force_tile():
    """the tile override is process-global: whatever a test forces is undone when it ends"""
    from dispu_amd import _lib
    L = _lib.lib()
    try:
        yield L.dispu_debug_linear_tile
    finally:
        L.dispu_debug_linear_tile(0)


def _strided(size, start, stride, ld, blocks):
    buf = np.full(size, np.nan, np.float32)
    for z, b in enumerate(blocks):
        rows, cols = b.shape
        # one strided view per batch entry (no Python loop over rows)
        view = np.lib.stride_tricks.as_strided(buf[start + z * stride:], shape=(rows, cols), strides=(4 * ld, 4))
        view[...] = b
    return buf


def run_case(dev, _lib, c):
    """launch one case; returns its outputs [batch, M, N] after checking that nothing else in the Y buffer was written"""
    L = _lib.lib()
    lo = LP.layout(c)
    x, w, _ = LP.product(c.batch, c.M, c.K, c.N, c.shared)
    bias, scale, shift, r1, r2, mk = LP.operands(c)
    wz = [w[z].T if c.transb else w[z] for z in range(w.shape[0])]
    host = dict(x=_strided(lo.xsize, lo.xoff, lo.sx, lo.ldx, list(x)), w=_strided(lo.wsize, lo.woff, lo.sw, lo.ldw, wz),
                y=np.full(lo.ysize, LP.SENTINEL, np.float32), r1=_strided(lo.rsize, 0, lo.sr, lo.ldr, list(r1)),
                r2=_strided(lo.rsize, 0, lo.sr, lo.ldr, list(r2)), m=_strided(lo.msize, 0, 0, lo.ldm, [mk]),
                b=np.concatenate([bias, np.full(8, np.nan, np.float32)]), sc=np.concatenate([scale, np.full(8, np.nan, np.float32)]),
                sh=np.concatenate([shift, np.full(8, np.nan, np.float32)]))
    t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    base = {k: v.data_ptr() for k, v in t.items()}
    assert all(p % 16 == 0 for p in base.values())
    a = LP.plan_args(c, base)
    plan = _lib.linear_plan(*a)
    assert plan == _lib.linear_plan(*LP.plan_args(c)), (c, plan)           # the plan the CPU census saw
    P = lambda v: C.c_void_p(v) if v is not None else None
    head = a[:4] + (P(a[4]),) + a[5:7] + (P(a[7]),) + a[8:11] + (P(a[11]),)
    y3, r13, r23 = (P(a[15]),) + a[16:18], (P(a[18]),) + a[19:21], (P(a[21]),) + a[22:24]
    st = _lib.stream_ptr(dev)
    if c.entry == "linear":
        rc = L.dispu_linear(*head, a[14], *y3, *r13, *r23, st)
    elif c.entry == "bn":
        rc = L.dispu_linear_bn(*head, P(a[12]), P(a[13]), a[14], *y3, *r13, *r23, st)
    else:
        rc = L.dispu_linear_masked(*head, a[14], *y3, *r13, P(a[24]), a[25], a[26], st)
    _lib.check(rc, "dispu_%s %r" % (c.entry, (c,)))
    got = t["y"].cpu().numpy()
    rows, c0 = c.M + 2 * LP.GUARD, lo.yoff - LP.GUARD * lo.ldy
    out = np.empty((c.batch, c.M, c.N), np.float32)
    for z in range(c.batch):
        blk = got[z * lo.sy:(z + 1) * lo.sy].reshape(rows, lo.ldy)
        out[z] = blk[LP.GUARD:LP.GUARD + c.M, c0:c0 + c.N]
        blk[LP.GUARD:LP.GUARD + c.M, c0:c0 + c.N] = LP.SENTINEL
    assert (got == LP.SENTINEL).all(), "%r wrote outside its output: %d elements" % (c, int((got != LP.SENTINEL).sum()))
    return out, plan


def check_case(dev, _lib, c):
    got, plan = run_case(dev, _lib, c)
    want, bn = LP.expected(c)
    if bn is None:
        assert np.array_equal(got, want), "%r (plan %r): %d of %d outputs differ from the chain, first at %r" % (
            c, plan, int((got != want).sum()), got.size, tuple(np.argwhere(got != want)[0]))
    else:
        bound, fused, unfused = bn
        BN_STATS["n"] += got.size
        BN_STATS["cases"] += 1
        BN_STATS["fused"] += int((got == fused).sum())
        BN_STATS["unfused"] += int((got == unfused).sum())
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), "%r (plan %r): BatchNorm fold off by up to %.3g x its bound" % (c, plan, float((err / bound).max()))
    return plan


@pytest.mark.parametrize("group", [g for g in LP.GROUPS if g != "split"])
def test_linear_path(dev, force_tile, group):
    """one (tile, load path) or one (skinny depth, transb): every K, shape, layout, epilogue and batch case of the group"""
    from dispu_amd import _lib
    cases = [c for c in LP.CASES if c.group == group]
    for c in cases:
        force_tile(c.tile)
        plan = check_case(dev, _lib, c)
        want = LP.expected_launch(c)
        l = plan[0]
        assert len(plan) == 1 and (("skinny", l[3], l[4]) if l[0] == "skinny" else l[:1] + l[3:8]) == want, (c, plan)
    if BN_STATS["n"]:
        print("[measured] BatchNorm fold so far: %d cases, %d outputs, %d equal the fused fp32 evaluation, %d the unfused one"
              % (BN_STATS["cases"], BN_STATS["n"], BN_STATS["fused"], BN_STATS["unfused"]))


def test_linear_n_tail_split(dev, force_tile):
    """N = 128 + t: the tail of t <= 32 columns is a second launch on the skinny kernel with bias, R1 and the mask offset by n0 = 128
    (mcols - n0 negative, zero, positive); t = 33 stays one tiled launch."""
    from dispu_amd import _lib
    force_tile(0)
    for c in (c for c in LP.CASES if c.group == "split"):
        plan = check_case(dev, _lib, c)
        if c.N - 128 <= 32:
            assert [(l[0], l[1], l[2]) for l in plan] == [("skinny", 128, c.N), ("tiled", 0, 128)], (c, plan)
        else:
            assert [(l[0], l[1], l[2]) for l in plan] == [("tiled", 0, c.N)], (c, plan)
