"""The generator's forward glue kernels, each ALONE through the C ABI against tests/generator_ops_oracle.py (plain numpy written from
the reference ops and held to oracle/generator.py and oracle/modules.py by tests/test_generator_ops_oracle.py), on every path their
launch code takes.

Entries under test: csrc/mlp_misc.hip (dispu_linear_small_k, dispu_linear_small_n, dispu_dup_grid, dispu_ps_prep,
dispu_ps_gather_sub_relu, dispu_ps_skip_max, dispu_ps_weight_net, dispu_ps_point_matmul), csrc/attention.hip (dispu_attention,
dispu_attention_project), csrc/mlp_chain.hip (dispu_mlp_chain, _sum3, _dup at 64-row workgroups) and csrc/modules.hip
(dispu_pool_nsample, dispu_group_center, dispu_idw_weights, dispu_l2_normalize_rows, dispu_scale_add, dispu_edge_feature,
dispu_row_mean_max).  The generator's own shapes reach one path of each; here the shapes are chosen from the launch code: the float4 /
scalar switches (by a width, a stride and a pointer offset of one float), the general skip-max kernel next to the (16, 128) one, the
second trip of every grid-stride loop behind its block cap, the XCD remap of the attention grid and of the skip max, one and two key
tiles, ragged query blocks, queries != keys, strides wider than the data on every operand.  The comment next to a case says which path
it is for.

Every output is pre-filled with a sentinel and sits between guards of it and, where it is strided, between columns of it
(train_ops_oracle.Strided): a kernel that writes one element outside its window fails the test.  Every case has at least two clouds
and every neighbour table holds index 0 and index n_per_cloud - 1.  No call passes an index out of range or a shape its entry point
does not refuse on the host.

Bounds.  Bit equality wherever the kernel is a definite sequence of float32 operations (the fmaf chains against oracle.generator.linear
/ matmul_nn, maxima, gathers, single subtractions, ordered float32 sums).  Otherwise float64 and, per element, with eps32 = 2^-23:
  linear_small_n / chains, mode 1   4 eps32 max(1, |want|): expf, a division, a subtraction and an addition of at most an ulp each
  ps_prep                           8 eps32 (|G| + sum |x| |Wc + Wr| + |b|), A: 8 eps32 sum |x| |Wc|: six rounded operations
  ps_weight_net                     8 eps32 (sum |dxyz| |Ww| + |bw|) |scale| + 2 eps32 |shift|
  attention(_project)               2e-5 max(1, max |want|), the bound of test_fused_attention(_project); on the four ill-conditioned
                                    cases twice the error of the float32 restatement of the online softmax on the same inputs
                                    (attention_train_oracle.recompute_f32) where that is larger
  pool mode 3                       4 eps32 sum_s |x|
  l2_normalize_rows                 4 eps32 |want| for c <= 9: the float32 sum of c squares is off by at most (c + 1) / 2 half-ulps, its
                                    inverse root by half of that plus the roundings of sqrt, division and product: ((c + 1) / 4 + 1.5) eps32
  row mean                          n eps32 mean |x|
Every float comparison prints its worst error as a fraction of its bound before it asserts (pytest -s).

Paths and the case that reaches each (the host branch that selects it is named; nothing is instrumented):
  linear_small_k scalar kernel, N = 16 / 24, K = 1..4   `v4` false in dispu_linear_small_k: test_linear_small_k[N-scalar_ldy] (ldy % 4 != 0),
                                                        [N-scalar_yoff] (Y one float off); float4 kernel: [N-v4]
  ps_prep scalar kernel                                 the co / ld / pointer test of dispu_ps_prep fails: test_ps_prep_float4_and_scalar_agree
                                                        (pointer offset, odd strides), test_ps_prep_scalar (co = 6, 130, 121)
  ps_skip_max general kernel                            `k == 16 && cf == 128` false: test_ps_skip_max[3-17-16-64..], [2-256-7-128..], [3-17-1-4..],
                                                        [2-19-16-124..]; the (16, 128) kernel with remap [2-256-16-128..], without [3-17-16-128..]
  second trip behind grid_for's 32768 blocks            test_ps_prep_scalar[70000-121], test_ps_gather_sub_relu[2-16500-16-64],
                                                        test_ps_weight_net[2-16500-16-16]
  dup_grid 65536-block cap / co / 4 > blockDim          test_dup_grid[3-22000-4-3-8-8] / test_dup_grid[2-21-260-4-264-268]
  up != 4, t_n != 16                                    test_dup_grid (up 1, 3), test_ps_weight_net[..-3-5]
  attention XCD remap (gridDim.y % 8 == 0)              test_attention_and_project[8-256-256..], [16-160-160..]
  m != nk, m % 32 != 0 / one, two tiles / m < 128       [3-130-160..] / [2-96-32..], [2-96-64..] / [2-40-512..], [1-1-32..]
  strided Q and O / scale != 0.125                      [2-96-64-128-96-0.125] / [2-96-64-64-64-0.3]
  ill-conditioned exponent arithmetic                   [3-130-160-64-64-0.125-k_offset70], [..-k_offset280], [..-big_logits4.5], [..-big_logits8]:
                                                        the inputs of tests/attention_train_oracle.py, max |s2| 70, 280, 129, 411
  pooling modes at other (ns, c), mgrid's cap           test_pool_nsample (24 cases), [70000-2-121-3], [70000-2-121-4]; test_group_center[70000-11-11],
                                                        test_idw_weights[8389608], test_l2_normalize_rows[8389608-1], test_scale_add[8389608],
                                                        test_edge_feature[2-16500-16-16-0]
  the 1e-10 / 1e-12 clamps                              test_idw_weights (zero, below, at and above the clamp), test_l2_normalize_rows (zero row,
                                                        sum of squares 1.1e-12 and 1e-14)

Mutations (arithmetic only, on a scratch build) and the tests that fail under each, all others passing:
  no `+ bias[o]` in linear_small_k_kernel               test_linear_small_k[16-scalar_ldy], [16-scalar_yoff], [24-scalar_ldy], [24-scalar_yoff]
  `sub < 5` in ps_skip_max_kernel's neighbour loop      the four general-kernel cases of test_ps_skip_max, each naming channel 5 (max of z)
  g0 and g1 swapped in dup_grid_kernel                  test_dup_grid, every case with up > 1
  alpha = 1 in flash_attention_kernel                   test_attention_and_project, every case with more than one tile
  mode 1 returns mx in pool_nsample_kernel              test_pool_nsample[37-16-32-1], [37-64-7-1], [37-33-130-1]

Measured on an MI355X, worst error as a fraction of its bound: attention 0.58, attention_project 0.62 (both at 16 x 160 x 160; on the
ill-conditioned cases 0.13 / 0.13 at k_offset70, 0.50 / 0.50 at k_offset280, 0.27 / 0.20 at big_logits4.5, 0.33 / 0.37 at big_logits8;
ATT_TOL is the larger bound in all but k_offset280, where twice the restatement's error is, 1.6e-3 / 2.2e-3 against errors of
7.9e-4 / 1.1e-3),
l2_normalize_rows 0.35, pool mode 3 0.33, mode 1 of linear_small_n 0.24 and of the chains 0.27, ps_prep G 0.23 / A 0.17, ps_weight_net
0.21, row mean 0.005; everything else bit-exact.  dispu_scale_add gives the unfused result in every element (the build pins
-ffp-contract=off).  No bound stated above had to be widened."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_train_oracle as AO  # noqa: E402
import generator_ops_oracle as GO  # noqa: E402
import train_ops_oracle as TO  # noqa: E402
from generator_ops_oracle import EPS32  # noqa: E402
from train_ops_oracle import F32, INVALID, SENT, Guarded, Strided, dv, p, same_bits  # noqa: E402

from oracle import generator as OG  # noqa: E402

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


def near(got, want, bound, what):
    """|got - want| <= bound per element (bound broadcasts), the worst fraction printed first; got must be finite."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert np.isfinite(got).all(), what + ": not finite"
    err = np.abs(got - want)
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("[measured] %s: worst error %.3f of its bound (largest absolute error %.3e)" % (what, frac, err.max() if err.size else 0.0))
    bad = err > bound
    assert not bad.any(), "%s: %d elements beyond the bound, worst %.3f of it" % (what, int(bad.sum()), frac)


def exact(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), want.size)


def table(rng, B, n, k):
    """cloud-local neighbour ids [B, n, k] that hold 0 and n - 1 in every cloud."""
    idx = rng.integers(0, n, (B, n, k)).astype(np.int32)
    idx[:, 0, 0] = 0
    idx[:, n - 1, k - 1] = n - 1
    return idx


def didx(idx, dev):
    return p(dv(np.ascontiguousarray(idx, np.int32), dev))


# ---------------------------------------------------------------------------------------- dispu_linear_small_k ----
# path: how the launch code's float4 test (ldy % 4 == 0 and Y, W, bias 16-byte aligned) comes out.  (ldy - N, offset of Y in floats)
SMALL_K_PATHS = {"v4": (4, 0), "scalar_ldy": (1, 0), "scalar_yoff": (4, 1)}


@pytest.mark.parametrize("path", sorted(SMALL_K_PATHS))
@pytest.mark.parametrize("N", [16, 24])
def test_linear_small_k(dev, L, N, path):
    pad, yoff = SMALL_K_PATHS[path]
    rng = np.random.default_rng(N)
    for K in (1, 2, 3, 4):
        W = rng.standard_normal((K, N)).astype(F32)
        b = rng.standard_normal(N).astype(F32)
        dW, db = dv(W, dev), dv(b, dev)
        for rows in (1, 63, 257, 1000):                         # 257 rows: a second block on the scalar path; 1000 x N / 4 quads: 24 on v4
            x = rng.standard_normal((rows, K)).astype(F32)
            sx = Strided(dev, rows, K, K + 3, 1, x)
            for act in (0, 1):
                for bias in (True, False):
                    sy = Strided(dev, rows, N, N + pad + (4 if yoff else 0), yoff)
                    ok(L, dev, "dispu_linear_small_k", rows, K, N, sx.ptr(), sx.ld, p(dW), p(db) if bias else None, act, sy.ptr(), sy.ld)
                    what = "linear_small_k %s rows %d K %d N %d act %d bias %d" % (path, rows, K, N, act, bias)
                    exact(sy.data(), OG.linear(x, W, b if bias else None, relu=bool(act)), what)
                    assert sy.rest_untouched(), what + ": wrote outside Y's window"
            assert sx.untouched()


# ---------------------------------------------------------------------------------------- dispu_linear_small_n ----
@pytest.mark.parametrize("K", [1, 64, 67])
def test_linear_small_n_mode0(dev, L, K):
    rng = np.random.default_rng(K)
    rows = 300
    x = rng.standard_normal((rows, K)).astype(F32)
    W, b = rng.standard_normal((K, 3)).astype(F32), rng.standard_normal(3).astype(F32)
    sx = Strided(dev, rows, K, K + 5, 2, x)
    for bias in (True, False):
        sy = Strided(dev, rows, 3, 7, 2)
        ok(L, dev, "dispu_linear_small_n", rows, K, 3, sx.ptr(), sx.ld, p(dv(W, dev)), p(dv(b, dev)) if bias else None, 0, None, 0,
           sy.ptr(), sy.ld)
        exact(sy.data(), OG.linear(x, W, b if bias else None), "linear_small_n mode 0 K %d bias %d" % (K, bias))
        assert sy.rest_untouched() and sx.untouched()


def mode1_inputs(rng, rows, K):
    """X whose rows 0..7 give pre-activations of about +-30 and +-100 (W's first row is 1): the sigmoid saturates both ways."""
    x = rng.standard_normal((rows, K)).astype(F32)
    W = (rng.standard_normal((K, 3)) / np.sqrt(K)).astype(F32)
    W[0] = 1.0
    for r, v in enumerate((30.0, -30.0, 100.0, -100.0)):
        if r < rows:
            x[r] = 0.0
            x[r, 0] = v
    return x, W


@pytest.mark.parametrize("K", [1, 64, 67])
def test_linear_small_n_mode1(dev, L, K):
    rng = np.random.default_rng(100 + K)
    rows = 300
    x, W = mode1_inputs(rng, rows, K)
    b = (rng.standard_normal(3) * 0.1).astype(F32)
    R = rng.standard_normal((rows, 3)).astype(F32)
    z = OG.linear(x, W, b)
    assert z[:4].max() >= 99 and z[:4].min() <= -99 and np.abs(z[:2]).min() >= 29 and np.abs(z[:2]).max() <= 31
    sx, sr, sy = Strided(dev, rows, K, K + 5, 2, x), Strided(dev, rows, 3, 4, 1, R), Strided(dev, rows, 3, 7, 2)
    ok(L, dev, "dispu_linear_small_n", rows, K, 3, sx.ptr(), sx.ld, p(dv(W, dev)), p(dv(b, dev)), 1, sr.ptr(), sr.ld, sy.ptr(), sy.ld)
    want = GO.linear_mode1(z, R)
    near(sy.data(), want, 4 * EPS32 * np.maximum(1.0, np.abs(want)), "linear_small_n mode 1 K %d" % K)
    assert sy.rest_untouched() and sx.untouched() and sr.untouched()


# ---------------------------------------------------------------------------------------------- dispu_dup_grid ----
DUP = [
    # (nclouds, n, co, up, ldh, ldy)
    (2, 37, 128, 4, 132, 136),           # co / 4 = 32: 32-thread blocks
    (2, 37, 256, 3, 260, 264),           # co / 4 = 64: 64-thread blocks
    (3, 19, 4, 1, 8, 12),                # one float4 per row, a single copy
    (2, 21, 260, 4, 264, 268),           # co / 4 = 65 > blockDim: a second pass of the channel loop
    (3, 22000, 4, 3, 8, 8),              # 66000 source rows > the 65536-block cap: a second trip of the row loop
]


@pytest.mark.parametrize("case", DUP, ids=ids(DUP))
def test_dup_grid(dev, L, case):
    nclouds, n, co, up, ldh, ldy = case
    kf = 8
    rng = np.random.default_rng(co + up)
    feat = rng.standard_normal((nclouds, n, kf)).astype(F32)
    W = (rng.standard_normal((kf + 2, co)) * 0.5).astype(F32)
    W[kf] *= 3.0                                                 # the two grid rows weigh differently: swapped grid channels show
    b = (rng.standard_normal(co) * 0.3).astype(F32)
    grid = OG.gen_grid(up)
    H = OG.linear(feat, W[:kf], None)
    sh, sy = Strided(dev, nclouds * n, co, ldh, 0, H), Strided(dev, nclouds * up * n, co, ldy, 0)
    ok(L, dev, "dispu_dup_grid", nclouds, n, co, up, sh.ptr(), ldh, p(dv(W[kf:], dev)), p(dv(b, dev)), p(dv(grid, dev)), sy.ptr(), ldy)
    # rows of the reference are copy-major by construction: (cloud * up + r) * n + i = [feat[cloud, i] | grid[r]]
    want = OG.linear(GO.dup_grid_input(feat, grid), W, b, relu=True)
    exact(sy.data(), want.reshape(-1, co), "dup_grid %s" % (case,))
    assert sy.rest_untouched() and sh.untouched()
    assert (want > 0).any() and (want == 0).any()


# ----------------------------------------------------------------------------------------------- dispu_ps_prep ----
def prep_call(dev, L, rows, co, Gf, xyz, W0, b, ldg, lda, goff=0, aoff=0):
    sg, sa = Strided(dev, rows, co, ldg, goff, Gf), Strided(dev, rows, co, lda, aoff)
    ok(L, dev, "dispu_ps_prep", rows, co, p(dv(xyz, dev)), p(dv(W0, dev)), p(dv(b, dev)), sg.ptr(), ldg, sa.ptr(), lda)
    assert sg.rest_untouched() and sa.rest_untouched(), "ps_prep wrote outside its windows"
    return sg.data().copy(), sa.data().copy()


def prep_data(rng, rows, co):
    Gf = rng.standard_normal((rows, co)).astype(F32)
    xyz = rng.uniform(-1, 1, (rows, 3)).astype(F32)
    W0 = (rng.standard_normal((6, co)) * 0.5).astype(F32)         # only the six xyz rows of conv0 are read
    b = (rng.standard_normal(co) * 0.2).astype(F32)
    return Gf, xyz, W0, b


def prep_check(G, A, Gf, xyz, W0, b, what):
    wG, wA, mG, mA = GO.ps_prep(Gf, xyz, W0, b)
    near(G, wG, 8 * EPS32 * mG, what + " G")
    near(A, wA, 8 * EPS32 * mA, what + " A")


@pytest.mark.parametrize("rows", [1, 37, 1000])
@pytest.mark.parametrize("co", [4, 128])
def test_ps_prep_float4_and_scalar_agree(dev, L, co, rows):
    """co % 4 == 0: the float4 kernel with aligned operands and even strides, the scalar one otherwise; same data, same bits."""
    Gf, xyz, W0, b = prep_data(np.random.default_rng(co + rows), rows, co)
    G4, A4 = prep_call(dev, L, rows, co, Gf, xyz, W0, b, co + 4, co + 8)
    prep_check(G4, A4, Gf, xyz, W0, b, "ps_prep float4 %d x %d" % (rows, co))
    for name, kw in (("G one float off", dict(ldg=co + 4, lda=co + 8, goff=1)), ("A one float off", dict(ldg=co + 4, lda=co + 8, aoff=1)),
                     ("odd strides", dict(ldg=co + 1, lda=co + 3))):
        G1, A1 = prep_call(dev, L, rows, co, Gf, xyz, W0, b, **kw)
        assert same_bits(G1, G4) and same_bits(A1, A4), "ps_prep %d x %d: the scalar path (%s) differs from the float4 path" % (rows, co, name)


PREP_SCALAR = [(1, 6), (37, 6), (1000, 6), (1, 130), (37, 130), (1000, 130),
               (70000, 121)]                                     # 8 470 000 elements > 32768 blocks x 256: a second trip of the loop


@pytest.mark.parametrize("case", PREP_SCALAR, ids=ids(PREP_SCALAR))
def test_ps_prep_scalar(dev, L, case):
    rows, co = case
    Gf, xyz, W0, b = prep_data(np.random.default_rng(rows + co), rows, co)
    wide = rows < 70000
    G, A = prep_call(dev, L, rows, co, Gf, xyz, W0, b, co + (2 if wide else 0), co + (4 if wide else 0))
    prep_check(G, A, Gf, xyz, W0, b, "ps_prep scalar %d x %d" % (rows, co))


# ------------------------------------------------------------------------------------ dispu_ps_gather_sub_relu ----
GSR = [(B, n, k, c) for (k, c) in [(16, 128), (1, 4), (5, 36)] for (B, n) in [(2, 17), (2, 256)]] + \
      [(2, 16500, 16, 64)]              # 8 448 000 float4 > 32768 blocks x 256: a second trip of the loop (X1 is 135 MB)


@pytest.mark.parametrize("case", GSR, ids=ids(GSR))
def test_ps_gather_sub_relu(dev, L, case):
    B, n, k, c = case
    rows = B * n
    rng = np.random.default_rng(n + k + c)
    G = rng.standard_normal((B, n, c), dtype=F32)
    A = rng.standard_normal((B, n, c), dtype=F32)
    idx = table(rng, B, n, k)
    big = rows > 10000
    sg = Strided(dev, rows, c, 320, 192, G)                     # G as the generator holds it: columns 192.. of a 320-wide buffer
    sa = Strided(dev, rows, c, c + 4, 0, A)
    sx = Strided(dev, rows * k, c, c if big else c + 4, 0)
    ok(L, dev, "dispu_ps_gather_sub_relu", rows, n, k, c, didx(idx, dev), sg.ptr(), sg.ld, sa.ptr(), sa.ld, sx.ptr(), sx.ld)
    want = GO.gather_sub_relu(G, A, idx).reshape(rows * k, c)
    got = sx.data()
    assert got.shape == want.shape and np.array_equal(got, want), "gather_sub_relu %s differs from max(G[j] - A[i], 0)" % (case,)
    assert sx.G.guards_intact() and (big or sx.rest_untouched()) and sg.untouched() and sa.untouched()


# ------------------------------------------------------------------------------------------- dispu_ps_skip_max ----
SKIP = [
    # (B, n, k, cf, ldo - (6 + cf), negative features)
    (2, 256, 16, 128, 0, False),         # (16, 128) kernel, rows / 8 = 64 blocks, a multiple of 8: the XCD remap
    (3, 17, 16, 128, 2, True),           # (16, 128) kernel, 51 rows = 7 blocks: no remap, a ragged last block
    (3, 17, 16, 64, 0, False),           # the general kernel from here on: half of the 32 lanes carry features
    (2, 256, 7, 128, 3, False),
    (3, 17, 1, 4, 1, True),              # one neighbour, one float4
    (2, 19, 16, 124, 0, True),           # the last lane without features
]


@pytest.mark.parametrize("case", SKIP, ids=ids(SKIP))
def test_ps_skip_max(dev, L, case):
    B, n, k, cf, opad, negative = case
    rows = B * n
    rng = np.random.default_rng(n + k + cf)
    xyz = rng.uniform(-1, 1, (B, n, 3)).astype(F32)
    feat = rng.standard_normal((B, n, cf)).astype(F32)
    if negative:
        feat = -np.abs(feat) - F32(0.25)                         # every maximum is negative: the -inf start shows, a 0 start would win
        xyz = xyz - F32(3.0)
    idx = table(rng, B, n, k)
    sf = Strided(dev, rows, cf, cf + 8, 4, feat)                # a 16-byte aligned column slice, ldf > cf
    so = Strided(dev, rows, 6 + cf, 6 + cf + opad, 0)
    ok(L, dev, "dispu_ps_skip_max", rows, n, k, cf, didx(idx, dev), p(dv(xyz, dev)), sf.ptr(), sf.ld, so.ptr(), so.ld)
    want = GO.skip_max(xyz, feat, idx).reshape(rows, 6 + cf)
    got = so.data()
    for ch, name in enumerate(("dx", "dy", "dz", "x", "y", "z")):
        exact(got[:, ch], want[:, ch], "skip_max %s channel %d (max of %s)" % (case, ch, name))
    exact(got[:, 6:], want[:, 6:], "skip_max %s feature channels" % (case,))
    assert so.rest_untouched() and sf.untouched()


# ----------------------------------------------------------------------------------------- dispu_ps_weight_net ----
WNET = [(B, n, k, t) for (k, t) in [(16, 16), (3, 5)] for (B, n) in [(2, 17), (2, 256)]] + \
       [(2, 16500, 16, 16)]            # 8 448 000 outputs > 32768 blocks x 256: a second trip of the loop


@pytest.mark.parametrize("case", WNET, ids=ids(WNET))
def test_ps_weight_net(dev, L, case):
    B, n, k, t_n = case
    rows = B * n
    rng = np.random.default_rng(n + k)
    xyz = rng.uniform(-1, 1, (B, n, 3)).astype(F32)
    idx = table(rng, B, n, k)
    Ww, bw = rng.standard_normal((3, t_n)).astype(F32), (rng.standard_normal(t_n) * 0.3).astype(F32)
    scale, shift = rng.uniform(0.5, 1.5, t_n).astype(F32), (rng.standard_normal(t_n) * 0.3).astype(F32)
    scale[0] = -scale[0]
    out = Guarded(dev, rows * k * t_n)
    ok(L, dev, "dispu_ps_weight_net", rows, n, k, t_n, didx(idx, dev), p(dv(xyz, dev)), p(dv(Ww, dev)), p(dv(bw, dev)), p(dv(scale, dev)),
       p(dv(shift, dev)), out.ptr())
    want, mag, sh = GO.weight_net(xyz, idx, Ww, bw, scale, shift)
    near(out.body().reshape(want.shape), want, 8 * EPS32 * mag + 2 * EPS32 * sh, "ps_weight_net %s" % (case,))
    assert out.guards_intact() and (want > 0).any() and (want == 0).any()


# --------------------------------------------------------------------------------------- dispu_ps_point_matmul ----
@pytest.mark.parametrize("rows", [1, 37])
def test_ps_point_matmul(dev, L, rows):
    rng = np.random.default_rng(rows)
    X2 = rng.standard_normal((rows, 16, 128)).astype(F32)
    wv = np.maximum(rng.standard_normal((rows, 16, 16)), 0).astype(F32)
    sx, so = Strided(dev, rows * 16, 128, 132, 0, X2), Strided(dev, rows, 2048, 2052, 0)
    ok(L, dev, "dispu_ps_point_matmul", rows, 16, 128, 16, sx.ptr(), sx.ld, p(dv(wv, dev)), so.ptr(), so.ld)
    exact(so.data(), GO.point_matmul(X2, wv), "ps_point_matmul %d rows" % rows)
    assert so.rest_untouched() and sx.untouched()
    for bad in ((15, 128, 16, 2052), (16, 64, 16, 2052), (16, 128, 8, 2052), (16, 128, 16, 2050)):      # k, c, t_n, ldo
        s2 = Strided(dev, rows, 2048, 2052, 0)
        assert run(L, dev, "dispu_ps_point_matmul", rows, bad[0], bad[1], bad[2], sx.ptr(), sx.ld, p(dv(wv, dev)), s2.ptr(), bad[3]) == INVALID
        assert s2.untouched()


# ------------------------------------------------------------------ dispu_attention, dispu_attention_project ----
ATT = [
    # (b, m, nk, ldq, ldo, scale)
    (8, 256, 256, 64, 64, 0.125),        # b % 8 == 0: the XCD remap, two query blocks
    (16, 160, 160, 64, 64, 0.125),       # the remap with a ragged second query block (32 of 128 rows)
    (2, 96, 32, 64, 64, 0.125),          # one key tile: the pipeline's prologue is all there is
    (2, 96, 64, 64, 64, 0.125),          # two tiles: no third load
    (1, 1, 32, 64, 64, 0.125),           # one query
    (3, 130, 160, 64, 64, 0.125),        # m % 32 != 0 (the qok lanes), m != nk
    (2, 40, 512, 64, 64, 0.125),         # m < 128, sixteen tiles
    (2, 96, 64, 128, 96, 0.125),         # Q read out of a wider buffer, O written into one
    (2, 96, 64, 64, 64, 0.3),            # a scale other than 1 / sqrt(d)
    # the ill-conditioned inputs of tests/attention_train_oracle.py (the same online-softmax scheme): a common offset on every key of a
    # cloud with max |s2| 70 and 280, and randn * 4.5 / * 8 (max |s2| about 130 and 420); a ragged query block, five tiles
    (3, 130, 160, 64, 64, 0.125, "k_offset70"),
    (3, 130, 160, 64, 64, 0.125, "k_offset280"),
    (3, 130, 160, 64, 64, 0.125, "big_logits4.5"),
    (3, 130, 160, 64, 64, 0.125, "big_logits8"),
]
ATT_TOL = 2e-5                           # of max(1, max |want|): test_fused_attention / test_fused_attention_project


def att_inputs(b, m, nk, scale, seed):
    """Q [b, m, 64], KV [b, nk, 128] (K | V as the generator holds them).  Query 0 of every cloud meets a larger logit in every later
    tile, the largest in the last one (every earlier tile gets rescaled); query m - 1 (m > 1) is 40 times the others, so its logits
    spread over more than 200 in the log2 domain and the smallest terms underflow."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((b, m, 64)).astype(F32)
    kv = rng.standard_normal((b, nk, 128)).astype(F32)
    for t in range(nk // 32):
        kv[:, 32 * t + 5, :64] = q[:, 0] * F32(0.5 * (t + 1))      # logit 32 scale (t + 1) among others of deviation 8 scale
    lg = np.einsum("bd,bkd->bk", q[:, 0].astype(np.float64), kv[..., :64].astype(np.float64)) * scale
    tmax = lg.reshape(b, nk // 32, 32).max(-1)
    assert (np.diff(tmax, axis=1) > 1.0).all() and (lg.argmax(1) == nk - 32 + 5).all()
    if m > 1:
        q[:, m - 1] *= F32(40.0)
        lg = np.einsum("bd,bkd->bk", q[:, m - 1].astype(np.float64), kv[..., :64].astype(np.float64)) * scale * np.log2(np.e)
        assert ((lg.max(1) - lg.min(1)) > 200).all()
    return q, kv


@pytest.mark.parametrize("case", ATT, ids=ids(ATT))
def test_attention_and_project(dev, L, case):
    b, m, nk, ldq, ldo, scale = case[:6]
    rng = np.random.default_rng(7)
    W = (rng.standard_normal((64, 256)) * 0.2).astype(F32)
    bias = (rng.standard_normal(256) * 0.1).astype(F32)
    extra = extrap = 0.0
    if len(case) == 6:
        q, kv = att_inputs(b, m, nk, scale, m + nk)
    else:
        # ATT_TOL stays unless twice the forward error of the float32 restatement of the algorithm on the same inputs is larger
        q, k, v, do = AO.build(case[6], b, m, nk)
        kv = np.concatenate([k, v], -1)
        Or = AO.recompute_f32(q, k, v, do, scale)["O"]
        extra = 2.0 * np.abs(Or - GO.attention(q, k, v, scale)).max()
        extrap = 2.0 * np.abs(np.maximum(Or @ W + bias, 0) - GO.attention_project(q, k, v, scale, W, bias)).max()
        print("[measured] %s: max |s2| %.0f, twice the restatement's error %.2e (attention), %.2e (attention_project)" % (
            case[6], AO.s2_max(q, k, scale), extra, extrap))
    sq, skv = Strided(dev, b * m, 64, ldq, ldq - 64, q), Strided(dev, b * nk, 128, 128, 0, kv)
    so = Strided(dev, b * m, 64, ldo, ldo - 64)
    kp, vp = skv.ptr(), skv.G.ptr(64)
    ok(L, dev, "dispu_attention", b, m, nk, 64, sq.ptr(), ldq, kp, 128, vp, 128, scale, so.ptr(), ldo)
    want = GO.attention(q, kv[..., :64], kv[..., 64:], scale).reshape(b * m, 64)
    near(so.data(), want, max(ATT_TOL * max(1.0, np.abs(want).max()), extra), "attention %s" % (case,))
    assert so.rest_untouched() and sq.untouched() and skv.untouched()
    ldy = 256 + (ldo - 64)
    sy = Strided(dev, b * m, 256, ldy, 0)
    ok(L, dev, "dispu_attention_project", b, m, nk, 64, sq.ptr(), ldq, kp, 128, vp, 128, scale, p(dv(W, dev)), p(dv(bias, dev)), 256,
       sy.ptr(), ldy)
    wantp = GO.attention_project(q, kv[..., :64], kv[..., 64:], scale, W, bias).reshape(b * m, 256)
    near(sy.data(), wantp, max(ATT_TOL * max(1.0, np.abs(wantp).max()), extrap), "attention_project %s" % (case,))
    assert sy.rest_untouched() and sq.untouched() and skv.untouched()
    assert (wantp > 0).any() and (wantp == 0).any()


def test_attention_refusals(dev, L):
    b, m, nk = 2, 40, 64
    q, kv = att_inputs(b, m, nk, 0.125, 1)
    sq, skv = Strided(dev, b * m, 64, 68, 0, q), Strided(dev, b * nk, 128, 136, 0, kv)
    so, sy = Strided(dev, b * m, 64, 68, 0), Strided(dev, b * m, 256, 260, 0)
    W, bias = Guarded(dev, 64 * 256 + 4, fill=0.5), Guarded(dev, 256 + 4, fill=0.5)

    def att(b_=b, m_=m, nk_=nk, d=64, Q=sq.ptr(), ldq=68, K=skv.ptr(), ldk=136, V=skv.G.ptr(64), ldv=136, O=so.ptr(), ldo=68):
        return run(L, dev, "dispu_attention", b_, m_, nk_, d, Q, ldq, K, ldk, V, ldv, 0.125, O, ldo)

    def prj(b_=b, m_=m, nk_=nk, d=64, Q=sq.ptr(), ldq=68, K=skv.ptr(), ldk=136, V=skv.G.ptr(64), ldv=136, W_=W.ptr(), bias_=bias.ptr(), n_out=256,
            Y=sy.ptr(), ldy=260):
        return run(L, dev, "dispu_attention_project", b_, m_, nk_, d, Q, ldq, K, ldk, V, ldv, 0.125, W_, bias_, n_out, Y, ldy)

    for f in (att, prj):
        assert f(b_=-1) == INVALID and f(m_=0) == INVALID and f(m_=-3) == INVALID and f(nk_=0) == INVALID
        assert f(nk_=48) == INVALID and f(nk_=33) == INVALID                                         # nk % 32
        assert f(d=32) == INVALID and f(d=128) == INVALID
        assert f(ldq=70) == INVALID and f(ldk=134) == INVALID and f(ldv=133) == INVALID
        assert f(Q=sq.G.ptr(1)) == INVALID and f(K=skv.G.ptr(2)) == INVALID and f(V=skv.G.ptr(67)) == INVALID
        assert f(b_=0) == 0
    assert prj(n_out=128) == INVALID and prj(ldy=258) == INVALID and prj(W_=None) == INVALID and prj(bias_=None) == INVALID
    assert prj(W_=W.ptr(1)) == INVALID and prj(bias_=bias.ptr(2)) == INVALID and prj(Y=sy.G.ptr(1)) == INVALID
    assert so.untouched() and sy.untouched() and sq.untouched() and skv.untouched()
    assert att() == 0 and prj() == 0 and not so.untouched() and not sy.untouched()                   # the same arguments, valid, do write


# ------------------------------------------------------ dispu_mlp_chain, dispu_mlp_chain_sum3, dispu_mlp_chain_dup ----
def chain_weights(seed, n1):
    rng = np.random.default_rng(seed)
    dims = [(256, n1), (n1, 256), (256, 64), (64, 3)]
    ws = []
    for k, n in dims:
        ws.append((rng.standard_normal((k, n)) * np.sqrt(2.0 / k)).astype(F32))
        ws.append((rng.standard_normal(n) * 0.1).astype(F32))
    return ws


def chain_finish(dev, rows, n1, mode, y1, ws, X, R, sy1, sr, so, what):
    """compare what a chain entry wrote with the pinned chain on the float32 input rows X."""
    wy1, z = GO.mlp_chain(X, *ws)
    if mode == 0:
        exact(so.data(), z, what + " head")
    else:
        want = GO.linear_mode1(z, R)
        near(so.data(), want, 4 * EPS32 * np.maximum(1.0, np.abs(want)), what + " head, mode 1")
    assert so.rest_untouched()
    if y1:
        exact(sy1.data(), wy1, what + " Y1")
        assert sy1.rest_untouched()
    assert sr is None or sr.untouched()
    assert (wy1 > 0).any() and (wy1 == 0).any()


CHAIN = [(rows, n1, mode, y1) for rows in (64, 320) for n1 in (128, 256) for mode in (0, 1) for y1 in (False, True)]


@pytest.mark.parametrize("case", CHAIN, ids=ids(CHAIN))
def test_mlp_chain(dev, L, case):
    """rows / 128 < 192: the 64-row workgroups (the 128-row ones are held to the separate launches in test_headline_gpu.py)."""
    rows, n1, mode, y1 = case
    rng = np.random.default_rng(rows + n1)
    ws = chain_weights(n1, n1)
    X = rng.standard_normal((rows, 256)).astype(F32)
    R = rng.standard_normal((rows, 3)).astype(F32)
    sx = Strided(dev, rows, 256, 264, 4, X)
    sy1 = Strided(dev, rows, n1, n1 + 4, 1) if y1 else None
    sr = Strided(dev, rows, 3, 4, 1, R) if mode else None
    so = Strided(dev, rows, 3, 5, 1)
    dw = [p(dv(w, dev)) for w in ws]
    ok(L, dev, "dispu_mlp_chain", rows, 256, n1, 256, 64, sx.ptr(), sx.ld, *(dw + [sy1.ptr() if y1 else None, sy1.ld if y1 else 0, mode,
       sr.ptr() if mode else None, sr.ld if mode else 0, so.ptr(), so.ld]))
    chain_finish(dev, rows, n1, mode, y1, ws, X, R, sy1, sr, so, "mlp_chain %s" % (case,))
    assert sx.untouched()


SUM3 = [(64, 128, 0, True), (320, 256, 1, False), (320, 128, 1, True), (64, 256, 0, False)]


@pytest.mark.parametrize("case", SUM3, ids=ids(SUM3))
def test_mlp_chain_sum3(dev, L, case):
    rows, n1, mode, y1 = case
    rng = np.random.default_rng(rows + n1 + 1)
    ws = chain_weights(n1 + 1, n1)
    Xs = [rng.standard_normal((rows, 256)).astype(F32) for _ in range(3)]
    R = rng.standard_normal((rows, 3)).astype(F32)
    sxs = [Strided(dev, rows, 256, 260, 0, x) for x in Xs]
    sy1 = Strided(dev, rows, n1, n1 + 4, 1) if y1 else None
    sr = Strided(dev, rows, 3, 4, 1, R) if mode else None
    so = Strided(dev, rows, 3, 5, 1)
    dw = [p(dv(w, dev)) for w in ws]
    ok(L, dev, "dispu_mlp_chain_sum3", rows, 256, n1, 256, 64, sxs[0].ptr(), sxs[1].ptr(), sxs[2].ptr(), 260,
       *(dw + [sy1.ptr() if y1 else None, sy1.ld if y1 else 0, mode, sr.ptr() if mode else None, sr.ld if mode else 0, so.ptr(), so.ld]))
    chain_finish(dev, rows, n1, mode, y1, ws, (Xs[0] + Xs[1]) + Xs[2], R, sy1, sr, so, "mlp_chain_sum3 %s" % (case,))
    assert all(s.untouched() for s in sxs)


DUPCHAIN = [(128, 0, True), (256, 1, False), (128, 1, True)]


@pytest.mark.parametrize("case", DUPCHAIN, ids=ids(DUPCHAIN))
def test_mlp_chain_dup(dev, L, case):
    """n = 80, up = 4: the 64-row tiles straddle the copies (and the clouds) of the copy-major row order."""
    n1, mode, y1 = case
    nclouds, n, up, kf = 2, 80, 4, 8
    rows = nclouds * up * n
    rng = np.random.default_rng(n1 + mode)
    ws = chain_weights(n1 + 2, n1)
    feat = rng.standard_normal((nclouds, n, kf)).astype(F32)
    Wd = (rng.standard_normal((kf + 2, 256)) * 0.5).astype(F32)
    Wd[kf] *= 3.0
    bd = (rng.standard_normal(256) * 0.3).astype(F32)
    grid = OG.gen_grid(up)
    X = OG.linear(GO.dup_grid_input(feat, grid), Wd, bd, relu=True).reshape(rows, 256)
    R = rng.standard_normal((rows, 3)).astype(F32)
    sh = Strided(dev, nclouds * n, 256, 260, 0, OG.linear(feat, Wd[:kf], None))
    sy1 = Strided(dev, rows, n1, n1 + 4, 1) if y1 else None
    sr = Strided(dev, rows, 3, 4, 1, R) if mode else None
    so = Strided(dev, rows, 3, 5, 1)
    dw = [p(dv(w, dev)) for w in ws]
    ok(L, dev, "dispu_mlp_chain_dup", nclouds, n, up, 256, n1, 256, 64, sh.ptr(), sh.ld, p(dv(Wd[kf:], dev)), p(dv(bd, dev)), p(dv(grid, dev)),
       *(dw + [sy1.ptr() if y1 else None, sy1.ld if y1 else 0, mode, sr.ptr() if mode else None, sr.ld if mode else 0, so.ptr(), so.ld]))
    chain_finish(dev, rows, n1, mode, y1, ws, X, R, sy1, sr, so, "mlp_chain_dup %s" % (case,))
    assert sh.untouched()


def test_mlp_chain_refusals(dev, L):
    rows, n1 = 64, 128
    ws = chain_weights(0, n1)
    gw = [Guarded(dev, w.size + 4, fill=np.concatenate([w.reshape(-1), np.zeros(4, F32)])) for w in ws]
    X = Guarded(dev, 2 * 64 * 260 + 8, fill=0.25)
    so, sy1 = Strided(dev, 2 * rows, 3, 5, 1), Strided(dev, 2 * rows, n1, n1 + 4, 0)
    R = Guarded(dev, 2 * rows * 4, fill=0.5)
    G8 = Guarded(dev, 64, fill=0.1)
    W = [g.ptr() for g in gw]

    def tail(y1=sy1.ptr(), mode=0, r=R.ptr(), out=so.ptr()):
        return [y1, sy1.ld, mode, r, 4, out, so.ld]

    def chain(rows_=rows, widths=(256, n1, 256, 64), x=X.ptr(), ldx=260, w=W, **kw):
        return run(L, dev, "dispu_mlp_chain", rows_, *(list(widths) + [x, ldx] + list(w) + tail(**kw)))

    def sum3(rows_=rows, widths=(256, n1, 256, 64), x=X.ptr(), x2=X.ptr(), x3=X.ptr(), ldx=260, w=W, **kw):
        return run(L, dev, "dispu_mlp_chain_sum3", rows_, *(list(widths) + [x, x2, x3, ldx] + list(w) + tail(**kw)))

    def dup(nclouds=1, n=16, up=4, widths=(256, n1, 256, 64), h=X.ptr(), ldh=260, wg=gw[0].ptr(), bg=gw[2].ptr(), grid=G8.ptr(), w=W, **kw):
        return run(L, dev, "dispu_mlp_chain_dup", nclouds, n, up, *(list(widths) + [h, ldh, wg, bg, grid] + list(w) + tail(**kw)))

    def without(i, val=None):
        w = list(W)
        w[i] = val
        return w

    for f in (chain, sum3):
        assert f(rows_=-64) == INVALID and f(rows_=96) == INVALID and f(rows_=1) == INVALID                 # rows % 64
        assert f(ldx=258) == INVALID and f(x=None) == INVALID and f(x=X.ptr(1)) == INVALID
        assert f(rows_=0) == 0
    assert sum3(x2=None) == INVALID and sum3(x3=None) == INVALID and sum3(x2=X.ptr(2)) == INVALID and sum3(x3=X.ptr(3)) == INVALID
    assert dup(nclouds=-1) == INVALID and dup(n=0) == INVALID and dup(up=0) == INVALID and dup(n=20) == INVALID   # 80 rows
    assert dup(ldh=262) == INVALID and dup(h=None) == INVALID and dup(wg=None) == INVALID and dup(bg=None) == INVALID and dup(grid=None) == INVALID
    assert dup(h=X.ptr(1)) == INVALID and dup(wg=gw[0].ptr(1)) == INVALID and dup(bg=gw[2].ptr(2)) == INVALID
    assert dup(nclouds=0) == 0
    for f in (chain, sum3, dup):
        for wrong in ((128, n1, 256, 64), (256, 64, 256, 64), (256, n1, 128, 64), (256, n1, 256, 32), (256, 256, 128, 64)):
            assert f(widths=wrong) == INVALID, wrong
        for i in range(8):
            assert f(w=without(i)) == INVALID, "a NULL weight or bias %d" % i
        for i in (0, 2, 4):
            assert f(w=without(i, gw[i].ptr(1))) == INVALID, "a misaligned W%d" % (i // 2 + 1)
        assert f(mode=1, r=None) == INVALID and f(out=None) == INVALID
    assert so.untouched() and sy1.untouched()
    assert chain() == 0 and not so.untouched() and not sy1.untouched()                                   # the same arguments, valid, do write
    so2 = Strided(dev, rows, 3, 5, 1)
    assert sum3(out=so2.ptr(), y1=None) == 0 and not so2.untouched()
    so3 = Strided(dev, rows, 3, 5, 1)
    assert dup(out=so3.ptr(), y1=None) == 0 and not so3.untouched()


# -------------------------------------------------------------------------------------------- csrc/modules.hip ----
POOL = [(37, 1, 1), (37, 16, 32), (37, 64, 7), (37, 33, 130),
        (70000, 2, 121)]                 # 8 470 000 outputs > 32768 blocks x 256: a second trip of the loop


# the loop is shared by the six modes: its second trip is taken with both output layouts (mode 4: two halves) and with mode 3's own exit
POOL_MODES = [c + (mode,) for c in POOL for mode in range(6) if c[0] < 10000 or mode in (3, 4)]


@pytest.mark.parametrize("case", POOL_MODES, ids=ids(POOL_MODES))
def test_pool_nsample(dev, L, case):
    rows, ns, c, mode = case
    rng = np.random.default_rng(ns + c)
    X = rng.standard_normal((rows, ns, c)).astype(F32)
    X[rows // 2] = -np.abs(X[rows // 2]) - F32(1)               # an all-negative row: max from -inf, "min" positive
    gx = (rng.standard_normal((rows, ns, 3)) * 0.1).astype(F32)
    co = 2 * c if mode == 4 else c
    gX = Guarded(dev, X.size, fill=X)
    out = Guarded(dev, rows * co)
    ok(L, dev, "dispu_pool_nsample", rows, ns, c, mode, gX.ptr(), p(dv(gx, dev)) if mode == 3 else None, out.ptr())
    got = out.body().reshape(rows, co)
    what = "pool_nsample %s mode %d" % (case, mode)
    if mode == 3:
        want, mag = GO.pool_nsample(X, 3, gx)
        near(got, want, 4 * EPS32 * mag, what)
    else:
        exact(got, GO.pool_nsample(X, mode), what)
    assert out.guards_intact() and gX.guards_intact() and same_bits(gX.body(), X.reshape(-1))


GC = [(37, 5, 3), (2, 1, 1), (70000, 11, 11)]                    # the last: 8 470 000 elements, above the block cap


@pytest.mark.parametrize("case", GC, ids=ids(GC))
def test_group_center(dev, L, case):
    rows, ns, c = case
    rng = np.random.default_rng(rows)
    g, ctr = rng.standard_normal((rows, ns, c)).astype(F32), rng.standard_normal((rows, c)).astype(F32)
    gg, gc = Guarded(dev, g.size, fill=g), Guarded(dev, ctr.size, fill=ctr)
    ok(L, dev, "dispu_group_center", rows, ns, c, gg.ptr(), gc.ptr())
    exact(gg.body().reshape(g.shape), GO.group_center(g, ctr), "group_center %s" % (case,))
    assert gg.guards_intact() and gc.guards_intact() and same_bits(gc.body(), ctr.reshape(-1))


@pytest.mark.parametrize("rows", [1000, 32768 * 256 + 1000])     # the second: above the block cap
def test_idw_weights(dev, L, rows):
    rng = np.random.default_rng(rows)
    d = np.abs(rng.standard_normal((rows, 3), dtype=F32)) * (F32(10.0) ** rng.integers(-6, 1, (rows, 1)).astype(F32))
    d[0] = [F32(1.0), F32(0.0), F32(2.0)]                       # one zero distance: the 1e-10 clamp, that neighbour takes all the weight
    d[1] = 0.0                                                  # three zeros: a third each
    d[2] = F32(1e-10)                                           # at the clamp
    d[3] = [F32(5e-11), F32(1e-10), F32(2e-10)]                 # below, at and above it
    d[rows - 1] = 0.0
    gd, out = Guarded(dev, d.size, fill=d), Guarded(dev, d.size)
    ok(L, dev, "dispu_idw_weights", rows, gd.ptr(), out.ptr())
    got = out.body().reshape(rows, 3)
    exact(got, GO.idw_weights(d), "idw_weights %d rows" % rows)
    assert got[0, 1] == 1.0 and np.abs(got[1] - 1.0 / 3.0).max() <= EPS32 / 3 and np.abs(got[rows - 1] - 1.0 / 3.0).max() <= EPS32 / 3
    assert got[3, 0] == got[3, 1] and got[3, 2] < got[3, 0]                  # 5e-11 is raised to the clamp
    assert out.guards_intact() and gd.guards_intact()


L2N = [(300, 1), (300, 3), (300, 8), (32768 * 256 + 1000, 1)]    # the last: above the block cap


@pytest.mark.parametrize("case", L2N, ids=ids(L2N))
def test_l2_normalize_rows(dev, L, case):
    rows, c = case
    rng = np.random.default_rng(rows + c)
    X = rng.standard_normal((rows, c), dtype=F32) * (F32(10.0) ** rng.integers(-3, 3, (rows, 1)).astype(F32))
    X[0] = 0.0                                                  # zeros, not NaN
    X[1] = F32(np.sqrt(1.1e-12 / c))                            # sum of squares just above the 1e-12 clamp
    X[2] = F32(np.sqrt(1e-14 / c))                              # below it: x * 1e6
    X[rows - 1] = 0.0
    gX, out = Guarded(dev, X.size, fill=X), Guarded(dev, X.size)
    ok(L, dev, "dispu_l2_normalize_rows", rows, c, gX.ptr(), out.ptr())
    got = out.body().reshape(rows, c)
    want = GO.l2_normalize_rows(X)
    assert (got[0] == 0).all() and (got[rows - 1] == 0).all()
    near(got, want, 4 * EPS32 * np.abs(want), "l2_normalize_rows %s" % (case,))
    assert abs(float((got[2].astype(np.float64) ** 2).sum()) - 1e-2) < 1e-4 and abs(float((got[1].astype(np.float64) ** 2).sum()) - 1.0) < 1e-5
    assert out.guards_intact() and gX.guards_intact()


@pytest.mark.parametrize("n", [1, 1000, 32768 * 256 + 1000])
def test_scale_add(dev, L, n):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n, dtype=F32), rng.standard_normal(n, dtype=F32)
    y[: n // 2] = -x[: n // 2] * F32(1.3)                        # cancellation: where one and two roundings differ most often
    gx, gy, out = Guarded(dev, n, fill=x), Guarded(dev, n, fill=y), Guarded(dev, n)
    ok(L, dev, "dispu_scale_add", n, gx.ptr(), 1.3, gy.ptr(), out.ptr())
    got = out.body()
    unfused, fused = GO.scale_add(x, 1.3, y)
    either = (got == unfused) | (got == fused)
    print("[measured] scale_add n %d: %d elements where the two forms differ, %d equal the fused one there"
          % (n, int((unfused != fused).sum()), int(((got == fused) & (unfused != fused)).sum())))
    assert either.all(), "scale_add: %d elements are neither the fused nor the unfused float32 result" % int((~either).sum())
    assert out.guards_intact() and gx.guards_intact() and gy.guards_intact()


EDGE = [(2, 17, 5, 7, 3), (2, 16500, 16, 16, 0)]                # (B, n, k, c, ldo - 2c); the second: 8 448 000 elements, above the block cap


@pytest.mark.parametrize("case", EDGE, ids=ids(EDGE))
def test_edge_feature(dev, L, case):
    B, n, k, c, opad = case
    rows = B * n
    rng = np.random.default_rng(5)
    F = rng.standard_normal((B, n, c), dtype=F32)
    idx = table(rng, B, n, k)
    wide = np.full((rows, k + 3), -1, np.int32)                 # ldi > k, ioff = 1: the ids sit in columns 1 .. k
    wide[:, 1:1 + k] = idx.reshape(rows, k)
    wide[:, 0] = 0
    wide[:, 1 + k:] = 0
    sf, so = Strided(dev, rows, c, c + 2, 1, F), Strided(dev, rows * k, 2 * c, 2 * c + opad, min(opad, 1))
    ok(L, dev, "dispu_edge_feature", rows, n, k, c, sf.ptr(), sf.ld, p(dv(wide, dev)), k + 3, 1, so.ptr(), so.ld)
    exact(so.data(), GO.edge_feature(F, idx).reshape(rows * k, 2 * c), "edge_feature %s" % (case,))
    assert so.rest_untouched() and sf.untouched()


@pytest.mark.parametrize("n", [1, 63, 256, 257, 5000])
def test_row_mean_max(dev, L, n):
    b = 3
    rng = np.random.default_rng(n)
    x = rng.standard_normal((b, n)).astype(F32)
    x[1] = -np.abs(x[1]) - F32(0.5)                             # an all-negative row
    x[2, n - 1] = F32(7.0)                                      # the maximum in the last element
    gx, gm, gM = Guarded(dev, x.size, fill=x), Guarded(dev, b), Guarded(dev, b)
    ok(L, dev, "dispu_row_mean_max", b, n, gx.ptr(), gm.ptr(), gM.ptr())
    mean, mx, mabs = GO.row_mean_max(x)
    exact(gM.body(), mx, "row max n %d" % n)
    near(gm.body(), mean, n * EPS32 * mabs, "row mean n %d" % n)
    assert gm.guards_intact() and gM.guards_intact() and gx.guards_intact()


# --------------------------------------------------------------------- sizes every entry refuses or ignores ----
def test_refusals_and_noops_write_nothing(dev, L):
    """every argument check of the wrappers in csrc/mlp_misc.hip and csrc/modules.hip returns hipErrorInvalidValue, rows = 0 (nclouds,
    b, n = 0) returns 0, and neither writes.  (attention and the chains: test_attention_refusals, test_mlp_chain_refusals.)"""
    rng = np.random.default_rng(0)
    bufs = [Guarded(dev, 1 << 16, fill=rng.standard_normal(1 << 16).astype(F32)) for _ in range(6)]
    a, b, c, d, e, f = [g.ptr() for g in bufs]
    a1 = bufs[0].ptr(1)
    before = [g.body().copy() for g in bufs]
    idx = p(dv(np.zeros(1 << 16, np.int32), dev))

    def r(name, *args):
        return run(L, dev, name, *args)

    # dispu_linear_small_k(rows, K, N, X, ldx, W, bias, act, Y, ldy)
    for rows, K, N, X, W, Y, want in [(-1, 3, 24, a, b, c, INVALID), (8, 0, 24, a, b, c, INVALID), (8, -1, 24, a, b, c, INVALID), (8, 5, 24, a, b, c, INVALID),
                                      (8, 3, 8, a, b, c, INVALID), (8, 3, 32, a, b, c, INVALID), (8, 3, 20, a, b, c, INVALID), (8, 3, 24, None, b, c, INVALID),
                                      (8, 3, 24, a, None, c, INVALID), (8, 3, 24, a, b, None, INVALID), (0, 3, 24, a, b, c, 0)]:
        assert r("dispu_linear_small_k", rows, K, N, X, 4, W, d, 1, Y, 24) == want
    # dispu_linear_small_n(rows, K, N, X, ldx, W, bias, mode, R, ldr, Y, ldy)
    for rows, K, N, X, W, mode, R, Y, want in [(-1, 64, 3, a, b, 0, d, c, INVALID), (8, 0, 3, a, b, 0, d, c, INVALID), (8, 64, 4, a, b, 0, d, c, INVALID),
                                               (8, 64, 2, a, b, 0, d, c, INVALID), (8, 64, 3, None, b, 0, d, c, INVALID), (8, 64, 3, a, None, 0, d, c, INVALID),
                                               (8, 64, 3, a, b, 0, d, None, INVALID), (8, 64, 3, a, b, 1, None, c, INVALID), (8, 64, 3, a, b, -1, d, c, INVALID),
                                               (8, 64, 3, a, b, 2, d, c, INVALID), (0, 64, 3, a, b, 1, d, c, 0)]:
        assert r("dispu_linear_small_n", rows, K, N, X, 64, W, e, mode, R, 3, Y, 3) == want
    # dispu_dup_grid(nclouds, n, co, up, H, ldh, Wg, bias, grid, Y, ldy)
    for nc, n, co, up, H, ldh, Wg, bias, Y, ldy, want in [
            (-1, 8, 8, 4, a, 8, b, c, d, 8, INVALID), (2, 0, 8, 4, a, 8, b, c, d, 8, INVALID), (2, 8, 0, 4, a, 8, b, c, d, 8, INVALID),
            (2, 8, 8, 0, a, 8, b, c, d, 8, INVALID), (2, 8, 6, 4, a, 8, b, c, d, 8, INVALID), (2, 8, 8, 4, a, 10, b, c, d, 8, INVALID),
            (2, 8, 8, 4, a, 8, b, c, d, 9, INVALID), (2, 8, 8, 4, a1, 8, b, c, d, 8, INVALID), (2, 8, 8, 4, a, 8, bufs[1].ptr(2), c, d, 8, INVALID),
            (2, 8, 8, 4, a, 8, b, bufs[2].ptr(3), d, 8, INVALID), (2, 8, 8, 4, a, 8, b, c, bufs[3].ptr(1), 8, INVALID), (0, 8, 8, 4, a, 8, b, c, d, 8, 0)]:
        assert r("dispu_dup_grid", nc, n, co, up, H, ldh, Wg, bias, e, Y, ldy) == want
    # dispu_ps_prep(rows, co, xyz, W0, bias, G, ldg, A, lda)
    for rows, co, want in [(-1, 8, INVALID), (8, 0, INVALID), (8, -4, INVALID), (0, 8, 0)]:
        assert r("dispu_ps_prep", rows, co, a, b, c, d, 8, e, 8) == want
    # dispu_ps_gather_sub_relu(rows, n_per_cloud, k, c, idx, G, ldg, A, lda, X1, ldx1)
    for rows, n, k, ch, ldg, lda, ldx1, want in [(-1, 8, 4, 8, 8, 8, 8, INVALID), (8, 0, 4, 8, 8, 8, 8, INVALID), (8, 8, 0, 8, 8, 8, 8, INVALID),
                                                 (8, 8, 4, 0, 8, 8, 8, INVALID), (8, 8, 4, 6, 8, 8, 8, INVALID), (8, 8, 4, 8, 9, 8, 8, INVALID),
                                                 (8, 8, 4, 8, 8, 10, 8, INVALID), (8, 8, 4, 8, 8, 8, 11, INVALID), (0, 8, 4, 8, 8, 8, 8, 0)]:
        assert r("dispu_ps_gather_sub_relu", rows, n, k, ch, idx, a, ldg, b, lda, c, ldx1) == want
    # dispu_ps_skip_max(rows, n_per_cloud, k, cf, idx, xyz, feat, ldf, out, ldo)
    for rows, n, k, cf, feat, ldf, want in [(-1, 8, 4, 8, b, 8, INVALID), (8, 0, 4, 8, b, 8, INVALID), (8, 8, 0, 8, b, 8, INVALID), (8, 8, 4, 0, b, 8, INVALID),
                                            (8, 8, 4, 132, b, 132, INVALID), (8, 8, 4, 6, b, 8, INVALID), (8, 8, 4, 8, b, 9, INVALID),
                                            (8, 8, 4, 8, bufs[1].ptr(1), 8, INVALID), (8, 8, 16, 128, bufs[1].ptr(2), 128, INVALID), (0, 8, 4, 8, b, 8, 0)]:
        assert r("dispu_ps_skip_max", rows, n, k, cf, idx, a, feat, ldf, c, 6 + max(cf, 1)) == want
    # dispu_ps_weight_net(rows, n_per_cloud, k, t_n, idx, xyz, Ww, bw, scale, shift, wv)
    for rows, n, k, t, want in [(-1, 8, 4, 16, INVALID), (8, 0, 4, 16, INVALID), (8, 8, 0, 16, INVALID), (8, 8, 4, 0, INVALID), (8, 8, -1, 16, INVALID), (0, 8, 4, 16, 0)]:
        assert r("dispu_ps_weight_net", rows, n, k, t, idx, a, b, c, d, e, f) == want
    # dispu_ps_point_matmul(rows, k, c, t_n, X2, ldx2, wv, out, ldo)
    for rows, k, ch, t, ldo, want in [(-1, 16, 128, 16, 2048, INVALID), (1, 15, 128, 16, 2048, INVALID), (1, 16, 64, 16, 2048, INVALID),
                                      (1, 16, 128, 8, 2048, INVALID), (1, 16, 128, 16, 2049, INVALID), (1, 16, 128, 16, 2050, INVALID), (0, 16, 128, 16, 2048, 0)]:
        assert r("dispu_ps_point_matmul", rows, k, ch, t, a, 128, b, c, ldo) == want
    # csrc/modules.hip
    for rows, ns, ch, want in [(-1, 4, 4, INVALID), (4, 0, 4, INVALID), (4, -1, 4, INVALID), (4, 4, 0, INVALID), (4, 4, -2, INVALID), (0, 4, 4, 0)]:
        assert r("dispu_group_center", rows, ns, ch, a, b) == want
        for mode in range(6):
            assert r("dispu_pool_nsample", rows, ns, ch, mode, b, c, a) == want
    assert r("dispu_pool_nsample", 4, 4, 4, -1, b, c, a) == INVALID and r("dispu_pool_nsample", 4, 4, 4, 6, b, c, a) == INVALID
    assert r("dispu_pool_nsample", 4, 4, 4, 3, b, None, a) == INVALID
    for rows, ch, want in [(-1, 4, INVALID), (4, 0, INVALID), (4, -1, INVALID), (0, 4, 0)]:
        assert r("dispu_l2_normalize_rows", rows, ch, b, a) == want
    assert r("dispu_scale_add", -1, b, 2.0, c, a) == INVALID and r("dispu_scale_add", 0, b, 2.0, c, a) == 0
    assert r("dispu_idw_weights", -1, b, a) == INVALID and r("dispu_idw_weights", 0, b, a) == 0
    for rows, n, k, ch, want in [(-1, 4, 2, 4, INVALID), (4, 0, 2, 4, INVALID), (4, 4, 0, 4, INVALID), (4, 4, 2, 0, INVALID), (4, -4, 2, 4, INVALID), (0, 4, 2, 4, 0)]:
        assert r("dispu_edge_feature", rows, n, k, ch, b, 4, idx, 2, 0, a, 8) == want
    for bb, n, want in [(-1, 4, INVALID), (4, 0, INVALID), (4, -1, INVALID), (0, 4, 0)]:
        assert r("dispu_row_mean_max", bb, n, c, a, b) == want
    for g, was in zip(bufs, before):
        assert same_bits(g.body(), was) and g.guards_intact()
    assert SENT != 0
