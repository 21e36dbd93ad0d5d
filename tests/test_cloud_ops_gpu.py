"""The whole-cloud glue kernels, each ALONE through the C ABI against tests/cloud_ops_oracle.py (plain numpy, held to oracle/upsample.py
by tests/test_cloud_ops_oracle.py), on every path their launch code takes and with ties at every place a selection can meet one.

Entries under test: csrc/cloud.hip (dispu_knn_patch, dispu_knn_patch_segments, dispu_normalize_patches, dispu_normalize_segments,
dispu_denormalize_patches), mode 0 of csrc/knn_general.hip (the radix select behind dispu_knn_patch above 8192 points) and
dispu_row_mean_std of csrc/mesh_eval.hip.

Every output is pre-filled with a sentinel and sits between guards of it (train_ops_oracle.Guarded): a kernel that writes one element
outside its rows, or leaves one of them unwritten, fails the test.  Every case with more than one cloud has clouds that differ.  No
call passes an index or a shape its entry point does not refuse on the host.

Standards.
  k-NN              index-exact: the oracle is a stable argsort of ((dx dx + dy dy) + dz dz) + 0 in float32, ties to the lower index.
  normalisation     centroid, furthest and every coordinate equal, as bits, the float32 replay of the kernel's own order of operations
                    (which tests/test_cloud_ops_oracle.py holds to oracle.upsample.normalize_point_cloud bit for bit); NaN where the
                    replay has NaN (n = 1, coincident points).  Also within cloud_ops_oracle.normalize_f64's bound of the float64
                    result, u = 2^-24:  centroid n u (1 + n u) mean |x_a| =: delta_a (the sequential sum);  furthest |delta|_2 + 4 u f;
                    coordinate (delta_a + |out| |delta|_2) / f^ + 6 u |out| f / f^ -- the centroid's error enters every coordinate
                    once directly and once through the furthest distance, both divided by it.
  denormalisation   bit-exact against centroid + x * furthest in float32, the product rounded before the sum.
  row mean / std    float64 np.nanmean / np.nanstd (ddof 0): mean within n 2^-52 mean |x|, std within max(n, 4) 2^-52 s +
                    mean_bound^2 / (2 s) of the root mean square deviation s (cloud_ops_oracle.nan_mean_std derives both); NaN for a
                    row without a number, exactly 0 for a row of one repeated value.
Every float comparison prints its worst error as a fraction of its bound before it asserts (pytest -s).

Paths and the case that reaches each (the host branch that selects it is named; nothing is instrumented):
  knn_patch_kernel, dense (n <= 8192)                  test_knn_bitonic[n]: n = 1, 2, 3 (npad = 2, 2, 4), 5, 255, 256, 257 (npad 256 / 512: one
                                                        and two trips of the key loop), 1000, 8192 (64 KiB of keys); k = 1, 256, n;
                                                        b = 1, 3; m = 1, 5; queries on and off the cloud
  knn_general_kernel<0>, dense (n > 8192)              test_knn_radix[n-k]: n = 8193 (one point in chunk 33), 9261, 24576; k = 1, 255, 256,
                                                        257 (kpad 2, 256, 256, 512), 1024, 4096 (KG_MAXK)
  ties at the k-th place, both kernels                 test_knn_ties[lattice20 / copies8192 / identical8192] (bitonic),
                                                        [lattice21 / copies24576 / identical9261] (radix: `base` across chunks, `wcnt`
                                                        across waves, `quota` below the number of equal keys)
  both kernels from one dispu_knn_patch_segments call   test_knn_segments[k-pattern]: segments of 1, 256, 300, 8000, 8192 points (npad per
                                                        segment inside a launch sized for 8192) and of 8193, 9261 points (seg_nmin = 8192);
                                                        m_c = 0, 1, 4; patterns `small_only` / `large_only` leave `mlarge` / `msmall` 0
  normalize_patches_kernel, dense / segments            test_normalize[n], test_normalize_coincident / test_normalize_segments: n < 64 (idle
                                                        lanes), 64, 65, 256, 300, 8192, 24576; b = 1, 3, 70
  denormalize_patches_kernel, one trip / two            test_denormalize[1-1], [3-5], [2-256], [12-4096] / [288-4096] (3 538 944 floats, the
                                                        16x shape), [3-240000] (2 160 000): past the 8192 x 256 = 2 097 152 of the grid cap
  row_mean_std_kernel                                   test_row_mean_std[b-n]: n = 1, 255 (idle threads), 257 (a second trip), 100000

Mutations (arithmetic only, on a scratch build; the two that take too many keys in the collect pass also got `pos < kpad` in front of
the LDS write so that they stay inside the key array) and the tests of this file that fail under each, all others passing.  They were
applied in three scratch builds, each with at most one mutation per kernel; a failure belongs to the mutation of the kernel its case
runs, which the message names (the path, and for the segment form the segment's size):
  `before = 0` for `before = base`, collect pass of     test_knn_ties[lattice21], [copies24576]; test_knn_segments[256-mixed_a], [256-mixed_b],
  knn_general_kernel                                    [256-large_only], each naming the 9261-point segment.  (identical9261 passes: with every
                                                        key equal the first chunk alone fills the k places, in index order)
  `key <= T` for `lt`, same pass                        the same five
  `a >= c` for `a > c`, knn_patch_kernel                none, as it must be: the keys hold the index, so no two are equal and `>=` is `>`
  compare-exchange on the distance bits alone (the      knn_patch_kernel: test_knn_bitonic[1000], [8192] (random float32 distances already tie
  key's index ignored), either kernel                   at these sizes), test_knn_ties[lattice20], [copies8192], [identical8192],
                                                        test_knn_segments[256-small_only], [256-mixed_a], [256-mixed_b] naming the 8000-point
                                                        segment;  knn_general_kernel: test_knn_radix[8193-4096], [24576-4096],
                                                        test_knn_ties[lattice21], [copies24576], [identical9261], test_knn_segments[256-mixed_a],
                                                        [256-mixed_b], [256-large_only] naming the 9261-point segment
  `s / (float)(n - 1)` in the centroid                  test_normalize (all nine), test_normalize_coincident (all three), test_normalize_segments
  `furthest[0]` for `furthest[b]`                       test_denormalize, every case with more than one patch
  `e / ((long)m * 3)` computed in int                   none, and none can: below 2^31 elements (8 GiB each way) int and long give the same
                                                        quotient, and past that the mutated index is negative -- an out-of-bounds read, which
                                                        no mutation here may make.  The unmutated line is 64-bit throughout by reading
  no NaN test in row_mean_std_kernel's second pass      test_row_mean_std[1-255], [3-257], [2-100000] (the rows with NaNs scattered: std not finite)
test_refusals passes under every one of them.

Measured on an MI355X: every k-NN index, every bit of the normalisation (the division and sqrtf of the build are the correctly rounded
ones) and of the denormalisation as the oracle has it.  Worst error as a fraction of its float64 bound: normalize_patches centroid
0.50, furthest 0.33, coordinates 0.43, all at n = 2 where the bound is tightest (at n = 24576, b = 70: 0.005, 0.003, 0.004 -- the
sequential sum uses a small part of what n u mean |x| allows); normalize_segments 0.43, 0.30, 0.39; row mean below 0.0001 (largest
absolute error 1.4e-17), row std 0.003.  No bound stated above had to be widened."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ops_oracle as CO  # noqa: E402
import train_ops_oracle as TO  # noqa: E402
from train_ops_oracle import F32, INVALID, SENT, Guarded, dv, p  # noqa: E402

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


def hp(a):
    """a host int32 array as the void* the segment entries read on the host."""
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return C.c_void_p(a.ctypes.data)


def ints(g):
    """the body of a Guarded buffer an entry wrote int32 into."""
    return np.ascontiguousarray(g.body()).view(np.int32)


def untouched(g):
    return g.guards_intact() and bool((g.body() == F32(SENT)).all())


def exact_idx(got, want, what):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d indices differ, first at %s: got %d, want %d" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def bits_or_nan(got, want, what):
    """float32 arrays equal as bits; where `want` is NaN, `got` is NaN (of any payload)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got)[nan].all(), "%s: a number where the replay has NaN" % what
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not diff.any(), "%s: %d of %d elements differ in bits, first at %s: got %r, want %r" % (
        what, int(diff.sum()), want.size, tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])


def near(got, want, bound, what):
    """|got - want| <= bound per element where `want` is a number, the worst fraction printed first; got must be finite there."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    use = ~np.isnan(want)
    assert np.isfinite(got[use]).all(), what + ": not finite"
    err = np.abs(got[use] - want[use])
    frac = float((err / np.maximum(bound[use], 1e-300)).max()) if err.size else 0.0
    print("[measured] %s: worst error %.4f of its bound (largest absolute error %.3e)" % (what, frac, err.max() if err.size else 0.0))
    assert (err <= bound[use]).all(), "%s: %d elements beyond the bound, worst %.3f of it" % (what, int((err > bound[use]).sum()), frac)


# ------------------------------------------------------------------------------------------------ dispu_knn_patch ----
def knn_dense(L, dev, pc, q, k):
    b, n, _ = pc.shape
    m = q.shape[1]
    out = Guarded(dev, b * m * k)
    gp, gq = Guarded(dev, pc.size, fill=pc), Guarded(dev, q.size, fill=q)
    ok(L, dev, "dispu_knn_patch", b, n, m, k, gp.ptr(), gq.ptr(), out.ptr())
    assert out.guards_intact(), "knn_patch b %d n %d m %d k %d wrote outside its rows" % (b, n, m, k)
    assert TO.same_bits(gp.body(), pc.reshape(-1)) and TO.same_bits(gq.body(), q.reshape(-1))
    return ints(out).reshape(b, m, k)


BITONIC_N = [1, 2, 3, 5, 255, 256, 257, 1000, 8192]


@pytest.mark.parametrize("n", BITONIC_N)
def test_knn_bitonic(dev, L, n):
    """path: n <= 8192 in dispu_knn_patch -> knn_patch_kernel with npad = max(2, the next power of two)."""
    for (b, m) in ((1, 1), (1, 5), (3, 1), (3, 5)):
        pc, q = CO.random_case(b, n, m, seed=1000 * n + 10 * b + m)
        for k in sorted(set([1, n] + ([256] if n >= 256 else []))):
            exact_idx(knn_dense(L, dev, pc, q, k), CO.knn_batch(q, pc, k), "knn_patch bitonic n %d k %d b %d m %d" % (n, k, b, m))


RADIX = [(8193, 1), (8193, 257), (8193, 4096), (9261, 255), (9261, 256), (9261, 1024), (24576, 1), (24576, 256), (24576, 1024), (24576, 4096)]


@pytest.mark.parametrize("case", RADIX, ids=ids(RADIX))
def test_knn_radix(dev, L, case):
    """path: n > 8192 in dispu_knn_patch -> knn_general_launch(mode 0): radix select, collect, bitonic sort of kpad keys."""
    n, k = case
    pc, q = CO.random_case(2, n, 5, seed=n + k)
    exact_idx(knn_dense(L, dev, pc, q, k), CO.knn_batch(q, pc, k), "knn_patch radix n %d k %d" % (n, k))


@pytest.mark.parametrize("case", CO.TIE_CASES, ids=[c[0] for c in CO.TIE_CASES])
def test_knn_ties(dev, L, case):
    """path: by the cloud's size, bitonic (8000, 8192 points) or radix (9261, 24576).  What each cloud's ties are is asserted from the
    oracle's distances by tests/test_cloud_ops_oracle.py::test_tie_inputs_hold_the_ties_they_are_for."""
    name, build, arg, ks, _ = case
    pc, q = build(arg)
    for k in ks:
        exact_idx(knn_dense(L, dev, pc, q, k), CO.knn_batch(q, pc, k), "knn_patch ties %s k %d" % (name, k))


# --------------------------------------------------------------------------------------- dispu_knn_patch_segments ----
SEG_SIZES = [1, 256, 300, 8000, 8192, 8193, 9261]
SEG_PATTERNS = {                                    # queries per segment, of 0, 1, 4
    "mixed_a": [1, 4, 0, 4, 1, 0, 4],
    "mixed_b": [4, 0, 1, 1, 4, 4, 1],
    "small_only": [1, 1, 4, 1, 1, 0, 0],            # mlarge = 0: the radix launch is skipped
    "large_only": [0, 0, 0, 0, 0, 1, 4],            # msmall = 0: the bitonic launch is skipped
}


def segment_inputs(sizes, ms):
    """-> list of (cloud [n, 3], queries [m, 3]): the lattices for 8000 and 9261 points, random clouds otherwise, all different."""
    segs = []
    for i, (n, m) in enumerate(zip(sizes, ms)):
        if n in (8000, 9261):
            pc, q = CO.lattice_case(20 if n == 8000 else 21)
            segs.append((pc[i % 2], q[i % 2][:m]))
        else:
            pc, q = CO.random_case(1, n, max(m, 1), seed=77 + n + i)
            segs.append((pc[0], q[0][:m]))
    return segs


SEG_CASES = [(k, name) for k in (1, 256) for name in sorted(SEG_PATTERNS)]


@pytest.mark.parametrize("case", SEG_CASES, ids=ids(SEG_CASES))
def test_knn_segments(dev, L, case):
    """one call over segments on both sides of 8192 points; every segment against the ORACLE.  A segment without queries owns no rows:
    its neighbours' rows hold exactly their own result and the guards hold."""
    k, name = case
    sizes, ms = list(SEG_SIZES), list(SEG_PATTERNS[name])
    if k > 1:
        sizes, ms = sizes[1:], ms[1:]                                          # without the 1-point segment
    segs = segment_inputs(sizes, ms)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    qoff = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
    cloud = np.concatenate([s[0] for s in segs])
    queries = np.concatenate([s[1] for s in segs] + [np.zeros((1, 3), F32)])   # one spare row: never an empty allocation
    out = Guarded(dev, int(qoff[-1]) * k)
    gp = Guarded(dev, cloud.size, fill=cloud)
    ok(L, dev, "dispu_knn_patch_segments", len(sizes), p(dv(off, dev)), p(dv(qoff, dev)), hp(off), hp(qoff), k, gp.ptr(), p(dv(queries, dev)),
       out.ptr())
    assert out.guards_intact() and TO.same_bits(gp.body(), cloud.reshape(-1))
    got = ints(out).reshape(-1, k)
    for c, (pc, q) in enumerate(segs):
        if len(q):
            exact_idx(got[qoff[c]:qoff[c + 1]], CO.knn(q, pc, k)[0], "knn_patch_segments %s k %d segment %d (%d points)" % (name, k, c, sizes[c]))


# ------------------------------------------------------------ dispu_normalize_patches, dispu_normalize_segments ----
NORM_N = [1, 2, 63, 64, 65, 256, 300, 8192, 24576]


def normalize_dense(L, dev, x):
    b, n, _ = x.shape
    gin, out, cen, fur = Guarded(dev, x.size, fill=x), Guarded(dev, x.size), Guarded(dev, 3 * b), Guarded(dev, b)
    ok(L, dev, "dispu_normalize_patches", b, n, gin.ptr(), out.ptr(), cen.ptr(), fur.ptr())
    assert out.guards_intact() and cen.guards_intact() and fur.guards_intact() and gin.guards_intact()
    assert TO.same_bits(gin.body(), x.reshape(-1))
    return out.body().reshape(b, n, 3), cen.body().reshape(b, 3), fur.body()


def check_normalized(got, x, what, f64=True):
    out, cen, fur = got
    w_out, w_cen, w_fur = CO.normalize_replay(x)
    bits_or_nan(cen, w_cen, what + " centroid")
    bits_or_nan(fur, w_fur, what + " furthest")
    bits_or_nan(out, w_out, what + " coordinates")
    if f64:
        ref = CO.normalize_f64(x)
        near(cen, ref["centroid"], ref["centroid_bound"], what + " centroid vs float64")
        near(fur, ref["furthest"], ref["furthest_bound"], what + " furthest vs float64")
        if x.shape[1] > 1:
            near(out, ref["out"], ref["out_bound"], what + " coordinates vs float64")


@pytest.mark.parametrize("n", NORM_N)
def test_normalize(dev, L, n):
    """path: one wave per cloud; n < 64 leaves lanes idle, n = 65 gives lane 0 a second trip; the sequential sum runs n terms."""
    for (b, first) in ((1, 0), (1, 1), (3, 0), (70, 2)):                       # b = 1 at +5 and at -300
        x = CO.offcentre_clouds(b, n, seed=n + b, first=first)
        check_normalized(normalize_dense(L, dev, x), x, "normalize_patches n %d b %d (first cloud %d)" % (n, b, first))


def coincident_clouds(n):
    """three clouds: n copies of a point whose sums are exact (furthest 0, every coordinate NaN), a random cloud, n copies of a point
    whose sum rounds (whatever the float32 sequence makes of it -- the replay says)."""
    x = CO.offcentre_clouds(3, n, seed=n)
    x[0] = (0.5, -2.0, 1.25)
    x[2] = (0.1, 299.7, -3.3)
    return x


@pytest.mark.parametrize("n", [2, 300, 24576])
def test_normalize_coincident(dev, L, n):
    x = coincident_clouds(n)
    assert np.isnan(CO.normalize_replay(x)[0][0]).all()
    check_normalized(normalize_dense(L, dev, x), x, "normalize_patches coincident n %d" % n, f64=False)   # float64 has 0 / 0 in cloud 2 too


def test_normalize_segments(dev, L):
    """the same sizes packed in one call, in two orders; the second holds the coincident clouds too."""
    for sizes, special in ((NORM_N, False), ([24576, 300, 1, 65, 300, 8192, 2, 64, 63, 256, 2], True)):
        clouds = [CO.offcentre_clouds(1, n, seed=5 * i + n, first=i)[0] for i, n in enumerate(sizes)]
        if special:
            clouds[1], clouds[4] = coincident_clouds(300)[0], coincident_clouds(300)[2]
        x = np.concatenate(clouds)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        Cn = len(sizes)
        gin, out, cen, fur = Guarded(dev, x.size, fill=x), Guarded(dev, x.size), Guarded(dev, 3 * Cn), Guarded(dev, Cn)
        ok(L, dev, "dispu_normalize_segments", Cn, p(dv(off, dev)), hp(off), gin.ptr(), out.ptr(), cen.ptr(), fur.ptr())
        assert out.guards_intact() and cen.guards_intact() and fur.guards_intact() and TO.same_bits(gin.body(), x.reshape(-1))
        o, c, f = out.body().reshape(-1, 3), cen.body().reshape(Cn, 3), fur.body()
        for i, n in enumerate(sizes):
            got = (o[off[i]:off[i + 1]][None], c[i:i + 1], f[i:i + 1])
            check_normalized(got, clouds[i][None], "normalize_segments segment %d (%d points)" % (i, n), f64=not special and n > 1)


# -------------------------------------------------------------------------------------- dispu_denormalize_patches ----
DENORM = [(1, 1), (3, 5), (2, 256), (12, 4096),
          (288, 4096), (3, 240000)]                  # 3 538 944 and 2 160 000 floats > 8192 blocks x 256: a second trip of the loop


@pytest.mark.parametrize("case", DENORM, ids=ids(DENORM))
def test_denormalize(dev, L, case):
    """every patch has its own centroid (1e-4 .. 1e4, either sign) and scale (1e-3 .. 1e3): a wrong patch index b = e / (3 m), or a
    scale taken from another patch, lands orders of magnitude off."""
    b, m = case
    rng = np.random.default_rng(b + m)
    x = rng.uniform(-1, 1, (b, m, 3)).astype(F32)
    cen = (rng.uniform(1, 9, (b, 3)) * 10.0 ** ((np.arange(b) % 9) - 4)[:, None] * np.where(np.arange(b) % 2, -1, 1)[:, None]).astype(F32)
    fur = (rng.uniform(1, 9, b) * 10.0 ** ((np.arange(b) % 7) - 3)).astype(F32)
    gin, gc, gf, out = Guarded(dev, x.size, fill=x), Guarded(dev, cen.size, fill=cen), Guarded(dev, b, fill=fur), Guarded(dev, x.size)
    ok(L, dev, "dispu_denormalize_patches", b, m, gin.ptr(), gc.ptr(), gf.ptr(), out.ptr())
    assert out.guards_intact() and gin.guards_intact() and gc.guards_intact() and gf.guards_intact()
    assert TO.same_bits(gin.body(), x.reshape(-1)) and TO.same_bits(gc.body(), cen.reshape(-1)) and TO.same_bits(gf.body(), fur)
    bits_or_nan(out.body().reshape(b, m, 3), CO.denormalize(x, cen, fur), "denormalize_patches b %d m %d" % (b, m))


# --------------------------------------------------------------------------------------------- dispu_row_mean_std ----
STAT = [(1, 1), (1, 255), (3, 257), (2, 100000)]


def doubles(g):
    return np.ascontiguousarray(g.body()).view(np.float64)


@pytest.mark.parametrize("case", STAT, ids=ids(STAT))
def test_row_mean_std(dev, L, case):
    """four calls: every kind of row (NaNs scattered, all NaN, one repeated value, 1000 + 1e-3 noise) in every row position, so each
    row's two outputs sit next to those of rows of another kind."""
    b, n = case
    for turn in range(4):
        x, kinds = CO.stat_rows(b, n, turn, seed=n)
        ref = CO.nan_mean_std(x)
        gin, out = Guarded(dev, x.size, fill=x), Guarded(dev, 4 * b)                  # [b, 2] doubles; the body is 16-byte aligned
        ok(L, dev, "dispu_row_mean_std", b, n, gin.ptr(), out.ptr())
        assert out.guards_intact() and gin.guards_intact()
        got = doubles(out).reshape(b, 2)
        for i, kind in enumerate(kinds):
            what = "row_mean_std b %d n %d row %d (%s)" % (b, n, i, kind)
            if kind == "allnan":
                assert np.isnan(got[i]).all(), what + ": %r" % (got[i],)
                continue
            near(got[i:i + 1, 0], ref["mean"][i:i + 1], ref["mean_bound"][i:i + 1], what + " mean")
            near(got[i:i + 1, 1], ref["std"][i:i + 1], ref["std_bound"][i:i + 1], what + " std")
            if kind == "constant":
                assert got[i, 1] == 0.0 and got[i, 0] == float(x[i, 0]), what


# ------------------------------------------------------------------------------------------------------ refusals ----
def test_refusals(dev, L):
    """every documented host-side refusal returns hipErrorInvalidValue and launches nothing; b = 0 / m = 0 / C = 0 return 0 and launch
    nothing; the same buffers with valid arguments are written."""
    pc, q = CO.random_case(2, 9261, 2, seed=9)
    gp, gq = Guarded(dev, pc.size, fill=pc), Guarded(dev, q.size, fill=q)
    idx = Guarded(dev, 2 * 2 * 4100)

    def knn(b=2, n=300, m=2, k=16):
        return run(L, dev, "dispu_knn_patch", b, n, m, k, gp.ptr(), gq.ptr(), idx.ptr())

    assert knn(k=301) == INVALID and knn(n=9261, k=9262) == INVALID                     # k > n on either path
    assert knn(k=0) == INVALID and knn(k=-1) == INVALID
    assert knn(n=0) == INVALID and knn(n=-5) == INVALID
    assert knn(n=9261, k=4097) == INVALID and knn(n=8193, k=4100) == INVALID              # n > 8192 with k > 4096
    assert knn(b=-1) == INVALID and knn(m=-1) == INVALID
    assert knn(b=0) == 0 and knn(m=0) == 0
    assert untouched(idx)
    assert knn() == 0 and not untouched(idx) and idx.guards_intact()

    # ---- segment entries
    sizes = np.array([300, 9261, 256], np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    qoff = np.array([0, 2, 3, 4], np.int32)
    cloud = CO.random_case(1, int(off[-1]), 4, seed=10)
    gc, gqs = Guarded(dev, cloud[0].size, fill=cloud[0]), Guarded(dev, cloud[1].size, fill=cloud[1])
    sidx = Guarded(dev, 4 * 4100)
    d_off, d_qoff = dv(off, dev), dv(qoff, dev)
    big = np.zeros(65538, np.int32)

    def seg(Cn=3, o=p(d_off), qo=p(d_qoff), oh=off, qh=qoff, k=16, cl=gc.ptr(), qs=gqs.ptr(), ix=sidx.ptr()):
        return run(L, dev, "dispu_knn_patch_segments", Cn, o, qo, hp(oh) if oh is not None else None, hp(qh) if qh is not None else None, k, cl, qs, ix)

    def moved(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    assert seg(Cn=-1) == INVALID and seg(k=0) == INVALID and seg(k=-2) == INVALID
    assert seg(Cn=0) == 0
    assert seg(Cn=65536, oh=big, qh=big) == INVALID                                       # C > 65535 (refused before any offset is read)
    assert seg(o=None) == INVALID and seg(qo=None) == INVALID and seg(oh=None) == INVALID and seg(qh=None) == INVALID
    assert seg(cl=None) == INVALID and seg(qs=None) == INVALID and seg(ix=None) == INVALID
    assert seg(oh=moved(off, 0, 1)) == INVALID and seg(qh=moved(qoff, 0, 1)) == INVALID   # off_host[0] != 0
    assert seg(oh=moved(off, 2, off[1])) == INVALID                                       # an empty segment
    assert seg(oh=moved(off, 2, off[1] - 1)) == INVALID                                   # a negative one
    assert seg(qh=moved(qoff, 2, 1)) == INVALID                                           # a negative query count
    assert seg(k=257) == INVALID                                                          # k > n of the 256-point segment
    big_first = np.array([0, 9261, 9561, 9817], np.int32)
    assert seg(oh=big_first, k=4097, Cn=1) == INVALID                                     # k <= n = 9261, but n > 8192 with k > 4096
    assert seg(oh=big_first, k=4096, Cn=2) == INVALID                                     # k > n of the second segment
    assert untouched(sidx)
    assert seg() == 0 and not untouched(sidx) and sidx.guards_intact()
    assert seg(Cn=2, k=300) == 0                                                          # 300 <= both sizes, <= 4096

    x = cloud[0]
    out, cen, fur = Guarded(dev, x.size), Guarded(dev, 9), Guarded(dev, 3)

    def nseg(Cn=3, o=p(d_off), oh=off, i=gc.ptr(), ou=out.ptr(), ce=cen.ptr(), fu=fur.ptr()):
        return run(L, dev, "dispu_normalize_segments", Cn, o, hp(oh) if oh is not None else None, i, ou, ce, fu)

    assert nseg(Cn=-1) == INVALID and nseg(Cn=0) == 0
    assert nseg(o=None) == INVALID and nseg(oh=None) == INVALID and nseg(i=None) == INVALID
    assert nseg(ou=None) == INVALID and nseg(ce=None) == INVALID and nseg(fu=None) == INVALID
    assert nseg(oh=moved(off, 0, 1)) == INVALID
    assert nseg(oh=moved(off, 2, off[1])) == INVALID and nseg(oh=moved(off, 2, off[1] - 1)) == INVALID      # an empty segment
    assert untouched(out) and untouched(cen) and untouched(fur)
    assert nseg() == 0 and not untouched(out) and not untouched(cen) and not untouched(fur)

    # ---- the dense glue
    out, cen, fur = Guarded(dev, x.size), Guarded(dev, 9), Guarded(dev, 3)

    def norm(b=3, n=256):
        return run(L, dev, "dispu_normalize_patches", b, n, gc.ptr(), out.ptr(), cen.ptr(), fur.ptr())

    def denorm(b=3, m=256):
        return run(L, dev, "dispu_denormalize_patches", b, m, gc.ptr(), gqs.ptr(), gqs.ptr(), out.ptr())

    stat = Guarded(dev, 4 * 3)

    def rms(b=3, n=256):
        return run(L, dev, "dispu_row_mean_std", b, n, gc.ptr(), stat.ptr())

    assert norm(b=-1) == INVALID and norm(n=0) == INVALID and norm(n=-1) == INVALID and norm(b=0) == 0
    assert denorm(b=-1) == INVALID and denorm(m=0) == INVALID and denorm(m=-1) == INVALID and denorm(b=0) == 0
    assert rms(b=-1) == INVALID and rms(n=0) == INVALID and rms(n=-1) == INVALID and rms(b=0) == 0
    assert untouched(out) and untouched(cen) and untouched(fur) and untouched(stat)
    assert norm() == 0 and not untouched(out) and not untouched(cen) and not untouched(fur)
    assert rms() == 0 and not untouched(stat) and stat.guards_intact()
    out2 = Guarded(dev, x.size)
    assert run(L, dev, "dispu_denormalize_patches", 3, 256, gc.ptr(), gqs.ptr(), gqs.ptr(), out2.ptr()) == 0 and not untouched(out2)
    assert gc.guards_intact() and TO.same_bits(gc.body(), x.reshape(-1))
