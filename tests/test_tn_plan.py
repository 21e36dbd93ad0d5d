"""CPU tests of the weight-gradient (TN) dispatches: dispu_linear_tn_plan, dispu_linear_tn_bf16_plan and dispu_linear_tn_bf16_stream_plan
export the host decision the three launchers run off; they make no HIP call and dereference nothing, so everything here runs without
a GPU.  A census sweeps the argument space for the set of instantiations each dispatch can reach, and the case table of the GPU
matrix (tests/tn_paths.py) is held to it: every reachable instantiation has a case, and every case takes the path its group names.

Census (batch 1 - 3; M 1 - 49, round every power of two up to 4096, 4080 - 4111, and on to 131072; K and N 1 - 2048 with
non-multiples of 4, 16 and 64; aligned / odd-stride / 4-bytes-off operands; aligned / odd-ldo / misaligned / odd-so outputs; accumulate
and dbias on and off):
  fp32    (kernel, TK, TNN, edge, direct, reduce): 34 reachable = the narrow kernel x {scalar, vec4} + six tiles x {interior, edge} x
          {direct, scalar, vec4} less four: <1,4> and <2,1> never store directly, interior or edge.  A direct store needs one split,
          i.e. M <= 256 rows or >= 768 output tiles, and either way the tile rule then asks 256 tiles of the candidate: 64 x 256 tiles
          of an N <= 2048 output are 8 x batch, 128 x 64 tiles of a K <= 2048 one 16 x batch.  Beyond the bounds they exist: batch 3,
          M 16, K 64 x N 22016 (interior; K 1 x N 21761 edge) is a direct <1,4>, K 11008 x N 64 (K 10881 x N 1) a direct <2,1>.
  bf16    (tile, split / single workgroup): all 6, each with the four storage masks = 24.  128 x 128 is reachable below 512 output tiles
          after all: a (K <= 64) x (32 < N <= 128) output is one or two 64 x 64 tiles, the plan then asks 512 - 1024 splits of >= 256
          rows, and 512 splits of ONE 128 x 128 tile meet the rule's 512 workgroups -- from M = 130817 rows on.  Without a split it takes
          512 tiles: batch 2, K = N = 2047.
  stream  (BN, storage): all 4.
"""
import itertools

import numpy as np
import pytest

import tn_paths as TP

A = TP.BASE

M_DENSE = list(range(1, 50)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 304, 511, 512, 513, 544, 1000, 1023, 1024, 1025, 2000, 2047,
                                2048, 2049, 3000] + list(range(4080, 4112)) + [5000, 8192, 8196, 8320, 10000, 16127, 16384, 32768, 33279,
                                                                               65536, 70000, 100000, 130816, 130817, 131072]
KN = [1, 2, 3, 4, 5, 7, 16, 17, 24, 32, 33, 63, 64, 65, 100, 127, 128, 129, 132, 192, 255, 256, 257, 272, 384, 512, 513, 640, 768, 1000,
      1024, 1025, 1028, 1536, 2047, 2048]
M_THIN = [1, 16, 17, 48, 256, 257, 304, 1000, 2048, 4096, 4100, 8192, 32768, 131072]
KN_THIN = [1, 4, 5, 64, 65, 128, 129, 256, 257, 1024, 1025, 2048]

F32_UNREACHABLE = {("f32", "tiled", tk, tnn, e, 1, "none") for tk, tnn in ((1, 4), (2, 1)) for e in (0, 1)}
BEYOND = {("f32", "tiled", 1, 4, 0, 1, "none"): (3, 16, 64, 22016), ("f32", "tiled", 1, 4, 1, 1, "none"): (3, 16, 1, 21761),
          ("f32", "tiled", 2, 1, 0, 1, "none"): (3, 16, 11008, 64), ("f32", "tiled", 2, 1, 1, 1, "none"): (3, 16, 10881, 1)}


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


def _f32_plan(L, b, M, K, N, lay="al", olay="al", acc=0, db=0, sf=None):
    ldx, ldz, ldo = (K + 3) // 4 * 4 + 4, (N + 3) // 4 * 4 + 4, (N + 3) // 4 * 4 + 8
    if lay == "oddld":
        ldx, ldz = ldx + 1, ldz + 3
    if olay == "oddld":
        ldo += 1
    so = (K + 4) * ldo + (5 if olay == "sodd" else 4)
    need = L.lib().dispu_linear_tn_scratch_floats(b, M, K, N) if sf is None else sf
    return L.linear_tn_plan(b, M, K, N, A + (4 if lay == "offx" else 0), ldx, (M + 1) * ldx, A + (4 if lay == "offz" else 0), ldz,
                            (M + 1) * ldz, A + (12 if olay == "off" else 0), ldo, so, acc, A if db else None, A, need), need


@pytest.fixture(scope="module")
def census(L):
    """{instantiation: smallest (batch, M, K, N) seen} per family, and the plan-consistency checks on every swept shape"""
    f32, bf, stream = {}, {}, {}
    lib = L.lib()

    def note(d, key, shape):
        size = shape[0] * (shape[1] * (shape[2] + shape[3]) + shape[2] * shape[3])
        if key not in d or d[key][0] > size:
            d[key] = (size,) + shape

    def one_f32(b, M, K, N, **kw):
        p, need = _f32_plan(L, b, M, K, N, **kw)
        assert p.rc == 0 and p.kind in ("narrow", "tiled"), (b, M, K, N, kw, p)
        # every row belongs to exactly one split, the last one is not empty, and the scratch the entry asks for holds the partials
        assert p.splits * p.rows >= M > (p.splits - 1) * p.rows, (b, M, K, N, p)
        assert p.direct or b * p.splits * (K + 1) * N <= need, (b, M, K, N, p, need)
        assert p.direct == (p.reduce == "none") and (p.kind == "tiled" or not p.direct)
        note(f32, ("f32", p.kind, p.TK, p.TNN, p.edge, p.direct, p.reduce), (b, M, K, N))

    for b, M, K, N in itertools.product((1, 2, 3), M_DENSE, KN, KN):
        one_f32(b, M, K, N, acc=0, db=0)
        nb = lib.dispu_linear_tn_bf16_scratch_floats(b, M, K, N)
        q = L.linear_tn_bf16_plan(b, M, K, N, A, K, M * K, A, N, M * N, A, N, K * N, 0, A if b == 1 else None, A, nb)
        assert q.rc == 0 and q.kind == "tiled" and q.rows % 64 == 0, (b, M, K, N, q)
        assert q.splits * q.rows >= M > (q.splits - 1) * q.rows, (b, M, K, N, q)
        assert q.reduce == (q.splits > 1) and (not q.reduce or b * q.splits * (K + 1) * N <= nb), (b, M, K, N, q, nb)
        note(bf, (q.tile, q.reduce), (b, M, K, N))
    for b, M, K, N in itertools.product((1, 2, 3), M_THIN, KN_THIN, KN_THIN):
        for lay, olay, acc, db in itertools.product(("al", "oddld", "offx", "offz"), ("al", "oddld", "off", "sodd"), (0, 1), (0, 1)):
            one_f32(b, M, K, N, lay=lay, olay=olay, acc=acc, db=db)
    for M, K, N, st in itertools.product(sorted(set(M_DENSE + [32 * i for i in range(1, 140)])), (128, 256, 384, 2048), (128, 256, 384, 512, 2048),
                                         (0, 3)):
        need = lib.dispu_linear_tn_bf16_stream_scratch_floats(M, K, N)
        p = L.linear_tn_bf16_stream_plan(M, K, N, A, K, A, N, st, A, N, 0, A, A, need)
        if M % 32:
            assert need == 0 and p.rc != 0
            continue
        assert p.rc == 0 and p.splits * p.rows == M and p.rows % 32 == 0 and (p.splits == 1 or p.rows >= 128), (M, K, N, p)
        assert p.splits * (K + 1) * N == need
        note(stream, (p.BN, p.storage), (1, M, K, N))
    return f32, bf, stream


def test_census_of_reachable_instantiations(L, census):
    f32, bf, stream = census
    tiles = [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4)]
    every = {("f32", "narrow", 0, 0, 0, 0, r) for r in ("scalar", "vec4")} | {
        ("f32", "tiled", tk, tnn, e, int(r == "none"), r) for tk, tnn in tiles for e in (0, 1) for r in ("none", "scalar", "vec4")}
    assert set(f32) == every - F32_UNREACHABLE, (sorted(set(f32) ^ (every - F32_UNREACHABLE)))
    assert len(f32) == 34
    assert set(bf) == {(t, r) for t in (128032, 64064, 128128) for r in (0, 1)}
    assert bf[(128128, 1)][1:] == (1, 130817, 1, 33) and bf[(128128, 0)][1:] == (2, 1, 2047, 2047)
    assert set(stream) == {(256, 0), (256, 3), (128, 0), (128, 3)}
    print("census: fp32 %d instantiations (4 more named by the dispatch, unreachable for K, N <= 2048), bf16 %d x 4 storage masks, stream %d"
          % (len(f32), len(bf), len(stream)))
    # the four the sweep cannot reach exist beyond its bounds
    for key, (b, M, K, N) in BEYOND.items():
        p, _ = _f32_plan(L, b, M, K, N)
        assert ("f32", p.kind, p.TK, p.TNN, p.edge, p.direct, p.reduce) == key, (key, p)


def test_every_reachable_instantiation_has_a_case(L, census):
    f32, bf, stream = census
    have = {TP.instantiation(c, TP.case_plan(c)) for c in TP.CASES if c.M > 0}
    want = set(f32) | {("bf16", t, r, st) for t, r in bf for st in (0, 1, 2, 3)} | {("stream",) + k for k in stream}
    assert want <= have, sorted(want - have)
    assert have <= want, sorted(have - want)
    # one float-data case per instantiation of the product kernels
    flt = {k[:5] if k[0] == "f32" else k for k in (TP.instantiation(c, TP.case_plan(c)) for c in TP.CASES if c.flt)}
    assert {k[:5] if k[0] == "f32" else k for k in want} <= flt


@pytest.mark.parametrize("group", TP.GROUPS)
def test_cases_take_the_path_their_group_names(L, group):
    for c in (c for c in TP.CASES if c.group == group):
        p = TP.case_plan(c)
        assert p.rc == 0, (c, p)
        for k, v in list(TP.group_path(c).items()) + list(c.want):
            assert getattr(p, k) == v, (c, k, v, p)
        if c.scratch == "null" and c.M > 0:
            assert (p.direct if c.fam == "f32" else not p.reduce), (c, p)
        lo = TP.layout(c)
        assert lo.ldx > c.K and lo.ldz > c.N and lo.ldo >= c.N + 6 and (c.batch == 1 or lo.so > (c.K + 2 * TP.GUARD - 1) * lo.ldo)


def test_cases_cover_the_named_edges(L):
    """what the issue lists by name, read off the plans of the table"""
    P = {c: TP.case_plan(c) for c in TP.CASES}
    f32 = {c: p for c, p in P.items() if c.fam == "f32"}
    tiled = {c: p for c, p in f32.items() if p.kind == "tiled"}
    assert {2, 7, 8, 9, 63, 64, 65, 130} <= {p.splits for p in tiled.values()}
    assert {2, 7, 8, 9, 63, 64, 65, 130} <= {p.splits for p in tiled.values() if p.reduce == "vec4"} | {
        p.splits for p in tiled.values() if p.reduce == "scalar"}
    assert any(p.splits > 1 and c.M % p.rows for c, p in tiled.items())                          # a last split shorter than the others
    assert {1, 2, 3} <= {(min(c.M, p.rows) + 15) // 16 for c, p in tiled.items()}                # nslab 1, 2, 3
    assert any(c.bias and c.K > 64 * p.TK for c, p in tiled.items())                             # bias with more than one K-tile
    assert any(c.batch == 3 and c.bias for c in tiled) and any(p.capped for p in f32.values() if p.reduce == "vec4")
    assert any(p.capped for p in f32.values() if p.reduce == "scalar")
    narrow = {c: p for c, p in f32.items() if p.kind == "narrow"}
    assert {128, 4096} <= {p.rows for p in narrow.values()} and any(p.splits > 64 for p in narrow.values())
    assert any(p.wpb < 16 for p in narrow.values()) and any(p.grid_y == 5 and p.wpb == 16 for p in narrow.values())
    assert any(c.M - (p.splits - 1) * p.rows == 4 for c, p in narrow.items())
    st = {c: p for c, p in P.items() if c.fam == "stream"}
    assert {1, 2, 256} <= {p.splits for p in st.values()}


def test_narrow_falls_back_past_2_29_elements(L):
    """M * ld >= 2^29 (the narrow kernel's 32-bit byte offsets) keeps a narrow shape on the tiled kernel: more than 2 GB of operands, so
    asserted from the plan only"""
    M, K, N = 4096 * 1024, 24, 16
    need = L.lib().dispu_linear_tn_scratch_floats(1, M, K, N)
    args = lambda ldx, ldz: (1, M, K, N, A, ldx, 0, A, ldz, 0, A, N, K * N, 0, A, A, need)
    assert L.linear_tn_plan(*args(127, 127)).kind == "narrow"
    assert L.linear_tn_plan(*args(128, 16)).kind == "tiled" and L.linear_tn_plan(*args(24, 128)).kind == "tiled"


def test_refusals_and_no_ops_of_the_plans(L):
    """the plans answer as the entries do (tests/test_tn_paths_gpu.py holds the entries to the same table)"""
    for (fam, args), rc_zero, kind in TP.refusals():
        p = {"f32": L.linear_tn_plan, "bf16": L.linear_tn_bf16_plan, "stream": L.linear_tn_bf16_stream_plan}[fam](*args)
        assert (p.rc == 0) == rc_zero, (fam, args, p)
        if fam != "stream":
            assert p.kind == kind, (fam, args, p)


# dispu_linear_tn_scratch_floats / _bf16_scratch_floats (batch, M, K, N) and _bf16_stream_scratch_floats (M, K, N) as the parent of the plan
# export returned them (the whole census grid was compared against that build; these are a sample of it)
SCRATCH_PINS = [((1, 1, 1, 1), 2, 0), ((1, 300, 37, 50), 3800, 3800), ((1, 4096, 96, 24), 74496, 37248), ((1, 4096, 256, 64), 361856, 263168),
                ((1, 8192, 256, 256), 2105344, 2105344), ((1, 8192, 2048, 256), 16785408, 4196352), ((1, 131072, 120, 24), 1486848, 1486848),
                ((2, 2000, 2048, 64), 2098176, 2098176), ((3, 257, 1025, 1025), 6309900, 6309900), ((1, 131072, 17, 100), 921600, 921600),
                ((1, 33279, 20, 9), 24570, 24570), ((2, 1, 2047, 2047), 8384512, 0)]
STREAM_PINS = [((256, 128, 256), 66048), ((32768, 128, 256), 8454144), ((8192, 2048, 256), 8392704), ((4128, 128, 512), 66048),
               ((250, 128, 256), 0), ((256, 130, 256), 0)]


def test_scratch_sizes_are_what_they_were(L):
    lib = L.lib()
    for shape, f32, bf in SCRATCH_PINS:
        assert (lib.dispu_linear_tn_scratch_floats(*shape), lib.dispu_linear_tn_bf16_scratch_floats(*shape)) == (f32, bf), shape
    for shape, n in STREAM_PINS:
        assert lib.dispu_linear_tn_bf16_stream_scratch_floats(*shape) == n, shape


def test_integer_references_agree(L):
    """the float64 product that stands in for the int64 einsum on the big cases gives the same integers, and every case's integer
    reference stays below 2^24 (asserted inside expected_int)"""
    for c in TP.CASES:
        size = c.batch * c.M * c.K * c.N
        if 2 ** 20 < size <= 2 ** 24:
            X, Z, _, _ = TP.operands(c, "int")
            f = np.matmul(X.astype(np.float64).transpose(0, 2, 1), Z.astype(np.float64))
            assert np.array_equal(TP.int_product(X, Z), f.astype(np.int64)), c
    small = [c for c in TP.CASES if c.batch * c.M * (c.K + c.N) <= 2 ** 21]
    for c in small:
        out, db = TP.expected_int(c, TP.operands(c, "int"))
        assert out.shape == (c.batch, c.K, c.N) and (db is None) == (not c.bias)
