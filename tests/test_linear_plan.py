"""CPU tests of the dense-layer dispatch through dispu_linear_plan / dispu_linear_bf16_plan (no GPU: the plan entries make no HIP call
and dereference nothing).  The launchers run off the same decision function, so what the plan says is what a call launches:

  * the plan's tile is dispu_linear_tile2's, and dispu_debug_linear_tile forces it;
  * census: a brute-force sweep over shapes, layouts, attachments and the tile override collects every (kernel, tile, BK, transb, edge,
    epilogue | unroll depth) the dispatch can reach -- 89: 5 tiles x 4 load paths x EPI {0, 1, 4, 5}, the EPI 6 twin, and the skinny
    kernel's 4 depths x transb -- and the case table of the GPU matrix (tests/linear_paths.py) must cover them all, each case on the
    path its group names;
  * no plan is a tiled, interior, untransposed launch at BK 32: the branch of launch_linear that instantiated those kernels was dead
    (K % 32 == 0 implies K % 16 == 0, the DMA pipeline) and is gone;
  * the profile names generator.py:_linear now builds from the plan are, for every product of a Generator forward at the A/B sizes of
    tests/test_generator_gpu.py, the names its hand-written copy of the dispatch produced (kept here as the fixture of record).
"""
import itertools

import pytest

import linear_paths as LP


@pytest.fixture(scope="module")
def lib():
    from dispu_amd import _lib
    L = _lib.lib()
    L.dispu_debug_linear_tile(0)
    yield _lib
    L.dispu_debug_linear_tile(0)


@pytest.fixture()
def force_tile(lib):
    yield lib.lib().dispu_debug_linear_tile
    lib.lib().dispu_debug_linear_tile(0)


A = 0x10000000          # made-up addresses: only NULL-ness and alignment are looked at


def simple_plan(lib, batch, M, K, N, transb, r2=True):
    """aligned, contiguous operands; R2 attached by default so that the product stays on the tiled kernel"""
    wc = K if transb else N
    return lib.linear_plan(batch, M, K, N, A, K, M * K, 2 * A, wc, K * N, transb, None, None, None, 0, 3 * A, N, M * N, None, 0, 0,
                           4 * A if r2 else None, N, M * N, None, 0, 0)


def test_plan_tile_is_tile2(lib):
    L = lib.lib()
    for batch, M, K, N, tb in itertools.product((1, 3, 64), (1, 64, 100, 128, 1000, 8192, 32768, 131072), (8, 16, 24, 32, 134, 480, 2048),
                                                (33, 64, 65, 100, 128, 134, 192, 256, 320, 512), (0, 1)):
        plan = simple_plan(lib, batch, M, K, N, tb)
        assert len(plan) == 1 and plan[0][0] == "tiled", (batch, M, K, N, tb, plan)
        code = L.dispu_linear_tile2(batch, M, K, N, tb)
        assert (plan[0][3], plan[0][4]) == LP.TILES[code][:2], (batch, M, K, N, tb, plan, code)
        assert (plan[0][1], plan[0][2]) == (0, N)


def test_tile_override(lib, force_tile):
    L = lib.lib()
    rule = simple_plan(lib, 1, 8192, 256, 256, 0)
    assert (rule[0][3], rule[0][4]) == (64, 128)
    for code, (bm, bn, bkr) in LP.TILES.items():
        force_tile(code)
        assert L.dispu_linear_tile2(1, 8192, 256, 256, 0) == code
        p = simple_plan(lib, 1, 8192, 256, 256, 0)
        assert p == [("tiled", 0, 256, bm, bn, 16, 0, 0, 4)], (code, p)
        p = simple_plan(lib, 1, 8192, 256, 256, 1)
        assert p == [("tiled", 0, 256, bm, bn, bkr, 1, 0, 4)], (code, p)
    force_tile(0)
    assert simple_plan(lib, 1, 8192, 256, 256, 0) == rule


def test_plan_refuses_what_the_entries_refuse(lib):
    L = lib.lib()
    buf = (lib.C.c_int * lib.LINEAR_PLAN_INTS)()
    ok = lambda *a: L.dispu_linear_plan(*a, buf)
    base = [1, 64, 64, 64, A, 64, 0, A, 64, 0, 0, None, None, None, 0, A, 64, 0, None, 0, 0, None, 0, 0, None, 0, 0]
    assert ok(*base) == 0 and buf[0] == 1
    for i, v in ((2, 0), (3, 0), (4, None), (7, None), (15, None), (14, 2), (12, A)):      # K, N, X, W, Y, act, scale without shift
        bad = list(base)
        bad[i] = v
        assert ok(*bad) != 0 and buf[0] == 0, i
    masked_batch = list(base)
    masked_batch[0], masked_batch[24], masked_batch[26] = 3, A, 64                          # dispu_linear_masked: a mask needs batch 1
    assert ok(*masked_batch) != 0
    empty = list(base)
    empty[1] = 0
    assert ok(*empty) == 0 and buf[0] == 0


def sweep(lib, force_tile):
    """every plan of a brute-force sweep over what the three entries accept"""
    seen = {}
    ptrs = dict(al=(0, 0, 0), oddld=(1, 0, 0), off=(0, 4, 0), yoff=(0, 0, 4))           # (ld increment, X/W byte offset, Y byte offset)
    Ms, Ns = (64, 100, 128), (16, 64, 100, 128, 160, 256)
    Ks = (16, 24, 32, 33, 48, 132, 260, 400, 1024)
    attach = [("linear", b, r1, r2, None) for b in (0, 1) for r1 in (0, 1) for r2 in (0, 1)]
    attach += [("bn", b, r1, r2, None) for b in (0, 1) for r1 in (0, 1) for r2 in (0, 1)]
    attach += [("masked", b, r1, 0, mc) for b in (0, 1) for r1 in (0, 1) for mc in (-5, 0, 7)]      # mcols below, at, above N
    for tile in (0,) + tuple(LP.TILES):
        force_tile(tile)
        for batch, M, N, K, tb, (lay, (dl, dxw, dy)) in itertools.product((1, 3), Ms, Ns, Ks, (0, 1), ptrs.items()):
            wc = K if tb else N
            ldx, ldw, ldy = (K + 3) // 4 * 4 + dl, (wc + 3) // 4 * 4 + dl, (N + 3) // 4 * 4 + dl
            for entry, b, r1, r2, mc in attach:
                if entry == "masked" and batch != 1:
                    continue
                plan = lib.linear_plan(batch, M, K, N, A + dxw, ldx, M * ldx, 2 * A + dxw, ldw, 4 * ((K * N + 3) // 4) + 4 * dl, tb,
                                       5 * A if b else None, 6 * A if entry == "bn" else None, 7 * A if entry == "bn" else None, 0,
                                       3 * A + dy, ldy, M * ldy, 4 * A if r1 else None, ldy, M * ldy, 8 * A if r2 else None, ldy, M * ldy,
                                       9 * A if mc is not None else None, ldy, N + mc if mc is not None else 0)
                assert 1 <= len(plan) <= 2
                for l in plan:
                    seen.setdefault(LP.plan_code(l), (tile, batch, M, K, N, tb, lay, entry, b, r1, r2, mc))
    force_tile(0)
    return seen


@pytest.fixture(scope="module")
def reachable(lib):
    tile = lib.lib().dispu_debug_linear_tile
    try:
        return sweep(lib, tile)
    finally:
        tile(0)


def table_plans(lib, force_tile):
    out = []
    for c in LP.CASES:
        force_tile(c.tile)
        out.append((c, lib.linear_plan(*LP.plan_args(c))))
    force_tile(0)
    return out


def test_census_reachable_set(reachable):
    """5 tiles x {DMA interior, transposed interior, edge, edge transposed} x EPI {0, 1, 4, 5}, the long-K EPI 6 twin, and the
    skinny kernel in 4 depths x transb: 89 instantiations, and nothing else."""
    want = set()
    for bm, bn, bkr in LP.TILES.values():
        for bk, tb, edge in ((16, 0, 0), (bkr, 1, 0), (bkr, 0, 1), (bkr, 1, 1)):
            want |= {("tiled", bm, bn, bk, tb, edge, epi) for epi in (0, 1, 4, 5)}
    want.add(("tiled", 128, 256, 16, 0, 0, 6))
    want |= {("skinny", ng, tb) for ng, tb in LP.SKINNY}
    got = set(reachable)
    assert got == want, (sorted(got - want), sorted(want - got))
    assert len(got) == 89


def test_no_interior_untransposed_bk32(reachable):
    """the dead branch of launch_linear: tiled, interior, untransposed, BK 32 -- no plan, so no kernel"""
    assert not [k for k in reachable if k[0] == "tiled" and k[4] == 0 and k[5] == 0 and k[3] != 16]


def test_case_table_covers_every_reachable_instantiation(lib, force_tile, reachable):
    covered = set()
    for c, plan in table_plans(lib, force_tile):
        covered |= {LP.plan_code(l) for l in plan}
    missing = sorted(set(reachable) - covered)
    assert not missing, "reachable kernel instantiations without a GPU case in tests/linear_paths.py (code: first sweep point that reached " \
                        "it):\n" + "\n".join("%s: %s" % (k, reachable[k]) for k in missing)
    assert covered <= set(reachable), sorted(covered - set(reachable))


def test_case_table_takes_the_paths_it_names(lib, force_tile):
    for c, plan in table_plans(lib, force_tile):
        want = LP.expected_launch(c)
        if want is None:
            continue
        assert len(plan) == 1, (c, plan)
        l = plan[0]
        got = ("skinny", l[3], l[4]) if l[0] == "skinny" else l[:1] + l[3:8]
        assert got == want and (l[1], l[2]) == (0, c.N), (c, plan)


def test_bf16_plan(lib):
    P = lib.lib().dispu_linear_bf16_plan
    assert P(1, 1000, 32, 1) == 128032 and P(8, 131072, 24, 1) == 128032
    assert P(1, 1000, 33, 1) == 64064
    assert P(1, 4096, 2048, 1) == 128128                    # 32 x 16 = 512 tiles of 128 x 128
    assert P(1, 4096, 1920, 1) == 64064                     # 32 x 15
    assert P(8, 1000, 1000, 1) == 128128 and P(7, 1000, 1000, 1) == 64064
    assert P(1, 256, 256, 128) == 128128 and P(1, 256, 256, 127) == 64064
    assert P(0, 10, 10, 1) == 0 and P(1, 0, 10, 1) == 0


# ---- profile names ------------------------------------------------------------------------------------------------------------------
def old_profile_name(batch, M, K, N, X, ldx, sx, W, ldw, sw, transb, bias, Y, ldy, sy, R1, ldr1, R2, ldr2, tile2):
    """generator.py:_linear's hand-written copy of the dispatch as it stood before the plan query (addresses instead of tensors): the
    fixture of record for the profile row names that profiles/ and EXPERIMENTS.md quote."""
    t = tile2(batch, M, K, N, int(bool(transb)))
    bm, bn = {128257: (128, 256), 128128: (128, 128), 64128: (64, 128), 128064: (128, 64)}.get(t, (64, 64))
    al = lambda q: q is None or q % 16 == 0
    ok = (M % bm == 0 and N % bn == 0 and ldx % 4 == 0 and ldw % 4 == 0 and sx % 4 == 0 and sw % 4 == 0 and al(X) and al(W)
          and ldy % 4 == 0 and sy % 4 == 0 and al(Y) and al(bias) and (R1 is None or (ldr1 % 4 == 0 and al(R1)))
          and (R2 is None or (ldr2 % 4 == 0 and al(R2))))
    bkr = 16 if t == 128257 else 32
    if ok and not transb and K % 16 == 0:
        bk, edge = 16, False
    elif ok and K % bkr == 0:
        bk, edge = bkr, False
    else:
        bk, edge = bkr, True
    epi = 0 if (R1 is None and R2 is None) else 4
    if epi == 0 and (bm, bn, bk) == (128, 256, 16) and not transb and not edge and K >= 1024:
        epi = 6
    name = "linear<%d, %d, 2, 2, %d, %s, %s, %d>[%dx%dx%d]" % (bm, bn, bk, "true" if transb else "false", "true" if edge else "false", epi,
                                                              M * batch, K, N)
    tiles64 = ((M + 63) // 64) * ((N + 63) // 64)
    if (batch == 1 and R2 is None and 4 <= K <= 384 and K % 4 == 0 and ldx % 4 == 0 and X % 16 == 0
            and not (transb and (ldw % 4 or W % 16))
            and ((N <= 64 and tiles64 < 256) or N <= 32 or (K <= 32 and N <= 128))):
        name = "linear_skinny<%d, %s>[%dx%dx%d]" % (2 if K <= 32 else 8 if K <= 128 else 16 if K <= 256 else 24,
                                                   "true" if transb else "false", M, K, N)
    return name


def generator_products(B, n):
    """every dispu_linear call Generator.forward can make at B patches of n points, under all of its switches (generator.py:_linear call
    sites), as dict(M, K, N, ...) with element offsets into 16-byte aligned buffers"""
    rn, rm, M = B * n, 4 * B * n, 4 * n
    P = lambda M_, K, N, ldx=None, ldw=None, ldy=None, bias=0, **kw: dict(dict(
        M=M_, K=K, N=N, ldx=K if ldx is None else ldx, ldw=N if ldw is None else ldw, ldy=N if ldy is None else ldy, bias=bias, batch=1, sx=0,
        sw=0, sy=0, transb=0, res=0, xoff=0, woff=0, yoff=0), **kw)
    out = [P(rn, 480 - col, 48, ldx=480, xoff=col) for col in (360, 240, 120)]                     # layer<d>_prep
    out += [P(rn, 480, 256, bias=None), P(rm, 256, 128), P(rm, 128, 256), P(rm, 256, 64)]          # duplicate_up, coarse regressor
    out += [P(rm, 128, 256, ldw=320, ldy=320), P(rm, 128, 64, ldw=320, ldy=320, bias=256, woff=256, yoff=256),
            P(rm, 128, 320, ldw=320, ldy=320)]                                                       # K|V, Q, conv0's feature part
    out += [P(M, 64, M, ldx=320, ldw=320, ldy=M, bias=None, batch=B, sx=M * 320, sw=M * 320, sy=M * M, transb=1, xoff=128),   # Q.K^T
            P(M, M, 64, ldx=M, ldw=320, ldy=64, bias=None, batch=B, sx=M * M, sw=M * 320, sy=M * 64, woff=64)]                  # att.V
    out += [P(rm, 64, 256), P(rm, 144, 256), P(rm * 16, 128, 128)]                                  # back-projection, skip, conv1 per pair
    out += [P(rm, 2048, 256), P(rm, 2048, 256, res=3)]                                              # after_conv alone / + skip + nl
    out += [P(rm, 256, 256), P(rm, 256, 64)]                                                        # aggregation, fine regressor
    return out


AB_SIZES = [(2, 256), (1, 1024), (1, 288), (2, 250)]       # tests/test_generator_gpu.py


@pytest.mark.parametrize("B,n", AB_SIZES)
def test_profile_names_are_the_old_ones(lib, B, n):
    from dispu_amd.generator import linear_profile_name
    L = lib.lib()
    X0, W0, Y0, B0, R10, R20 = (i * A for i in range(1, 7))
    for q in generator_products(B, n):
        X, W, Y = X0 + 4 * q["xoff"], W0 + 4 * q["woff"], Y0 + 4 * q["yoff"]
        bias = None if q["bias"] is None else B0 + 4 * q["bias"]
        R1, R2 = (R10 if q["res"] & 1 else None), (R20 if q["res"] & 2 else None)
        old = old_profile_name(q["batch"], q["M"], q["K"], q["N"], X, q["ldx"], q["sx"], W, q["ldw"], q["sw"], q["transb"], bias, Y, q["ldy"],
                               q["sy"], R1, 256, R2, 256, L.dispu_linear_tile2)
        plan = lib.linear_plan(q["batch"], q["M"], q["K"], q["N"], X, q["ldx"], q["sx"], W, q["ldw"], q["sw"], q["transb"], bias, None, None, 1,
                               Y, q["ldy"], q["sy"], R1, 256 if R1 else 0, 0, R2, 256 if R2 else 0, 0, None, 0, 0)
        assert linear_profile_name(plan, q["batch"], q["M"], q["K"], q["N"]) == old, (q, plan)
