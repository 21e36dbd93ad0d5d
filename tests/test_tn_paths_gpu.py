"""Every weight-gradient (TN) kernel the split plans can pick, alone, through the C ABI: dispu_linear_tn (csrc/train_gemm.hip),
dispu_linear_tn_bf16s (csrc/linear_bf16.hip), dispu_linear_tn_bf16_stream (csrc/linear_bf16_stream.hip) and the grouped reduction
dispu_tn_reduce_grouped.  The case table is tests/tn_paths.py; tests/test_tn_plan.py proves on the CPU that it covers every instantiation
the dispatches can reach and that every case takes the path its group names.  Here each case's plan is asked again with the real device
pointers and must be the one the CPU saw.

Every case runs on small-integer data and is compared with array_equal against the integer reference (out and dbias): a wrong row
range, tile offset, split boundary, bias tile or reduce stride fails outright.  `out` sits in a wider buffer of sentinels (guard rows,
>= 3 columns each side, ldo > N, so > K ldo), dbias and the exactly-sized scratch between sentinel guards, all compared bitwise after
the call; operand padding and the row past M are NaN.  One case per instantiation also runs standard-normal data against a float64
product under the project's existing bounds (tn_paths.expected_flt), batch-1 ones twice into fresh buffers for bit-equal results.

kernel x path -> host branch (tn_decide / tn_bf16_decide / tn_stream_decide) -> group of the table
  linear_tn_kernel<TK,TNN,EDGE>      kind tiled, edge 0 / 1             f32/T11 T12 T14 T21 T22 T24 / int, edge
    direct store (dst = out, ldd = ldo)   splits == 1, !accumulate, !dbias    the scratch="null" cases of each T group (none for T14, T21)
    bias row (K-tile 0 only)              dbias                               f32/T11/edge M=300 K=130; batch 3: T11/int M=304, T22/edge, T24/edge
  linear_tn_narrow_kernel            kind narrow                        f32/narrow (K x N grid, wpb 2 and 16 x grid.y 5, rows 128 / 4096,
                                                                        4-row last chunk, 65 chunks); f32/fallback for what keeps off it
  tn_reduce4_kernel / tn_reduce_kernel    reduce vec4 / scalar          by N % 4, ldo % 4, so % 4, alignment of out: olay al / oddld / off / sodd;
                                                                        splits 2, 7, 8, 9, 63, 64, 65, 130: f32/T11; capped grids: f32/reduce
  hipMemset2DAsync                   kind clear (M == 0)                f32/clear, bf16/clear
  gemm_bf16_kernel<128,32 / 64,64 / 128,128, false, false>   tile, reduce 0 / 1    bf16/<tile>/single, split x storage 0 - 3
  gemm_bf16_reduce_kernel            reduce 1                           bf16/*/split
  gemm_bf16_tn_stream_kernel<BN,ST>, tn_stream_reduce_kernel            stream/<BN>/<storage>: splits 1, 2, 64, 256, the plan's fall to fewer
  tn_reduce_grouped_kernel           dispu_tn_reduce_grouped            test_grouped_reduction_*

[measured on the MI355X] worst error / bound over the float-data cases (one per instantiation; every bound is the existing one):
  fp32 out   0.058 of 2e-5 max|ref| (narrow kernel, 131072 x 256 x 64); 0.046 of 1e-5 max|ref| at M <= 2000 (<2,2> interior, 304 rows)
  fp32 dbias 0.056 of 2e-5 max|ref| (the same narrow case)
  bf16 out   0.047 of 4e-6 |x|^T |z| + 1e-6 (1 + |ref|);   bf16 dbias   0.018 of 2e-6 max colsum|z| + 1e-6
  stream out 0.024 of the same elementwise bound;           stream dbias 0.022
and out / dbias of every float-data case equal the host replay of the documented association over the partial tiles bit for bit.

Mutations tried on a scratch build of csrc/train_gemm.hip (arithmetic only, every access stays inside its buffer; nothing mutated is
committed) and what fails under each:
  last slab of a split skipped (nslab - 1)          test_tn_path[f32/T11 .. T24 / int and edge, f32/fallback, f32/reduce/scalar, vec4],
                                                    test_grouped_reduction_table[int]: 16 tests
  m_begin one slab early for split > 0              the same 16 (first failing case of T11: M=300 / M=544, the multi-split ones)
  ldo replaced by N in the direct store             test_tn_path[T11, T12, T22, T24 / int and edge] ("wrote outside its output window"),
                                                    test_direct_store_equals_split_and_reduce: 9 tests
  reduce group order reversed (g = 7 .. 0)          test_tn_path[f32/T11/int, T14/int and edge, T21/int and edge, narrow/kn, narrow/rows]
                                                    through check_association (the float-data cases of more than two splits: two
                                                    non-empty groups add to the same bits either way), test_grouped_reduction_table[flt];
                                                    the integer runs cannot see it (the sums are exact in any order)
  narrow kernel: bias tile's 1 in row 1, not 0      test_tn_path[f32/narrow/kn, f32/narrow/rows], test_grouped_reduction_table[int]
  bias row taken from K-tile 1                      nothing, and nothing can: every K-tile of an N-tile stages the same Z slab, so its
                                                    column sums are the same numbers whichever K-tile writes them (an equivalent mutant)
  narrow amask dropped                              nothing, and nothing can: amask zeroes the rows k >= K of the 16-row tile, which the
                                                    store's `k < K` guard never writes, and the loads behind them are clamped to column K - 1
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tn_paths as TP

pytestmark = pytest.mark.gpu

SENT_BITS = np.float32(TP.SENTINEL).view(np.uint32)
WORST = {}                                                       # bound name -> worst measured error / bound


def _entry(L, c):
    return {"f32": L.dispu_linear_tn, "bf16": L.dispu_linear_tn_bf16s, "stream": L.dispu_linear_tn_bf16_stream}[c.fam]


_PTR_SLOTS = {17: (4, 7, 10, 14, 15), 18: (4, 7, 10, 14, 15), 14: (3, 5, 8, 11, 12)}      # pointer arguments by arity (f32, bf16, stream)


def upload(dev, c, ops):
    host = TP.host_buffers(c, ops)
    t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    if c.storage & 1:
        t["x"] = t["x"].bfloat16()
    if c.storage & 2:
        t["z"] = t["z"].bfloat16()
    base = {k: v.data_ptr() for k, v in t.items()}
    assert all(p % 16 == 0 for p in base.values())
    return host, t, base


def launch(dev, _lib, c, t, base, desc=None, scratch_buf=None):
    """scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .floats) in place of the case's sentinel-filled one"""
    L = _lib.lib()
    if scratch_buf is not None:
        assert c.scratch == "exact" and scratch_buf.floats >= TP.scratch_floats(c) and scratch_buf.ptr().value % 16 == 0
        base = dict(base, s=scratch_buf.ptr().value)
    args = TP.entry_args(c, base)
    p = TP.plan(c, base)
    assert p == TP.case_plan(c), (c, p, TP.case_plan(c))           # the plan the CPU census saw
    if desc is not None:
        _lib.check(L.dispu_tn_defer(desc), "dispu_tn_defer")
    ptr = _PTR_SLOTS[len(args)]
    rc = _entry(L, c)(*[C.c_void_p(a) if i in ptr else a for i, a in enumerate(args)], _lib.stream_ptr(dev))
    _lib.check(rc, "%r" % (c,))
    return p


def collect(c, host, t):
    """(out window [batch, K, N], dbias [N] or None) after checking bitwise that nothing else was written"""
    lo = TP.layout(c)
    win, rest = TP.out_window(c, t["o"].cpu().numpy())
    bad = rest.view(np.uint32) != SENT_BITS
    assert not bad.any(), "%r wrote outside its output window: %d elements, first at flat index %d" % (c, int(bad.sum()), int(np.argmax(bad)))
    b = t["b"].cpu().numpy().copy()
    db = b[lo.boff:lo.boff + c.N].copy() if c.bias else None
    if c.bias:
        b[lo.boff:lo.boff + c.N] = TP.SENTINEL
        assert (b.view(np.uint32) == SENT_BITS).all(), "%r wrote round its dbias" % (c,)
    else:
        assert np.array_equal(b.view(np.uint32), host["b"].view(np.uint32)), "%r touched a dbias it was not given" % (c,)
    tail = t["s"][TP.scratch_floats(c):].cpu().numpy()
    assert (tail.view(np.uint32) == SENT_BITS).all(), "%r wrote past the scratch *_scratch_floats sized" % (c,)
    return win, db


def run_case(dev, _lib, c, kind):
    ops = TP.operands(c, kind)
    host, t, base = upload(dev, c, ops)
    p = launch(dev, _lib, c, t, base)
    torch.cuda.synchronize()
    win, db = collect(c, host, t)
    return ops, win, db, p, t


def check_int(dev, _lib, c):
    ops, win, db, p, _ = run_case(dev, _lib, c, "int")
    want, wdb = TP.expected_int(c, ops)
    bad = win.astype(np.float64) != want
    assert not bad.any(), "%r (plan %r): %d of %d outputs differ from the integer reference, first at %r: %r != %r" % (
        c, p, int(bad.sum()), win.size, tuple(np.argwhere(bad)[0]), win[bad][0], want[bad][0])
    if c.bias:
        assert np.array_equal(db.astype(np.float64), wdb), "%r (plan %r): dbias differs at %r" % (c, p, np.argwhere(db != wdb)[:4].tolist())
    return win


def _worst(name, err, bound):
    f = float((err / bound).max()) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), f)
    return f


def check_flt(dev, _lib, c):
    ops, win, db, p, t = run_case(dev, _lib, c, "flt")
    ref, ob, rdb, dbb = TP.expected_flt(c, ops)
    name = {"f32": "fp32 out (1e-5 / 2e-5 of max|ref|)", "bf16": "bf16 out (elementwise)", "stream": "stream out (elementwise)"}[c.fam]
    f = _worst(name, np.abs(win - ref), ob)
    fb = 0.0
    if c.bias:
        fb = _worst({"f32": "fp32 dbias (2e-5)", "bf16": "bf16 dbias", "stream": "stream dbias"}[c.fam], np.abs(db - rdb), dbb)
    print("[measured] %s batch %d %d x %d x %d: out %.3f of its bound, dbias %.3f" % (c.group, c.batch, c.M, c.K, c.N, f, fb))
    assert f <= 1.0, "%r (plan %r): out off by %.3g x its bound" % (c, p, f)
    assert fb <= 1.0, "%r (plan %r): dbias off by %.3g x its bound" % (c, p, fb)
    check_association(c, p, ops, win, db, t)
    if c.batch == 1:                                              # deterministic: the same bits into fresh buffers
        _, t2, base2 = upload(dev, c, ops)
        launch(dev, _lib, c, t2, base2)
        torch.cuda.synchronize()
        assert torch.equal(t["o"], t2["o"]) and torch.equal(t["b"], t2["b"]), "%r: two runs differ" % (c,)


def check_association(c, p, ops, win, db, t):
    """the reduction after a split product adds the partial tiles it left in the scratch in the documented association (`replay`):
    out and dbias are that sum bit for bit (dbias of a batched fp32 product goes through float atomics: skipped)"""
    if not p.splits or (c.fam == "f32" and p.reduce == "none") or (c.fam == "bf16" and not p.reduce):
        return
    rows_p = c.K + 1 if c.fam == "f32" else c.K + int(bool(c.bias))
    e = rows_p * c.N
    part = t["s"][:c.batch * p.splits * e].cpu().numpy().reshape(c.batch, p.splits, e)
    for z in range(c.batch):
        tot = replay(part[z], int(c.fam != "f32"))
        want = tot[:c.K * c.N].reshape(c.K, c.N)
        want = ops[2][z] + want if c.acc else want
        assert np.array_equal(win[z].view(np.uint32), want.view(np.uint32)), "%r: out is not the documented sum of its partials" % (c,)
    if c.bias and c.batch == 1:
        keep = c.acc or not TP.bias_follows_accumulate(c)
        wb = ops[3] + tot[c.K * c.N:] if keep else tot[c.K * c.N:]
        assert np.array_equal(db.view(np.uint32), wb.view(np.uint32)), "%r: dbias is not the documented sum of its partials" % (c,)


@pytest.mark.parametrize("group", TP.GROUPS)
def test_tn_path(dev, group):
    """every case of one instantiation (or one named path): integer data bit for bit, its float-data cases under the existing bounds"""
    from dispu_amd import _lib
    for c in (c for c in TP.CASES if c.group == group):
        check_int(dev, _lib, c)
        if c.flt:
            check_flt(dev, _lib, c)
    print("[measured] worst fraction of each float bound so far: %r" % ({k: round(v, 4) for k, v in WORST.items()},))


def test_direct_store_equals_split_and_reduce(dev):
    """the direct store and the partial + reduction of the same product give the same bits on integer data (both equal the reference,
    checked per case above; here against each other, and on float data where one split makes the two the same sum)"""
    from dispu_amd import _lib
    d = next(c for c in TP.CASES if c.group == "f32/T11/int" and c.scratch == "null" and c.olay == "al")
    r = d._replace(scratch="exact", acc=1)
    assert TP.case_plan(d).direct == 1 and TP.case_plan(r).direct == 0 and TP.case_plan(r).splits == 1
    for kind in ("int", "flt"):
        ops = TP.operands(d, kind)
        ops = (ops[0], ops[1], np.zeros_like(ops[2]), ops[3])      # accumulate onto zeros
        outs = []
        for c in (d, r):
            host, t, base = upload(dev, c, ops)
            launch(dev, _lib, c, t, base)
            torch.cuda.synchronize()
            outs.append(collect(c, host, t)[0])
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), kind


def test_refusals_and_no_ops(dev):
    """negative sizes, empty products, NULL pointers, NULL / short scratch, dbias with a batch (bf16), the stream kernel's shape, stride,
    alignment and storage rules: the entry answers what its plan answers, and a refused or empty call writes nothing"""
    from dispu_amd import _lib
    L = _lib.lib()
    n = 70000
    t = dict(x=torch.ones(n, device=dev), z=torch.ones(n, device=dev), o=torch.full((n,), TP.SENTINEL, device=dev),
             b=torch.full((512,), TP.SENTINEL, device=dev), s=torch.full((n,), TP.SENTINEL, device=dev))
    base = {k: v.data_ptr() for k, v in t.items()}
    clean = {k: v.clone() for k, v in t.items()}
    plans = {"f32": _lib.linear_tn_plan, "bf16": _lib.linear_tn_bf16_plan, "stream": _lib.linear_tn_bf16_stream_plan}
    entries = {"f32": L.dispu_linear_tn, "bf16": L.dispu_linear_tn_bf16s, "stream": L.dispu_linear_tn_bf16_stream}
    for (fam, args), ok, kind in TP.refusals(base):
        p = plans[fam](*args)
        assert (p.rc == 0) == ok, (fam, args, p)
        ptr = _PTR_SLOTS[len(args)]
        rc = entries[fam](*[C.c_void_p(a) if i in ptr else a for i, a in enumerate(args)], _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        assert rc == p.rc, (fam, args, rc, p)
        if not ok or kind == "none":
            assert all(torch.equal(t[k], clean[k]) for k in t), (fam, args)
        else:
            for k in "obs":
                t[k].copy_(clean[k])


# ---- grouped reduction ---------------------------------------------------------------------------------------------------------------
# (K, N, splits, rows_p, assoc, accumulate, bias_accumulate, dbias: 0 none / 1 aligned / 2 four bytes off, ldo - N, out offset in floats)
GROUPED = [
    (1, 5, 1, 1, 0, 0, 0, 0, 3, 0),            # one chunk, first
    (64, 64, 130, 65, 0, 1, 1, 1, 8, 4),       # float4, three trips of s += 64
    (3, 4, 7, 4, 0, 0, 1, 1, 4, 4),            # one chunk (4 quads) between two large ones
    (37, 50, 9, 38, 1, 0, 1, 1, 7, 3),         # scalar by N % 4
    (20, 24, 8, 21, 0, 1, 0, 0, 9, 4),         # scalar by ldo % 4; rows_p = K + 1 with dbias NULL: the bias row is dropped
    (16, 16, 63, 16, 1, 1, 0, 0, 8, 3),        # scalar by the alignment of out; rows_p = K
    (8, 32, 64, 9, 0, 1, 0, 2, 8, 4),          # scalar by the alignment of dbias
    (128, 128, 65, 129, 1, 0, 0, 1, 8, 4),     # float4, the bf16 kernels' order
    (100, 36, 2, 100, 0, 1, 0, 0, 4, 8),       # float4, rows_p = K
    (5, 7, 1, 6, 0, 0, 1, 1, 5, 3),            # one split
    (256, 64, 33, 257, 0, 1, 1, 1, 8, 4),
    (24, 17, 130, 25, 1, 1, 1, 1, 3, 5),
    (2, 3, 3, 3, 1, 0, 0, 1, 6, 3),            # one chunk, last
]


def replay(part, assoc):
    """the reductions' association on the host in fp32: eight groups over the splits g, g + 8, ...; assoc 0 (tn_reduce(4)_kernel)
    alternates between two running sums per group and adds them, assoc 1 (the bf16 kernels) keeps one; groups are added in order"""
    splits = part.shape[0]
    red = []
    for g in range(8):
        v0 = np.zeros(part.shape[1], np.float32)
        v1 = np.zeros(part.shape[1], np.float32)
        for pos, s in enumerate(range(g, splits, 8)):
            if assoc == 0 and pos % 2:
                v1 = v1 + part[s]
            else:
                v0 = v0 + part[s]
        red.append(v0 + v1 if assoc == 0 else v0)
    t = red[0]
    for g in range(1, 8):
        t = t + red[g]
    return t


@pytest.mark.parametrize("kind", ["int", "flt"])
def test_grouped_reduction_table(dev, kind):
    """thirteen synthetic descriptors and four left by real products (narrow fp32, tiled fp32, bf16, stream; strided outputs between
    guards) in ONE dispatch of dispu_tn_reduce_grouped: exact on integer data, bit-equal to the host replay of the association and to
    each product's own reduction on float data; everything round the destinations untouched"""
    from dispu_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    rng = np.random.default_rng(11 + (kind == "flt"))
    vals = np.array([0, 0, 0, -3, -2, -1, 1, 2, 3], np.float32)
    draw = (lambda *s: vals[rng.integers(0, 9, s)]) if kind == "int" else (lambda *s: rng.standard_normal(s, dtype=np.float32))
    real = [next(c for c in TP.CASES if c.group == g and c.bias and TP.case_plan(c).splits > 1 and c.M <= 8192)
            for g in ("f32/narrow/kn", "f32/T11/edge", "bf16/64064/split", "stream/128/0")]
    order = [0, 1, "r0", 2, 3, "r1", 4, 5, 6, "r2", 7, 8, 9, "r3", 10, 11, 12]
    descs = (_lib.TnReduceDesc * len(order))()
    keep, synth, reals = [], {}, {}
    for slot, what in enumerate(order):
        dp = C.c_void_p(C.addressof(descs) + slot * C.sizeof(_lib.TnReduceDesc))
        if isinstance(what, str):
            c = real[int(what[1])]
            ops = TP.operands(c, kind)
            host, t, base = upload(dev, c, ops)
            launch(dev, _lib, c, t, base)                              # the product's own reduction
            host2, t2, base2 = upload(dev, c, ops)
            launch(dev, _lib, c, t2, base2, desc=dp)                   # the same product leaving its reduction to the table
            assert descs[slot].splits == TP.case_plan(c).splits and descs[slot].assoc == int(c.fam != "f32"), (c, descs[slot].splits)
            reals[slot] = (c, host, t, t2, ops)
            continue
        K, N, splits, rows_p, assoc, acc, bacc, dbk, pad, ooff = GROUPED[what]
        ldo = N + pad
        part = draw(splits, rows_p * N)
        o0 = np.full((K + 2) * ldo + 8, TP.SENTINEL, np.float32)
        win0 = draw(K, N)
        np.lib.stride_tricks.as_strided(o0[ldo + ooff:], shape=(K, N), strides=(4 * ldo, 4))[...] = win0
        b0 = np.full(N + 16, TP.SENTINEL, np.float32)
        boff = 4 if dbk == 1 else 5
        bw0 = draw(N)
        b0[boff:boff + N] = bw0
        tp, to, tb = (torch.from_numpy(a).to(dev) for a in (part, o0, b0))
        keep += [tp, to, tb]
        d = descs[slot]
        d.part, d.out, d.dbias = tp.data_ptr(), to.data_ptr() + 4 * (ldo + ooff), (tb.data_ptr() + 4 * boff if dbk else None)
        d.ldo, d.stride, d.K, d.N, d.splits, d.rows_p = ldo, rows_p * N, K, N, splits, rows_p
        d.accumulate, d.bias_accumulate, d.assoc, d.reserved = acc, bacc, assoc, 0
        synth[slot] = (what, part, win0, bw0, to, tb, ldo, ooff, boff)
    raw = C.string_at(C.addressof(descs), C.sizeof(descs))
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    _lib.check(L.dispu_tn_reduce_grouped(len(order), C.c_void_p(C.addressof(descs)), C.c_void_p(table.data_ptr()), st), "grouped")
    torch.cuda.synchronize()
    for slot, (what, part, win0, bw0, to, tb, ldo, ooff, boff) in synth.items():
        K, N, splits, rows_p, assoc, acc, bacc, dbk, pad, _ = GROUPED[what]
        got = to.cpu().numpy()
        win = np.lib.stride_tricks.as_strided(got[ldo + ooff:], shape=(K, N), strides=(4 * ldo, 4)).copy()
        np.lib.stride_tricks.as_strided(got[ldo + ooff:], shape=(K, N), strides=(4 * ldo, 4))[...] = TP.SENTINEL
        assert (got.view(np.uint32) == SENT_BITS).all(), "descriptor %d wrote outside its window" % what
        gb = tb.cpu().numpy()
        bw = gb[boff:boff + N].copy()
        gb[boff:boff + N] = TP.SENTINEL
        assert (gb.view(np.uint32) == SENT_BITS).all(), "descriptor %d wrote round its dbias" % what
        if kind == "int":
            tot = part.astype(np.int64).sum(0)
            want = tot[:K * N].reshape(K, N) + (win0.astype(np.int64) if acc else 0)
            wb = tot[K * N:] + (bw0.astype(np.int64) if bacc else 0) if (rows_p > K and dbk) else bw0.astype(np.int64)
            assert np.array_equal(win.astype(np.int64), want) and np.array_equal(bw.astype(np.int64), wb), (what, GROUPED[what])
        else:
            tot = replay(part, assoc)
            want = tot[:K * N].reshape(K, N)
            want = win0 + want if acc else want
            wb = ((bw0 + tot[K * N:]) if bacc else tot[K * N:]) if (rows_p > K and dbk) else bw0
            assert np.array_equal(win.view(np.uint32), want.view(np.uint32)), (what, GROUPED[what], float(np.abs(win - want).max()))
            assert np.array_equal(bw.view(np.uint32), wb.view(np.uint32)), (what, GROUPED[what])
    for slot, (c, host, t, t2, ops) in reals.items():
        win, db = collect(c, host, t)
        win2, db2 = collect(c, host, t2)
        assert np.array_equal(win.view(np.uint32), win2.view(np.uint32)) and np.array_equal(db.view(np.uint32), db2.view(np.uint32)), c
        if kind == "int":
            want, wdb = TP.expected_int(c, ops)
            assert np.array_equal(win2.astype(np.float64), want) and np.array_equal(db2.astype(np.float64), wdb), c


def test_grouped_reduction_refusals(dev):
    from dispu_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    buf = torch.full((4096,), TP.SENTINEL, device=dev)
    clean = buf.clone()

    def rc(**kw):
        d = (_lib.TnReduceDesc * 1)()
        f = dict(part=buf.data_ptr(), out=buf.data_ptr() + 8192, dbias=None, ldo=8, stride=40, K=4, N=8, splits=2, rows_p=5, accumulate=0,
                 bias_accumulate=0, assoc=0, reserved=0)
        f.update(kw)
        for k, v in f.items():
            setattr(d[0], k, v)
        table = torch.frombuffer(bytearray(C.string_at(C.addressof(d), C.sizeof(d))), dtype=torch.uint8).to(dev)
        r = L.dispu_tn_reduce_grouped(1, C.c_void_p(C.addressof(d)), C.c_void_p(table.data_ptr()), st)
        torch.cuda.synchronize()
        return r
    for kw in (dict(rows_p=3), dict(rows_p=6), dict(assoc=2), dict(assoc=-1), dict(splits=0), dict(splits=-1), dict(part=None), dict(out=None),
               dict(K=0), dict(N=0)):
        assert rc(**kw) != 0, kw
        assert torch.equal(buf, clean), kw
    assert L.dispu_tn_reduce_grouped(-1, None, None, st) != 0 and L.dispu_tn_reduce_grouped(1, None, None, st) != 0
    assert L.dispu_tn_reduce_grouped(0, None, None, st) == 0
    assert rc() == 0                                               # the unmodified descriptor is a valid one
