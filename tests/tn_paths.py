"""Case table, operand layouts and references of the weight-gradient (TN) kernel matrix (tests/test_tn_paths_gpu.py), importable without
a GPU: tests/test_tn_plan.py asks the plan of every case here on the CPU (dispu_linear_tn_plan, dispu_linear_tn_bf16_plan and
dispu_linear_tn_bf16_stream_plan dereference nothing) and holds the table to the set of instantiations the three dispatches can reach.

A case names the family ("f32": dispu_linear_tn, "bf16": dispu_linear_tn_bf16s, "stream": dispu_linear_tn_bf16_stream), the shape, an
operand layout, an output layout, accumulate, dbias, the bf16 storage mask, how the scratch is sized, and what its plan must say:
  lay   "al"    X and Z 16-byte aligned, row and batch strides multiples of 4 (8 for bf16-stored operands): what the interior paths need
        "oddld" odd row strides
        "offx"  X starts 4 bytes past an aligned address, strides aligned;  "offz": Z does
  olay  "al"    out 16-byte aligned, ldo and so multiples of 4 (the float4 reduction when N % 4 == 0)
        "oddld" odd ldo;  "off": out starts 12 bytes past an aligned address;  "sodd": odd batch stride  (each: the scalar reduction)
  scratch "exact" what *_scratch_floats says, "null" no scratch at all (direct / single-workgroup plans), "short" one float less than the
        narrow kernel's chunks need (its fallback to the tiled kernel, whose splits need less)
Every operand carries NaN in its padding columns (ldx > K, ldz > N) and in the row past M; `out` sits inside a wider buffer with GUARD
rows above and below and at least 3 sentinel columns on each side, dbias and the scratch between sentinel guards.

Data: "int" small integers (|v| <= 3, a third zeros): every product and partial sum is an integer below 2^24, exact in fp32 and bf16, so
the result does not depend on the summation order and is compared with array_equal against an integer reference.  The reference is an
int64 einsum; products of more than 2^24 multiply-adds are formed by a float64 matrix product instead (the same integers: every
intermediate is an integer below 2^53, so it is exact too -- the int64 einsum of the 131072-row cases takes minutes), and
test_tn_plan.py holds the two to each other.  "flt": standard-normal data against a float64 product (of the bf16-rounded operands for
the bf16 families), one case per instantiation (flt = 1), under the bounds of tests/test_train_gpu.py::test_linear_tn and
tests/test_train_bf16_gpu.py::test_linear_tn_bf16.
"""
import collections
import functools

import numpy as np

GUARD = 2
SENTINEL = -77.0
SCRATCH_TAIL = 64
BASE = 0x10000000                       # a 16-byte aligned address for the CPU plans

Case = collections.namedtuple("Case", "group fam batch M K N lay olay acc bias storage scratch flt want")
Layout = collections.namedtuple("Layout", "xoff ldx sx xsize zoff ldz sz zsize ooff ldo so osize boff bsize")


def _c(group, fam, batch, M, K, N, lay="al", olay="al", acc=0, bias=0, storage=0, scratch="exact", flt=0, **want):
    return Case(group, fam, batch, M, K, N, lay, olay, acc, bias, storage, scratch, flt, tuple(sorted(want.items())))


def _r(v, q):
    return (v + q - 1) // q * q


def layout(c):
    """element offsets and strides of X, Z, out, dbias inside their buffers (elements of the stored type)"""
    q = 8 if c.fam != "f32" else 4
    ldx, ldz = _r(c.K, q) + q, _r(c.N, q) + q
    if c.lay == "oddld":
        ldx, ldz = ldx + 1, ldz + 3
    xoff = {"offx": 1}.get(c.lay, 0) * (2 if c.storage & 1 else 1)
    zoff = {"offz": 1}.get(c.lay, 0) * (2 if c.storage & 2 else 1)
    rows = c.M + 1
    sx, sz = rows * ldx + (1 if c.lay == "oddld" else 2 * q), rows * ldz + (3 if c.lay == "oddld" else q)
    ldo = _r(c.N, 4) + 8 + (1 if c.olay == "oddld" else 0)
    c0 = 3 if c.olay == "off" else 4
    so = (c.K + 2 * GUARD) * ldo + (5 if c.olay == "sodd" else 4 if c.olay != "oddld" else 1)
    return Layout(xoff, ldx, sx, xoff + c.batch * sx, zoff, ldz, sz, zoff + c.batch * sz, GUARD * ldo + c0, ldo, so, c.batch * so,
                  4, c.N + 8)


def scratch_need(c):
    from dispu_amd import _lib
    L = _lib.lib()
    if c.fam == "f32":
        return L.dispu_linear_tn_scratch_floats(c.batch, c.M, c.K, c.N)
    if c.fam == "bf16":
        return L.dispu_linear_tn_bf16_scratch_floats(c.batch, c.M, c.K, c.N)
    return L.dispu_linear_tn_bf16_stream_scratch_floats(c.M, c.K, c.N)


def scratch_floats(c):
    """floats of scratch the case hands to the entry"""
    need = scratch_need(c)
    return {"exact": need, "null": 0, "short": need - 1}[c.scratch]


def entry_args(c, base=None):
    """the arguments of the case's entry without the stream; `base` maps x, z, o, b, s to the addresses of their buffers (the CPU plans
    use aligned stand-ins)"""
    lo = layout(c)
    base = base or dict(x=BASE, z=BASE, o=BASE, b=BASE, s=BASE)
    ex, ez = (2 if c.storage & 1 else 4), (2 if c.storage & 2 else 4)
    X, Z, out = base["x"] + ex * lo.xoff, base["z"] + ez * lo.zoff, base["o"] + 4 * lo.ooff
    db = base["b"] + 4 * lo.boff if c.bias else None
    sf = scratch_floats(c)
    sc = base["s"] if c.scratch != "null" else None
    if c.fam == "stream":
        return (c.M, c.K, c.N, X, lo.ldx, Z, lo.ldz, c.storage, out, lo.ldo, c.acc, db, sc, sf)
    a = (c.batch, c.M, c.K, c.N, X, lo.ldx, lo.sx, Z, lo.ldz, lo.sz, out, lo.ldo, lo.so, c.acc, db, sc, sf)
    return a + (c.storage,) if c.fam == "bf16" else a


def plan(c, base=None):
    from dispu_amd import _lib
    f = {"f32": _lib.linear_tn_plan, "bf16": _lib.linear_tn_bf16_plan, "stream": _lib.linear_tn_bf16_stream_plan}[c.fam]
    return f(*entry_args(c, base))


def instantiation(c, p):
    """the census key of a plan: what distinguishes one compiled path from another"""
    if c.fam == "f32":
        return ("f32", p.kind, p.TK, p.TNN, p.edge, p.direct, p.reduce)
    if c.fam == "bf16":
        return ("bf16", p.tile, p.reduce, c.storage)
    return ("stream", p.BN, p.storage)


def group_path(c):
    """what the group's name promises about the plan, as a dict of plan fields"""
    g = c.group.split("/")
    if g[0] == "f32" and g[1][0] == "T":
        return dict(kind="tiled", TK=int(g[1][1]), TNN=int(g[1][2]), edge=int(g[2] == "edge"))
    if g[0] == "f32" and g[1] == "narrow":
        return dict(kind="narrow")
    if g[0] == "f32" and g[1] == "fallback":
        return dict(kind="tiled")
    if g[1] == "clear":
        return dict(kind="clear")
    if g[0] == "f32":
        return dict(reduce=g[2])                                          # f32/reduce/<kind>
    if g[0] == "bf16":
        return dict(kind="tiled", tile=int(g[1]), reduce=int(g[2] == "split"))
    return dict(BN=int(g[1]), storage=int(g[2]))


# ---- data and references -------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _seed(c):
    return (c.M * 1000003 + c.K * 1009 + c.N * 17 + c.batch) % (2 ** 31)


def operands(c, kind):
    """X [batch, M, K], Z [batch, M, N], out0 [batch, K, N], db0 [N] as float32; kind "int" or "flt" """
    rng = np.random.default_rng(_seed(c) + (kind == "flt"))
    if kind == "int":
        vals = np.array([0, 0, 0, -3, -2, -1, 1, 2, 3], np.float32)
        draw = lambda *s: vals[rng.integers(0, 9, s, dtype=np.int8)]
    else:
        draw = lambda *s: rng.standard_normal(s, dtype=np.float32)
    return draw(c.batch, c.M, c.K), draw(c.batch, c.M, c.N), draw(c.batch, c.K, c.N), draw(c.N)


def int_product(X, Z):
    """sum_m X[z][m][k] Z[z][m][n] of integer-valued arrays, as int64 (module docstring: einsum, or the float64 product of the same
    integers where the einsum would take minutes)"""
    b, M, K = X.shape
    N = Z.shape[2]
    if b * M * K * N <= 2 ** 24:
        return np.einsum("zmk,zmn->zkn", X.astype(np.int64), Z.astype(np.int64))
    p = np.matmul(X.astype(np.float64).transpose(0, 2, 1), Z.astype(np.float64))
    assert np.abs(p).max(initial=0) < 2.0 ** 53 and (p == np.rint(p)).all()
    return p.astype(np.int64)


def bias_follows_accumulate(c):
    """the fp32 entry's dbias always accumulates, the bf16 entries' dbias follows `accumulate` (include/dispu_hip.h)"""
    return c.fam != "f32"


def expected_int(c, ops):
    """(out [batch, K, N], dbias [N] or None) as int64, with every value asserted below 2^24"""
    X, Z, o0, b0 = ops
    out = int_product(X, Z) + (o0.astype(np.int64) if c.acc else 0)
    db = None
    if c.bias:
        keep = c.acc or not bias_follows_accumulate(c)
        db = Z.astype(np.int64).sum((0, 1)) + (b0.astype(np.int64) if keep else 0)
    # every partial sum of |x z| stays below the total of |x| |z| <= 9 M: exact in fp32 whatever the order
    assert 9 * c.M + 3 < 2 ** 24 and np.abs(out).max(initial=0) < 2 ** 24 and (db is None or np.abs(db).max(initial=0) < 2 ** 24), c
    return out, db


def expected_flt(c, ops):
    """float64 references and bounds of the float-data run: (out, out_bound, dbias, dbias_bound); bounds are elementwise arrays or
    scalars, the project's existing ones (module docstring)"""
    X, Z, o0, b0 = ops
    if c.fam == "f32":
        ref = np.matmul(X.astype(np.float64).transpose(0, 2, 1), Z.astype(np.float64)) + (o0 if c.acc else 0)
        ob = (2e-5 if c.M > 2000 else 1e-5) * np.abs(ref).max()
        db = dbb = None
        if c.bias:
            db = b0 + Z.astype(np.float64).sum((0, 1))
            dbb = 2e-5 * np.abs(db).max()
        return ref, ob, db, dbb
    xr, zr = bf16_round(X).astype(np.float64), bf16_round(Z).astype(np.float64)
    ref = np.matmul(xr.transpose(0, 2, 1), zr) + (o0 if c.acc else 0)
    ob = 4e-6 * np.matmul(np.abs(xr).transpose(0, 2, 1), np.abs(zr)) + 1e-6 * (1 + np.abs(ref))
    db = dbb = None
    if c.bias:
        zs = zr if (c.storage & 2) else Z.astype(np.float64)              # a bf16-stored Z sums its stored (rounded) values
        db = zs.sum((0, 1)) + (b0 if c.acc else 0)
        dbb = 2e-6 * np.abs(zs).sum((0, 1)).max() + 1e-6
    return ref, ob, db, dbb


def host_buffers(c, ops):
    """float32 images of the five buffers: x, z (NaN padding; converted to bf16 by the caller where stored so), o (sentinels, the
    initial values in its windows), b, s (NaN, sentinel tail)"""
    X, Z, o0, b0 = ops
    lo = layout(c)

    def strided(size, off, ld, stride, blocks, fill):
        buf = np.full(size, fill, np.float32)
        for z, blk in enumerate(blocks):
            r, w = blk.shape
            np.lib.stride_tricks.as_strided(buf[off + z * stride:], shape=(r, w), strides=(4 * ld, 4))[...] = blk
        return buf
    x = strided(lo.xsize, lo.xoff, lo.ldx, lo.sx, list(X), np.nan)
    z = strided(lo.zsize, lo.zoff, lo.ldz, lo.sz, list(Z), np.nan)
    o = strided(lo.osize, lo.ooff, lo.ldo, lo.so, list(o0), SENTINEL)
    b = np.full(lo.bsize, SENTINEL, np.float32)
    b[lo.boff:lo.boff + c.N] = b0
    sf = scratch_floats(c)
    s = np.full(sf + SCRATCH_TAIL, np.nan, np.float32)
    s[sf:] = SENTINEL
    return dict(x=x, z=z, o=o, b=b, s=s)


def out_window(c, obuf):
    """(the [batch, K, N] window of an output buffer image, the image with the window painted over by sentinels)"""
    lo = layout(c)
    rest = obuf.copy()
    win = np.empty((c.batch, c.K, c.N), np.float32)
    for z in range(c.batch):
        v = np.lib.stride_tricks.as_strided(rest[lo.ooff + z * lo.so:], shape=(c.K, c.N), strides=(4 * lo.ldo, 4))
        win[z] = v
        v[...] = SENTINEL
    return win, rest


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def _tiled(tk, tnn, edge, *a, **k):
    return _c("f32/T%d%d/%s" % (tk, tnn, "edge" if edge else "int"), "f32", *a, **k)


def _f32_tiled_cases():
    cs = []
    # <1,1> interior: 1, 2, 3 slabs of 16 rows (the pipeline prologue), one split
    for M in (16, 32, 48):
        cs.append(_tiled(1, 1, 0, 1, M, 64, 64, acc=1, bias=1, splits=1, reduce="vec4"))
    cs.append(_tiled(1, 1, 0, 1, 48, 64, 64, scratch="null", flt=1, direct=1))                       # direct store, ldo > N, no scratch
    cs.append(_tiled(1, 1, 0, 1, 48, 64, 64, olay="oddld", scratch="null", direct=1))
    cs.append(_tiled(1, 1, 0, 1, 48, 64, 64, acc=1, direct=0, splits=1))                               # the same through split + reduce
    cs.append(_tiled(1, 1, 0, 1, 48, 64, 64, bias=1, olay="oddld", reduce="scalar"))
    cs.append(_tiled(1, 1, 0, 1, 48, 64, 64, bias=1, olay="off", reduce="scalar"))
    cs.append(_tiled(1, 1, 0, 1, 544, 64, 64, bias=1, splits=3, rows=192, flt=1))                      # last split 160 rows < 192
    # split counts round a multiple of 8, and the reduction's second trip (s += 64)
    for M, s in ((304, 2), (1792, 7), (2048, 8), (2304, 9), (16128, 63), (16384, 64), (16640, 65), (33280, 130)):
        cs.append(_tiled(1, 1, 0, 2, M, 64, 64, acc=s % 2, bias=0, splits=s, reduce="vec4"))
    cs.append(_tiled(1, 1, 0, 2, 2304, 64, 64, olay="sodd", acc=1, splits=9, reduce="scalar"))
    cs.append(_tiled(1, 1, 0, 3, 304, 64, 128, acc=1, bias=1, splits=2))                               # batch 3, dbias by float atomics
    # <1,1> edge: ragged M round the slab, ragged K and N, every operand layout
    for M in (1, 15, 16, 17, 32, 33, 48):
        cs.append(_tiled(1, 1, 1, 1, M, 5, 7, acc=M % 2, bias=1, splits=1, reduce="scalar"))
    cs.append(_tiled(1, 1, 1, 1, 33, 6, 10, scratch="null", direct=1))                                 # aligned float4 loads with c + 3 < climit tails
    cs.append(_tiled(1, 1, 1, 1, 33, 64, 64, bias=1, reduce="vec4"))                                   # edge only by M % 16
    for lay in ("oddld", "offx", "offz"):
        cs.append(_tiled(1, 1, 1, 1, 48, 64, 64, lay=lay, acc=1, bias=1, reduce="vec4"))               # edge only by the layout
        cs.append(_tiled(1, 1, 1, 1, 33, 23, 41, lay=lay, scratch="null", direct=1))
    cs.append(_tiled(1, 1, 1, 1, 300, 37, 50, bias=1, splits=2, rows=160, flt=1))                      # last split 140 rows
    cs.append(_tiled(1, 1, 1, 1, 300, 130, 20, bias=1, acc=1, splits=2, reduce="vec4"))                # three K-tiles: the bias row is K-tile 0's
    cs.append(_tiled(1, 1, 1, 1, 300, 130, 70, bias=1, splits=2, reduce="scalar"))                     # ... with two N-tiles
    for M, s in ((1791, 7), (16127, 63), (16639, 65), (33279, 130)):
        cs.append(_tiled(1, 1, 1, 1, M, 20, 9, acc=1, bias=1, splits=s, reduce="scalar"))
    cs.append(_tiled(1, 1, 1, 3, 257, 37, 50, lay="oddld", olay="sodd", acc=1, bias=1, splits=2))      # batch 3: distinct sx, sz, so
    cs.append(_tiled(1, 1, 1, 3, 33, 37, 50, scratch="null", direct=1))
    # the other five tiles at the smallest shapes the plan gives them
    cs.append(_tiled(1, 2, 0, 1, 304, 1024, 1024, acc=1, bias=1, splits=2, reduce="vec4", flt=1))
    cs.append(_tiled(1, 2, 0, 1, 304, 1024, 1024, olay="oddld", splits=2, reduce="scalar"))
    cs.append(_tiled(1, 2, 0, 1, 16, 1024, 2048, scratch="null", direct=1))
    cs.append(_tiled(1, 2, 0, 2, 16, 2048, 512, bias=1, splits=1))
    cs.append(_tiled(1, 2, 1, 2, 257, 2047, 129, bias=1, acc=1, splits=2, reduce="scalar", flt=1))
    cs.append(_tiled(1, 2, 1, 2, 257, 2047, 132, lay="offz", bias=1, splits=2, reduce="vec4"))
    cs.append(_tiled(1, 2, 1, 3, 1, 2047, 257, scratch="null", direct=1))
    cs.append(_tiled(1, 2, 1, 1, 32767, 1, 129, bias=1, splits=128))
    cs.append(_tiled(1, 4, 0, 1, 8192, 64, 2048, acc=1, bias=1, splits=32, reduce="vec4", flt=1))
    cs.append(_tiled(1, 4, 0, 1, 8192, 64, 2048, olay="off", splits=32, reduce="scalar"))
    cs.append(_tiled(1, 4, 1, 1, 32767, 1, 257, bias=1, splits=128, reduce="scalar", flt=1))
    cs.append(_tiled(1, 4, 1, 2, 4100, 3, 2044, acc=1, splits=17, reduce="vec4"))
    cs.append(_tiled(2, 1, 0, 1, 4096, 2048, 64, acc=1, bias=1, reduce="vec4", flt=1))
    cs.append(_tiled(2, 1, 0, 2, 2000, 2048, 64, olay="oddld", reduce="scalar"))
    cs.append(_tiled(2, 1, 1, 1, 4100, 2047, 1, bias=1, splits=17, reduce="scalar", flt=1))
    cs.append(_tiled(2, 1, 1, 2, 16383, 129, 4, acc=1, splits=64, reduce="vec4"))
    cs.append(_tiled(2, 2, 0, 1, 304, 1024, 2048, acc=1, bias=1, splits=2, reduce="vec4", flt=1))
    cs.append(_tiled(2, 2, 0, 1, 304, 1024, 2048, olay="oddld", splits=2, reduce="scalar"))
    cs.append(_tiled(2, 2, 0, 1, 16, 2048, 2048, scratch="null", direct=1))
    cs.append(_tiled(2, 2, 1, 3, 257, 513, 1025, bias=1, acc=1, splits=2, reduce="scalar", flt=1))
    cs.append(_tiled(2, 2, 1, 1, 304, 1024, 2048, lay="oddld", bias=1, splits=2, reduce="vec4"))
    cs.append(_tiled(2, 2, 1, 1, 1, 2047, 2047, scratch="null", direct=1))
    cs.append(_tiled(2, 2, 1, 1, 16383, 129, 129, splits=64))
    cs.append(_tiled(2, 4, 0, 1, 304, 2048, 2048, acc=1, bias=1, splits=2, reduce="vec4", flt=1))
    cs.append(_tiled(2, 4, 0, 1, 304, 2048, 2048, olay="off", splits=2, reduce="scalar"))
    cs.append(_tiled(2, 4, 0, 2, 16, 2048, 2048, scratch="null", direct=1))
    cs.append(_tiled(2, 4, 1, 3, 257, 1025, 1025, bias=1, acc=1, splits=2, reduce="scalar", flt=1))
    cs.append(_tiled(2, 4, 1, 1, 304, 2048, 2048, lay="offx", splits=2, reduce="vec4"))
    cs.append(_tiled(2, 4, 1, 2, 1, 2047, 2047, scratch="null", direct=1))
    cs.append(_tiled(2, 4, 1, 1, 16383, 129, 257, bias=1, splits=64))
    return cs


def _f32_narrow_cases():
    cs = []
    g = lambda *a, **k: _c("f32/narrow/kn", "f32", 1, *a, **k)
    # every K x N round the 16 x 16 wave tile: 1 - 17 k-tiles (+ the bias tile), 1 - 4 n-tiles
    for i, K in enumerate((1, 3, 15, 16, 17, 24, 64, 240, 256)):
        for j, N in enumerate((1, 3, 15, 16, 17, 24, 64)):
            cs.append(g(4096, K, N, acc=(i + j) % 2, bias=(i + 2 * j) % 3 != 0, lay=("al", "oddld", "offx")[(i + j) % 3],
                        flt=int((K, N) == (24, 17))))
    g = lambda *a, **k: _c("f32/narrow/rows", "f32", 1, *a, **k)
    cs.append(g(4096, 16, 16, bias=1, wpb=2, grid_y=1, rows=128, splits=32))             # jobs = 2 < 16: a two-wave block; rows clamped up to 128
    cs.append(g(4096, 256, 64, bias=1, acc=1, wpb=16, grid_y=5, reduce="vec4"))          # jobs = 68: five grid.y, twelve idle waves in the last
    cs.append(g(4100, 16, 16, bias=1, rows=128, splits=33))                              # last chunk: 4 rows
    cs.append(g(8320, 16, 16, bias=1, acc=1, rows=128, splits=65))                       # more than 64 chunks: the reduction's second trip
    cs.append(g(131072, 256, 64, bias=1, rows=4096, splits=32, flt=1))                   # rows clamped down to 4096
    cs.append(g(4096, 24, 17, olay="oddld", bias=1, reduce="scalar"))
    cs.append(g(4096, 24, 16, olay="off", acc=1, reduce="scalar"))
    # what keeps a narrow shape off the narrow kernel
    f = lambda *a, **k: _c("f32/fallback", "f32", *a, **k)
    cs.append(f(1, 4098, 24, 16, bias=1, kind="tiled"))                                  # M % 4 != 0
    cs.append(f(1, 4092, 24, 16, bias=1, kind="tiled"))                                  # M < 4096
    cs.append(f(2, 4096, 24, 16, bias=1, kind="tiled"))                                  # batch > 1
    cs.append(f(1, 4096, 256, 64, bias=1, scratch="short", kind="tiled", splits=16))     # scratch short of the 22 chunks, enough for 16 splits
    return cs


def _f32_reduce_cases():
    """the grid-stride trips of the two reduction kernels: more 32-quad (64-element) chunks than the 16384 (8192) workgroups launched"""
    return [_c("f32/reduce/vec4", "f32", 1, 300, 2048, 1028, acc=1, bias=1, capped=1, reduce_grid=16384, splits=2),
            _c("f32/reduce/scalar", "f32", 1, 300, 1024, 513, acc=1, bias=1, capped=1, reduce_grid=8192, splits=2),
            _c("f32/reduce/vec4", "f32", 3, 300, 64, 64, acc=1, bias=1, capped=0),
            _c("f32/reduce/scalar", "f32", 3, 300, 64, 62, bias=1, capped=0)]


def _bf16_cases():
    cs = []
    g = lambda tile, split, *a, **k: _c("bf16/%d/%s" % (tile, "split" if split else "single"), "bf16", *a, **k)
    for st in (0, 1, 2, 3):
        cs.append(g(128032, 0, 1, 100, 7, 9, storage=st, bias=1, acc=st % 2, scratch="null", flt=1))
        cs.append(g(128032, 1, 1, 1000, 130, 31, storage=st, bias=1, acc=st // 2, flt=1))
        cs.append(g(64064, 0, 1, 200, 70, 33, storage=st, bias=1, acc=1 - st % 2, scratch="null", flt=1))   # out as its own residual
        cs.append(g(64064, 1, 1, 1000, 134, 255, storage=st, bias=1, acc=st % 2, flt=1))
        cs.append(g(128128, 0, 2, 1, 2047, 2047, storage=st, acc=st % 2, scratch="null", flt=1))
        cs.append(g(128128, 1, 1, 131072, 5, 40, storage=st, bias=1, acc=st // 2, splits=512, flt=1))
    cs.append(g(128032, 0, 3, 130, 129, 32, lay="oddld", olay="sodd", acc=1, scratch="null"))        # batched, two K-tiles
    cs.append(g(128032, 1, 1, 4096, 96, 24, lay="offx", olay="oddld", acc=1))                          # no dbias: partials of K rows
    cs.append(g(128032, 1, 2, 1000, 130, 31, olay="off"))
    cs.append(g(64064, 0, 3, 64, 65, 100, lay="oddld", olay="oddld", scratch="null"))
    cs.append(g(64064, 0, 1, 256, 64, 64, bias=1, scratch="null"))                                     # full tiles
    cs.append(g(64064, 1, 2, 1000, 134, 255, lay="offz", acc=1))
    cs.append(g(64064, 1, 1, 300, 65, 33, bias=1, splits=2, rows=192))                                 # last split 108 rows
    cs.append(g(128128, 1, 1, 131072, 1, 33, acc=1, splits=512))
    return cs


def _stream_cases():
    cs = []
    for st in (0, 3):
        g = lambda bn, *a, **k: _c("stream/%d/%d" % (bn, st), "stream", 1, *a, storage=st, **k)
        cs.append(g(256, 32, 128, 256, bias=1, splits=1, flt=1))                                      # one 32-row slab
        cs.append(g(256, 96, 128, 256, acc=1, splits=1))                                              # three slabs: once round the ring
        cs.append(g(256, 256, 256, 256, bias=1, acc=1, splits=2, rows=128))
        cs.append(g(256, 32768, 128, 256, bias=1, splits=256, rows=128, flt=1))                       # the most splits the plan gives
        cs.append(g(256, 4128, 128, 512, bias=1, splits=1))                                           # 129 slabs: no split divides them
        cs.append(g(128, 64, 256, 128, bias=1, acc=1, splits=1, flt=1))
        cs.append(g(128, 256, 128, 384, olay="oddld", splits=2))
        cs.append(g(128, 8192, 128, 128, bias=1, splits=64, rows=128, flt=1))
        cs.append(g(128, 4160, 256, 128, bias=1, acc=1, splits=2, rows=2080))                         # 130 slabs: 2 is the last split that divides
    return cs


def refusals(base=None):
    """[((family, plan arguments), accepted, kind)]: negative sizes, empty products, M == 0, NULL pointers, NULL / short scratch, dbias
    with a batch, the stream kernel's shape, stride, alignment and storage rules"""
    from dispu_amd import _lib
    lib = _lib.lib()
    base = base or dict(x=BASE, z=BASE, o=BASE, b=BASE, s=BASE)
    AX, AZ, AO, AB, AS = (base[k] for k in "xzobs")
    out = []
    M, K, N = 300, 37, 50
    need = lib.dispu_linear_tn_scratch_floats(1, M, K, N)

    def f32(b=1, M=M, K=K, N=N, X=AX, Z=AZ, o=AO, acc=0, db=AB, sc=AS, sf=need):
        return ("f32", (b, M, K, N, X, 40, M * 40, Z, 52, M * 52, o, 56, K * 56, acc, db, sc, sf))
    nb = lib.dispu_linear_tn_bf16_scratch_floats(1, M, K, N)

    def bf(b=1, M=M, K=K, N=N, X=AX, Z=AZ, o=AO, acc=0, db=AB, sc=AS, sf=nb):
        return ("bf16", (b, M, K, N, X, 40, M * 40, Z, 52, M * 52, o, 56, K * 56, acc, db, sc, sf, 0))
    for mk in (f32, bf):
        out += [(mk(b=-1), False, "none"), (mk(M=-1), False, "none"), (mk(K=-1), False, "none"), (mk(N=-1), False, "none"),
                (mk(b=0, db=None), True, "none"), (mk(K=0), True, "none"), (mk(N=0), True, "none"), (mk(M=0), True, "clear"),
                (mk(M=0, X=None, Z=None), True, "clear"), (mk(o=None), False, "none"), (mk(X=None), False, "none"),
                (mk(Z=None), False, "none"), (mk(sc=None), False, "none"), (mk(sf=mk()[1][16] - 1), False, "none"), (mk(), True, "tiled")]
    out += [(bf(b=2, db=AB, sf=2 * nb), False, "none"), (bf(b=2, db=None, sf=2 * nb), True, "tiled"),
            (f32(M=48, db=None, sc=None, sf=0), True, "tiled"), (f32(M=48, db=None, acc=1, sc=None, sf=0), False, "none"),
            (bf(M=48, sc=None, sf=0), True, "tiled")]
    M, K, N = 256, 128, 256
    ns = lib.dispu_linear_tn_bf16_stream_scratch_floats(M, K, N)

    def st(M=M, K=K, N=N, X=AX, ldx=K + 8, Z=AZ, ldz=N + 8, sto=0, o=AO, sc=AS, sf=ns):
        return ("stream", (M, K, N, X, ldx, Z, ldz, sto, o, N, 0, AB, sc, sf))
    out += [(st(), True, None), (st(sto=3), True, None), (st(K=130), False, None), (st(N=192), False, None), (st(M=250), False, None),
            (st(M=0), False, None), (st(M=-32), False, None), (st(ldx=K + 2), False, None), (st(ldz=N + 1), False, None),
            (st(sto=3, ldx=K + 4), False, None), (st(ldx=K - 4), False, None), (st(sto=1), False, None), (st(sto=2), False, None),
            (st(X=AX + 4), False, None), (st(Z=AZ + 8), False, None), (st(X=None), False, None), (st(Z=None), False, None),
            (st(o=None), False, None), (st(sc=None), False, None), (st(sf=ns - 1), False, None)]
    return out


def _clear_cases():
    """M == 0: exactly the K x N window of a strided `out` is cleared unless accumulating; the fp32 entry leaves dbias alone (it only ever
    adds to it), the bf16 entry clears it unless accumulating"""
    cs = []
    for fam in ("f32", "bf16"):
        for acc in (0, 1):
            cs.append(_c(fam + "/clear", fam, 1, 0, 37, 50, acc=acc, bias=1, scratch="null"))
            cs.append(_c(fam + "/clear", fam, 3, 0, 5, 7, olay="oddld", acc=acc, scratch="null"))
    return cs


CASES = _clear_cases() + _f32_tiled_cases() + _f32_narrow_cases() + _f32_reduce_cases() + _bf16_cases() + _stream_cases()
GROUPS = sorted(set(c.group for c in CASES))


@functools.lru_cache(maxsize=None)
def case_plan(c):
    return plan(c)
