"""Case table, operand layouts and references of the dense-layer kernel matrix (tests/test_linear_paths_gpu.py), importable without
a GPU: tests/test_linear_plan.py computes the dispatch plan of every case here on the CPU (dispu_linear_plan dereferences nothing) and
holds the table to the set of kernel instantiations the dispatch can reach.

A case names the ABI entry, the forced block tile, the shape, what is attached to the epilogue and an operand layout:
  "al"    every base 16-byte aligned, every row / batch stride a multiple of 4 floats (what the interior paths need)
  "oddld" every row stride odd
  "off"   X and W start 4 bytes past an aligned address, strides aligned
  "yodd"  X and W as "al", Y with an odd row stride (full vector loads next to the scalar epilogue)
Every output sits inside a wider buffer: GUARD rows above and below, at least 3 sentinel columns left and right.
"""
import collections
import functools

import numpy as np

TILES = {128257: (128, 256, 16), 128128: (128, 128, 32), 64128: (64, 128, 32), 128064: (128, 64, 32), 64064: (64, 64, 32)}   # code: BM, BN, BKR
PATHS = ("dma", "tr", "edge", "edget")       # interior DMA pipeline, interior transposed-B, edge, edge transposed-B
SKINNY = [(ng, tb) for ng in (2, 8, 16, 24) for tb in (0, 1)]
GUARD = 2
SENTINEL = -77.0

# res: bit 0 = R1, bit 1 = R2.  mask: None, ("ptr", mcols) or ("null", mcols) -- a NULL mask with mcols > 0.  shared: batch stride of W = 0.
Case = collections.namedtuple("Case", "group entry tile batch M K N transb act bias res mask lay shared")


def _c(group, tile, M, K, N, transb, entry="linear", batch=None, act=0, bias=0, res=0, mask=None, lay="al", shared=0):
    if batch is None:
        # the skinny kernel takes batch 1 products of these shapes unless R2 or a BatchNorm fold is attached: a second batch entry keeps
        # the case on the tiled kernel (the masked entry needs batch 1: its cases use N >= 128 with K > 32, or K % 4 != 0)
        skinny_shape = K % 4 == 0 and K <= 384 and (N <= 64 or (K <= 32 and N <= 128))
        batch = 2 if (skinny_shape and entry == "linear" and not (res & 2)) else 1
    return Case(group, entry, tile, batch, M, K, N, transb, act, bias, res, mask, lay, shared)


def _epilogues(group, tile, M, K, N, transb):
    """every epilogue of one (tile, load path): plain +- bias +- ReLU; BatchNorm fold alone and with R1; R1, R2, both; the mask with
    mcols in {0, N - 5, N, N + 7} and a NULL mask with mcols > 0."""
    out = [_c(group, tile, M, K, N, transb, act=a, bias=b) for a in (0, 1) for b in (0, 1)]
    out += [_c(group, tile, M, K, N, transb, entry="bn", act=1, bias=1, res=r) for r in (0, 1)]
    out += [_c(group, tile, M, K, N, transb, act=1, bias=1, res=r) for r in (1, 2, 3)]
    out += [_c(group, tile, M, K, N, transb, entry="masked", bias=1, res=1, mask=("ptr", mc)) for mc in (0, N - 5, N, N + 7)]
    out += [_c(group, tile, M, K, N, transb, entry="masked", res=1, mask=("null", N))]
    return out


def _tile_cases(code):
    BM, BN, BKR = TILES[code]
    g = lambda path: "%d/%s" % (code, path)
    NE = max(BN, 128)                         # width of the batch 1 epilogue cases: past the skinny kernel's N <= 64
    cs = []
    # interior DMA pipeline: 1 - 5 and 7 slabs of 16 = the prologue (issue(0..2), wait_newer), one trip round the 4-stage ring, the wrap
    for i, K in enumerate((16, 32, 48, 64, 80, 112)):
        cs.append(_c(g("dma"), code, BM * (1 + i % 2), K, BN * (2 - i % 2), 0, bias=i % 2))
    cs.append(_c(g("dma"), code, 2 * BM, 48, 2 * BN, 0, act=1, bias=1, res=1))
    cs += _epilogues(g("dma"), code, BM, 48, NE, 0)
    # interior transposed-B: 1 - 5 slabs through the two-register-set loop that steps by two
    for i in range(1, 6):
        cs.append(_c(g("tr"), code, BM * (1 + i % 2), i * BKR, BN * (2 - i % 2), 1, bias=i % 2))
    cs.append(_c(g("tr"), code, 2 * BM, 3 * BKR, 2 * BN, 1, act=1, bias=1, res=1))
    cs += _epilogues(g("tr"), code, BM, 3 * BKR, NE, 1)
    for tb, path in ((0, "edge"), (1, "edget")):
        # ragged M, N, K on aligned operands (the float4 loads with their k + 3 < K / n + 3 < N tails)
        shapes = [(BM + 1, BN - 3), (2 * BM - 1, BN + 1), (BM + 1, BN + 1), (2 * BM - 1, BN - 3), (BM + 1, BN + 1)]
        for (M, N), K in zip(shapes, (1, 3, BKR - 1, BKR + 1, 2 * BKR + 5)):
            cs.append(_c(g(path), code, M, K, N, tb, bias=1))
        cs.append(_c(g(path), code, BM + 1, BKR + 1, BN + 1, tb, lay="oddld", bias=1, res=1))
        cs.append(_c(g(path), code, 2 * BM - 1, 2 * BKR + 5, BN - 3, tb, lay="off", act=1))
        cs.append(_c(g(path), code, BM + 1, BKR + 3, BN + 1, tb, lay="yodd", bias=1))
        cs.append(_c(g(path), code, BM, 24, BN, tb, bias=1))                 # aligned full tiles: an edge kernel only because of K
        cs += _epilogues(g(path), code, BM + 1, BKR + 1, NE + 1, tb)
    # batched: distinct strides for X, W, Y and R1, and one W for every batch entry
    for path, tb, (M, K, N) in (("dma", 0, (BM, 80, 2 * BN)), ("tr", 1, (BM, 2 * BKR, 2 * BN)),
                                ("edge", 0, (BM + 1, BKR + 1, BN + 1)), ("edget", 1, (BM + 1, BKR + 1, BN + 1))):
        cs.append(_c(g(path), code, M, K, N, tb, batch=3, act=1, bias=1, res=1))
        cs.append(_c(g(path), code, M, K, N, tb, batch=3, bias=1, shared=1))
    if code == 128257:
        cs.append(_c(g("dma"), code, 128, 1024, 256, 0))                     # EPI 6: the long-K twin of EPI 0
    return cs


def _skinny_cases(ng, tb):
    g = "skinny/%d/%d" % (ng, tb)
    Ks = {2: (4, 16, 20, 32), 8: (36, 128), 16: (132, 256), 24: (260, 384)}[ng]       # both sides of every NG boundary, the partial 16-group
    cs = []
    for K in Ks:
        Ns = (1, 15, 16, 17, 33, 64) + ((65, 128) if K <= 32 else ())                 # 1-, 3- and 4-wave blocks, a second grid.y
        cs += [_c(g, 0, 17, K, N, tb, batch=1, bias=N % 2, act=N % 3 == 0) for N in Ns]
        cs += [_c(g, 0, M, K, 17, tb, batch=1, bias=1) for M in (1, 15, 1000)]
        cs.append(_c(g, 0, 1000, K, 64, tb, batch=1, act=1, bias=1, res=1))
    cs.append(_c(g, 0, 17, Ks[-1], 33, tb, batch=1, entry="masked", bias=1, res=1, mask=("ptr", 20)))
    cs.append(_c(g, 0, 1000, Ks[0], 17, tb, batch=1, entry="masked", mask=("ptr", 16)))
    return cs


def _split_cases():
    """N = 128 + t: t <= 32 goes to the skinny kernel as a second launch, with bias, R1 and the mask offset by n0 = 128."""
    cs = []
    for tb in (0, 1):
        for t in (1, 32, 33):
            cs.append(_c("split", 0, 200, 64, 128 + t, tb, batch=1, act=1, bias=1, res=1))
        cs.append(_c("split", 0, 256, 64, 160, tb, batch=1, bias=1, res=1))                       # interior head
        for mc in (123, 128, 131, 160):                                                        # the tail sees mcols - n0 = -5, 0, 3, 32
            cs.append(_c("split", 0, 200, 64, 160, tb, batch=1, entry="masked", bias=1, res=1, mask=("ptr", mc)))
        cs.append(_c("split", 0, 256, 64, 160, tb, batch=1, entry="masked", res=1, mask=("ptr", 160)))
    return cs


CASES = [c for code in TILES for c in _tile_cases(code)] + [c for ng, tb in SKINNY for c in _skinny_cases(ng, tb)] + _split_cases()
GROUPS = sorted(set(c.group for c in CASES))


def expected_launch(case):
    """What the group of a case promises about its plan: (kind, BM, BN, BK, transb, edge) of the tiled launch or ("skinny", NG, transb);
    None for the split group (launch counts are asserted where the cases are run)."""
    parts = case.group.split("/")
    if parts[0] == "skinny":
        return ("skinny", int(parts[1]), int(parts[2]))
    if parts[0] == "split":
        return None
    BM, BN, BKR = TILES[int(parts[0])]
    if case.mask is not None and case.mask[0] == "ptr" and 0 < case.mask[1] < case.N and parts[1] in ("dma", "tr"):
        # a mask narrower than the product takes the guarded per-column epilogue even on full, aligned tiles: the edge kernel
        return ("tiled", BM, BN, BKR, case.transb, 1)
    return {"dma": ("tiled", BM, BN, 16, 0, 0), "tr": ("tiled", BM, BN, BKR, 1, 0), "edge": ("tiled", BM, BN, BKR, 0, 1),
            "edget": ("tiled", BM, BN, BKR, 1, 1)}[parts[1]]


def plan_code(launch):
    """a launch of _lib.linear_plan without its column range: the kernel instantiation"""
    return (launch[0],) + tuple(launch[3:])


# ---- operand layout -----------------------------------------------------------------------------------------------------------------
def _r4(n):
    return (n + 3) // 4 * 4


Layout = collections.namedtuple("Layout", "ldx xoff sx xsize ldw woff sw wsize ldy yoff sy ysize ldr sr rsize ldm msize")


def layout(c):
    """row strides, batch strides, offsets of the first element and buffer sizes, all in floats"""
    odd = c.lay == "oddld"
    off = 1 if c.lay == "off" else 0
    wr, wc = (c.N, c.K) if c.transb else (c.K, c.N)
    ldx = _r4(c.K) + (5 if odd else 4)
    ldw = _r4(wc) + (5 if odd else 4)
    xoff, woff = (0 if odd else 4) + off, off
    sx = c.M * ldx + 8
    sw = 0 if c.shared else wr * ldw + 12
    yodd = odd or c.lay == "yodd"
    ldy = _r4(c.N) + (9 if yodd else 8)
    rows = c.M + 2 * GUARD
    sy = rows * ldy
    yoff = GUARD * ldy + (3 if yodd else 4)
    ldr = _r4(c.N) + (5 if odd else 4)
    sr = c.M * ldr + 16
    ldm = _r4(c.N) + (13 if odd else 12)
    return Layout(ldx, xoff, sx, c.batch * sx + 16, ldw, woff, sw, (1 if c.shared else c.batch) * (wr * ldw + 12) + 16, ldy, yoff, sy,
                  c.batch * sy, ldr, sr, c.batch * sr + 16, ldm, c.M * ldm + 16)


FAKE = dict(x=0x10000000, w=0x20000000, y=0x30000000, r1=0x40000000, r2=0x50000000, m=0x60000000, b=0x70000000, sc=0x71000000,
            sh=0x72000000)


def plan_args(c, base=None):
    """the arguments of dispu_linear_plan for a case; `base`: buffer name -> address (default: made-up 16-byte aligned addresses --
    the plan looks at NULL-ness and alignment only)"""
    base = FAKE if base is None else base
    lo = layout(c)
    mptr, mcols = None, 0
    if c.mask is not None:
        mptr, mcols = (base["m"] if c.mask[0] == "ptr" else None), c.mask[1]
    bn = c.entry == "bn"
    return (c.batch, c.M, c.K, c.N, base["x"] + 4 * lo.xoff, lo.ldx, lo.sx, base["w"] + 4 * lo.woff, lo.ldw, lo.sw, c.transb,
            base["b"] if c.bias else None, base["sc"] if bn else None, base["sh"] if bn else None, c.act, base["y"] + 4 * lo.yoff, lo.ldy, lo.sy,
            base["r1"] if c.res & 1 else None, lo.ldr, lo.sr, base["r2"] if c.res & 2 else None, lo.ldr, lo.sr, mptr, lo.ldm, mcols)


# ---- data and references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def product(batch, M, K, N, shared):
    """x [batch, M, K], w [batch or 1, K, N] and the pinned ascending-k fmaf chain x . w (oracle/mlp_oracle.c) -- computed once per
    shape and shared by every case on it; read-only."""
    from oracle import generator as OG
    rng = np.random.default_rng([batch, M, K, N, shared])
    x = rng.standard_normal((batch, M, K)).astype(np.float32)
    w = (rng.standard_normal((1 if shared else batch, K, N)) * 0.25).astype(np.float32)
    y = np.stack([OG.linear(x[z], w[0 if shared else z], None, relu=False) for z in range(batch)])
    for a in (x, w, y):
        a.setflags(write=False)
    return x, w, y


def operands(c):
    """the epilogue operands of a case (deterministic): bias, scale, shift [N]; r1, r2 [batch, M, N]; mask [M, N + 8]"""
    rng = np.random.default_rng([c.batch, c.M, c.K, c.N, 77])
    bias = rng.standard_normal(c.N).astype(np.float32)
    scale = (1 + 0.3 * rng.standard_normal(c.N)).astype(np.float32)
    shift = rng.standard_normal(c.N).astype(np.float32)
    r1 = rng.standard_normal((c.batch, c.M, c.N)).astype(np.float32)
    r2 = rng.standard_normal((c.batch, c.M, c.N)).astype(np.float32)
    mk = np.maximum(rng.standard_normal((c.M, c.N + 8)), 0).astype(np.float32)           # a ReLU output: half of it exact zeros
    mk[rng.random(mk.shape) < 0.05] = -0.0
    mk[rng.random(mk.shape) < 0.05] = -1.5
    return bias, scale, shift, r1, r2, mk


def expected(c):
    """fp32 replay of the kernel's epilogue on the bit-exact chain: bias, [BatchNorm fold], ReLU, + R1, + R2, mask.
    Returns (want fp32, None) for the bit-exact cases and (want float64, (bound, fused fp32, unfused fp32)) for the BatchNorm fold,
    whose v * scale + shift may or may not be contracted: float64 on the bit-exact y = chain + bias, bound 2^-22 (|y sc| + |sh| + |R1|
    + |R2|) = four fp32 roundings, each at most 2^-24 of a magnitude that sum dominates."""
    _, _, y = product(c.batch, c.M, c.K, c.N, c.shared)
    bias, scale, shift, r1, r2, mk = operands(c)
    f32 = np.float32
    v = y + bias if c.bias else y.copy()
    lo = f32(0) if c.act else f32(-np.inf)
    if c.entry == "bn":
        v64 = v.astype(np.float64)
        ref = np.maximum(v64 * scale + shift, lo)
        fused = np.maximum((v64 * scale.astype(np.float64) + shift).astype(f32), lo)
        unfused = np.maximum((v * scale).astype(f32) + shift, lo)
        bound = np.abs(v64 * scale) + np.abs(shift)
        for r in ([r1] if c.res & 1 else []) + ([r2] if c.res & 2 else []):
            ref, fused, unfused, bound = ref + r, fused + r, unfused + r, bound + np.abs(r)
        return ref, (2.0 ** -22 * bound, fused, unfused)
    v = np.maximum(v, lo)
    if c.res & 1:
        v = v + r1
    if c.res & 2:
        v = v + r2
    if c.mask is not None and c.mask[0] == "ptr" and c.mask[1] > 0:
        mc = min(c.mask[1], c.N)
        v[:, :, :mc] = np.where(mk[None, :, :mc] > 0, v[:, :, :mc], f32(0))
    return v.astype(f32), None
