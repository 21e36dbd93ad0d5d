"""Products (dis-pu_amd/products.py) on the device: for every route, at the smallest shape that reaches it, what Products launches equals
bit for bit what the library entry gives when it is called directly, with arguments written out by hand, on the same inputs.  (Which
entry a shape goes to is held to hand-written tables on the CPU: tests/test_products.py.)  Scratch buffers of the direct calls have the
size Products gives its own (1 << 20 floats: a plan may depend on it)."""
import pytest
import torch

from dispu_amd import _lib
from dispu_amd.products import Products
from dispu_amd.schedule import StepSchedule

BF, F32 = torch.bfloat16, torch.float32
SC = 1 << 20


def products(dev, bf16=True, **sched_kw):
    sched = StepSchedule(dev, **sched_kw)
    sched.st = _lib.stream_ptr(dev)
    p = Products(dev, sched, bf16, lambda: None)
    p.bf16_min_macs = 0.0
    return p


def rand(dev, seed, *shapes):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(*s, device=dev, generator=g) * (0.1 if i else 1.0) for i, s in enumerate(shapes)]


def ptr(t, off=0):
    return t.data_ptr() + t.element_size() * off if t is not None else None


# (id, M, K, N, X storage, Y storage, X / Y column offsets, act, expected route and splits)
FORWARD = [
    ("stream-1-split", 128, 32, 128, F32, F32, (0, 0), 1, "stream", 1),
    ("stream-2-splits", 128, 512, 128, F32, F32, (0, 0), 1, "stream", 2),
    ("stream-bf16-stored", 128, 512, 128, BF, BF, (0, 0), 1, "stream", 1),
    ("stream-offsets", 128, 64, 128, F32, F32, (8, 128), 0, "stream", 1),
    ("bf16s", 64, 32, 32, BF, F32, (0, 0), 1, "bf16s", 1),
    ("bf16", 64, 32, 32, F32, F32, (4, 16), 1, "bf16", 1),
    ("f32", 64, 32, 32, F32, F32, (4, 16), 1, "f32", 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,M,K,N,xt,yt,offs,act,route,nsp", FORWARD, ids=[c[0] for c in FORWARD])
def test_forward_routes_equal_the_direct_entry(dev, name, M, K, N, xt, yt, offs, act, route, nsp):
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    p = products(dev, bf16=route != "f32")
    xoff, yoff = offs
    x, w, b = rand(dev, M + K + N, (M, K + xoff), (K, N), (1, N))
    x = x.to(xt)
    ldx, ldy = K + xoff, N + yoff
    y, ref = torch.zeros(M, ldy, dtype=yt, device=dev), torch.zeros(M, ldy, dtype=yt, device=dev)
    p.linear(M, K, N, x, xoff, w, 0, 0, b, act, y, yoff)
    xb, yb = int(xt is BF), int(yt is BF)
    if route == "stream":
        assert list(p.packs) == [(w.data_ptr(), K, N, 1)]
        bt = torch.empty(N, K, dtype=BF, device=dev)
        _lib.check(L.dispu_bf16_pack(K, N, ptr(w), N, 1, ptr(bt), st), "pack")
        if nsp == 2:
            parts = torch.empty(SC, device=dev)
            _lib.check(L.dispu_linear_bf16_stream(M, K, N, ptr(x, xoff), ldx, xb, ptr(bt), K, None, 0, ptr(parts), N, 0, 2, M * N, st), "stream")
            _lib.check(L.dispu_linear_splitk_finish(M, N, 2, ptr(parts), M * N, ptr(b), act, ptr(ref, yoff), ldy, st), "finish")
        else:
            _lib.check(L.dispu_linear_bf16_stream(M, K, N, ptr(x, xoff), ldx, xb, ptr(bt), K, ptr(b), act, ptr(ref, yoff), ldy, yb, 1, 0, st), "stream")
    else:
        assert not p.packs
        if route == "bf16s":
            _lib.check(L.dispu_linear_bf16s(1, M, K, N, ptr(x), ldx, 0, ptr(w), N, 0, 0, ptr(b), act, ptr(ref), ldy, 0, None, 0, 0, xb | 4 * yb, st), "bf16s")
        else:
            fn = L.dispu_linear_bf16 if route == "bf16" else L.dispu_linear
            _lib.check(fn(1, M, K, N, ptr(x, xoff), ldx, 0, ptr(w), N, 0, 0, ptr(b), act, ptr(ref, yoff), ldy, 0, None, 0, 0, None, 0, 0, st), route)
    assert (len(p.scratch) == 1) == (nsp == 2)
    torch.cuda.synchronize()
    assert torch.equal(y, ref) and bool((y[:, yoff:].float().abs().sum() > 0).item()) and bool((y[:, :yoff] == 0).all().item())


@pytest.mark.gpu
def test_dx_routes_equal_the_direct_entry(dev):
    """dX = dZ . W^T of a layer [48 -> 32] over 64 rows with and without the W^T copy, accumulating at a shape the streaming kernel
    would take, and on the streaming kernel (packed from W itself although a copy is at hand)."""
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    p = products(dev)
    dz, w = rand(dev, 7, (64, 32), (48, 32))
    wT = w.t().contiguous()
    got = [torch.empty(64, 48, device=dev) for _ in range(2)]
    ref = [torch.empty(64, 48, device=dev) for _ in range(2)]
    p.linear(64, 32, 48, dz, 0, w, 0, 1, None, 0, got[0], 0, False, wT)
    p.linear(64, 32, 48, dz, 0, w, 0, 1, None, 0, got[1], 0)
    _lib.check(L.dispu_linear_bf16(1, 64, 32, 48, ptr(dz), 32, 0, ptr(wT), 48, 0, 0, None, 0, ptr(ref[0]), 48, 0, None, 0, 0, None, 0, 0, st), "dX by W^T")
    _lib.check(L.dispu_linear_bf16(1, 64, 32, 48, ptr(dz), 32, 0, ptr(w), 32, 0, 1, None, 0, ptr(ref[1]), 48, 0, None, 0, 0, None, 0, 0, st), "dX by W")
    dz2, w2, acc0 = rand(dev, 8, (128, 128), (128, 128), (128, 128))
    w2T = w2.t().contiguous()
    acc, acc_ref = acc0.clone(), acc0.clone()
    p.linear(128, 128, 128, dz2, 0, w2, 0, 1, None, 0, acc, 0, True, w2T)
    assert not p.packs                                                               # accumulating: the stream route is not taken
    _lib.check(L.dispu_linear_bf16(1, 128, 128, 128, ptr(dz2), 128, 0, ptr(w2T), 128, 0, 0, None, 0, ptr(acc_ref), 128, 0, ptr(acc_ref), 128, 0,
                                   None, 0, 0, st), "dX +=")
    s, s_ref = torch.empty(128, 128, device=dev), torch.empty(128, 128, device=dev)
    p.linear(128, 128, 128, dz2, 0, w2, 0, 1, None, 0, s, 0, False, w2T)
    assert list(p.packs) == [(w2.data_ptr(), 128, 128, 0)]
    bt = torch.empty(128, 128, dtype=BF, device=dev)
    _lib.check(L.dispu_bf16_pack(128, 128, ptr(w2), 128, 0, ptr(bt), st), "pack")
    _lib.check(L.dispu_linear_bf16_stream(128, 128, 128, ptr(dz2), 128, 0, ptr(bt), 128, None, 0, ptr(s_ref), 128, 0, 1, 0, st), "stream")
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(acc, acc_ref) and torch.equal(s, s_ref)
    assert not torch.equal(acc, acc0) and torch.equal(p.packs[(w2.data_ptr(), 128, 128, 0)], bt)


# (id, M, K, N, X storage, Z storage, mode bf16, expected entry)
TN = [
    ("stream-mask0", 128, 128, 128, F32, F32, True, "dispu_linear_tn_bf16_stream"),
    ("stream-mask3", 128, 128, 128, BF, BF, True, "dispu_linear_tn_bf16_stream"),
    ("bf16s-mask1", 128, 128, 128, BF, F32, True, "dispu_linear_tn_bf16s"),
    ("bf16", 64, 32, 32, F32, F32, True, "dispu_linear_tn_bf16"),
    ("f32", 64, 32, 32, F32, F32, False, "dispu_linear_tn"),
]


def tn_direct(L, entry, M, K, N, x, z, out, db, sc, st):
    sto = int(x.dtype is BF) | 2 * int(z.dtype is BF)
    if entry == "dispu_linear_tn_bf16_stream":
        return L.dispu_linear_tn_bf16_stream(M, K, N, ptr(x), K, ptr(z), N, sto, ptr(out), N, 1, ptr(db), ptr(sc), SC, st)
    if entry == "dispu_linear_tn_bf16s":
        return L.dispu_linear_tn_bf16s(1, M, K, N, ptr(x), K, 0, ptr(z), N, 0, ptr(out), N, 0, 1, ptr(db), ptr(sc), SC, sto, st)
    return getattr(L, entry)(1, M, K, N, ptr(x), K, 0, ptr(z), N, 0, ptr(out), N, 0, 1, ptr(db), ptr(sc), SC, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name,M,K,N,xt,zt,mode,entry", TN, ids=[c[0] for c in TN])
def test_tn_routes_equal_the_direct_entry(dev, name, M, K, N, xt, zt, mode, entry):
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    p = products(dev, bf16=mode)
    x, z, out0, db0 = rand(dev, M + K + N + 1, (M, K), (M, N), (K, N), (1, N))
    x, z = x.to(xt), z.to(zt)
    out, db, out_ref, db_ref = out0.clone(), db0.clone(), out0.clone(), db0.clone()
    p.tn(1, M, K, N, x, 0, K, 0, z, 0, N, 0, out, 0, N, 0, 1, dbias=db)          # not a weight gradient: the product reduces itself
    (sc,) = p.scratch.values()
    assert sc.numel() == SC and not p.sched.reduce_groups
    _lib.check(tn_direct(L, entry, M, K, N, x, z, out_ref, db_ref, torch.empty(SC, device=dev), st), entry)
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref) and torch.equal(db, db_ref) and not torch.equal(out, out0) and not torch.equal(db, db0)


@pytest.mark.gpu
def test_grouped_tn_on_a_side_stream_then_join(dev):
    """a weight gradient on a side stream: the streaming kernel leaves its 8 partial sums of 128 rows to the stream's grouped reduction,
    which join() launches; the result equals the entry reducing itself."""
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    M, K, N = 1024, 128, 128
    assert _lib.linear_tn_bf16_stream_plan(M, K, N, 256, K, 256, N, 0, 256, N, 1, 256, 256, SC).splits == 8
    p = products(dev)
    x, z, out0, db0 = rand(dev, 11, (M, K), (M, N), (K, N), (1, N))
    out, db, out_ref, db_ref = out0.clone(), db0.clone(), out0.clone(), db0.clone()
    torch.cuda.synchronize()
    p.tn(1, M, K, N, x, 0, K, 0, z, 0, N, 0, out, 0, N, 0, 1, dbias=db, side=True, wgrad=True)
    p.sched.join()
    assert list(p.scratch) == [("tn", out.data_ptr(), K, N)] and len(p.sched.reduce_groups) == 1 and len(p.sched.tables) == 1
    _lib.check(tn_direct(L, "dispu_linear_tn_bf16_stream", M, K, N, x, z, out_ref, db_ref, torch.empty(SC, device=dev), st), "direct")
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref) and torch.equal(db, db_ref) and not torch.equal(out, out0)
