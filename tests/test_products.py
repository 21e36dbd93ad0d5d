"""The dense-product dispatch (dis-pu_amd/products.py) without a device.  The route tables below are written out by hand from the rules:
  use_bf16     bf16 and K > 4 and N > 4 and batch * M * K * N >= bf16_min_macs
  forward/dX   mask = x_bf16 | 4 * y_bf16; 16-bit operands wanted if mask or use_bf16(1, ...).  "stream": wanted, not accumulating, mode bf16,
               bf16_stream, rows % 128 == 0, contraction % 32 == 0, out % 128 == 0, X's row stride and offset multiples of 16 bytes, unit
               inner strides; else "bf16s" if mask (zero offsets, no accumulate: asserted); else "bf16" / "f32" by use_bf16.
               splits of "stream": tiles = (rows / 128) * (out / (256 if out % 256 == 0 else 128)); from 1, doubled while tiles < 192, Y not
               bf16-stored, splits < 8, tiles * splits < 256, contraction % (64 * splits) == 0 and contraction // (2 * splits) >= 256
  TN           mask = x_bf16 | 2 * z_bf16; bf = use_bf16(batch, ...) or mask.  "stream": bf, bf16_stream, batch 1, mask 0 or 3, K % 128 == 0,
               N % 128 == 0, offsets 0 and a non-zero answer of the stream's size query; else "bf16s" if mask, "bf16" if bf, "f32".
               scratch = max(the family's query, the stream's)
  grouped      group_reduce and wgrad and batch == 1 and (side stream or key == "main")
Then a Products whose library, allocation and synchronize are recorders issues, per route, exactly the expected entries on CPU tensors."""
import ctypes

import pytest
import torch

from dispu_amd.products import Linear, Products, Tn, Y_BF16, Z_BF16, linear_route, storage_mask, tn_grouped, tn_route, use_bf16
from test_schedule import Recorded as RecordedSchedule

DEFAULT = 1.5e9


def lin(M, K, N, xb=False, yb=False, ldx=None, xoff=0, yoff=0, inner=(1, 1, 1), acc=False, mode=True, stream=True, macs=0.0):
    return linear_route(mode, stream, macs, M, K, N, xb, yb, K if ldx is None else ldx, xoff, yoff, inner, acc)


# (arguments of lin) -> (route, mask, splits).  bf16 mode, bf16_stream on and bf16_min_macs = 0 unless the row says otherwise
LINEAR = [
    # rows
    (dict(M=127, K=256, N=256), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=256), ("stream", 0, 1)),             # one tile; 256 // 2 = 128 < 256: no split
    (dict(M=129, K=256, N=256), ("bf16", 0, 1)),
    (dict(M=256, K=256, N=256), ("stream", 0, 1)),
    (dict(M=384, K=256, N=256), ("stream", 0, 1)),
    (dict(M=192, K=256, N=256), ("bf16", 0, 1)),               # rm of (2, 24)
    # contraction
    (dict(M=128, K=31, N=128), ("bf16", 0, 1)),
    (dict(M=128, K=32, N=128), ("stream", 0, 1)),
    # out width
    (dict(M=128, K=256, N=127), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128), ("stream", 0, 1)),
    (dict(M=128, K=256, N=384), ("stream", 0, 1)),
    # X's row stride / column offset: 8 bytes off and 16 bytes off, at 4 and at 2 bytes per element
    (dict(M=128, K=256, N=128, ldx=258), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128, ldx=260), ("stream", 0, 1)),
    (dict(M=128, K=256, N=128, ldx=480, xoff=2), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128, ldx=480, xoff=4), ("stream", 0, 1)),
    (dict(M=128, K=256, N=128, xb=True, ldx=260), ("bf16s", 1, 1)),
    (dict(M=128, K=256, N=128, xb=True, ldx=264), ("stream", 1, 1)),
    (dict(M=128, K=256, N=128, xb=True, ldx=480, xoff=4), AssertionError),      # off the stream, and "bf16s" takes no column offset
    (dict(M=128, K=256, N=128, xb=True, ldx=480, xoff=8), ("stream", 1, 1)),
    (dict(M=128, K=256, N=128, yoff=64), ("stream", 0, 1)),                      # the output's offset is free
    (dict(M=127, K=256, N=128, yb=True, yoff=64), AssertionError),
    # inner strides of X, Y, W
    (dict(M=128, K=256, N=128, inner=(2, 1, 1)), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128, inner=(1, 2, 1)), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128, inner=(1, 1, 2)), ("bf16", 0, 1)),
    # storage
    (dict(M=128, K=256, N=128, yb=True), ("stream", 4, 1)),
    (dict(M=128, K=256, N=128, xb=True, yb=True), ("stream", 5, 1)),
    (dict(M=64, K=256, N=128, xb=True), ("bf16s", 1, 1)),
    (dict(M=64, K=256, N=128, yb=True), ("bf16s", 4, 1)),
    (dict(M=64, K=256, N=128, xb=True, yb=True), ("bf16s", 5, 1)),
    # accumulate (dX)
    (dict(M=128, K=256, N=128, acc=True), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128, acc=True, macs=DEFAULT), ("f32", 0, 1)),
    (dict(M=128, K=256, N=128, acc=True, xb=True), AssertionError),
    # bf16_stream off
    (dict(M=128, K=256, N=128, stream=False), ("bf16", 0, 1)),
    (dict(M=128, K=256, N=128, stream=False, xb=True), ("bf16s", 1, 1)),
    # dtype f32
    (dict(M=128, K=256, N=128, mode=False), ("f32", 0, 1)),
    (dict(M=8192, K=2048, N=256, mode=False, macs=DEFAULT), ("f32", 0, 1)),
    # narrow layers stay fp32
    (dict(M=128, K=3, N=128), ("f32", 0, 1)),
    (dict(M=8192, K=64, N=3), ("f32", 0, 1)),
    (dict(M=128, K=4, N=128), ("f32", 0, 1)),
    (dict(M=128, K=5, N=5), ("bf16", 0, 1)),
    # bf16_min_macs: 8192 * 2048 * 256 = 4.29e9, 1024 * 2048 * 256 = 5.4e8, 8192 * 128 * 128 = 1.3e8
    (dict(M=8192, K=2048, N=256, macs=DEFAULT), ("stream", 0, 4)),
    (dict(M=1024, K=2048, N=256, macs=DEFAULT), ("f32", 0, 1)),
    (dict(M=8192, K=128, N=128, macs=DEFAULT), ("f32", 0, 1)),
    (dict(M=8192, K=128, N=128, macs=DEFAULT, xb=True), ("stream", 1, 1)),       # bf16-stored operands: 16-bit whatever the threshold
    (dict(M=8192, K=128, N=128, macs=DEFAULT, yb=True), ("stream", 4, 1)),
    (dict(M=8192, K=2048, N=256, macs=1e12), ("f32", 0, 1)),
    (dict(M=8192, K=2048, N=256, macs=1e12, mode=False), ("f32", 0, 1)),
    (dict(M=5859, K=1000, N=256, macs=DEFAULT), ("f32", 0, 1)),                  # 1 499 904 000 multiply-adds
    (dict(M=5860, K=1000, N=256, macs=DEFAULT), ("bf16", 0, 1)),                 # 1 500 160 000
    # split counts
    (dict(M=8192, K=2048, N=256), ("stream", 0, 4)),            # 64 tiles: 1 -> 2 -> 4, then 64 * 4 = 256 is not < 256
    (dict(M=1024, K=2048, N=256), ("stream", 0, 8)),            # 8 tiles: 1 -> 2 -> 4 -> 8 (2048 // 8 = 256), capped at 8
    (dict(M=1024, K=1024, N=256), ("stream", 0, 4)),            # 1024 // 8 = 128 < 256 stops at 4
    (dict(M=8192, K=256, N=256), ("stream", 0, 1)),             # contraction too short: 256 // 2 = 128
    (dict(M=32768, K=2048, N=256), ("stream", 0, 1)),           # 256 tiles
    (dict(M=8192, K=2048, N=256, yb=True), ("stream", 4, 1)),   # Y is bf16-stored
    (dict(M=1024, K=2048, N=256, xb=True, yb=True), ("stream", 5, 1)),
    (dict(M=1024, K=2048, N=256, xb=True), ("stream", 1, 8)),   # X's storage does not matter
    (dict(M=128, K=512, N=128), ("stream", 0, 2)),              # 512 // 4 = 128 stops at 2
    (dict(M=128, K=544, N=128), ("stream", 0, 1)),              # 544 = 17 * 32: no multiple of 64
    (dict(M=128, K=576, N=128), ("stream", 0, 2)),              # 576 = 9 * 64: no multiple of 128
    (dict(M=24576, K=2048, N=128), ("stream", 0, 1)),           # 192 tiles: not < 192
    (dict(M=24448, K=2048, N=128), ("stream", 0, 2)),           # 191 tiles: one doubling, 382 >= 256
    (dict(M=16384, K=2048, N=128), ("stream", 0, 2)),           # 128 tiles: 128 * 2 = 256 stops
    (dict(M=16256, K=2048, N=128), ("stream", 0, 4)),           # 127 tiles: 254 < 256, one more
    (dict(M=1024, K=2048, N=384), ("stream", 0, 8)),            # 384: 128-wide tiles, 24 of them
]


@pytest.mark.parametrize("kw,want", LINEAR, ids=[" ".join("%s=%s" % i for i in c[0].items()) for c in LINEAR])
def test_linear_route_table(kw, want):
    if want is AssertionError:
        with pytest.raises(AssertionError):
            lin(**kw)
        return
    got = lin(**kw)
    assert got == Linear(*want)
    assert got.sto == storage_mask(kw.get("xb", False), kw.get("yb", False), Y_BF16)


def test_use_bf16_and_masks():
    assert (Y_BF16, Z_BF16) == (4, 2)
    assert [storage_mask(x, o, b) for x, o, b in ((0, 0, 4), (1, 0, 4), (0, 1, 4), (1, 1, 4), (0, 1, 2), (1, 1, 2))] == [0, 1, 4, 5, 2, 3]
    assert use_bf16(True, DEFAULT, 1, 8192, 2048, 256) is True and use_bf16(False, 0.0, 1, 8192, 2048, 256) is False
    assert use_bf16(True, DEFAULT, 4, 256, 64, 256) is False and use_bf16(True, 0.0, 4, 256, 64, 256) is True
    assert use_bf16(True, 1.6e9, 1, 1024, 1024, 1024) is False and use_bf16(True, 1.6e9, 2, 1024, 1024, 1024) is True     # the batch counts
    assert use_bf16(True, 0.0, 1, 8192, 4, 256) is False and use_bf16(True, 0.0, 1, 8192, 256, 4) is False


def sizes(f32, bf16, stream):
    table = {"dispu_linear_tn_scratch_floats": f32, "dispu_linear_tn_bf16_scratch_floats": bf16, "dispu_linear_tn_bf16_stream_scratch_floats": stream}
    return lambda name, *shape: table[name]


Q = sizes(100, 200, 300)             # the three size queries
Q_REFUSED = sizes(100, 200, 0)       # the streaming kernel refuses
Q_SMALL = sizes(100, 200, 50)        # ... asks for less than the family


def tn(batch, M, K, N, xb=False, zb=False, xoff=0, zoff=0, mode=True, stream=True, macs=0.0, q=Q):
    return tn_route(mode, stream, macs, batch, M, K, N, xb, zb, xoff, zoff, q)


TN = [
    (dict(batch=1, M=8192, K=128, N=128), ("stream", 0, 300)),
    (dict(batch=1, M=8192, K=128, N=128, xb=True, zb=True), ("stream", 3, 300)),
    (dict(batch=1, M=8192, K=128, N=128, xb=True), ("bf16s", 1, 200)),            # mixed storage: not the streaming kernel's
    (dict(batch=1, M=8192, K=128, N=128, zb=True), ("bf16s", 2, 200)),
    (dict(batch=2, M=8192, K=128, N=128), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=64, N=128), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=128, N=64), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=128, N=192), ("bf16", 0, 200)),
    (dict(batch=1, M=8100, K=128, N=128), ("stream", 0, 300)),                    # no rule on the rows
    (dict(batch=1, M=8192, K=128, N=128, xoff=64), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=128, N=128, zoff=64), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=128, N=128, xb=True, zb=True, xoff=64), AssertionError),
    (dict(batch=1, M=8192, K=128, N=128, zb=True, zoff=64), AssertionError),
    (dict(batch=1, M=8192, K=128, N=128, stream=False), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=128, N=128, stream=False, xb=True, zb=True), ("bf16s", 3, 200)),
    (dict(batch=1, M=8192, K=128, N=128, q=Q_REFUSED), ("bf16", 0, 200)),
    (dict(batch=1, M=8192, K=128, N=128, xb=True, zb=True, q=Q_REFUSED), ("bf16s", 3, 200)),
    (dict(batch=1, M=8192, K=128, N=128, q=Q_SMALL), ("stream", 0, 200)),         # scratch: the larger of the two answers
    (dict(batch=1, M=8192, K=128, N=128, mode=False), ("f32", 0, 100)),
    (dict(batch=1, M=8192, K=2, N=256), ("f32", 0, 100)),                         # duplicate_up's grid code
    (dict(batch=1, M=8192, K=128, N=3), ("f32", 0, 100)),
    (dict(batch=1, M=8192, K=128, N=128, macs=DEFAULT), ("f32", 0, 100)),         # 1.3e8 multiply-adds
    (dict(batch=1, M=8192, K=128, N=128, macs=DEFAULT, xb=True, zb=True), ("stream", 3, 300)),
    (dict(batch=1, M=8192, K=2048, N=256, macs=DEFAULT), ("stream", 0, 300)),
    (dict(batch=1, M=8192, K=2048, N=256, macs=1e12), ("f32", 0, 100)),
    (dict(batch=4, M=256, K=256, N=64, macs=DEFAULT), ("f32", 0, 100)),           # the gemm attention path's dK / dV at (4, 64)
    (dict(batch=4, M=256, K=256, N=64), ("bf16", 0, 200)),
]


@pytest.mark.parametrize("kw,want", TN, ids=[" ".join("%s=%s" % i for i in c[0].items() if i[0] != "q") + (" q%d" % n) for n, c in enumerate(TN)])
def test_tn_route_table(kw, want):
    if want is AssertionError:
        with pytest.raises(AssertionError):
            tn(**kw)
        return
    assert tn(**kw) == Tn(*want)


def test_tn_grouped_needs_all_of_its_inputs():
    assert tn_grouped(True, True, 1, True, "dw0") is True             # on a side stream, whatever the schedule's key
    assert tn_grouped(True, True, 1, True, "aux0") is True
    assert tn_grouped(True, True, 1, False, "main") is True           # on the main stream
    assert tn_grouped(True, True, 1, False, "aux0") is False          # inside a branch: that stream is not joined
    assert tn_grouped(False, True, 1, True, "main") is False
    assert tn_grouped(True, False, 1, True, "main") is False
    assert tn_grouped(True, True, 2, True, "main") is False


# ------------------------------------------------------------------------------------------------ recorders ----
ST = 0x1000


class Lib(object):
    """every entry is recorded as (name, arguments) with pointers as integers (None: null) and answers 0; size queries answer 4096"""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if "scratch_floats" in name:
            return lambda *a: 4096

        def fn(*args):
            self.log.append((name,) + tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args))
            return 0
        return fn


class Group(object):
    def __init__(self, log, real):
        self.log, self.real = log, real

    def commit(self):
        self.log.append(("commit",))
        self.real.commit()


class Sched(RecordedSchedule):
    def __init__(self, **kw):
        RecordedSchedule.__init__(self, **kw)
        self.st = ctypes.c_void_p(ST)

    def reduce_slot(self, st, out_ptr, bias_ptr):
        slot, g = RecordedSchedule.reduce_slot(self, st, out_ptr, bias_ptr)
        self.log.append(("slot", st.value, out_ptr, bias_ptr, slot.value))
        return slot, Group(self.log, g)


class Recorded(Products):
    _floats = staticmethod(Q)

    def __init__(self, bf16=True, **kw):
        self.sync = self.dropped = 0
        Products.__init__(self, "cpu", Sched(**kw), bf16, self._drop)
        self.bf16_min_macs = 0.0
        self.lib = Lib(self.sched.log)

    def _drop(self):
        assert self.sync == self.dropped + 1                 # synchronize first
        self.dropped += 1

    def _L(self):
        return self.lib

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype)

    def _synchronize(self):
        self.sync += 1

    def calls(self):
        """the library calls and the bracket of a grouped product since the last look"""
        out = [e for e in self.sched.log if e[0].startswith("dispu_") or e[0] in ("slot", "commit")]
        del self.sched.log[:]
        return out


def T(rows, cols, dtype=torch.float32):
    return torch.empty((rows, cols), dtype=dtype)


def at(t, off=0):
    return t.data_ptr() + t.element_size() * off


BF = torch.bfloat16


def test_products_construction_touches_nothing():
    p = Products("cuda:0", None, True, None)
    assert (p.bf16, p.bf16_stream, p.bf16_min_macs, p.packs, p.scratch) == (True, True, 1.5e9, {}, {})


def test_library_hook_is_looked_up_per_call(monkeypatch):
    """tests count a step's launches through a proxy set on _lib.tape_lib (train_step_checks.recording): the dispatch must go through it"""
    from dispu_amd import _lib
    monkeypatch.setattr(_lib, "tape_lib", lambda: "proxy")
    assert Products._L() == "proxy" and Products("cpu", None, True, None)._L() == "proxy"


def test_trainer_forwards_its_switches_and_holds_products_without_a_cycle():
    import gc
    import weakref
    from dispu_amd.train import Trainer
    tr = Trainer(params=None, dtype="bf16")
    assert (tr.bf16_stream, tr.bf16_min_macs, tr.prod.bf16) == (True, 1.5e9, True) and tr._scratch is tr.prod.scratch and tr.prod.sched is tr.sched
    tr.bf16_stream, tr.bf16_min_macs = False, 5e8
    assert (tr.prod.bf16_stream, tr.prod.bf16_min_macs) == (False, 5e8)
    assert tr.prod.use_bf16(1, 1024, 2048, 256) and not tr.prod.use_bf16(1, 512, 2048, 256) and not Trainer(params=None).prod.bf16
    tr.prod._invalidate()                                    # reaches the Trainer's _invalidate_recordings (nothing recorded: no device access)
    enabled, ref = gc.isenabled(), weakref.ref(tr)
    gc.disable()
    try:
        del tr
        assert ref() is None                                 # freed by its reference count: its device memory does not wait for the collector
    finally:
        if enabled:
            gc.enable()


def test_stream_route_calls_and_pack_reuse():
    p = Recorded()
    X, W, b, Y = T(128, 512), T(512, 128), T(1, 128), T(128, 128)
    p.linear(128, 512, 128, X, 0, W, 0, 0, b, 1, Y, 0)
    (bt,), (parts,) = p.packs.values(), p.scratch.values()
    assert list(p.packs) == [(at(W), 512, 128, 1)] and bt.shape == (128, 512) and bt.dtype == BF and list(p.scratch) == ["main"]
    assert parts.numel() == 1 << 20 and parts.dtype == torch.float32
    two_splits = [("dispu_bf16_pack", 512, 128, at(W), 128, 1, at(bt), ST),
                  ("dispu_linear_bf16_stream", 128, 512, 128, at(X), 512, 0, at(bt), 512, None, 0, at(parts), 128, 0, 2, 128 * 128, ST),
                  ("dispu_linear_splitk_finish", 128, 128, 2, at(parts), 128 * 128, at(b), 1, at(Y), 128, ST)]
    assert p.calls() == two_splits
    p.linear(128, 512, 128, X, 0, W, 0, 0, b, 1, Y, 0)                      # the same weight again: the same image
    assert p.calls() == two_splits and len(p.packs) == 1
    # one split, bf16-stored X and Y, column offsets, no bias: a slice of a wide weight, a column slice of wide activations
    Xb, Wide, Yb = T(128, 96, BF), T(64, 256), T(128, 384, BF)
    p.linear(128, 32, 128, Xb, 8, Wide, 32 * 256 + 128, 0, None, 0, Yb, 256)
    bt2 = p.packs[(at(Wide, 32 * 256 + 128), 32, 128, 1)]
    assert p.calls() == [("dispu_bf16_pack", 32, 128, at(Wide, 32 * 256 + 128), 256, 1, at(bt2), ST),
                         ("dispu_linear_bf16_stream", 128, 32, 128, at(Xb, 8), 96, 1, at(bt2), 32, None, 0, at(Yb, 256), 384, 1, 1, 0, ST)]
    # dX = dZ . W^T on the same weight: packed from W itself (never from the W^T copy), an image of its own
    dZ, dX, WT = T(128, 128), T(128, 512), T(128, 512)
    p.linear(128, 128, 512, dZ, 0, W, 0, 1, None, 0, dX, 0, False, WT)
    bt3 = p.packs[(at(W), 128, 512, 0)]
    assert bt3.shape == (512, 128) and len(p.packs) == 3 and len({at(t) for t in p.packs.values()}) == 3
    assert p.calls() == [("dispu_bf16_pack", 512, 128, at(W), 128, 0, at(bt3), ST),
                         ("dispu_linear_bf16_stream", 128, 128, 512, at(dZ), 128, 0, at(bt3), 128, None, 0, at(dX), 512, 0, 1, 0, ST)]
    for key in ((at(W), 512, 128, 1), (at(W) + 4, 512, 128, 1), (at(W), 256, 128, 1), (at(W), 512, 256, 1)):     # address, K, N, transpose
        assert (key in p.packs) == (key == (at(W), 512, 128, 1))
    assert (p.sync, p.dropped) == (0, 0)


def test_other_routes_calls():
    p = Recorded()
    X, Xb, W, b, Y, Yb = T(64, 32), T(64, 32, BF), T(32, 32), T(1, 32), T(64, 48), T(64, 32, BF)
    p.linear(64, 32, 32, Xb, 0, W, 0, 0, b, 1, Yb, 0)                       # bf16s, mask 5
    p.linear(64, 32, 16, X, 8, W, 16, 0, b, 1, Y, 24)                       # bf16: fp32 storage, offsets
    p.bf16_min_macs = 1.5e9
    p.linear(64, 32, 16, X, 8, W, 16, 0, b, 1, Y, 24)                       # f32: under the threshold
    assert p.calls() == [
        ("dispu_linear_bf16s", 1, 64, 32, 32, at(Xb), 32, 0, at(W), 32, 0, 0, at(b), 1, at(Yb), 32, 0, None, 0, 0, 5, ST),
        ("dispu_linear_bf16", 1, 64, 32, 16, at(X, 8), 32, 0, at(W, 16), 32, 0, 0, at(b), 1, at(Y, 24), 48, 0, None, 0, 0, None, 0, 0, ST),
        ("dispu_linear", 1, 64, 32, 16, at(X, 8), 32, 0, at(W, 16), 32, 0, 0, at(b), 1, at(Y, 24), 48, 0, None, 0, 0, None, 0, 0, ST)]
    # dX: W as [out][contraction] (transb 1), or the W^T copy untransposed; accumulating: dX is its own residual
    p.bf16_min_macs = 0.0
    dZ, dZb, dX, Wl, WT = T(64, 32), T(64, 32, BF), T(64, 48), T(16, 32), T(32, 16)
    p.linear(64, 32, 16, dZ, 0, Wl, 0, 1, None, 0, dX, 8)
    p.linear(64, 32, 16, dZ, 0, Wl, 0, 1, None, 0, dX, 8, False, WT)
    p.linear(64, 32, 16, dZ, 0, Wl, 0, 1, None, 0, dX, 8, True, WT)
    p.linear(64, 32, 16, dZb, 0, Wl, 0, 1, None, 0, dX, 0, False, WT)
    assert p.calls() == [
        ("dispu_linear_bf16", 1, 64, 32, 16, at(dZ), 32, 0, at(Wl), 32, 0, 1, None, 0, at(dX, 8), 48, 0, None, 0, 0, None, 0, 0, ST),
        ("dispu_linear_bf16", 1, 64, 32, 16, at(dZ), 32, 0, at(WT), 16, 0, 0, None, 0, at(dX, 8), 48, 0, None, 0, 0, None, 0, 0, ST),
        ("dispu_linear_bf16", 1, 64, 32, 16, at(dZ), 32, 0, at(WT), 16, 0, 0, None, 0, at(dX, 8), 48, 0, at(dX, 8), 48, 0, None, 0, 0, ST),
        ("dispu_linear_bf16s", 1, 64, 32, 16, at(dZb), 32, 0, at(WT), 16, 0, 0, None, 0, at(dX), 48, 0, None, 0, 0, 1, ST)]
    # an accumulating dX at a shape the streaming kernel would take stays off it
    dZ2, W2, dX2 = T(128, 128), T(128, 128), T(128, 128)
    p.linear(128, 128, 128, dZ2, 0, W2, 0, 1, None, 0, dX2, 0, True)
    assert [c[0] for c in p.calls()] == ["dispu_linear_bf16"] and not p.packs and not p.scratch
    # the batched products of the gemm attention path
    p.batched(4, 256, 64, 256, "rest", ST)
    p.bf16_min_macs = 1.5e9
    p.batched(4, 256, 64, 256, "rest", ST)
    assert p.calls() == [("dispu_linear_bf16", 4, 256, 64, 256, "rest", ST), ("dispu_linear", 4, 256, 64, 256, "rest", ST)]
    f = Recorded(bf16=False)
    f.linear(128, 512, 128, T(128, 512), 0, T(512, 128), 0, 0, None, 0, T(128, 128), 0)
    assert [c[0] for c in f.calls()] == ["dispu_linear"]


def test_tn_calls_per_route():
    p = Recorded(overlap_dw=False)
    X, Xb, Z, Zb, out, db = T(256, 128), T(256, 128, BF), T(256, 256), T(256, 128, BF), T(128, 384), T(1, 128)
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 256, 0, out, 128, 384, 0, 1, dbias=db)            # stream, mask 0
    p.tn(1, 256, 128, 128, Xb, 0, 128, 0, Zb, 0, 128, 0, out, 0, 384, 0, 0)                      # stream, mask 3
    p.tn(1, 256, 128, 128, Xb, 0, 128, 0, Z, 0, 256, 0, out, 0, 384, 0, 1, dbias=db)             # bf16s, mask 1
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 128, 256, 0, out, 0, 384, 0, 1)                      # bf16: Z's offset
    p.tn(2, 128, 128, 64, X, 64, 128, 7, Z, 0, 256, 9, out, 0, 384, 11, 0)                       # bf16, batched
    p.bf16_min_macs = 1.5e9
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 256, 0, out, 0, 384, 0, 1)                        # f32
    (sc,) = p.scratch.values()
    n = sc.numel()
    assert list(p.scratch) == ["main"] and n == 1 << 20
    assert p.calls() == [
        ("dispu_linear_tn_bf16_stream", 256, 128, 128, at(X), 128, at(Z), 256, 0, at(out, 128), 384, 1, at(db), at(sc), n, ST),
        ("dispu_linear_tn_bf16_stream", 256, 128, 128, at(Xb), 128, at(Zb), 128, 3, at(out), 384, 0, None, at(sc), n, ST),
        ("dispu_linear_tn_bf16s", 1, 256, 128, 128, at(Xb), 128, 0, at(Z), 256, 0, at(out), 384, 0, 1, at(db), at(sc), n, 1, ST),
        ("dispu_linear_tn_bf16", 1, 256, 128, 128, at(X), 128, 0, at(Z, 128), 256, 0, at(out), 384, 0, 1, None, at(sc), n, ST),
        ("dispu_linear_tn_bf16", 2, 128, 128, 64, at(X, 64), 128, 7, at(Z), 256, 9, at(out), 384, 11, 0, None, at(sc), n, ST),
        ("dispu_linear_tn", 1, 256, 128, 128, at(X), 128, 0, at(Z), 256, 0, at(out), 384, 0, 1, None, at(sc), n, ST)]


def test_grouped_tn_brackets_the_product():
    p = Recorded(defer_side=False)
    s = p.sched
    X, Z, out, db = T(256, 128), T(256, 128), T(128, 128), T(1, 128)
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 128, 0, out, 0, 128, 0, 1, dbias=db, side=True, wgrad=True)
    dw0 = s.side_streams[0].cuda_stream
    sc = p.scratch[("tn", at(out), 128, 128)]                                                     # a buffer of this product's own
    got = p.calls()
    slot = got[0][4]
    assert got == [("slot", dw0, at(out), at(db), slot), ("dispu_tn_defer", slot), ("dispu_linear_tn_bf16_stream", 256, 128, 128, at(X), 128,
                   at(Z), 128, 0, at(out), 128, 1, at(db), at(sc), sc.numel(), dw0), ("commit",)]
    # on the main stream: grouped as well; inside a branch, without wgrad, with group_reduce off or side streams off: the stream's scratch
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 128, 0, out, 0, 128, 0, 1, wgrad=True)
    assert [c[0] for c in p.calls()] == ["slot", "dispu_tn_defer", "dispu_linear_tn_bf16_stream", "commit"]
    with s.branch(0):
        p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 128, 0, out, 0, 128, 0, 1, wgrad=True)
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 128, 0, out, 0, 128, 0, 1, side=True)
    s.group_reduce = False
    p.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 128, 0, out, 0, 128, 0, 1, side=True, wgrad=True)
    assert [(c[0], c[-1]) for c in p.calls()] == [("dispu_linear_tn_bf16_stream", s._aux[0][0].cuda_stream),
                                                   ("dispu_linear_tn_bf16_stream", s.side_streams[1].cuda_stream), ("dispu_linear_tn_bf16_stream", dw0)]
    assert sorted(map(str, p.scratch)) == sorted(map(str, [("tn", at(out), 128, 128), "aux0", "dw1", "dw0"]))
    # deferral on: nothing is launched before the schedule flushes
    d = Recorded()
    d.tn(1, 256, 128, 128, X, 0, 128, 0, Z, 0, 128, 0, out, 0, 128, 0, 1, side=True, wgrad=True)
    assert not d.calls()
    d.sched.flush()
    assert [c[0] for c in d.calls()] == ["slot", "dispu_tn_defer", "dispu_linear_tn_bf16_stream", "commit"]


def test_scratch_regrow_rule_and_act_bias_grad():
    p = Recorded()
    a = p.scratch_floats(100)
    assert a.numel() == 1 << 20 and p.scratch_floats(1 << 20) is a and p.scratch_floats(5, "edge1") is not a
    assert (p.sync, p.dropped) == (0, 0)                                    # requests that fit, a new key: never
    b = p.scratch_floats((1 << 20) + 1)
    assert b is not a and b.numel() == (1 << 20) + 1 and (p.sync, p.dropped) == (1, 1)      # outgrown: synchronize, then invalidate, once
    assert p.scratch_floats(1 << 20) is b and (p.sync, p.dropped) == (1, 1)
    dY, Y, dbias = T(64, 48), T(64, 48), T(1, 48)
    p.act_bias_grad(64, 48, dY, 0, Y, 0, 1, dY, 0, None)
    p.act_bias_grad(64, 16, dY, 8, None, 0, 0, None, 0, dbias)
    assert p.calls() == [("dispu_act_bias_grad", 64, 48, at(dY), 48, at(Y), 48, 1, at(dY), 48, None, 1, at(b), b.numel(), ST),
                         ("dispu_act_bias_grad", 64, 16, at(dY, 8), 48, None, 0, 0, None, 0, at(dbias), 1, at(b), b.numel(), ST)]
