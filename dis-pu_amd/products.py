"""Which GEMM entry a dense product of the training step goes to (train.Trainer names the layers and their order, schedule.StepSchedule
decides where and when a launch is submitted).  Two layers:
  * the decision, as pure functions of shapes, storage flags, strides, column offsets, the accumulate flag and the three switches
    (bf16, bf16_stream, bf16_min_macs): use_bf16, linear_route (the forward and the dX product: ONE ladder), tn_route, tn_grouped.
    Nothing is launched or allocated; the results are small immutable records (tests/test_products.py holds them to hand-written tables);
  * Products: the bf16 images of the weights, the per-stream scratch and the launches.  Each launch method asks the pure function
    for its route and issues exactly the calls that route names.
Routes of both products: "stream" (csrc/linear_bf16_stream.hip), "bf16s" (bf16-STORED operands, csrc/linear_bf16.hip), "bf16" (fp32
storage, operands rounded on their way into LDS), "f32"."""
# torch.cuda and the library are touched by the hooks at the head of Products only: a subclass that replaces them with recorders runs
# the whole dispatch on CPU tensors (tests/test_products.py).
import collections
import functools

import torch

from . import _lib

Y_BF16, Z_BF16 = 4, 2        # the storage mask's second bit: the output of a forward / dX product, Z of a TN product (the first operand is bit 0)
Linear = collections.namedtuple("Linear", "route sto splits")      # splits: split-K count of the streaming kernel (1 elsewhere)
Tn = collections.namedtuple("Tn", "route sto need")               # need: scratch floats


def storage_mask(x_bf16, other_bf16, other_bit):
    return (1 if x_bf16 else 0) | (other_bit if other_bf16 else 0)


def use_bf16(bf16, min_macs, batch, M, K, N):
    """bf16 products for this GEMM?  Mixed precision is per product: the narrow 3-wide layers always stay fp32, and so do products
    below `min_macs` multiply-adds -- at 8192 rows the K <= 256 products are launch / prologue-bound and the bf16 kernel (fp32
    operands rounded on their way into LDS) is no faster than the fp32 one, often slower (24 - 29 us vs 15 - 24 us)."""
    return bool(bf16 and K > 4 and N > 4 and float(batch) * M * K * N >= min_macs)


@functools.lru_cache(maxsize=None)
def linear_route(bf16, bf16_stream, min_macs, M, K, N, x_bf16, y_bf16, ldx, xoff, yoff, inner, acc):
    """Y[M, N] (+)= act(X[M, K] . B + bias).  ldx, xoff, yoff: X's row stride and the column offsets, in elements; inner: the inner
    strides of X, Y and W; acc: Y is accumulated into (a dX product)."""
    sto = storage_mask(x_bf16, y_bf16, Y_BF16)
    bf = use_bf16(bf16, min_macs, 1, M, K, N)
    es = 2 if x_bf16 else 4
    if ((sto or bf) and not acc and bf16 and bf16_stream and M % 128 == 0 and K % 32 == 0 and N % 128 == 0
            and (ldx * es) % 16 == 0 and (xoff * es) % 16 == 0 and inner == (1, 1, 1)):
        tiles, splits = (M // 128) * (N // (256 if N % 256 == 0 else 128)), 1
        if tiles < 192 and not y_bf16:
            while splits < 8 and tiles * splits < 256 and K % (64 * splits) == 0 and K // (2 * splits) >= 256:
                splits *= 2
        return Linear("stream", sto, splits)
    if sto:
        assert not acc and xoff == 0 and yoff == 0
    return Linear("bf16s" if sto else "bf16" if bf else "f32", sto, 1)


@functools.lru_cache(maxsize=None)
def tn_route(bf16, bf16_stream, min_macs, batch, M, K, N, x_bf16, z_bf16, xoff, zoff, floats):
    """out[K, N] (+)= X[M, K]^T . Z[M, N] per batch.  floats(entry name, *shape): the library's host-only scratch size queries; the
    streaming kernel (after_conv's 2048 x 256: 37 vs 59 us at 8192 rows; the pair tensors' 128 x 128 over 131072 bf16-stored rows: 22 vs
    47 us) is dropped where its query answers 0."""
    sto = storage_mask(x_bf16, z_bf16, Z_BF16)
    bf = use_bf16(bf16, min_macs, batch, M, K, N) or bool(sto)
    need = floats("dispu_linear_tn_bf16_scratch_floats" if bf else "dispu_linear_tn_scratch_floats", batch, M, K, N)
    stream = 0
    if bf and bf16_stream and batch == 1 and sto in (0, 3) and K % 128 == 0 and N % 128 == 0 and xoff == 0 and zoff == 0:
        stream = floats("dispu_linear_tn_bf16_stream_scratch_floats", M, K, N)
    if sto and not stream:
        assert xoff == 0 and zoff == 0
    return Tn("stream" if stream else "bf16s" if sto else "bf16" if bf else "f32", sto, max(need, stream))


def tn_grouped(group_reduce, wgrad, batch, side_stream, key):
    """the split reduction of a TN product waits for its stream's grouped launch?  side_stream: the launch goes to one; key: the schedule's."""
    return bool(group_reduce and wgrad and batch == 1 and (side_stream or key == "main"))


def _p(t, off=0):
    """Device pointer of element `off` of t's storage (in t's own element size: a bf16-stored activation advances 2 bytes per column)."""
    return _lib.C.c_void_p(t.data_ptr() + t.element_size() * off) if t is not None else _lib.C.c_void_p(0)


class Products(object):
    def __init__(self, device, sched, bf16, invalidate):
        """sched: the step's StepSchedule (the stream launches go to, the side streams, the grouped reductions).  invalidate(): called, after
        a device synchronize, when a scratch buffer that recorded launches may point into is about to be replaced."""
        self.device, self.sched, self.bf16, self._invalidate = device, sched, bool(bf16), invalidate
        self.bf16_stream = True    # dtype="bf16": the large dense products on the streaming bf16 kernel (csrc/linear_bf16_stream.hip) where its shape rules hold
        self.bf16_min_macs = 1.5e9            # dtype="bf16": products below this many multiply-adds stay on the fp32 kernel (use_bf16)
        self.packs = {}                       # bf16 images of the weights for the streaming kernel, by (weight address, K, N, transpose)
        self.scratch = {}                     # per stream: scratch of the split reductions / column sums

    # ---- every contact with torch.cuda and the library (a test replaces these with recorders)
    _L = staticmethod(lambda: _lib.tape_lib())           # (looked up per call: tests count launches through a proxy set on _lib.tape_lib)
    _floats = staticmethod(lambda name, *shape: getattr(_lib.lib(), name)(*shape))          # the host-only scratch size queries

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _synchronize(self):
        torch.cuda.synchronize(self.device)

    # ---- device memory
    def scratch_floats(self, n, key=None):
        """scratch of the launches queued on ONE stream (they run in order, so they can share it): a dW stream's (key "dw<i>"), or the
        current stream's (main or a branch)."""
        key = key if key else self.sched.key
        cur = self.scratch.get(key)
        if cur is None or cur.numel() < n:
            if cur is not None:
                self._synchronize()                          # a launch on that stream may still be using the old buffer
                self._invalidate()                           # ... and a tape recorded at a smaller shape points into it
            cur = self.scratch[key] = self._empty(max(int(n), 1 << 20), torch.float32)
        return cur

    # ---- launches
    def use_bf16(self, batch, M, K, N):
        return use_bf16(self.bf16, self.bf16_min_macs, batch, M, K, N)

    def batched(self, batch, M, K, N, *rest):
        """dispu_linear, or its bf16-product twin when the trainer runs mixed precision (narrow 3-wide layers stay fp32)."""
        L = self._L()
        return (L.dispu_linear_bf16 if self.use_bf16(batch, M, K, N) else L.dispu_linear)(batch, M, K, N, *rest)

    def linear(self, M, K, N, X, xoff, W, woff, wt, bias, act, Y, yoff, acc=False, WT=None):
        """Y[:, yoff:yoff+N] (+)= act(X[:, xoff:xoff+K] . B + bias).  wt = 0: B = W[woff..] as [K][N], a forward product.  wt = 1: B = W^T
        with W[woff..] as [N][K], the dX product dX (+)= dZ . W^T (acc: accumulated); WT, the step's transposed copy of W ([K, N] row-major),
        then runs the product untransposed (the forward GEMM's fast path) on every route but "stream", which packs its weights to bf16
        [N][K] from W itself, right here, on the same stream (weights change every step; 0.5 M elements at most)."""
        L, st, bfl = self._L(), self.sched.st, torch.bfloat16
        (ldx, ix), (ldy, iy), (ldw, iw) = X.stride(), Y.stride(), W.stride()
        r = linear_route(self.bf16, self.bf16_stream, self.bf16_min_macs, M, K, N, X.dtype == bfl, Y.dtype == bfl, ldx, xoff, yoff, (ix, iy, iw),
                         bool(acc))
        if r.route == "stream":
            key = (W.data_ptr() + 4 * woff, K, N, 1 - wt)
            bt = self.packs.get(key)
            if bt is None:
                bt = self.packs[key] = self._empty((N, K), bfl)
            _lib.check(L.dispu_bf16_pack(*((N, K) if wt else (K, N)), _p(W, woff), ldw, 1 - wt, _p(bt), st), "dispu_bf16_pack")
            nsp = r.splits
            parts = self.scratch_floats(nsp * M * N) if nsp > 1 else None
            dst = (None, 0, _p(parts), N, 0, nsp, M * N) if nsp > 1 else (_p(bias), act, _p(Y, yoff), ldy, r.sto >> 2, 1, 0)
            _lib.check(L.dispu_linear_bf16_stream(M, K, N, _p(X, xoff), ldx, r.sto & 1, _p(bt), K, *dst, st), "dispu_linear_bf16_stream")
            if nsp > 1:                                      # the partial products summed in order, then bias and activation
                _lib.check(L.dispu_linear_splitk_finish(M, N, nsp, _p(parts), M * N, _p(bias), act, _p(Y, yoff), ldy, st), "splitk_finish")
            return
        wp, ldb, tb = (_p(WT), WT.stride(0), 0) if WT is not None else (_p(W, woff), ldw, wt)
        if r.route == "bf16s":
            _lib.check(L.dispu_linear_bf16s(1, M, K, N, _p(X), ldx, 0, wp, ldb, 0, tb, _p(bias), act, _p(Y), ldy, 0, None, 0, 0, r.sto, st),
                       "dispu_linear_bf16s")
            return
        fn = L.dispu_linear_bf16 if r.route == "bf16" else L.dispu_linear
        _lib.check(fn(1, M, K, N, _p(X, xoff), ldx, 0, wp, ldb, 0, tb, _p(bias), act, _p(Y, yoff), ldy, 0, _p(Y, yoff) if acc else None,
                      ldy if acc else 0, 0, None, 0, 0, st), "dispu_linear")

    def tn(self, batch, M, K, N, X, xoff, ldx, sx, Zt, zoff, ldz, sz, out, ooff, ldo, so, accumulate, dbias=None, side=False, after=None,
           wgrad=False):
        """out (+)= X^T . Zt.  side=True: on a side stream (the caller guarantees nothing overwrites X / Zt before join), ordered after
        `after` (an event or a StepSchedule.fork_group()) / this point of the current stream; the launch itself may be deferred (StepSchedule.defer).
        wgrad=True: `out` is a weight gradient -- nothing reads it before join(), so its split reduction may wait for the stream's
        grouped launch (StepSchedule.group_reduce)."""
        L, sched, bfl = self._L(), self.sched, torch.bfloat16
        r = tn_route(self.bf16, self.bf16_stream, self.bf16_min_macs, batch, M, K, N, X.dtype == bfl, Zt.dtype == bfl, xoff, zoff, self._floats)

        def launch(st, key):
            if not tn_grouped(sched.group_reduce, wgrad, batch, key is not None, sched.key):
                return product(st, self.scratch_floats(r.need, key))
            # a descriptor slot of its stream and a scratch buffer of this product's own (it must survive until the grouped reduction)
            slot, grp = sched.reduce_slot(st, out.data_ptr() + 4 * ooff, dbias.data_ptr() if dbias is not None else 0)
            sc = self.scratch_floats(r.need, ("tn", out.data_ptr() + 4 * ooff, K, N))
            _lib.check(L.dispu_tn_defer(slot), "dispu_tn_defer")
            try:
                product(st, sc)
            finally:
                grp.commit()

        def product(st, sc):
            o, rest = _p(out, ooff), (accumulate, _p(dbias), _p(sc), sc.numel())
            if r.route == "stream":
                rc = L.dispu_linear_tn_bf16_stream(M, K, N, _p(X), ldx, _p(Zt), ldz, r.sto, o, ldo, *rest, st)
            elif r.route == "bf16s":
                rc = L.dispu_linear_tn_bf16s(batch, M, K, N, _p(X), ldx, sx, _p(Zt), ldz, sz, o, ldo, so, *rest, r.sto, st)
            else:
                fn = L.dispu_linear_tn_bf16 if r.route == "bf16" else L.dispu_linear_tn
                rc = fn(batch, M, K, N, _p(X, xoff), ldx, sx, _p(Zt, zoff), ldz, sz, o, ldo, so, *rest, st)
            _lib.check(rc, "dispu_linear_tn")

        if not (side and sched.overlap_dw):
            launch(sched.st, None)
            return
        ev = after if after is not None else sched.fork_point()
        sched.defer(lambda: launch(*sched.side_stream(ev)))

    def act_bias_grad(self, M, N, dY, dyoff, Y, yoff, act, dZ, dzoff, dbias):
        L = self._L()
        sc = self.scratch_floats(L.dispu_act_bias_grad_scratch_floats(M, N))
        _lib.check(L.dispu_act_bias_grad(M, N, _p(dY, dyoff), dY.stride(0), _p(Y, yoff) if Y is not None else None,
                                         Y.stride(0) if Y is not None else 0, act, _p(dZ, dzoff) if dZ is not None else None,
                                         dZ.stride(0) if dZ is not None else 0, _p(dbias), 1, _p(sc), sc.numel(), self.sched.st),
                   "dispu_act_bias_grad")
