"""Where and when the launches of a training step are submitted (train.Trainer decides WHAT is launched, products.Products which GEMM
entry a dense product goes to): side and auxiliary streams, the events between them, the deferral of side work behind the chain's
kernels, the grouped split reductions."""
# torch.cuda and the library are touched by the hooks at the head of StepSchedule only: a subclass that replaces them with recorders
# runs the whole schedule without a device (tests/test_schedule.py).
import contextlib
import ctypes

import torch

from . import _lib

# Streams are shared by every Trainer of a process (per device): HIP maps streams onto a few hardware queues, and a process that
# builds Trainer after Trainer (bench.py's side table, the test suite) would otherwise keep adding streams to them.  Trainers of one
# process run one after the other on the host thread, so sharing is safe: events order the work.  (Which of torch's pooled streams
# the step gets does not matter: skipping 0 - 7 of them first leaves the step at 1.945 ms.)
_STREAM_POOL = {}
_RG_MAX = 64


class ReduceGroup(object):
    """the split reductions that the weight-gradient products of ONE stream left undone: one launch on that stream at flush().
    slot() -> address of the next free descriptor, for the product that accumulates into out_ptr / bias_ptr; commit() follows that product."""

    def __init__(self, sched, stream_ptr):
        self.sched = sched
        self.desc = (_lib.TnReduceDesc * _RG_MAX)()      # host descriptor array
        self.n, self.pairs = 0, []                       # descriptors pending, their (out pointer, bias pointer)
        self.stream = ctypes.c_void_p(stream_ptr)

    def slot(self, out_ptr, bias_ptr):
        if self.n >= _RG_MAX:
            self.flush()
        self._open = (out_ptr, bias_ptr)
        return ctypes.c_void_p(ctypes.addressof(self.desc) + self.n * ctypes.sizeof(_lib.TnReduceDesc))

    def commit(self):
        if self.desc[self.n].splits > 0:                 # the product left a reduction behind (0: it wrote its result itself)
            self.n += 1
            self.pairs.append(self._open)

    def flush(self):
        if not self.n:
            return
        raw = ctypes.string_at(ctypes.addressof(self.desc), self.n * ctypes.sizeof(_lib.TnReduceDesc))
        tables = self.sched.tables
        dev = tables.get(raw)
        if dev is None:                                  # first step with this table (steady state: the same pointers every step)
            dev = tables[raw] = self.sched._upload(raw)
        self.sched._reduce_grouped(self.n, ctypes.c_void_p(ctypes.addressof(self.desc)), ctypes.c_void_p(dev.data_ptr()), self.stream)
        self.n, self.pairs = 0, []


class StepSchedule(object):
    def __init__(self, device, overlap_dw=True, dw_streams=2, defer_side=True, group_reduce=True):
        self.device = device
        self.overlap_dw, self.dw_streams, self.defer_side, self.group_reduce = overlap_dw, dw_streams, defer_side, group_reduce
        self.st = None                        # stream pointer the launches go to (set by the Trainer's forward() / zero_grad(), swapped inside branch())
        self.key = "main"                     # ... and that stream's scratch key
        self._aux = []                        # branch i -> (auxiliary stream, fork event, completion event)
        self.side_streams = []                # the weight-gradient streams (side_stream)
        self._side_rr = -1
        # Side work (weight-gradient products, the non-local / skip branches) is QUEUED ON THE HOST AFTER the chain's kernels: every
        # launch costs ~10 us of Python / ctypes, and a chain kernel that is submitted behind a dozen side launches leaves the GPU's
        # main queue idle for that long (round 4, profiles/r04_a_train_timeline.txt: 145 us before the fused local cell, 137 us before
        # its backward).  Side work records its fork event where it belongs and is submitted later, at points where the main queue
        # holds enough work (flush).  `defer_side` is on up to 16 patches per step (set by Trainer.forward()): at 32 the chip is
        # saturated by the chain's own kernels, side work submitted later only lengthens the tail (4.58 -> 4.63 ms)
        self._deferred = []                   # (priority, submission, the branch it is or None)
        self.reduce_groups = {}               # stream pointer -> ReduceGroup
        self.tables = {}                      # descriptor table bytes -> device copy (content-addressed: tapes keep pointing at theirs)

    # ---- every contact with torch.cuda and the library (a test replaces these with recorders)
    _event = staticmethod(torch.cuda.Event)
    _enter = staticmethod(torch.cuda.stream)              # "launches and torch ops inside go to this stream"

    def _pool_stream(self, kind, i):
        key = (torch.device(self.device).index or 0, kind, i)
        st = _STREAM_POOL.get(key)
        if st is None:
            with torch.cuda.device(self.device):
                st = _STREAM_POOL[key] = torch.cuda.Stream(device=self.device)
        return st

    def _current_stream(self):
        return torch.cuda.current_stream(self.device)

    def _upload(self, raw):
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)

    def _reduce_grouped(self, n, host, dev, stream):
        _lib.check(_lib.tape_lib().dispu_tn_reduce_grouped(n, host, dev, stream), "dispu_tn_reduce_grouped")

    # ---- stream / event operations (recorded on the launch tape as raw HIP calls when one is being taken, see Trainer.train_step_taped)
    def rec(self, ev, stream):
        ev.record(stream)
        self._tape("event_record", ev, stream, ev.cuda_event, stream.cuda_stream)

    def wait(self, stream, ev):
        stream.wait_event(ev)
        self._tape("stream_wait_event", ev, stream, stream.cuda_stream, ev.cuda_event)

    def _tape(self, what, ev, stream, a, b):
        t = _lib.taping()
        if t is not None:
            t.keep += [ev, stream]
            t.calls.append((getattr(_lib.lib(), "dispu_" + what), (ctypes.c_void_p(a), ctypes.c_void_p(b)), what))

    # ---- side stream(s) for the weight-gradient products (dw_streams of them, used round-robin; each has its own scratch)
    def _make_sides(self):
        if not self.side_streams:
            n = max(1, int(self.dw_streams))
            self.side_streams = [self._pool_stream("dw", j) for j in range(n)]
            self._join_evs = [self._event() for _ in range(n)]
            self._side_busy = [False] * n

    def fork_point(self):
        """an event at the current position of the current stream, for side work queued later (see Trainer._lin_bwd, Products.tn)."""
        ev = self._event()
        self.rec(ev, self._current_stream())
        return ev

    def fork_group(self):
        """-> what several dW products that all depend on THIS point of the current stream (the four weight gradients of a fused head
        chain) are ordered after: one event, one wait per side stream (side_stream).  None without side streams."""
        if self.overlap_dw:
            self._make_sides()
            return self.fork_point(), set()              # the event, the side streams that already wait for it

    def side_stream(self, after):
        """-> (stream pointer, scratch key) of the next side stream, which waits for the event `after`, or -- `after` a fork_group() --
        for that group's event unless it already does."""
        self._make_sides()
        i = self._side_rr = (self._side_rr + 1) % len(self.side_streams)
        ev, waited = after if isinstance(after, tuple) else (after, set())
        if i not in waited:
            self.wait(self.side_streams[i], ev)
            waited.add(i)
        self._side_busy[i] = True
        return ctypes.c_void_p(self.side_streams[i].cuda_stream), "dw%d" % i

    # ---- deferred submission
    @property
    def deferring(self):
        return self.defer_side and self.overlap_dw       # (only while side streams are in use)

    def defer(self, fn, prio=1, branch=None):
        """run the side-stream submission `fn` now, or at a later flush() when deferral is on.
        prio 0: branches the chain will wait for (non-local / skip / recompute); 1: weight gradients, read by Adam only."""
        if self.deferring:
            self._deferred.append((prio, fn, branch))
        else:
            fn()

    def flush(self, n=None, prio=1):
        """submit the deferred side launches of priority <= prio, in their order: all of them, or the first n."""
        i = 0
        while i < len(self._deferred) and (n is None or n > 0):
            if self._deferred[i][0] <= prio:
                self._deferred.pop(i)[1]()                # (may append: a branch defers its own weight gradients)
                if n is not None:
                    n -= 1
            else:
                i += 1

    def defer_branch(self, i, body, after=None):
        """`with branch(i, after): body()` -- submitted now, or at the next flush() / merge(i) when deferral is on.  The branch
        is ordered after `after`, or after THIS point of the current stream (the event is recorded now, whenever the body is submitted)."""
        if self.deferring and after is None:
            after = self.fork_point()

        def run():
            with self.branch(i, after):
                body()
        self.defer(run, 0, i)

    # ---- branches on auxiliary streams
    @contextlib.contextmanager
    def branch(self, i, after=None):
        """Launches inside run on auxiliary stream i, after everything queued on the current stream so far (or after the event
        `after`, recorded earlier on it); `merge(i)` makes the current stream wait for them.  At 8 patches per GPU a chain of 10 us kernels
        leaves most of the 256 CUs idle: independent sub-graphs (non-local cell | skip + local cell; the two Chamfer terms) run side by side."""
        if not self.overlap_dw:
            yield
            return
        while len(self._aux) <= i:
            self._aux.append((self._pool_stream("aux", len(self._aux)), self._event(), self._event()))
        aux, ev_fork, ev_done = self._aux[i]
        if after is None:
            after = ev_fork
            self.rec(after, self._current_stream())
        self.wait(aux, after)
        old = self.st, self.key
        with self._enter(aux):
            self.st, self.key = ctypes.c_void_p(aux.cuda_stream), "aux%d" % i
            try:
                yield
            finally:
                self.st, self.key = old
                # recorded HERE, not in merge: streams share hardware queues (GPU_MAX_HW_QUEUES = 4), and a marker queued at merge
                # time lands behind whatever the other streams of that queue were given in between (measured: the local cell's
                # backward started 0.33 ms late, behind dW products it does not depend on)
                self.rec(ev_done, aux)

    def merge(self, i):
        if any(b == i for _, _, b in self._deferred):
            self.flush(prio=0)                           # a branch whose submission is still deferred cannot be waited for
        if self.overlap_dw and i < len(self._aux):
            self.wait(self._current_stream(), self._aux[i][2])

    # ---- grouped split reductions (dispu_tn_defer / dispu_tn_reduce_grouped) ----
    def reduce_slot(self, st, out_ptr, bias_ptr):
        """-> (address of the next free descriptor of stream `st`, its ReduceGroup).  A product whose destination another pending
        reduction also accumulates into flushes that group first (two descriptors of one launch must not alias)."""
        for g in self.reduce_groups.values():
            if g.n and any(o == out_ptr or (bias_ptr and b == bias_ptr) for o, b in g.pairs):
                g.flush()
        g = self.reduce_groups.get(st.value)
        if g is None:
            g = self.reduce_groups[st.value] = ReduceGroup(self, st.value)
        return g.slot(out_ptr, bias_ptr), g

    def flush_reductions(self):
        for g in self.reduce_groups.values():
            g.flush()

    def drop_tables(self):
        self.tables.clear()                              # (the caller has synchronised the device: no launch reads them any more)

    def flush_all(self):
        self.flush()
        self.flush_reductions()                          # each stream's pending split reductions: one launch per stream, behind its products

    def join(self):
        """the current stream waits for every dW product queued so far (before a buffer they read is overwritten, before Adam)."""
        self.flush_all()
        for i, side in enumerate(self.side_streams):
            if self._side_busy[i]:
                self.rec(self._join_evs[i], side)
                self.wait(self._current_stream(), self._join_evs[i])
                self._side_busy[i] = False
