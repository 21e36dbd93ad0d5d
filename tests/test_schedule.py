"""StepSchedule (dis-pu_amd/schedule.py) without a device: streams, events, the table upload and the grouped launch are recorders, the
schedule's own code (rec / wait included) runs unchanged, and every test asserts on the list of recorded operations."""
import contextlib

from dispu_amd import _lib
from dispu_amd.schedule import _RG_MAX, StepSchedule


class Ev(object):
    def __init__(self, log):
        self.log, self.cuda_event = log, id(self)

    def record(self, stream):
        self.log.append(("record", self, stream))


class St(object):
    def __init__(self, log, name, ptr):
        self.log, self.name, self.cuda_stream = log, name, ptr

    def wait_event(self, ev):
        self.log.append(("wait", self, ev))


class Table(object):
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


class Recorded(StepSchedule):
    def __init__(self, **kw):
        StepSchedule.__init__(self, "cpu", **kw)
        self.log, self.streams, self.uploads = [], {}, []
        self.cur = [St(self.log, "main", 0x1000)]

    def _event(self):
        self.log.append(("event",))
        return Ev(self.log)

    def _pool_stream(self, kind, i):
        name = "%s%d" % (kind, i)
        assert name not in self.streams                      # the schedule keeps what it fetched
        self.log.append(("stream", name))
        self.streams[name] = St(self.log, name, 0x2000 + 0x100 * len(self.streams))
        return self.streams[name]

    def _current_stream(self):
        return self.cur[-1]

    @contextlib.contextmanager
    def _enter(self, stream):
        self.cur.append(stream)
        try:
            yield
        finally:
            self.cur.pop()

    def _upload(self, raw):
        self.uploads.append(raw)
        return Table(0x9000 + len(self.uploads))

    def _reduce_grouped(self, n, host, dev, stream):
        self.log.append(("reduce", n, stream.value, dev.value))

    # ---- helpers of the tests
    def body(self, name):
        return lambda: self.log.append(("run", name, self.key))

    def ops(self, *kinds):
        return [e for e in self.log if e[0] in kinds]

    def product(self, st, out, bias=0, splits=2):
        """what Trainer._tn does around a weight-gradient product that leaves `splits` partial sums behind"""
        slot, g = self.reduce_slot(st, out, bias)
        d = _lib.TnReduceDesc.from_address(slot.value)
        d.out, d.dbias, d.splits = out, bias, splits
        g.commit()
        return g


def test_deferral_off_runs_bodies_at_once():
    s = Recorded(defer_side=False)
    s.defer(s.body("A"))
    s.defer_branch(0, s.body("X"))
    assert s.ops("run") == [("run", "A", "main"), ("run", "X", "aux0")] and not s._deferred
    assert s.key == "main"

    s = Recorded(overlap_dw=False)
    s.st = "main stream"
    s.defer(s.body("A"))
    s.defer_branch(0, s.body("X"))
    with s.branch(1):
        s.body("Y")()
        assert s.st == "main stream"
    s.merge(0)
    s.merge(1)
    assert s.fork_group() is None
    s.join()
    assert s.log == [("run", "A", "main"), ("run", "X", "main"), ("run", "Y", "main")]      # no stream, no event, no wait


def test_deferral_on_order_of_submission():
    """A, X, B, C deferred in that order (X a priority-0 branch).  flush() counts every item of priority <= prio, as it always has, so
    flush(n=2) right away would take A and X: the branch is merged first here, then flush(n=2) finds A and B."""
    s = Recorded()
    s.defer(s.body("A"))
    s.defer_branch(0, s.body("X"))
    s.defer(s.body("B"))
    s.defer(s.body("C"))
    assert not s.ops("run")
    s.merge(0)
    assert s.ops("run") == [("run", "X", "aux0")]                                           # X, and only X ...
    done = s._aux[0][2]
    i_run, i_wait = s.log.index(("run", "X", "aux0")), s.log.index(("wait", s.cur[0], done))
    assert i_run < i_wait == len(s.log) - 1                                                 # ... before main waits for its completion
    s.flush(n=2)
    assert s.ops("run")[1:] == [("run", "A", "main"), ("run", "B", "main")]
    s.join()
    assert s.ops("run")[3:] == [("run", "C", "main")] and not s._deferred

    def outer():
        s.body("D")()
        s.defer(s.body("E"))
    s.defer(outer)
    s.flush()
    assert s.ops("run")[4:] == [("run", "D", "main"), ("run", "E", "main")] and not s._deferred

    s.defer(s.body("F"))
    s.defer_branch(1, s.body("Y"))
    s.defer(s.body("G"))
    s.flush(n=2)                                             # the first two of priority <= 1, the branch among them
    assert s.ops("run")[6:] == [("run", "F", "main"), ("run", "Y", "aux1")]
    n = len(s.log)
    s.merge(1)                                               # already submitted: nothing else is flushed for it
    assert s.log[n:] == [("wait", s.cur[0], s._aux[1][2])] and len(s._deferred) == 1


def test_fork_event_at_defer_time_and_completion_event_at_branch_exit():
    s = Recorded()
    main = s.cur[0]
    s.defer_branch(0, s.body("X"))
    (rec,) = s.ops("record")                                 # the fork event: recorded now, on the main stream
    assert rec[2] is main and not s.ops("run", "wait")
    fork = rec[1]
    s.flush(prio=0)
    later = s.fork_point()                                   # a later record on another stream
    aux, _, done = s._aux[0]
    tail = [e for e in s.log if e[0] in ("record", "wait", "run")][1:]
    assert tail == [("wait", aux, fork), ("run", "X", "aux0"), ("record", done, aux), ("record", later, main)]
    n = len(s.log)
    s.merge(0)
    assert s.log[n:] == [("wait", main, done)]               # merging records nothing


def test_fork_group_one_record_one_wait_per_side_stream():
    s = Recorded(dw_streams=2)
    first = s.side_stream(s.fork_point())
    n = len(s.log)
    g = s.fork_group()
    got = [s.side_stream(g) for _ in range(4)]
    dw0, dw1 = s.side_streams
    want = [(dw0.cuda_stream, "dw0"), (dw1.cuda_stream, "dw1")]
    assert [(p.value, k) for p, k in [first] + got] == [want[0], want[1], want[0], want[1], want[0]]     # the round-robin goes on where it was
    ops = [e for e in s.log[n:] if e[0] != "event"]
    assert ops == [("record", g[0], s.cur[0]), ("wait", dw1, g[0]), ("wait", dw0, g[0])]


def test_join_waits_for_busy_side_streams_only():
    s = Recorded(dw_streams=2)
    s.side_stream(s.fork_point())
    n = len(s.log)
    s.join()
    dw0, dw1 = s.side_streams
    assert s.log[n:] == [("record", s._join_evs[0], dw0), ("wait", s.cur[0], s._join_evs[0])]
    s.join()
    assert len(s.log) == n + 2


def test_grouped_reductions_alias_rule():
    a, b = _lib.C.c_void_p(0xA00), _lib.C.c_void_p(0xB00)
    s = Recorded()
    s.product(a, out=100)
    s.product(b, out=200)                                    # another destination, both without a bias: nothing in common
    assert not s.ops("reduce")
    s.product(b, out=100)                                    # the same destination on another stream: a's group goes first
    assert [e[:3] for e in s.ops("reduce")] == [("reduce", 1, 0xA00)]
    assert [g.n for g in s.reduce_groups.values()] == [0, 2]
    s.product(a, out=300, bias=7)
    s.product(b, out=400, bias=7)                            # the same bias gradient
    assert [e[:3] for e in s.ops("reduce")][1:] == [("reduce", 1, 0xA00)]
    s.flush_reductions()
    assert [e[:3] for e in s.ops("reduce")][2:] == [("reduce", 3, 0xB00)]


def test_grouped_reductions_overflow_and_products_that_left_nothing():
    a = _lib.C.c_void_p(0xA00)
    s = Recorded()
    g = s.product(a, out=1, splits=0)
    assert g.n == 0 and g.pairs == []
    s.flush_reductions()
    assert not s.ops("reduce")
    for i in range(_RG_MAX):
        s.product(a, out=1000 + i)
    assert g.n == _RG_MAX == 64 and not s.ops("reduce")
    s.product(a, out=5000)                                   # the 65th slot
    assert [e[:3] for e in s.ops("reduce")] == [("reduce", 64, 0xA00)] and g.n == 1


def test_grouped_reductions_identical_tables_share_one_device_copy():
    a = _lib.C.c_void_p(0xA00)
    s = Recorded()
    for _ in range(2):
        s.product(a, out=100)
        s.product(a, out=200, bias=7)
        s.flush_reductions()
    s.product(a, out=100)
    s.flush_reductions()
    assert len(s.uploads) == 2 and len(s.tables) == 2
    tabs = [e[3] for e in s.ops("reduce")]
    assert tabs[0] == tabs[1] != tabs[2]
    s.drop_tables()
    assert not s.tables
