"""GPU tests of the cross-cloud k-NN and the attribute transfer (csrc/attributes.hip, dispu_amd.attributes) against
tests/attributes_oracle.py: indices, d2 and the weighted features bit for bit, labels exactly, through the C ABI with sentinel-filled
outputs; ragged batches, flagged and refused input, the Python surface, and tools/upsample.py --attributes end to end.  Every cloud
has at most 4127 points (65 cells: one more than a 64-lane sweep of the box table); the oracle's neighbours are computed once per
pair of clouds at k = 32 and sliced (lru_cache)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attributes_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue
ALL_K = (1, 3, 8, 9, 16, 17, 32)                                # the template edges 8 | 9 and 16 | 17, and both ends
GEOMETRIES = ("cube", "lattice", "subset", "far", "plane", "large")
# every size of {1, 2, 63, 64, 65, 129, 4127} with at least two others on each side
SIZE_PAIRS = ((1, 4127), (4127, 1), (4127, 4127), (1, 1), (1, 64), (2, 63), (2, 129), (63, 2), (63, 65), (64, 2), (64, 129), (65, 1),
              (65, 64), (129, 63), (129, 65), (129, 4127), (4127, 64), (4127, 129), (63, 4127), (2, 2))


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return off


@functools.lru_cache(maxsize=None)
def pair(name, nq, m):
    """-> (queries [nq, 3], references [m, 3]) fp32, seeded"""
    r = np.random.RandomState(1000 * nq + m)
    if name == "cube":
        return r.random_sample((nq, 3)).astype(np.float32), r.random_sample((m, 3)).astype(np.float32)
    if name == "lattice":                                       # 125 sites: exact d2 ties everywhere, duplicated references
        return r.randint(0, 5, (nq, 3)).astype(np.float32), r.randint(0, 5, (m, 3)).astype(np.float32)
    if name == "subset":                                        # every query is a reference point: d2 = 0
        p = r.random_sample((m, 3)).astype(np.float32)
        return np.ascontiguousarray(p[r.randint(0, m, nq)]), p
    if name == "far":                                           # the queries' box is disjoint from the references' and far from it
        return (r.random_sample((nq, 3)) * 0.5 + [40.0, -25.0, 3.0]).astype(np.float32), r.random_sample((m, 3)).astype(np.float32)
    if name == "plane":                                         # references on z = 0, queries off it
        p = np.concatenate([r.random_sample((m, 2)), np.zeros((m, 1))], axis=1).astype(np.float32)
        return (r.random_sample((nq, 3)) + [0.0, 0.0, 0.25]).astype(np.float32), p
    if name == "large":                                         # millimetre structure at coordinates of 1e4
        c = np.array([1e4, -1e4, 1e4])
        return (c + 1e-3 * r.random_sample((nq, 3)) * 20).astype(np.float32), (c + 1e-3 * r.random_sample((m, 3)) * 20).astype(np.float32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle32(name, nq, m):
    return A.knn_cross(*pair(name, nq, m), 32)


def oracle_knn(name, nq, m, k):
    """knn_cross at k by slicing the k = 32 answer: the keys' order does not depend on k, and the padding begins at min(k, m) either way"""
    idx, d2 = oracle32(name, nq, m)
    return idx[:, :k], d2[:, :k]


@functools.lru_cache(maxsize=None)
def attrs(m, F, seed=0):
    r = np.random.RandomState(seed + 7 * m + F)
    return (r.random_sample((m, F)) * 4 - 1).astype(np.float32), r.randint(-3, 40, m).astype(np.int32)


class Abi(object):
    """one packed batch of (queries, references) pairs on the device and what the C entries need; outputs are pre-filled with sentinels.
    scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the zero-filled one"""

    def __init__(self, dev, qs, rs, qoff=None, roff=None, C_arg=None, scratch_buf=None):
        self.scratch_buf = scratch_buf
        import torch
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        self.torch, self._lib, self.L, self.dev = torch, _lib, _lib.lib(), dev
        self.gq, self.gr = offsets(qs), offsets(rs)
        self.qoff = self.gq if qoff is None else np.ascontiguousarray(qoff, np.int32)
        self.roff = self.gr if roff is None else np.ascontiguousarray(roff, np.int32)
        self.nC = len(qs) if C_arg is None else C_arg
        self.q = torch.from_numpy(np.concatenate(qs).astype(np.float32)).to(dev)
        self.r = torch.from_numpy(np.concatenate(rs).astype(np.float32)).to(dev)
        self.nq, self.nr = self.q.shape[0], self.r.shape[0]
        self.d_qoff, self.d_roff = torch.from_numpy(self.qoff).to(dev), torch.from_numpy(self.roff).to(dev)
        self.st = _lib.stream_ptr(dev)
        self.status = torch.full((len(qs),), -7, dtype=torch.int32, device=dev)

    def scratch(self, how):
        """-> (pointer, size) of a scratch that is right ("ok"), NULL, one byte short or misaligned"""
        full = self.L.dispu_knn_cross_scratch_bytes(len(self.gq) - 1, C.c_void_p(self.gq.ctypes.data), C.c_void_p(self.gr.ctypes.data))
        assert full > 0
        self.buf = self.torch.zeros((full + 64,), dtype=self.torch.uint8, device=self.dev)
        if self.scratch_buf is not None:
            assert how in ("ok", "short"), "with scratch_buf only a right or a one-byte-short size can be asked for"
            return self.scratch_buf.ptr(), self.scratch_buf.nbytes - (1 if how == "short" else 0)
        if how == "null":
            return C.c_void_p(0), full
        if how == "short":
            return self._lib.ptr(self.buf), full - 1
        if how == "misaligned":
            return C.c_void_p(self.buf.data_ptr() + 4), full
        return self._lib.ptr(self.buf), full

    def head(self, a):
        return (self.nC, a["qoff"], C.c_void_p(self.qoff.ctypes.data), a["roff"], C.c_void_p(self.roff.ctypes.data))

    def knn(self, k, scratch="ok", null=()):
        """-> rc, idx [nq, k] (sentinel -7), d2 [nq, k] (sentinel 7), status (sentinel -7)"""
        t, p = self.torch, self._lib.ptr
        sp, sb = self.scratch(scratch)
        kk = max(k, 1)
        idx = t.full((self.nq, kk), -7, dtype=t.int32, device=self.dev)
        d2 = t.full((self.nq, kk), 7.0, dtype=t.float32, device=self.dev)
        a = dict(qoff=p(self.d_qoff), roff=p(self.d_roff), q=p(self.q), r=p(self.r), idx=p(idx), d2=p(d2), status=p(self.status))
        a.update({n: C.c_void_p(0) for n in null})
        rc = self.L.dispu_knn_cross_segments(*(self.head(a) + (k, a["q"], a["r"], a["idx"], a["d2"], a["status"], sp, sb, self.st)))
        t.cuda.synchronize(self.dev)
        return rc, N(idx), N(d2), N(self.status)

    def transfer(self, k, mode, F, feat, labels, scratch="ok", null=()):
        """feat [nr, F] / labels [nr] numpy or None -> rc, out_feat [nq, max(F, 1)] (sentinel 7), out_labels [nq] (sentinel -7), status"""
        t, p = self.torch, self._lib.ptr
        sp, sb = self.scratch(scratch)
        of = t.full((self.nq, max(F, 1)), 7.0, dtype=t.float32, device=self.dev)
        ol = t.full((self.nq,), -7, dtype=t.int32, device=self.dev)
        df = None if feat is None else t.from_numpy(np.ascontiguousarray(feat, np.float32)).to(self.dev)
        dl = None if labels is None else t.from_numpy(np.ascontiguousarray(labels, np.int32)).to(self.dev)
        a = dict(qoff=p(self.d_qoff), roff=p(self.d_roff), q=p(self.q), r=p(self.r), feat=p(df), of=p(of if feat is not None else None),
                 labels=p(dl), ol=p(ol if labels is not None else None), status=p(self.status))
        a.update({n: C.c_void_p(0) for n in null})
        rc = self.L.dispu_transfer_attributes_segments(*(self.head(a) + (k, mode, a["q"], a["r"], F, a["feat"], a["of"], a["labels"], a["ol"],
                                                                         a["status"], sp, sb, self.st)))
        t.cuda.synchronize(self.dev)
        return rc, N(of), N(ol), N(self.status)


def check_pair(dev, name, nq, m, k, F=3):
    """knn, then idw features and labels in one transfer call, all against the oracle"""
    q, r = pair(name, nq, m)
    want_idx, want_d2 = oracle_knn(name, nq, m, k)
    a = Abi(dev, [q], [r])
    rc, idx, d2, status = a.knn(k)
    assert rc == 0 and status[0] == 0, (name, nq, m, k)
    assert np.array_equal(idx, want_idx), (name, nq, m, k, np.nonzero((idx != want_idx).any(axis=1))[0][:10])
    assert np.array_equal(bits(d2), bits(want_d2)), (name, nq, m, k)
    feat, labels = attrs(m, F)
    rc, of, ol, status = a.transfer(k, 0, F, feat, labels)
    assert rc == 0 and status[0] == 0
    assert np.array_equal(bits(of), bits(A.transfer_from_knn(want_idx, want_d2, feat, "idw"))), (name, nq, m, k)
    assert np.array_equal(ol, labels[want_idx[:, 0]]), (name, nq, m, k)


# ---- sizes, k values, geometries --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,m", SIZE_PAIRS)
def test_every_size_pair(dev, nq, m):
    """cell edges 63 | 64 | 65 on both sides, q tails (qcnt < 64), one reference, 65 reference cells; k = 3 and one more k each"""
    check_pair(dev, "cube", nq, m, 3)
    check_pair(dev, "cube", nq, m, ALL_K[(nq + m) % len(ALL_K)])
    if (nq, m) in ((1, 4127), (4127, 1), (4127, 4127)):
        check_pair(dev, "cube", nq, m, 32)


@pytest.mark.parametrize("name", GEOMETRIES)
def test_every_k_on_every_geometry(dev, name):
    """193 queries (a tail of one lane) against 1000 references (16 cells), and against 5 references: m < k from k = 8 on"""
    for k in ALL_K:
        check_pair(dev, name, 193, 1000, k)
        check_pair(dev, name, 65, 5, k)
    if name in ("lattice", "far", "subset"):
        check_pair(dev, name, 4127, 4127, 16)


def test_lattice_has_the_ties_it_is_for():
    q, r = pair("lattice", 193, 1000)
    idx, d2 = oracle_knn("lattice", 193, 1000, 32)
    assert (d2[:, 1:] == d2[:, :-1]).mean() > 0.5 and len(np.unique(r, axis=0)) <= 125
    same = d2[:, 1:] == d2[:, :-1]
    assert (idx[:, 1:][same] > idx[:, :-1][same]).all()        # equal d2: ascending index
    qf, rf = pair("far", 193, 1000)
    assert (qf.min(axis=0) > rf.max(axis=0) + 1.0).any()        # disjoint boxes
    assert (oracle_knn("subset", 193, 1000, 1)[1] == 0).all()


# ---- transfer ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3, 7])
@pytest.mark.parametrize("mode", [0, 1])
def test_transfer_equals_knn_then_the_oracles_arithmetic(dev, F, mode):
    """features only, labels only, both: from the GPU's own knn_cross output through the oracle's arithmetic, bit for bit"""
    name, nq, m = "cube", 300, 1000
    q, r = pair(name, nq, m)
    feat, labels = attrs(m, F)
    a = Abi(dev, [q], [r])
    for k in (1, 3, 9, 32):
        rc, idx, d2, _ = a.knn(k)
        assert rc == 0 and np.array_equal(idx, oracle_knn(name, nq, m, k)[0])
        want = A.transfer_from_knn(idx, d2, feat, "idw" if mode == 0 else "nearest")
        if mode == 1:
            assert np.array_equal(bits(want), bits(feat[idx[:, 0]]))
        for fe, la in ((feat, None), (None, labels), (feat, labels)):
            rc, of, ol, status = a.transfer(k, mode, F, fe, la)
            assert rc == 0 and status[0] == 0
            if fe is not None:
                assert np.array_equal(bits(of), bits(want)), (k, F, mode)
            else:
                assert (of == 7).all()
            if la is not None:
                assert np.array_equal(ol, labels[idx[:, 0]])
            else:
                assert (ol == -7).all()


def test_nan_feature_propagates(dev):
    """feature values are not inspected: a NaN reaches exactly the outputs the oracle says, everything else is bit-equal"""
    q, r = pair("subset", 193, 1000)
    feat = attrs(1000, 3)[0].copy()
    idx, d2 = oracle_knn("subset", 193, 1000, 3)
    feat[idx[5, 1], 2] = np.nan
    a = Abi(dev, [q], [r])
    rc, of, _, _ = a.transfer(3, 0, 3, feat, None)
    want = A.transfer_from_knn(idx, d2, feat, "idw")
    assert rc == 0 and np.isnan(of[5, 2]) and not np.isnan(of[5, :2]).any()
    assert np.array_equal(np.isnan(of), np.isnan(want))
    assert np.array_equal(bits(np.nan_to_num(of, nan=0.0)), bits(np.nan_to_num(want, nan=0.0)))


# ---- batches, repeats, flagged segments -------------------------------------------------------------------------------------------------

def ragged():
    """C = 3, q = (70, 1, 4127), m = (4127, 65, 2).  The single query of segment 1 has exact duplicates among the references of segments
    0 and 2 (its packed neighbours on both sides), while its own references are all at least 0.5 away"""
    q0, r0 = (x.copy() for x in pair("cube", 70, 4127))
    q2, r2 = (x.copy() for x in pair("cube", 4127, 2))
    r1 = pair("cube", 1, 65)[1].copy()
    q1 = np.float32([[2.0, 2.0, 2.0]])
    r0[-1] = q1[0]
    r2[0] = q1[0]
    q0[-1] = r1[0]                                              # and a query of segment 0 sits on a reference of segment 1
    return [q0, q1, q2], [r0, r1, r2]


def test_ragged_batch_equals_each_segment_alone(dev):
    qs, rs = ragged()
    a = Abi(dev, qs, rs)
    feats = [attrs(len(r), 3, seed=c)[0] for c, r in enumerate(rs)]
    labels = [attrs(len(r), 3, seed=c)[1] for c, r in enumerate(rs)]
    for k in (3, 17):
        rc, idx, d2, status = a.knn(k)
        assert rc == 0 and not status.any()
        rc, of, ol, status = a.transfer(k, 0, 3, np.concatenate(feats), np.concatenate(labels))
        assert rc == 0 and not status.any()
        o = 0
        for c, (q, r) in enumerate(zip(qs, rs)):
            wi, wd = A.knn_cross(q, r, k)
            assert np.array_equal(idx[o:o + len(q)], wi) and np.array_equal(bits(d2[o:o + len(q)]), bits(wd)), (c, k)
            assert np.array_equal(bits(of[o:o + len(q)]), bits(A.transfer_from_knn(wi, wd, feats[c], "idw"))), (c, k)
            assert np.array_equal(ol[o:o + len(q)], labels[c][wi[:, 0]]), (c, k)
            o += len(q)
        assert d2[70, 0] >= 0.25                                # the duplicates next door were not taken


def test_two_calls_give_identical_bytes(dev):
    qs, rs = ragged()
    feat, labels = attrs(sum(len(r) for r in rs), 7)
    runs = []
    for _ in range(2):
        a = Abi(dev, qs, rs)
        rc, idx, d2, _ = a.knn(16)
        rc2, of, ol, _ = a.transfer(16, 0, 7, feat, labels)
        assert rc == 0 and rc2 == 0
        runs.append([x.tobytes() for x in (idx, d2, of, ol)])
    assert runs[0] == runs[1]


@pytest.mark.parametrize("side", ["queries", "refs"])
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_non_finite_segment_is_flagged_and_left_alone(dev, side, poison):
    import torch
    from dispu_amd import attributes as M
    sizes = ((300, 200), (129, 65), (70, 500))
    qs = [pair("cube", nq, m)[0].copy() for nq, m in sizes]
    rs = [pair("cube", nq, m)[1].copy() for nq, m in sizes]
    (qs if side == "queries" else rs)[1][40, 1] = poison
    feat, labels = attrs(765, 3)
    a = Abi(dev, qs, rs)
    rc, idx, d2, status = a.knn(8)
    assert rc == 0 and list(status) == [0, 1, 0] and (idx[300:429] == -7).all() and (d2[300:429] == 7).all()
    rc, of, ol, status = a.transfer(8, 0, 3, feat, labels)
    assert rc == 0 and list(status) == [0, 1, 0] and (of[300:429] == 7).all() and (ol[300:429] == -7).all()
    for c, lo, hi, ro in ((0, 0, 300, 0), (2, 429, 499, 265)):
        wi, wd = A.knn_cross(qs[c], rs[c], 8)
        assert np.array_equal(idx[lo:hi], wi) and np.array_equal(bits(d2[lo:hi]), bits(wd))
        assert np.array_equal(bits(of[lo:hi]), bits(A.transfer_from_knn(wi, wd, feat[ro:ro + len(rs[c])], "idw")))
        assert np.array_equal(ol[lo:hi], labels[ro:ro + len(rs[c])][wi[:, 0]])
    dq, dr = [torch.from_numpy(x).to(dev) for x in qs], [torch.from_numpy(x).to(dev) for x in rs]
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):
        M.knn_cross(dq, dr, 8)
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):
        M.transfer_attributes(dq, dr, labels=[torch.zeros(len(x), dtype=torch.int32, device=dev) for x in rs])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_abi_refusals_touch_nothing(dev):
    qs = [pair("cube", 300, 200)[0], pair("cube", 129, 65)[0]]
    rs = [pair("cube", 300, 200)[1], pair("cube", 129, 65)[1]]
    feat, labels = attrs(265, 3)

    def fresh(**kw):
        return Abi(dev, qs, rs, **kw)

    def knn_untouched(a, **kw):
        args = dict(k=3)
        args.update(kw)
        rc, idx, d2, status = a.knn(**args)
        assert rc == INVALID and (idx == -7).all() and (d2 == 7).all() and (status == -7).all(), kw

    def transfer_untouched(a, **kw):
        args = dict(k=3, mode=0, F=3, feat=feat, labels=labels)
        args.update(kw)
        rc, of, ol, status = a.transfer(**args)
        assert rc == INVALID and (of == 7).all() and (ol == -7).all() and (status == -7).all(), kw

    for kw in (dict(qoff=np.int32([0, 300, 200])), dict(qoff=np.int32([0, 300, 300])), dict(qoff=np.int32([1, 300, 429])),
               dict(roff=np.int32([0, 200, 100])), dict(roff=np.int32([0, 200, 200])), dict(roff=np.int32([1, 200, 265])), dict(C_arg=0),
               dict(C_arg=65536)):
        knn_untouched(fresh(**kw))
        transfer_untouched(fresh(**kw))
    for kw in (dict(k=0), dict(k=33), dict(k=-1), dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"),
               dict(null=("idx", "d2")), dict(null=("qoff",)), dict(null=("roff",)), dict(null=("q",)), dict(null=("r",)),
               dict(null=("status",))):
        knn_untouched(fresh(), **kw)
    for kw in (dict(k=0), dict(k=33), dict(mode=2), dict(mode=-1), dict(F=0), dict(F=-3), dict(feat=None, labels=None),
               dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"), dict(null=("of",)), dict(null=("ol",)),
               dict(null=("qoff",)), dict(null=("roff",)), dict(null=("q",)), dict(null=("r",)), dict(null=("status",))):
        transfer_untouched(fresh(), **kw)
    a = fresh()                                                 # the same calls, legal; one output alone is enough
    assert a.knn(3)[0] == 0 and a.knn(3, null=("idx",))[0] == 0 and a.knn(3, null=("d2",))[0] == 0
    assert a.transfer(3, 0, 3, feat, labels)[0] == 0
    L = a.L
    hq, hr = C.c_void_p(a.gq.ctypes.data), C.c_void_p(a.gr.ctypes.data)
    assert L.dispu_knn_cross_scratch_bytes(2, hq, hr) > 0
    big, one = np.int32([0, (1 << 24) + 1]), np.int32([0, 5])
    hb, ho = C.c_void_p(big.ctypes.data), C.c_void_p(one.ctypes.data)
    assert L.dispu_knn_cross_scratch_bytes(1, ho, ho) > 0
    for n_c, x, y in ((0, hq, hr), (65536, hq, hr), (1, hb, ho), (1, ho, hb), (2, hq, C.c_void_p(0)), (2, C.c_void_p(0), hr)):
        assert L.dispu_knn_cross_scratch_bytes(n_c, x, y) == 0


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------

def test_python_surface(dev):
    import torch
    from dispu_amd import attributes as M
    q, r = pair("cube", 193, 1000)
    feat, labels = attrs(1000, 3)
    dq, dr = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
    df, dl = torch.from_numpy(feat).to(dev), torch.from_numpy(labels).to(dev)
    wi, wd = oracle_knn("cube", 193, 1000, 5)
    idx, d2 = M.knn_cross(dq, dr, 5)
    assert isinstance(idx, torch.Tensor) and idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert np.array_equal(N(idx), wi) and np.array_equal(bits(N(d2)), bits(wd))
    only = M.knn_cross(dq, dr, 5, return_distance=False)
    assert isinstance(only, torch.Tensor) and np.array_equal(N(only), wi)
    w3 = oracle_knn("cube", 193, 1000, 3)
    out = M.transfer_attributes(dq, dr, features=df)                                                 # k = 3, idw
    assert isinstance(out, torch.Tensor) and out.shape == (193, 3) and np.array_equal(bits(N(out)), bits(A.transfer_from_knn(*w3, feat, "idw")))
    lab = M.transfer_attributes(dq, dr, labels=dl)
    assert isinstance(lab, torch.Tensor) and lab.dtype == torch.int32 and np.array_equal(N(lab), labels[w3[0][:, 0]])
    both = M.transfer_attributes(dq, dr, features=df, labels=dl, mode="nearest")
    assert isinstance(both, tuple) and np.array_equal(bits(N(both[0])), bits(feat[w3[0][:, 0]])) and np.array_equal(N(both[1]), N(lab))
    # lists in, lists out: clouds of different sizes in one packed launch sequence
    q2, r2 = pair("cube", 65, 5)
    f2, l2 = attrs(5, 3)
    lq, lr = [dq, torch.from_numpy(q2).to(dev)], [dr, torch.from_numpy(r2).to(dev)]
    li, ld = M.knn_cross(lq, lr, 8)
    assert isinstance(li, list) and isinstance(ld, list) and len(li) == 2 and li[1].shape == (65, 8)
    assert np.array_equal(N(li[0]), oracle_knn("cube", 193, 1000, 8)[0]) and np.array_equal(N(li[1]), oracle_knn("cube", 65, 5, 8)[0])
    assert np.array_equal(bits(N(ld[1])), bits(oracle_knn("cube", 65, 5, 8)[1]))
    lf, ll = M.transfer_attributes(lq, lr, features=[df, torch.from_numpy(f2).to(dev)], labels=[dl, torch.from_numpy(l2).to(dev)], k=8)
    assert isinstance(lf, list) and isinstance(ll, list)
    assert np.array_equal(bits(N(lf[1])), bits(A.transfer_from_knn(*oracle_knn("cube", 65, 5, 8), f2, "idw")))
    assert np.array_equal(N(ll[1]), l2[oracle_knn("cube", 65, 5, 1)[0][:, 0]])
    one = M.transfer_attributes([dq], [dr], features=[df])
    assert isinstance(one, list) and len(one) == 1

    def refused(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)

    for k in (0, 33, 3.0, True):
        refused("k must be an integer in 1 .. 32", M.knn_cross, dq, dr, k)
        refused("k must be an integer in 1 .. 32", M.transfer_attributes, dq, dr, features=df, k=k)
    refused("mode must be 'idw' or 'nearest'", M.transfer_attributes, dq, dr, features=df, mode="median")
    refused("needs features, labels or both", M.transfer_attributes, dq, dr)
    refused("refs must be one too", M.knn_cross, dq, [dr], 3)
    refused("2 query clouds but 1 reference clouds", M.knn_cross, [dq, dq], [dr], 3)
    refused("at least one cloud", M.knn_cross, [], [], 3)
    refused("must be float32", M.knn_cross, dq.double(), dr, 3)
    refused(r"expected an \[n, 3\] tensor", M.knn_cross, dq, dr[:, :2], 3)
    refused("has 0 points", M.knn_cross, dq[:0], dr, 3)
    refused("ROCm device", M.knn_cross, dq, dr.cpu(), 3)
    refused("features of cloud 0 has 999 rows but the cloud has 1000 reference points", M.transfer_attributes, dq, dr, features=df[:999])
    refused("expected a float32 tensor of 2", M.transfer_attributes, dq, dr, features=df.double())
    refused("expected a float32 tensor of 2", M.transfer_attributes, dq, dr, features=df[:, 0])
    refused("expected a int32 tensor of 1", M.transfer_attributes, dq, dr, labels=dl.long())
    refused("labels: expected 2 tensors", M.transfer_attributes, lq, lr, labels=[dl])
    refused("has 2 columns, expected 3", M.transfer_attributes, lq, lr, features=[df, torch.from_numpy(f2[:, :2].copy()).to(dev)])


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------

def test_upsample_tool_carries_attributes(dev, tmp_path):
    """a random-weight checkpoint; a sphere with two attribute columns: a smooth value and an integer label"""
    from dispu_amd import checkpoint as CK
    from oracle import generator as OG
    from normals_oracle import sphere
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    p = sphere(2048, seed=9)
    value = (10.0 + 3.0 * p[:, 0] + p[:, 1] * p[:, 2]).astype(np.float32)
    label = (np.floor(3.0 * (p[:, 2] + 1.0)).astype(np.int32) * 5 + 2).astype(np.float32)             # 2, 7, 12, ..., by height
    np.savetxt(str(data / "test" / "ball.xyz"), np.concatenate([p, value[:, None], label[:, None]], axis=1), fmt="%.6f")
    src = np.loadtxt(str(data / "test" / "ball.xyz"), ndmin=2)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    runs = {"plain": [], "off": ["--attributes", "none"], "idw": ["--attributes", "idw"],
            "nearest": ["--attributes", "nearest", "--attributes_k", "1"],
            "grid": ["--attributes", "idw", "--attributes_k", "8", "--grid_size", "0.1", "--normals", "pca"]}
    procs = {name: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for name, extra in runs.items()}
    for name, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    text = {name: open(str(tmp_path / name / "ball_X4.xyz"), "rb").read() for name in runs}
    assert text["off"] == text["plain"]
    plain = text["plain"].splitlines()
    assert len(plain) == 4 * 2048 and all(len(row.split()) == 3 for row in plain)
    for name in ("idw", "nearest"):
        rows = text[name].splitlines()
        assert len(rows) == len(plain) and all(len(row.split()) == 5 for row in rows)
        assert [b" ".join(row.split()[:3]) for row in rows] == plain                                 # the xyz columns, byte for byte
    idw = np.loadtxt(str(tmp_path / "idw" / "ball_X4.xyz"), ndmin=2)
    for col in (3, 4):                                          # a weighted mean stays within its sources, up to the 5e-7 of %.6f
        assert idw[:, col].min() >= src[:, col].min() - 5e-7 and idw[:, col].max() <= src[:, col].max() + 5e-7
    assert idw[:, 3].std() > 0.0                                # and it is not a constant
    near = np.loadtxt(str(tmp_path / "nearest" / "ball_X4.xyz"), ndmin=2)
    assert set(np.unique(near[:, 4])) <= set(np.unique(src[:, 4])) and len(np.unique(near[:, 4])) > 1
    rowset = {tuple(row) for row in src[:, 3:]}
    assert all(tuple(row) in rowset for row in near[:, 3:])     # nearest copies whole rows
    grid = np.loadtxt(str(tmp_path / "grid" / "ball_X4.xyz"), ndmin=2)
    assert grid.shape[1] == 3 + 2 + 3 and 4 * 256 <= grid.shape[0] < 4 * 2048
    for col in (3, 4):
        assert grid[:, col].min() >= src[:, col].min() - 5e-7 and grid[:, col].max() <= src[:, col].max() + 5e-7
    assert np.isfinite(grid).all() and np.all(np.linalg.norm(grid[:, 5:], axis=1) <= 1.0 + 1e-4)


def test_upsample_tool_refuses_a_file_without_attributes(dev, tmp_path):
    from normals_oracle import sphere
    (tmp_path / "test").mkdir()
    np.savetxt(str(tmp_path / "test" / "bare.xyz"), sphere(300, seed=1), fmt="%.6f")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--data_dir", str(tmp_path), "--attributes", "idw"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and b"bare.xyz" in r.stdout and b"--attributes" in r.stdout
