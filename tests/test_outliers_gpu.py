"""GPU tests of the outlier filters (csrc/outliers.hip, dispu_amd.outliers) against tests/outliers_oracle.py: the mean neighbour distance
bit for bit, the radius counts exactly, the per-cloud statistics to 1e-10, the kept indices exactly, ragged batches, flagged and refused
input, and tools/upsample.py --clean_output end to end.  Every cloud the search sees has at most 4127 points (the oracle's sorted
distances are shared through lru_cache); the compaction alone also runs on a million rows, against a numpy mask."""
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
import outliers_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue
INT_MAX = 2 ** 31 - 1
ALL_K = (1, 7, 8, 15, 16, 31)                                   # k + 1 crosses the template edges 8 | 9 and 16 | 17 and reaches 32


def N(t):
    return t.detach().cpu().numpy()


def offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return off


class Abi(object):
    """one packed batch on the device and what every C entry needs; outputs are pre-filled with sentinels.
    scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the zero-filled one"""

    def __init__(self, dev, clouds, off=None, C_arg=None, scratch_buf=None):
        self.scratch_buf = scratch_buf
        import torch
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        self.torch, self._lib, self.L, self.dev = torch, _lib, _lib.lib(), dev
        self.good = offsets(clouds)
        self.off = self.good if off is None else np.ascontiguousarray(off, np.int32)
        self.nC = len(self.off) - 1 if C_arg is None else C_arg
        self.cloud = torch.from_numpy(np.concatenate(clouds).astype(np.float32)).to(dev)
        self.total = self.cloud.shape[0]
        self.hp = C.c_void_p(self.off.ctypes.data)
        self.d_off = torch.from_numpy(self.off).to(dev)
        self.st = _lib.stream_ptr(dev)
        self.status = torch.full((len(clouds),), -7, dtype=torch.int32, device=dev)

    def scratch(self, full, how):
        """-> (pointer, size) of a scratch that is right ("ok"), NULL, one byte short or misaligned"""
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

    def mean_dist(self, k, scratch="ok", null=()):
        p = self._lib.ptr
        full = self.L.dispu_knn_mean_dist_scratch_bytes(len(self.good) - 1, C.c_void_p(self.good.ctypes.data), 16)
        sp, sb = self.scratch(full, scratch)
        md = self.torch.full((self.total,), 7.0, dtype=self.torch.float32, device=self.dev)
        a = dict(off=p(self.d_off), cloud=p(self.cloud), md=p(md), status=p(self.status))
        a.update({n: C.c_void_p(0) for n in null})
        rc = self.L.dispu_knn_mean_dist_segments(self.nC, a["off"], self.hp, k, a["cloud"], a["md"], a["status"], sp, sb, self.st)
        self.torch.cuda.synchronize(self.dev)
        self.md = md
        return rc, N(md), N(self.status)

    def count(self, radius, cap, scratch="ok", null=()):
        p = self._lib.ptr
        full = self.L.dispu_radius_count_scratch_bytes(len(self.good) - 1, C.c_void_p(self.good.ctypes.data))
        sp, sb = self.scratch(full, scratch)
        cnt = self.torch.full((self.total,), -7, dtype=self.torch.int32, device=self.dev)
        a = dict(off=p(self.d_off), cloud=p(self.cloud), cnt=p(cnt), status=p(self.status))
        a.update({n: C.c_void_p(0) for n in null})
        rc = self.L.dispu_radius_count_segments(self.nC, a["off"], self.hp, radius, cap, a["cloud"], a["cnt"], a["status"], sp, sb, self.st)
        self.torch.cuda.synchronize(self.dev)
        self.cnt = cnt
        return rc, N(cnt), N(self.status)

    def threshold(self, ratio, null=()):
        """on the mean_dist and status the last mean_dist call left"""
        p = self._lib.ptr
        stats = self.torch.full((len(self.good) - 1, 3), 7.0, dtype=self.torch.float64, device=self.dev)
        a = dict(off=p(self.d_off), md=p(self.md), status=p(self.status), stats=p(stats))
        a.update({n: C.c_void_p(0) for n in null})
        rc = self.L.dispu_outlier_threshold_segments(self.nC, a["off"], self.hp, a["md"], a["status"], ratio, a["stats"], self.st)
        self.torch.cuda.synchronize(self.dev)
        self.stats = stats
        return rc, N(stats)

    def compact(self, rule, src, stats=None, min_neighbors=0, scratch="ok", null=(), status=True):
        p = self._lib.ptr
        full = self.L.dispu_compact_scratch_bytes(len(self.good) - 1, C.c_void_p(self.good.ctypes.data))
        sp, sb = self.scratch(full, scratch)
        pts = self.torch.full((self.total, 3), 7.0, dtype=self.torch.float32, device=self.dev)
        idx = self.torch.full((self.total,), -7, dtype=self.torch.int32, device=self.dev)
        new_off = self.torch.full((len(self.good),), -7, dtype=self.torch.int32, device=self.dev)
        a = dict(off=p(self.d_off), cloud=p(self.cloud), src=p(src), idx=p(idx), new_off=p(new_off))
        a.update({n: C.c_void_p(0) for n in null})
        rc = self.L.dispu_compact_segments(self.nC, a["off"], self.hp, a["cloud"], rule, a["src"], p(stats), min_neighbors,
                                           p(self.status if status else None), p(pts), a["idx"], a["new_off"], sp, sb, self.st)
        self.torch.cuda.synchronize(self.dev)
        return rc, N(pts), N(idx), N(new_off)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def cloud(name):
    r = np.random.RandomState(0)
    if name in O.MASK_CLOUDS:
        return O.mask_cloud(name)
    if name == "sphere":
        return O.sphere(4097)
    if name == "lattice":
        return O.lattice(9)                                     # 729 points, exact ties
    if name == "clusters":                                      # two clusters 100 apart and 5 isolated points midway
        a = (r.random_sample((600, 3)) - 0.5).astype(np.float32)
        b = (r.random_sample((600, 3)) - 0.5).astype(np.float32) + np.float32([100, 0, 0])
        mid = np.float32([50, 0, 0]) + (r.random_sample((5, 3)) - 0.5).astype(np.float32)
        return np.concatenate([a, mid, b])
    if name == "coincident":
        return np.tile(np.float32([[0.25, 0.5, 0.75]]), (100, 1))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sorted_d2(name, n=None):
    return O.sorted_d2(cloud(name) if n is None else cloud(name)[:n], 32)


def oracle_md(name, k, n=None):
    sd2 = sorted_d2(name, n)
    return O.mean_dist_from_sorted(sd2, len(sd2), k)


def radius_for_16(name):
    """a radius with about 16 neighbours: the median distance to the 17th key (the point itself is the first)"""
    return float(np.sqrt(np.median(sorted_d2(name)[:, 16].astype(np.float64))))


# ---- the mean neighbour distance, bit for bit -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", ALL_K)
def test_mean_dist_at_every_size(dev, k):
    """cell edges 63 | 64 | 65, n around k + 1, and 4097 points: 65 cells, so the box walk takes a second step"""
    import torch
    from dispu_amd.outliers import knn_mean_distance
    sizes = sorted({1, 2, 3, 63, 64, 65, 129, 2049, 4097, k, k + 1, k + 2})
    for n in sizes:
        rc, md, status = Abi(dev, [cloud("sphere")[:n]]).mean_dist(k)
        assert rc == 0 and status[0] == 0
        assert np.array_equal(bits(md), bits(oracle_md("sphere", k, n))), (n, k)
    got = knn_mean_distance([torch.from_numpy(cloud("sphere")[:n]).to(dev) for n in sizes], k=k)      # one packed launch sequence
    assert isinstance(got, list) and len(got) == len(sizes)
    for n, g in zip(sizes, got):
        assert g.dtype == torch.float32 and g.shape == (n,) and np.array_equal(bits(N(g)), bits(oracle_md("sphere", k, n))), (n, k)


@pytest.mark.parametrize("name", ["lattice", "ellipsoid", "clusters", "coincident"])
def test_mean_dist_with_ties_far_cells_and_duplicates(dev, name):
    """lattice: exact ties; ellipsoid: 1 cm of structure at coordinates of 1000; clusters: the 5 points midway have all their neighbours
    in far cells; coincident: 100 equal points, more duplicates than k + 1: every term is 0"""
    import torch
    from dispu_amd.outliers import knn_mean_distance
    a = Abi(dev, [cloud(name)])
    for k in ALL_K:
        rc, md, status = a.mean_dist(k)
        assert rc == 0 and status[0] == 0
        want = oracle_md(name, k)
        assert np.array_equal(bits(md), bits(want)), (k, np.nonzero(md != want)[0][:10])
    one = knn_mean_distance(torch.from_numpy(cloud(name)).to(dev))                                   # a tensor in, a tensor out, k = 16
    assert isinstance(one, torch.Tensor) and np.array_equal(bits(N(one)), bits(oracle_md(name, 16)))
    if name == "coincident":
        assert not oracle_md(name, 16).any()


# ---- the radius count, exact ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 4, INT_MAX])
def test_radius_count_on_the_lattice(dev, cap):
    """at r = 1 the axis neighbours lie at d2 = r2 exactly and must count: 3 .. 6 of them"""
    a = Abi(dev, [cloud("lattice")])
    for radius in (1.0, 1.5, 2.0):
        rc, cnt, status = a.count(radius, cap)
        want = O.radius_count(cloud("lattice"), radius, None if cap == INT_MAX else cap)
        assert rc == 0 and status[0] == 0 and np.array_equal(cnt, want), (radius, cap)
        if cap == INT_MAX and radius == 1.0:
            assert cnt.min() == 3 and cnt.max() == 6
        if cap != INT_MAX:
            assert (cnt == cap).any() and cnt.max() == cap      # saturated at the cap


@pytest.mark.parametrize("name", ["sphere", "ellipsoid"])
def test_radius_count_at_about_16_neighbours(dev, name):
    import torch
    from dispu_amd.outliers import radius_neighbor_count
    radius = radius_for_16(name)
    exact = O.radius_count(cloud(name), radius)
    assert 12 <= np.median(exact) <= 20
    a = Abi(dev, [cloud(name)])
    for cap in (1, 4, INT_MAX):
        rc, cnt, status = a.count(radius, cap)
        assert rc == 0 and status[0] == 0 and np.array_equal(cnt, np.minimum(exact, cap)), cap
    p = torch.from_numpy(cloud(name)).to(dev)
    got = radius_neighbor_count(p, radius)
    assert got.dtype == torch.int32 and np.array_equal(N(got), exact)
    assert np.array_equal(N(radius_neighbor_count(p, radius, cap=4)), np.minimum(exact, 4))


# ---- threshold and mask -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", O.MASK_K)
def test_statistics_and_kept_indices(dev, k):
    """stats against float64 numpy to 1e-10 relative: for n <= 4127 positive terms any summation order stays within n * 2^-53 = 5e-13.
    The kept indices equal the oracle's exactly once no oracle mean_dist lies within 1e-9 relative of the oracle threshold."""
    import torch
    from dispu_amd.outliers import remove_statistical_outliers
    clouds = [cloud(name) for name in O.MASK_CLOUDS]
    a = Abi(dev, clouds)
    rc, md, status = a.mean_dist(k)
    assert rc == 0 and not status.any()
    want_md = [oracle_md(name, k) for name in O.MASK_CLOUDS]
    assert np.array_equal(bits(md), bits(np.concatenate(want_md)))
    dclouds = [torch.from_numpy(c).to(dev) for c in clouds]
    for ratio in O.MASK_RATIO:
        rc, stats = a.threshold(ratio)
        assert rc == 0
        want = [O.statistical_keep(c, k, ratio, md=m) for c, m in zip(clouds, want_md)]
        for c, (keep, st, m) in enumerate(want):
            rel = np.abs(stats[c] - np.float64(st)) / np.float64(st)
            print(O.MASK_CLOUDS[c], k, ratio, "stats", stats[c], "relative error", rel, "band", O.band(m, st[2]))
            assert (rel <= 1e-10).all(), (c, ratio, rel)
            assert O.band(m, st[2]) > O.BAND
        rc, pts, idx, new_off = a.compact(1, a.md, a.stats)
        assert rc == 0
        assert np.array_equal(new_off, offsets([w[0] for w in want]))
        kept = new_off[-1]
        assert np.array_equal(idx[:kept], np.concatenate([w[0] for w in want]).astype(np.int32))
        assert np.array_equal(bits(pts[:kept]), bits(np.concatenate([c[w[0]] for c, w in zip(clouds, want)])))     # input order
        assert (pts[kept:] == 7).all() and (idx[kept:] == -7).all()
        got, gidx, gstats = remove_statistical_outliers(dclouds, k=k, std_ratio=ratio, return_index=True, return_stats=True)
        for c, (keep, st, _) in enumerate(want):
            assert gidx[c].dtype == torch.int64 and np.array_equal(N(gidx[c]), keep)
            assert np.array_equal(bits(N(got[c])), bits(clouds[c][keep]))
            assert np.array_equal(N(gstats[c]), stats[c])


def test_planted_strays_are_removed(dev):
    import torch
    from dispu_amd.outliers import remove_statistical_outliers
    p = torch.from_numpy(cloud("planted4097")).to(dev)
    kept, idx = remove_statistical_outliers(p, return_index=True)                                    # k = 16, std_ratio = 2
    assert kept.shape == (4097, 3) and np.array_equal(N(idx), np.arange(4097))
    same = torch.from_numpy(cloud("coincident")).to(dev)
    kept, idx, st = remove_statistical_outliers(same, return_index=True, return_stats=True)          # all duplicates: everything stays
    assert kept.shape == (100, 3) and np.array_equal(N(idx), np.arange(100)) and not N(st).any()


def test_compact_by_plain_flags(dev):
    import torch
    clouds = [cloud("sphere")[:1], cloud("sphere")[:65], cloud("sphere")[:2049]]
    r = np.random.RandomState(4)
    flags = (r.random_sample(1 + 65 + 2049) < 0.5).astype(np.int32) * r.randint(1, 9, 1 + 65 + 2049).astype(np.int32)
    flags[0] = 0                                                # a segment that keeps nothing
    a = Abi(dev, clouds)
    rc, pts, idx, new_off = a.compact(0, torch.from_numpy(flags).to(dev), status=False)
    assert rc == 0
    off = offsets(clouds)
    keep = [np.nonzero(flags[off[c]:off[c + 1]])[0] for c in range(3)]
    assert np.array_equal(new_off, offsets(keep)) and new_off[1] == 0
    assert np.array_equal(idx[:new_off[-1]], np.concatenate(keep).astype(np.int32))
    assert np.array_equal(bits(pts[:new_off[-1]]), bits(np.concatenate([c[k] for c, k in zip(clouds, keep)])))


SCAN_TOTALS = (524289, 1050625)                                # rows in all: 257 and 514 tile sums in the scan of the flags


@pytest.mark.parametrize("total", SCAN_TOTALS)
def test_compact_past_one_scan_sum_per_thread(dev, total):
    """more than 256 tile sums in the device-wide scan of the flags: 257 sums (two per thread of the one-workgroup tier, the last threads
    idle) and 514 (three per thread); tests/test_second_trips.py restates the thresholds.  Three ragged clouds: about half kept, nothing
    kept, everything kept; the expected rows come from the numpy mask."""
    import torch
    sizes = (total - 4099 - 70001, 4099, 70001)
    r = np.random.RandomState(total % 1000)
    packed = r.random_sample((total, 3)).astype(np.float32)
    off = np.zeros(4, np.int32)
    np.cumsum(sizes, out=off[1:])
    clouds = [packed[off[c]:off[c + 1]] for c in range(3)]
    flags = (r.random_sample(total) < 0.5).astype(np.int32) * r.randint(1, 9, total).astype(np.int32)
    flags[off[1]:off[2]] = 0                                    # a segment that keeps nothing
    flags[off[2]:] = r.randint(-9, 0, sizes[2]).astype(np.int32)  # and one that keeps everything (any non-zero word is a flag)
    a = Abi(dev, clouds)
    rc, pts, idx, new_off = a.compact(0, torch.from_numpy(flags).to(dev), status=False)
    assert rc == 0
    mask = flags != 0
    kept = int(mask.sum())
    assert 0.45 * sizes[0] < mask[:off[1]].sum() < 0.55 * sizes[0]
    local = np.arange(total, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), sizes)
    want_off = np.concatenate([[0], np.cumsum([mask[off[c]:off[c + 1]].sum() for c in range(3)])]).astype(np.int32)
    assert np.array_equal(new_off, want_off) and new_off[1] == new_off[2] and new_off[3] - new_off[2] == sizes[2] and new_off[3] == kept
    assert np.array_equal(idx[:kept], local[mask].astype(np.int32))
    assert np.array_equal(bits(pts[:kept]), bits(packed[mask]))
    assert (pts[kept:] == 7).all() and (idx[kept:] == -7).all()                                       # nothing behind the kept rows is touched


# ---- batches, repeats, flagged segments -------------------------------------------------------------------------------------------------

def test_ragged_batch_equals_each_cloud_alone(dev):
    import torch
    from dispu_amd.outliers import remove_radius_outliers, remove_statistical_outliers
    sizes = (1, 65, 2049, 130)
    clouds = [cloud("sphere")[:n] for n in sizes]
    radius = 0.2
    a = Abi(dev, clouds)
    rc, md, status = a.mean_dist(16)
    rc2, cnt, status2 = a.count(radius, INT_MAX)
    assert rc == 0 and rc2 == 0 and not status.any() and not status2.any()
    o = 0
    for n, c in zip(sizes, clouds):
        one = Abi(dev, [c])
        assert np.array_equal(bits(md[o:o + n]), bits(one.mean_dist(16)[1])) and np.array_equal(bits(md[o:o + n]), bits(oracle_md("sphere", 16, n)))
        assert np.array_equal(cnt[o:o + n], one.count(radius, INT_MAX)[1]) and np.array_equal(cnt[o:o + n], O.radius_count(c, radius))
        o += n
    d = [torch.from_numpy(c).to(dev) for c in clouds]
    for fn, kw in ((remove_statistical_outliers, dict(k=8, std_ratio=1.0)), (remove_radius_outliers, dict(radius=radius, min_neighbors=3))):
        pts, idx = fn(d, return_index=True, **kw)
        for c in range(len(sizes)):
            p1, i1 = fn(d[c], return_index=True, **kw)
            assert np.array_equal(N(idx[c]), N(i1)) and np.array_equal(bits(N(pts[c])), bits(N(p1)))
            assert np.array_equal(bits(N(pts[c])), bits(clouds[c][N(idx[c])]))
    for c, n in enumerate(sizes):                               # the radius filter against the oracle
        assert np.array_equal(N(idx[c]), O.radius_keep(clouds[c], radius, 3))


def test_two_calls_give_identical_bytes(dev):
    clouds = [cloud("planted2000"), cloud("ellipsoid")]
    radius = radius_for_16("ellipsoid")
    runs = []
    for _ in range(2):
        a = Abi(dev, clouds)
        rc, md, _ = a.mean_dist(16)
        rc2, stats = a.threshold(2.0)
        rc3, pts, idx, new_off = a.compact(1, a.md, a.stats)
        rc4, cnt, _ = a.count(radius, INT_MAX)
        assert rc == 0 and rc2 == 0 and rc3 == 0 and rc4 == 0
        runs.append([x.tobytes() for x in (md, stats, pts, idx, new_off, cnt)])
    assert runs[0] == runs[1]


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_non_finite_segment_is_flagged_and_left_alone(dev, poison):
    import torch
    from dispu_amd import outliers as M
    a_, b_, c_ = cloud("sphere")[:300], cloud("plane")[:200].copy(), cloud("ellipsoid")[:129]
    b_[77, 1] = poison
    a = Abi(dev, [a_, b_, c_])
    rc, md, status = a.mean_dist(16)
    assert rc == 0 and list(status) == [0, 1, 0] and (md[300:500] == 7).all()
    rc, stats = a.threshold(2.0)
    assert rc == 0 and (stats[1] == 7).all() and (stats[0] != 7).all() and (stats[2] != 7).all()
    rc, pts, idx, new_off = a.compact(1, a.md, a.stats)
    assert rc == 0 and new_off[1] == new_off[2]                 # a flagged segment keeps nothing
    rc, cnt, status = a.count(0.1, INT_MAX)
    assert rc == 0 and list(status) == [0, 1, 0] and (cnt[300:500] == -7).all()
    for lo, hi, p in [(0, 300, a_), (500, 629, c_)]:
        one = Abi(dev, [p])
        assert np.array_equal(bits(md[lo:hi]), bits(one.mean_dist(16)[1])) and np.array_equal(cnt[lo:hi], one.count(0.1, INT_MAX)[1])
    d = [torch.from_numpy(x).to(dev) for x in (a_, b_, c_)]
    for fn, kw in ((M.knn_mean_distance, {}), (M.remove_statistical_outliers, {}), (M.radius_neighbor_count, dict(radius=0.1)),
                   (M.remove_radius_outliers, dict(radius=0.1))):
        with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):
            fn(d, **kw)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_python_entry_refusals(dev):
    import torch
    from dispu_amd import outliers as M
    p = torch.from_numpy(cloud("plane")).to(dev)
    for bad in (dict(k=0), dict(k=32), dict(k=16.0), dict(k=True)):
        with pytest.raises(ValueError):
            M.knn_mean_distance(p, **bad)
        with pytest.raises(ValueError):
            M.remove_statistical_outliers(p, **bad)
    for bad in (dict(std_ratio=np.nan), dict(std_ratio=np.inf), dict(std_ratio="2")):
        with pytest.raises(ValueError):
            M.remove_statistical_outliers(p, **bad)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=1e39), dict(radius=1e-46),
                dict(radius="1")):
        with pytest.raises(ValueError):
            M.radius_neighbor_count(p, **bad)
        with pytest.raises(ValueError):
            M.remove_radius_outliers(p, **bad)
    for bad in (dict(cap=0), dict(cap=2 ** 31), dict(cap=1.5)):
        with pytest.raises(ValueError):
            M.radius_neighbor_count(p, 0.1, **bad)
    for bad in (dict(min_neighbors=0), dict(min_neighbors=2.0)):
        with pytest.raises(ValueError):
            M.remove_radius_outliers(p, 0.1, **bad)
    for bad in (p.double(), p[:, :2], p.reshape(1, -1, 3), p[:0], p.cpu(), [], [p, p.cpu()], "cloud"):
        for fn, kw in ((M.knn_mean_distance, {}), (M.remove_statistical_outliers, {}), (M.radius_neighbor_count, dict(radius=0.1)),
                       (M.remove_radius_outliers, dict(radius=0.1))):
            with pytest.raises(ValueError):
                fn(bad, **kw)


def test_abi_refusals_touch_nothing(dev):
    p = [cloud("sphere")[:500], cloud("plane")[:300]]
    bad_offs = [dict(off=np.int32([0, 500, 400])), dict(off=np.int32([0, 500, 500])), dict(off=np.int32([1, 500, 800])), dict(C_arg=0),
                dict(C_arg=65536)]

    def fresh(**kw):
        return Abi(dev, p, **kw)

    for kw in bad_offs:
        a = fresh(**kw)
        rc, md, status = a.mean_dist(16)
        assert rc == INVALID and (md == 7).all() and (status == -7).all(), kw
        rc, cnt, status = a.count(0.1, 4)
        assert rc == INVALID and (cnt == -7).all() and (status == -7).all(), kw
        rc, stats = a.threshold(2.0)
        assert rc == INVALID and (stats == 7).all(), kw
        rc, pts, idx, new_off = a.compact(2, a.cnt, min_neighbors=1)
        assert rc == INVALID and (pts == 7).all() and (idx == -7).all() and (new_off == -7).all(), kw
    for kw in (dict(k=0), dict(k=32), dict(k=16, scratch="null"), dict(k=16, scratch="short"), dict(k=16, scratch="misaligned"),
               dict(k=16, null=("off",)), dict(k=16, null=("cloud",)), dict(k=16, null=("md",)), dict(k=16, null=("status",))):
        rc, md, status = fresh().mean_dist(**kw)
        assert rc == INVALID and (md == 7).all() and (status == -7).all(), kw
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(cap=0), dict(cap=-1),
               dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"), dict(null=("off",)), dict(null=("cloud",)),
               dict(null=("cnt",)), dict(null=("status",))):
        args = dict(radius=0.1, cap=4)
        args.update(kw)
        rc, cnt, status = fresh().count(**args)
        assert rc == INVALID and (cnt == -7).all() and (status == -7).all(), kw
    a = fresh()
    assert a.mean_dist(16)[0] == 0 and a.count(0.1, 4)[0] == 0                                  # the same calls, legal
    for kw in (dict(ratio=float("nan")), dict(ratio=float("inf")), dict(null=("off",)), dict(null=("md",)), dict(null=("status",)),
               dict(null=("stats",))):
        args = dict(ratio=2.0)
        args.update(kw)
        rc, stats = a.threshold(**args)
        assert rc == INVALID and (stats == 7).all(), kw
    assert a.threshold(2.0)[0] == 0
    for kw in (dict(rule=3), dict(rule=-1), dict(rule=1, stats=None), dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"),
               dict(null=("off",)), dict(null=("src",)), dict(null=("cloud",)), dict(null=("idx",)), dict(null=("new_off",))):
        args = dict(rule=1, src=a.md, stats=a.stats)
        args.update(kw)
        rc, pts, idx, new_off = a.compact(**args)
        assert rc == INVALID and (pts == 7).all() and (idx == -7).all() and (new_off == -7).all(), kw
    assert a.compact(1, a.md, a.stats)[0] == 0
    L = a.L
    hp = C.c_void_p(a.good.ctypes.data)
    assert L.dispu_knn_mean_dist_scratch_bytes(2, hp, 16) > 0 and L.dispu_radius_count_scratch_bytes(2, hp) > 0
    assert L.dispu_compact_scratch_bytes(2, hp) > 0
    assert L.dispu_knn_mean_dist_scratch_bytes(2, hp, 0) == 0 and L.dispu_knn_mean_dist_scratch_bytes(2, hp, 32) == 0
    big = np.int32([0, (1 << 24) + 1])
    for n_c, h in ((0, hp), (65536, hp), (1, C.c_void_p(big.ctypes.data))):                   # C = 0, too many, a segment above 2^24 points
        assert L.dispu_knn_mean_dist_scratch_bytes(n_c, h, 16) == 0 and L.dispu_radius_count_scratch_bytes(n_c, h) == 0
        assert L.dispu_compact_scratch_bytes(n_c, h) == 0


def test_radius_filter_may_remove_everything(dev):
    import torch
    from dispu_amd.outliers import remove_radius_outliers
    p = torch.from_numpy(cloud("lattice")).to(dev)
    kept, idx = remove_radius_outliers(p, 0.5, min_neighbors=1, return_index=True)                  # the nearest neighbour is 1 away
    assert kept.shape == (0, 3) and kept.dtype == torch.float32 and idx.shape == (0,) and idx.dtype == torch.int64
    both = remove_radius_outliers([p, p[:10]], 1.0, min_neighbors=3)
    assert both[0].shape == (729, 3) and both[1].shape[0] == int((O.radius_count(cloud("lattice")[:10], 1.0) >= 3).sum())


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------

def test_upsample_tool_cleans_its_output(dev, tmp_path):
    from dispu_amd import checkpoint as CK
    from oracle import generator as OG
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    np.savetxt(str(data / "test" / "ball.xyz"), O.sphere(2048, seed=9), fmt="%.6f")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    runs = {"plain": [], "off": ["--clean_input", "none", "--clean_output", "none"],
            "clean": ["--clean_output", "statistical", "--outliers_k", "8", "--outliers_std", "1.0"]}
    procs = {name: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for name, extra in runs.items()}
    for name, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    plain = open(str(tmp_path / "plain" / "ball_X4.xyz"), "rb").read()
    assert open(str(tmp_path / "off" / "ball_X4.xyz"), "rb").read() == plain
    rows, clean = plain.splitlines(), open(str(tmp_path / "clean" / "ball_X4.xyz"), "rb").read().splitlines()
    assert len(rows) == 4 * 2048 and 0 < len(clean) < len(rows)
    assert set(clean) <= set(rows)                              # every written row also occurs in the uncleaned output
    it = iter(rows)
    assert all(r in it for r in clean)                          # and in its order
