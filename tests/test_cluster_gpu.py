"""dis-pu_amd/clusters.py on the GPU against tests/cluster_oracle.py, BIT FOR BIT throughout (labels, core flags, sizes, counts, kept
indices and points): the labels are a pure function of the input, so there is no tolerance anywhere in this file.  The cases sit where
the kernels can go wrong, not at workload size: one lane, the 64-point cell edge, past 4096 points the second trip of the 64-box table
step, d2 == r2 exactly, a non-core bridge between two clusters, coincident points, deep chains, permuted input."""
import ctypes as C

import numpy as np
import pytest

import cluster_oracle as O

pytestmark = pytest.mark.gpu
INVALID = 1                                                      # hipErrorInvalidValue
G = 1.0 / 16.0
SIZES = (1, 2, 63, 64, 65, 500, 4200)
_ORACLE = {}


def cloud(n, seed):
    """n points: two blobs of different density and a few strays, so that every n has clusters, borders and noise"""
    g = np.random.RandomState(1000 + seed)
    a = g.randn(n - n // 3, 3) * 0.08
    b = g.randn(n // 3, 3) * 0.05 + np.float32([0.9, 0.1, 0.0])
    p = np.concatenate([a, b]).astype(np.float32)
    p[::17] = g.uniform(-1.5, 1.5, p[::17].shape)
    return g.permutation(p)


def oracle(key, p, eps, mp):
    """computed once per case and shared"""
    if key not in _ORACLE:
        _ORACLE[key] = tuple(a.copy() for a in O.dbscan(p, eps, mp))
        for a in _ORACLE[key]:
            a.setflags(write=False)
    return _ORACLE[key]


def run(dev, p, eps, mp):
    """one cloud or a list of numpy clouds -> (labels, core, sizes) as numpy, per cloud"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import clusters as M
    if isinstance(p, list):
        out = M.dbscan([torch.from_numpy(c).to(dev) for c in p], eps, mp, return_core=True, return_sizes=True)
        return [tuple(t.cpu().numpy() for t in one) for one in zip(*out)]
    return tuple(t.cpu().numpy() for t in M.dbscan(torch.from_numpy(p).to(dev), eps, mp, return_core=True, return_sizes=True))


def run_abi(dev, clouds, eps, mp, scratch="ok", scratch_buf=None):
    """dispu_cluster_segments itself on a packed batch (run() goes through clusters.py, which allocates its own scratch), every output
    pre-filled with a sentinel -> dict(rc, labels, core, sizes, nclusters, status).  scratch_buf: the caller's own scratch
    (tests/scratch_contract.py: .ptr(), .nbytes) in place of a zero-filled one; scratch "short": one byte less than that"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    total, nC = int(off[-1]), len(clouds)
    cloud_t = torch.from_numpy(np.concatenate(clouds).astype(np.float32)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    full = L.dispu_cluster_scratch_bytes(nC, C.c_void_p(off.ctypes.data))
    assert full > 0
    buf = torch.zeros((full,), dtype=torch.uint8, device=dev)
    assert scratch in ("ok", "short")
    sp, sb = (p(buf), full) if scratch_buf is None else (scratch_buf.ptr(), scratch_buf.nbytes)
    if scratch == "short":
        sb -= 1
    labels = torch.full((total,), -7, dtype=torch.int32, device=dev)
    core = torch.full((total,), 9, dtype=torch.uint8, device=dev)
    sizes = torch.full((total,), -7, dtype=torch.int32, device=dev)
    ncl = torch.full((nC,), -7, dtype=torch.int32, device=dev)
    status = torch.full((nC,), -7, dtype=torch.int32, device=dev)
    rc = L.dispu_cluster_segments(nC, p(d_off), C.c_void_p(off.ctypes.data), eps, mp, p(cloud_t), p(labels), p(core), p(sizes), p(ncl),
                                  p(status), sp, sb, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    if scratch_buf is not None:
        scratch_buf.inputs = dict(cloud=cloud_t.cpu().numpy(), off=d_off.cpu().numpy())    # as the call left them
    return dict(rc=rc, labels=labels.cpu().numpy(), core=core.cpu().numpy(), sizes=sizes.cpu().numpy(), nclusters=ncl.cpu().numpy(),
                status=status.cpu().numpy())


def check(got, want):
    labels, core, sizes = got
    assert labels.dtype == np.int32 and core.dtype == np.bool_ and sizes.dtype == np.int32
    assert np.array_equal(core, want[1])
    assert np.array_equal(labels, want[0])
    assert sizes.shape == want[2].shape and np.array_equal(sizes, want[2])


@pytest.mark.parametrize("mp", [1, 2, 6])
def test_batch_of_every_size_as_a_list_and_one_by_one(dev, mp):
    eps = 0.06
    clouds = [cloud(n, i) for i, n in enumerate(SIZES)]
    want = [oracle(("sizes", n, mp), c, eps, mp) for n, c in zip(SIZES, clouds)]
    got = run(dev, clouds, eps, mp)
    for g, w in zip(got, want):
        check(g, w)
    for c, g in zip(clouds, got):                                # the labels of a list call equal those of the per-cloud calls
        one = run(dev, c, eps, mp)
        for a, b in zip(one, g):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,eps,mp", O.SHELL_CASES)
def test_sphere_shells_plus_strays(dev, n, eps, mp):
    p = O.shells(n)
    check(run(dev, p, eps, mp), oracle(("shells", n), p, eps, mp))


def test_min_points_above_n_makes_everything_noise(dev):
    import torch
    from dispu_amd import clusters as M
    p = cloud(500, 5)
    labels, core, sizes = run(dev, p, 0.06, 501)
    assert (labels == -1).all() and not core.any() and sizes.shape == (0,)
    t = torch.from_numpy(p).to(dev)
    pts, idx, lab = M.keep_clusters(t, 0.06, min_points=501, return_index=True, return_labels=True)
    assert tuple(pts.shape) == (0, 3) and tuple(idx.shape) == (0,) and bool((lab == -1).all())
    pts = M.keep_clusters([t, t[:64]], 0.06, min_points=501)
    assert [tuple(x.shape) for x in pts] == [(0, 3), (0, 3)]


def lattice(m):
    """m^3 points at spacing 0.25: every d2 is exact"""
    a = np.arange(m, dtype=np.float32) * np.float32(0.25)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("mp", [1, 2, 7])
def test_exact_ties_exist_only_because_the_boundary_is_included(dev, mp):
    p = np.random.RandomState(3).permutation(lattice(5))          # 125 points: two cells
    labels, core, sizes = got = run(dev, p, 0.25, mp)
    check(got, oracle(("lattice", mp), p, 0.25, mp))
    if mp <= 2:
        assert sizes.tolist() == [125]                           # one cluster, through pairs at d2 == r2 only
    else:                                                        # 27 interior core points, 54 face points as borders at tied d2 == r2;
        assert core.sum() == 27 and sizes.tolist() == [81]       # the 44 edge and corner points touch no core point: noise
    below = float(np.nextafter(np.float32(0.25), np.float32(0.0)))
    labels, core, sizes = got = run(dev, p, below, mp)
    check(got, oracle(("lattice below", mp), p, below, mp))
    if mp == 1:
        assert labels.tolist() == list(range(125)) and sizes.tolist() == [1] * 125
    else:
        assert (labels == -1).all() and sizes.shape == (0,)


def bridge(first):
    a = np.float32([[0, 0, 0], [0, G, 0], [0, 0, G], [0, G, G]])
    b = a + np.float32([8 * G, 0, 0])
    return np.concatenate(([a, b] if first == "a" else [b, a]) + [np.float32([[4 * G, 0, 0]])])


@pytest.mark.parametrize("first", ["a", "b"])
def test_a_non_core_bridge_never_joins_two_clusters(dev, first):
    p = bridge(first)
    labels, core, sizes = got = run(dev, p, 4 * G, 4)
    check(got, oracle(("bridge", first), p, 4 * G, 4))
    assert core.tolist() == [True] * 8 + [False] and sizes.tolist() == [5, 4]
    assert labels.tolist() == [0] * 4 + [1] * 4 + [0]             # equidistant: to the core point of smaller index


def test_bridge_inside_a_large_cloud(dev):
    """the same trap with the bridge and the blobs in different cells: 70 copies of every blob point.  The bridge counts itself and
    2 x 70 points, a blob point 4 x 70 (one of them the bridge too): min_points = 200 separates them"""
    p = bridge("a")
    p = np.concatenate([np.repeat(p[:4], 70, 0), np.repeat(p[4:8], 70, 0), p[8:]])
    p = np.random.RandomState(2).permutation(p)
    labels, core, sizes = got = run(dev, p, 4 * G, 200)
    check(got, oracle(("bridge large",), p, 4 * G, 200))
    assert sizes.shape == (2,) and sizes.sum() == len(p) and core.sum() == len(p) - 1


@pytest.mark.parametrize("n,mp", [(1, 1), (1, 2), (64, 64), (64, 65), (200, 200), (200, 201)])
def test_coincident_points(dev, n, mp):
    p = np.zeros((n, 3), np.float32) + np.float32(0.37)
    labels, core, sizes = got = run(dev, p, 0.01, mp)
    check(got, oracle(("coincident", n, mp), p, 0.01, mp))
    assert (labels == (0 if n >= mp else -1)).all()


def test_duplicates_of_a_core_point_and_two_far_groups_in_one_cloud(dev):
    g = np.random.RandomState(7)
    a = (g.randn(300, 3) * 0.05).astype(np.float32)
    a[100:140] = a[7]                                            # 40 duplicates of one point
    b = (g.randn(300, 3) * 0.05).astype(np.float32) + np.float32([1e6, -1e6, 1e6])
    p = g.permutation(np.concatenate([a, b]))
    got = run(dev, p, 0.04, 5)
    check(got, oracle(("far",), p, 0.04, 5))
    assert got[2].shape[0] >= 2


@pytest.mark.parametrize("order", ["input", "reversed", "shuffled"])
def test_a_line_of_4200_points_is_one_cluster_in_any_order(dev, order):
    eps = 0.01
    x = np.arange(4200, dtype=np.float64) * (0.9 * eps)
    p = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1).astype(np.float32)
    if order == "reversed":
        p = p[::-1].copy()
    elif order == "shuffled":
        p = np.random.RandomState(11).permutation(p)
    labels, core, sizes = run(dev, p, eps, 2)                    # a set cap status would raise RuntimeError here
    assert core.all() and (labels == 0).all() and sizes.tolist() == [4200]
    check((labels, core, sizes), oracle(("line", order), p, eps, 2))


@pytest.mark.parametrize("mp", [1, 5])
def test_a_permutation_gives_the_same_partition_renumbered(dev, mp):
    p = cloud(1500, 9)
    perm = np.random.RandomState(5).permutation(len(p))
    l0, c0, s0 = got0 = run(dev, p, 0.05, mp)
    l1, c1, s1 = got1 = run(dev, p[perm], 0.05, mp)
    check(got0, oracle(("perm", mp, 0), p, 0.05, mp))
    check(got1, oracle(("perm", mp, 1), p[perm], 0.05, mp))
    assert np.array_equal(c1, c0[perm])
    m0 = l0[perm]                                                # the first run's labels at the permuted positions
    assert np.array_equal(m0 == -1, l1 == -1)
    pairs = set(zip(m0[m0 >= 0].tolist(), l1[l1 >= 0].tolist()))
    assert len(pairs) == len(s0) == len(s1)                      # a bijection between the two numberings
    first = {}
    for i in np.nonzero(c1)[0]:                                  # the numbering follows the permuted smallest core index
        first.setdefault(int(l1[i]), int(i))
    assert [first[k] for k in range(len(s1))] == sorted(first.values())


def test_two_runs_give_identical_bytes(dev):
    import torch
    from dispu_amd import clusters as M
    ts = [torch.from_numpy(cloud(n, 20 + i)).to(dev) for i, n in enumerate((4200, 777))]
    a = M.dbscan(ts, 0.05, 4, return_core=True, return_sizes=True)
    b = M.dbscan(ts, 0.05, 4, return_core=True, return_sizes=True)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    ka = M.keep_clusters(ts, 0.05, min_points=4, keep=2)
    kb = M.keep_clusters(ts, 0.05, min_points=4, keep=2)
    for u, v in zip(ka, kb):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


def blobs():
    """five far-apart blobs of sizes 30, 50, 50, 8, 20 (clusters 0 .. 4 in input order): more clusters than keep, one size tie"""
    g = np.random.RandomState(4)
    parts = [(g.rand(m, 3) * 0.05).astype(np.float32) + np.float32([3.0 * i, 0, 0]) for i, m in enumerate((30, 50, 50, 8, 20))]
    return np.concatenate(parts)


@pytest.mark.parametrize("keep,min_size", [(1, 1), (2, 1), (3, 1), (32, 1), (32, 25), (2, 51), (4, 9)])
def test_keep_clusters(dev, keep, min_size):
    import torch
    from dispu_amd import clusters as M
    p = blobs()
    labels, core, sizes = oracle(("blobs",), p, 0.1, 1)
    assert sizes.tolist() == [30, 50, 50, 8, 20]
    want = O.keep(labels, sizes, keep, min_size)
    t = torch.from_numpy(p).to(dev)
    pts, idx, lab = M.keep_clusters(t, 0.1, min_points=1, keep=keep, min_size=min_size, return_index=True, return_labels=True)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(lab.cpu().numpy(), labels)
    assert pts.cpu().numpy().tobytes() == p[want].tobytes()      # the kept points equal points[index] bit for bit
    if (keep, min_size) == (1, 1):
        assert set(labels[want].tolist()) == {1}                 # the size tie 50 = 50 goes to the smaller id
    # in a batch, beside a cloud with other clusters
    q = cloud(500, 31)
    lq, _, sq = oracle(("blobs q",), q, 0.06, 1)
    out = M.keep_clusters([torch.from_numpy(q).to(dev), t], 0.06, min_points=1, keep=keep, min_size=min_size, return_index=True)
    assert np.array_equal(out[1][0].cpu().numpy(), O.keep(lq, sq, keep, min_size))
    l2, _, s2 = oracle(("blobs 0.06",), p, 0.06, 1)
    assert np.array_equal(out[1][1].cpu().numpy(), O.keep(l2, s2, keep, min_size))
    assert out[0][0].cpu().numpy().tobytes() == q[O.keep(lq, sq, keep, min_size)].tobytes()


def test_refusals(dev):
    import torch
    from dispu_amd import clusters as M
    t = torch.from_numpy(cloud(100, 1)).to(dev)
    bad = t.clone()
    bad[5, 1] = float("nan")
    for fn in (M.dbscan, M.keep_clusters):
        with pytest.raises(ValueError, match="cloud 1 holds a NaN"):          # after the launch
            fn([t, bad, t], 0.1)
        for eps in (0.0, -1.0, float("nan"), float("inf"), 1e39, "0.1", True):
            with pytest.raises(ValueError, match="radius"):
                fn(t, eps)
        for mp in (0, -3, 2.0, True, 2 ** 31):
            with pytest.raises(ValueError, match="min_points"):
                fn(t, 0.1, min_points=mp)
    for keep in (0, 33, 1.0):
        with pytest.raises(ValueError, match="keep"):
            M.keep_clusters(t, 0.1, keep=keep)
    with pytest.raises(ValueError, match="min_size"):
        M.keep_clusters(t, 0.1, min_size=0)
    bad[5, 1] = float("inf")
    with pytest.raises(ValueError, match="cloud 0 holds a NaN or an infinite"):
        M.dbscan(bad, 0.1)


def test_raw_abi_refuses_null_pointers_and_bad_arguments(dev):
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    good, short = np.int32([0, 5, 8]), np.int32([0, 0])
    ok, bad = C.c_void_p(good.ctypes.data), C.c_void_p(short.ctypes.data)
    assert L.dispu_cluster_scratch_bytes(1, bad) == 0 and L.dispu_cluster_scratch_bytes(0, ok) == 0
    nb = L.dispu_cluster_scratch_bytes(2, ok)
    assert nb > 0
    cl = torch.rand((8, 3), generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    d_off = torch.from_numpy(good).to(dev)
    scratch = torch.zeros((nb,), dtype=torch.uint8, device=dev)
    i = torch.full((8,), -7, dtype=torch.int32, device=dev)
    b = torch.full((8,), 9, dtype=torch.uint8, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    N = None

    def cluster(nC=2, off=d_off, offh=ok, eps=0.5, mp=2, cloud=cl, labels=i, ncl=i, stat=status, scr=scratch, nbytes=nb):
        return L.dispu_cluster_segments(nC, p(off), offh, eps, mp, p(cloud), p(labels), p(b), p(i), p(ncl), p(stat), p(scr), nbytes, st)

    def select(nC=2, off=d_off, offh=ok, labels=i, sizes=i, ncl=i, stat=status, keep=1, min_size=1, flags=i):
        return L.dispu_cluster_select_segments(nC, p(off), offh, p(labels), p(sizes), p(ncl), p(stat), keep, min_size, p(flags), st)

    rcs = {
        "bad offsets": cluster(nC=1, offh=bad), "C = 0": cluster(nC=0), "eps = 0": cluster(eps=0.0), "eps < 0": cluster(eps=-1.0),
        "eps nan": cluster(eps=float("nan")), "eps inf": cluster(eps=float("inf")), "min_points = 0": cluster(mp=0),
        "off null": cluster(off=N), "cloud null": cluster(cloud=N), "labels null": cluster(labels=N), "nclusters null": cluster(ncl=N),
        "status null": cluster(stat=N), "scratch null": cluster(scr=N), "scratch short": cluster(nbytes=nb - 1),
        "select: bad offsets": select(nC=1, offh=bad), "select: keep = 0": select(keep=0), "select: keep = 33": select(keep=33),
        "select: min_size = 0": select(min_size=0), "select: off null": select(off=N), "select: labels null": select(labels=N),
        "select: sizes null": select(sizes=N), "select: nclusters null": select(ncl=N), "select: status null": select(stat=N),
        "select: flags null": select(flags=N),
    }
    torch.cuda.synchronize(dev)
    assert rcs == {k: INVALID for k in rcs}
    assert bool((i == -7).all()) and bool((b == 9).all()) and bool((status == -7).all()) and not bool(scratch.any())
