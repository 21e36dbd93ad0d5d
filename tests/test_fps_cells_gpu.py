"""The cell-skipping farthest point sampling for large clouds (csrc/fps_cells.hip: dispu_fps_cells, dispu_fps_segments_auto) against
oracle.farthest_point_sample, bit for bit, in both arithmetic flavours.  Everything goes through dispu_fps_cells or path="cells", so
the new kernels run whatever dispu_fps_cells_wanted says."""
import functools

import numpy as np
import pytest
import torch

from oracle import generator as OG
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S = 64                                                   # the automatic cell size at small n
CELLS = [64, 128, 256, 512, 1024, 2048, 4096]            # every cell size the dispatch can choose


def N(t):
    return t.detach().cpu().numpy()


def _cloud(rng, n, dup=False):
    """the layout of tests/test_ragged_gpu.py:_cloud"""
    pc = rng.random((n, 3)).astype(np.float32)
    if n > 10:
        pc[10] = pc[3]
    if dup and n > 1:
        h = n // 2
        pc[h:] = pc[:n - h]                              # every point twice, half a cloud apart in index
    return pc


def _sphere(rng, n):
    g = rng.standard_normal((n, 3))
    pc = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    pc[n // 3] = pc[5]
    pc[n - 1] = pc[n // 2]
    pc[7] = pc[700 % n]
    return pc


def _cells(dev, clouds, ms, arith, cell=0, path="cells"):
    from dispu_amd import upsample as U
    off, moff = U.segment_offsets([c.shape[0] for c in clouds]), U.segment_offsets(ms)
    got = N(U.fps_segments(torch.from_numpy(np.concatenate(clouds)).to(dev), off, moff, arith=arith, path=path, cell=cell))
    return [got[moff[c]:moff[c + 1]] for c in range(len(clouds))]


def _want(pc, m, arith):
    return O.farthest_point_sample(m, pc[None], contract=arith)[0]


def _check(dev, clouds, ms, arith, cell=0):
    for pc, m, got in zip(clouds, ms, _cells(dev, clouds, ms, arith, cell)):
        want = _want(pc, m, arith)
        assert np.array_equal(got, want), (pc.shape[0], m, arith, cell, int(np.argmax(got != want)))


@pytest.mark.parametrize("arith", [0, 1])
def test_cell_edges(dev, arith):
    rng = np.random.default_rng(1 + arith)
    shapes = [(n, m) for n in (1, 2, 63, S - 1, S, S + 1, 3 * S + 5) for m in sorted({1, 2, n})] + [(300, 700)]
    clouds = [_cloud(rng, n) for n, _ in shapes]
    for pc, (_, m) in zip(clouds, shapes):               # each cloud alone ...
        _check(dev, [pc], [m], arith)
    _check(dev, clouds, [m for _, m in shapes], arith)  # ... and all of them as one ragged batch


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("n,m,dup", [(24577, 2000, False), (40000, 64, True), (30000, 3, True)])
def test_across_the_threshold(dev, arith, n, m, dup):
    _check(dev, [_cloud(np.random.default_rng(n + arith), n, dup)], [m], arith)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("shuffled", [False, True])
def test_mass_ties_on_a_lattice(dev, arith, shuffled):
    g = np.arange(32, dtype=np.float32) / 32
    pc = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    if shuffled:
        pc = pc[np.random.default_rng(5).permutation(len(pc))]
    _check(dev, [np.ascontiguousarray(pc)], [3000], arith)


@pytest.mark.parametrize("arith", [0, 1])
def test_degenerate_geometry(dev, arith):
    rng = np.random.default_rng(7 + arith)
    same = np.tile(rng.random((1, 3)).astype(np.float32), (1000, 1))
    got = _cells(dev, [same], [10], arith)[0]
    assert np.array_equal(got, np.zeros(10, np.int32))   # every pick after the first is index 0 by the tie rule
    assert np.array_equal(got, _want(same, 10, arith))
    plane = rng.random((5000, 3)).astype(np.float32)
    plane[:, 2] = 0.25
    line = np.outer(rng.random(5000), np.array([1.0, -2.0, 0.5])).astype(np.float32) + np.float32(0.3)
    _check(dev, [plane, line], [500, 500], arith)
    far = rng.random((26000, 3)).astype(np.float32) * np.float32(1e-3) + np.float32(1e3)   # tiny extent far out: many rounded duplicates
    _check(dev, [far], [1000], arith)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("cell", CELLS)
def test_every_cell_size(dev, arith, cell):
    _check(dev, [_sphere(np.random.default_rng(3), 50021)], [2000], arith, cell)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("n,m", [(70001, 600), (140003, 300), (200000, 200)])
def test_more_than_1024_cells(dev, arith, n, m):
    """above 65536 points a thread owns 2, 3 or 4 cells (1094 / 2188 / 3125 cells of 64): the slot loop of the sampling kernel"""
    _check(dev, [_sphere(np.random.default_rng(n), n)], [m], arith)


SLOT_BOUNDARY = (262144, 262145)                         # 4096 cells of 64: the full slot loop; one point more: 2049 cells of 128
MANY = {257: (1, 63, 64, 65, 130), 65535: (1, 2, 3)}     # segments: sizes in a cycle


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("n", SLOT_BOUNDARY)
def test_at_the_slot_boundary(dev, arith, n):
    """the automatic cell size: the last n that keeps cells of 64 (exactly 4096 of them: every slot of the sampling kernel's cell loop
    is taken) and the first that doubles them (tests/test_second_trips.py restates both from the sources).  One planted point is the
    strict maximum of all three axes: its Morton code is the largest, so it sorts into the last cell (at 262145 points that cell's only
    point), and as the farthest point from everything it is the second pick -- a sampler that drops the last cell or slot misses it."""
    pc = _sphere(np.random.default_rng(n), n)
    plant = n // 7
    pc[plant] = np.float32([3.0, 3.0, 3.0])                # the far corner of the box: Morton cell (1023, 1023, 1023)
    assert (pc[plant] > np.delete(pc, plant, axis=0).max(axis=0)).all()
    assert _want(pc, 64, arith)[1] == plant
    _check(dev, [pc], [64], arith)


def _cells_packed(dev, packed, off, moff, arith):
    """dispu_fps_cells itself on packed arrays -> (idx, status)"""
    from dispu_amd import _lib
    L = _lib.lib()
    hp = lambda a: _lib.C.c_void_p(a.ctypes.data)
    nC = len(off) - 1
    x = torch.from_numpy(packed).to(dev)
    d_off, d_moff = torch.from_numpy(off).to(dev), torch.from_numpy(moff).to(dev)
    need = L.dispu_fps_cells_scratch_bytes(nC, hp(off), hp(moff), 0)
    assert need > 0
    sc = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = torch.full((int(moff[-1]),), -1, dtype=torch.int32, device=dev)
    status = torch.full((nC,), 9, dtype=torch.int32, device=dev)
    _lib.check(L.dispu_fps_cells(nC, _lib.ptr(d_off), _lib.ptr(d_moff), hp(off), hp(moff), _lib.ptr(x), _lib.ptr(sc), need, _lib.ptr(out),
                                 _lib.ptr(status), arith, 0, _lib.stream_ptr(dev)), "dispu_fps_cells")
    torch.cuda.synchronize()
    return N(out), N(status)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("nC", sorted(MANY))
def test_many_segments(dev, arith, nC):
    """9 and 16 segment bits above the 30 Morton bits of the pre-pass's keys: sorting passes 5 and 6, c << 30 with large c.  One packed
    call, m_c = min(n_c, 5); the oracle runs once per distinct cloud and is asserted for every repeat of it at its own offset."""
    cycle = MANY[nC]
    rng = np.random.default_rng(nC + arith)
    distinct = {n: _cloud(rng, n) for n in cycle}
    sizes = np.array(cycle)[np.arange(nC) % len(cycle)]
    ms = np.minimum(sizes, 5)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    moff = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
    got, status = _cells_packed(dev, np.concatenate([distinct[n] for n in sizes]), off, moff, arith)
    assert not status.any()
    for n in cycle:
        want = _want(distinct[n], min(n, 5), arith)
        rows = moff[:-1][sizes == n][:, None] + np.arange(min(n, 5))[None, :]
        assert (got[rows] == want[None, :]).all(), n


@pytest.mark.parametrize("arith", [0, 1])
def test_ragged_and_batched(dev, arith):
    from dispu_amd.tf_sampling import farthest_point_sample
    rng = np.random.default_rng(13 + arith)
    clouds = [_cloud(rng, 1), _cloud(rng, 300), _cloud(rng, 24577), _cloud(rng, 30000, True), _cloud(rng, 5000)]
    _check(dev, clouds, [1, 450, 700, 64, 1200], arith)
    x = rng.random((3, 26000, 3)).astype(np.float32)
    got = N(farthest_point_sample(3, torch.from_numpy(x).to(dev), arith=arith, path="cells"))
    assert np.array_equal(got, O.farthest_point_sample(3, x, contract=arith))


@pytest.mark.parametrize("arith", [0, 1])
def test_auto_entry_equals_segments_on_every_family(dev, arith):
    from dispu_amd import _lib
    from dispu_amd import upsample as U
    from test_ragged_gpu import FPS_CASES
    from test_ragged_gpu import _cloud as ragged_cloud
    rng = np.random.default_rng(11 + arith)
    cases = FPS_CASES + [(30000, 1000, True), (26000, 700, False)]     # two segments the rule may send to the cell kernels
    clouds = [ragged_cloud(rng, n, d) for n, _, d in cases]
    off, moff = U.segment_offsets([c.shape[0] for c in clouds]), U.segment_offsets([m for _, m, _ in cases])
    x = torch.from_numpy(np.concatenate(clouds)).to(dev)
    want = N(U.fps_segments(x, off, moff, arith=arith, path="stream"))
    # the C entry itself, with a canary behind its stated scratch and the status it reports
    L = _lib.lib()
    hp = lambda a: _lib.C.c_void_p(a.ctypes.data)
    C = len(cases)
    need = L.dispu_fps_segments_auto_scratch_bytes(C, hp(off), hp(moff))
    assert need >= L.dispu_fps_segments_scratch_bytes(C, hp(off), hp(moff))
    sc = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    out = torch.full((int(moff[-1]),), -1, dtype=torch.int32, device=dev)
    status = torch.full((C,), 9, dtype=torch.int32, device=dev)
    d_off, d_moff = torch.from_numpy(off).to(dev), torch.from_numpy(moff).to(dev)
    _lib.check(L.dispu_fps_segments_auto(C, _lib.ptr(d_off), _lib.ptr(d_moff), hp(off), hp(moff), _lib.ptr(x), _lib.ptr(sc), need,
                                         _lib.ptr(out), _lib.ptr(status), arith, _lib.stream_ptr(dev)), "dispu_fps_segments_auto")
    assert np.array_equal(N(out), want)
    assert not N(status).any()
    assert bool((sc[need:] == 0x5A).all())
    assert np.array_equal(N(U.fps_segments(x, off, moff, arith=arith)), want)                   # the Python default
    assert np.array_equal(N(U.fps_segments(x, off, moff, arith=arith, path="cells")), want)     # and every segment on the cell kernels


def test_scratch_contract(dev):
    from dispu_amd import _lib
    from dispu_amd import upsample as U
    L = _lib.lib()
    hp = lambda a: _lib.C.c_void_p(a.ctypes.data)
    rng = np.random.default_rng(17)
    clouds, ms = [_cloud(rng, 700), _cloud(rng, 25000)], [100, 300]
    off, moff = U.segment_offsets([c.shape[0] for c in clouds]), U.segment_offsets(ms)
    x = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_off, d_moff = torch.from_numpy(off).to(dev), torch.from_numpy(moff).to(dev)
    need = L.dispu_fps_cells_scratch_bytes(2, hp(off), hp(moff), 0)
    assert need > 0 and need % 4 == 0

    def call(sc, nbytes, cell=0):
        out = torch.full((int(moff[-1]),), -1, dtype=torch.int32, device=dev)
        status = torch.full((2,), 9, dtype=torch.int32, device=dev)
        rc = L.dispu_fps_cells(2, _lib.ptr(d_off), _lib.ptr(d_moff), hp(off), hp(moff), _lib.ptr(x), _lib.ptr(sc), nbytes, _lib.ptr(out),
                               _lib.ptr(status), 1, cell, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, N(out), N(status)

    sc = torch.full((need + 65536,), 0x5A, dtype=torch.uint8, device=dev)
    rc, out, status = call(sc, need)
    assert rc == 0 and not status.any()
    for c in range(2):
        assert np.array_equal(out[moff[c]:moff[c + 1]], _want(clouds[c], ms[c], 1))
    assert bool((sc[need:] == 0x5A).all()), "dispu_fps_cells wrote behind scratch_bytes"
    sc.fill_(0x5A)
    for s, nbytes in ((sc, need - 4), (None, need), (sc, 0)):
        rc, out, status = call(s, nbytes)
        assert rc != 0 and (out == -1).all() and (status == 9).all()
    assert bool((sc == 0x5A).all()), "a refused call must not touch the scratch"
    for cell in (1, 32, 96, 8192, -64):                   # not a cell size
        assert L.dispu_fps_cells_scratch_bytes(2, hp(off), hp(moff), cell) == 0
        assert call(sc, need, cell)[0] != 0
    assert bool((sc == 0x5A).all())


def test_non_finite_input(dev):
    from dispu_amd import _lib
    from dispu_amd import upsample as U
    from dispu_amd.tf_sampling import farthest_point_sample
    L = _lib.lib()
    hp = lambda a: _lib.C.c_void_p(a.ctypes.data)
    rng = np.random.default_rng(19)
    for bad in (np.nan, np.inf):
        clouds, ms = [_cloud(rng, 500), _cloud(rng, 26000), _cloud(rng, 2000)], [50, 400, 100]
        clouds[1][12345, 1] = bad
        off, moff = U.segment_offsets([c.shape[0] for c in clouds]), U.segment_offsets(ms)
        x = torch.from_numpy(np.concatenate(clouds)).to(dev)
        d_off, d_moff = torch.from_numpy(off).to(dev), torch.from_numpy(moff).to(dev)
        need = L.dispu_fps_cells_scratch_bytes(3, hp(off), hp(moff), 0)
        sc = torch.empty((need,), dtype=torch.uint8, device=dev)
        out = torch.full((int(moff[-1]),), -1, dtype=torch.int32, device=dev)
        status = torch.full((3,), 9, dtype=torch.int32, device=dev)
        _lib.check(L.dispu_fps_cells(3, _lib.ptr(d_off), _lib.ptr(d_moff), hp(off), hp(moff), _lib.ptr(x), _lib.ptr(sc), need, _lib.ptr(out),
                                     _lib.ptr(status), 1, 0, _lib.stream_ptr(dev)), "dispu_fps_cells")
        got = N(out)
        assert N(status).tolist() == [0, 1, 0]
        assert (got[moff[1]:moff[2]] == -1).all(), "no indices for the non-finite segment"
        for c in (0, 2):
            assert np.array_equal(got[moff[c]:moff[c + 1]], _want(clouds[c], ms[c], 1))
        # the Python layer samples such a segment again through the existing entry: all paths agree
        want = N(U.fps_segments(x, off, moff, path="stream"))
        assert np.array_equal(N(U.fps_segments(x, off, moff, path="cells")), want)
        assert np.array_equal(N(U.fps_segments(x, off, moff, path="auto")), want)
        t = torch.from_numpy(clouds[1][None]).to(dev)
        want = N(farthest_point_sample(400, t, path="stream"))
        assert np.array_equal(N(farthest_point_sample(400, t, path="auto")), want)
        assert np.array_equal(N(farthest_point_sample(400, t, path="cells")), want)


@pytest.mark.parametrize("forced", [True, False])
def test_upsample_end_to_end(dev, forced, monkeypatch):
    """a 2304-point cloud: the merged stage has 27648 points, above the 24576 of the register kernels"""
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    if forced:
        monkeypatch.setattr(U, "farthest_point_sample", functools.partial(U.farthest_point_sample, path="cells"))
        monkeypatch.setattr(U, "fps_segments", functools.partial(U.fps_segments, path="cells"))
    rng = np.random.default_rng(23)
    gen = Generator(params=OG.init_params(seed=4), device=dev)
    clouds = [_sphere(rng, n) for n in (2304, 700, 2500)]
    singles = []
    for pc in clouds:
        res, st = U.upsample_cloud(gen, pc, return_stages=True)
        merged = N(st["merged"])
        assert merged.shape[1] == int(pc.shape[0] / 256 * 3) * 1024
        assert np.array_equal(N(st["sel"]), O.farthest_point_sample(4 * pc.shape[0], merged, contract=1))
        assert np.array_equal(N(st["seeds"]), O.farthest_point_sample(N(st["seeds"]).shape[1], N(st["cloud_n"]), contract=1))
        singles.append(res)
    assert int(clouds[0].shape[0] / 256 * 3) * 1024 == 27648
    outs = U.upsample_ragged(gen, clouds)
    for got, want in zip(outs, singles):
        assert np.array_equal(got, want)
