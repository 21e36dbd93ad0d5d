"""GPU tests of the device-wide Poisson-disk tier (dis-pu_amd/poisson_cells.py, csrc/poisson_disk_cells.hip) against the sequential numpy
restatement of tests/mesh_sample_oracle.py and against the one-workgroup tier: keep flags, indices and counts exact, radii bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mesh_oracle as MO  # noqa: E402
import mesh_sample_oracle as SO  # noqa: E402
from oracle import generator as OG  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def N(t):
    return t.detach().cpu().numpy()


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plane(rng, n):
    p = np.zeros((n, 3), f32)
    p[:, :2] = rng.random((n, 2), dtype=f32)
    return p


def _sphere(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _line(n, r):
    p = np.zeros((n, 3), f32)
    p[:, 0] = (0.9 * r) * np.arange(n)
    return p


def _min_pair_d2(points):
    """SO.min_pair_d2_f32 in row chunks: the smallest fp32 plain-order d2 over all pairs"""
    p = np.ascontiguousarray(points, f32)
    best = f32(np.inf)
    for a in range(0, p.shape[0], 512):
        d2 = SO._d2_plain(p[a:a + 512, None, :], p[None, :, :])
        d2[np.arange(d2.shape[0]), np.arange(a, a + d2.shape[0])] = np.inf
        best = min(best, f32(d2.min()))
    return best


def _check_keep(pts, r, keep, count):
    want = SO.poisson_keep(pts, f32(r))
    got = N(keep)
    assert got.dtype == np.uint8 and got.shape == (pts.shape[0],)
    assert np.array_equal(got.astype(bool), want) and got.max() <= 1
    assert int(count.item()) == int(want.sum())
    return want


# ------------------------------------------------------------------------------------------------------------------ 1. keep ----------
def _keep_cases():
    rng = np.random.default_rng(77)
    r_lat = f32(0.25)
    g = np.arange(6, dtype=f32) * r_lat                                           # multiples of 2^-2: every distance below is exact
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(f32)
    outlier = np.concatenate([rng.random((2000, 3), dtype=f32), np.array([[100.0, 0.0, 0.0]], f32)])
    return [("plane", _plane(rng, 3000), 0.02),                                   # ~ a third kept; 12 workgroups of 256
            ("sphere", _sphere(rng, 2500), 0.06),
            ("identical", np.tile(np.array([[0.3, -1.5, 2.0]], f32), (300, 1)), 0.01),
            ("lattice_at_r", lattice, float(r_lat)),
            ("lattice_above_r", lattice, float(f32(r_lat) * f32(1 + 2.0 ** -20))),
            ("one_point", np.array([[1.0, 2.0, 3.0]], f32), 0.5),
            ("r_zero", _plane(rng, 700), 0.0),
            ("r_negative", _plane(rng, 700), -1.0),
            ("outlier", outlier, 5e-4)]


@pytest.mark.parametrize("case", range(9))
def test_keep_matches_oracle(case, dev):
    from dispu_amd import poisson_cells as PC
    name, pts, r = _keep_cases()[case]
    keep, count = PC.keep(D(pts, dev), r)
    want = _check_keep(pts, r, keep, count)
    n = pts.shape[0]
    if name == "plane":
        assert 0.25 * n < want.sum() < 0.45 * n
    if name == "identical":
        assert want[0] and want.sum() == 1
    if name in ("lattice_at_r", "one_point", "r_zero", "r_negative"):
        assert want.all()                                                         # d2 == r r is no conflict: the comparison is strict
    if name == "lattice_above_r":
        assert not want.all()
    if name == "outlier":
        assert want[-1]


# ------------------------------------------------------------------------------------------------------------------ 2. ragged --------
RAGGED_SIZES = (1, 5, 257, 3000, 2048)
RAGGED_R = (0.3, 0.0, 0.05, 0.02, 0.07)
RAGGED_M = (1, 3, 100, 1000, 400)


def _ragged_clouds():
    rng = np.random.default_rng(5)
    return [_plane(rng, n) if i % 2 else _sphere(rng, n) for i, n in enumerate(RAGGED_SIZES)]


def test_keep_ragged_equals_single_calls_and_oracle(dev):
    from dispu_amd import poisson_cells as PC
    clouds = _ragged_clouds()
    keep, count = PC.keep([D(c, dev) for c in clouds], list(RAGGED_R))
    assert len(keep) == len(count) == len(clouds)
    for c, pts in enumerate(clouds):
        _check_keep(pts, RAGGED_R[c], keep[c], count[c])
        k1, c1 = PC.keep(D(pts, dev), RAGGED_R[c])
        assert N(k1).tobytes() == N(keep[c]).tobytes() and int(c1.item()) == int(count[c].item())
    order = [3, 0, 4, 2, 1]
    keep2, count2 = PC.keep([D(clouds[c], dev) for c in order], [RAGGED_R[c] for c in order])
    for j, c in enumerate(order):
        assert N(keep2[j]).tobytes() == N(keep[c]).tobytes() and int(count2[j].item()) == int(count[c].item())


# ------------------------------------------------------------------------------------------------------------------ 3. tiers ---------
@pytest.fixture(scope="module")
def fandisk(golden_dir, tmp_path_factory, dev):
    from dispu_amd import mesh as M
    d = tmp_path_factory.mktemp("pugan_cells")
    MO.extract_pugan(golden_dir, str(d))
    v, f = M.load_off(os.path.join(str(d), "fandisk.off"))
    return M.Mesh(v, f, dev)


@pytest.mark.parametrize("n", [4096, 49152])
def test_keep_and_select_equal_the_one_workgroup_tier(n, dev):
    from dispu_amd import _lib
    from dispu_amd import mesh_sample as S
    from dispu_amd import poisson_cells as PC
    assert n <= _lib.POISSON_MAX_N
    pts = D(_plane(np.random.default_rng(n), n), dev)
    m = n // 4
    r_keep = 0.7 * S.hex_radius(1.0, m)
    k0, c0 = S.poisson_disk_keep(pts, r_keep)
    k1, c1 = PC.keep(pts, r_keep)
    assert N(k0).tobytes() == N(k1).tobytes() and int(c0.item()) == int(c1.item())
    i0, r0, n0 = S.poisson_disk_select(pts, m, S.hex_radius(1.0, m))
    i1, r1, n1 = PC.select(pts, m, S.hex_radius(1.0, m))
    assert N(i0).tobytes() == N(i1).tobytes() and N(r0).tobytes() == N(r1).tobytes() and int(n0.item()) == int(n1.item())


def test_mesh_cloud_equals_poisson_disk_cloud(fandisk, dev):
    from dispu_amd import mesh_sample as S
    from dispu_amd import poisson_cells as PC
    p0, r0 = S.poisson_disk_cloud(fandisk, 2048, 4)
    p1, r1 = PC.mesh_cloud(fandisk, 2048, 4)
    assert p1.shape == (2048, 3) and N(p0).tobytes() == N(p1).tobytes() and r0 == r1


# ------------------------------------------------------------------------------------------------------------------ 4. large ---------
def test_keep_above_the_old_limit(dev):
    from dispu_amd import _lib
    from dispu_amd import poisson_cells as PC
    n, r = 60000, f32(0.0037)
    assert n > _lib.POISSON_MAX_N
    pts = _plane(np.random.default_rng(60), n)
    keep, count = PC.keep(D(pts, dev), float(r))
    nbr, dd = SO.conflicts(pts, r)                                                # once: SO.poisson_keep is these two lines
    want = SO.greedy_keep(n, nbr, dd, r)
    got = N(keep).astype(bool)
    assert np.array_equal(got, want) and int(count.item()) == int(want.sum())
    # the definition itself, from the conflict lists of the oracle: no two kept points conflict, every rejected point has a kept
    # conflicting point of lower index
    for i in range(n):
        kept_lower = any(got[j] for j in nbr[i])
        assert kept_lower != got[i], i
    assert 0.2 * n < want.sum() < 0.5 * n


BIG_LATTICE = (80, 12289)                                 # 80^3 + 12289 = 524289 points: 257 tile sums in the scans over the points
MANY = (257, (1, 63, 64, 65, 130))                        # 9 segment bits above the 30 cell bits: a fifth sorting pass


def test_keep_past_one_scan_sum_per_thread(dev):
    """524289 points whose answer follows from their construction (SO.lattice_with_close_pairs, confirmed against the greedy oracle at
    about 5000 points in tests/test_second_trips.py): the cell sort, the run numbering and the scan of the active list at a size where
    the one-workgroup tier of the scan gives every thread two sums"""
    from dispu_amd import poisson_cells as PC
    pts, want = SO.lattice_with_close_pairs(*BIG_LATTICE)
    assert pts.shape[0] == 524289 and int((~want).sum()) == BIG_LATTICE[1]
    keep, count = PC.keep(D(pts, dev), 0.4)
    got = N(keep)
    assert got.dtype == np.uint8 and got.max() <= 1 and np.array_equal(got.astype(bool), want)
    assert int(count.item()) == int(want.sum())


def keep_abi(dev, packed, off, radii):
    """dispu_poisson_cells_keep on a packed batch -> (flags u8 [N], count [C], status [C])"""
    import ctypes as C
    from dispu_amd import _lib
    L = _lib.lib()
    nC, total = len(off) - 1, packed.shape[0]
    off = np.ascontiguousarray(off, np.int32)
    d_off, d_pts, d_r = D(off, dev), D(packed, dev), D(np.asarray(radii, f32), dev)
    flags = torch.full((total,), 9, dtype=torch.uint8, device=dev)
    count = torch.full((nC,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(nC, dtype=torch.int32, device=dev)
    rounds = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = L.dispu_poisson_cells_scratch_bytes(nC, total)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.dispu_poisson_cells_keep(nC, _lib.ptr(d_off), C.c_void_p(off.ctypes.data), _lib.ptr(d_pts), _lib.ptr(d_r), _lib.ptr(flags),
                                          _lib.ptr(count), _lib.ptr(rounds), _lib.ptr(scratch), nbytes, _lib.ptr(status),
                                          _lib.stream_ptr(dev)), "dispu_poisson_cells_keep")
    torch.cuda.synchronize(dev)
    return N(flags), N(count), N(status)


def test_keep_with_257_segments(dev):
    """one packed call; the oracle runs once per distinct cloud and is asserted for every repeat at its own offset"""
    nC, cycle = MANY
    rng = np.random.default_rng(257)
    distinct = {n: _sphere(rng, n) for n in cycle}
    radius = {n: 0.9 * math.sqrt(4 * math.pi / n) for n in cycle}                # about the mean spacing: a good part is rejected
    sizes = np.array(cycle)[np.arange(nC) % len(cycle)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    flags, count, status = keep_abi(dev, np.concatenate([distinct[n] for n in sizes]), off, [radius[n] for n in sizes])
    assert not status.any()
    for n in cycle:
        want = SO.poisson_keep(distinct[n], f32(radius[n]))
        assert n < 63 or 0.2 * n < want.sum() < 0.9 * n
        rows = off[:-1][sizes == n][:, None] + np.arange(n)[None, :]
        assert flags.max() <= 1 and (flags[rows].astype(bool) == want[None, :]).all(), n
        assert (count[sizes == n] == int(want.sum())).all(), n


# ------------------------------------------------------------------------------------------------------------------ 5. select --------
def _check_selection(pts, idx, r, count, m, want, steps):
    widx, wr, wcount = want
    idx = N(idx)
    assert idx.dtype == np.int32 and idx.shape == (m,) and np.array_equal(idx, widx)
    assert N(r).astype(f32).tobytes() == f32(wr).tobytes() and int(count.item()) == wcount
    assert wcount >= m and np.all(np.diff(idx) > 0)
    rr = f32(N(r))
    if m > 1 and rr > 0:
        assert _min_pair_d2(pts[idx]) >= f32(rr * rr)                      # every pair at distance >= r, in the kernel's arithmetic
    if steps == 12:
        print("n %d m %d: r %.6g, surplus %d" % (pts.shape[0], m, float(rr), wcount - m))
        assert wcount - m <= math.ceil(0.02 * m)


@pytest.mark.parametrize("n,m,steps", [(6000, 1500, 12), (6000, 1500, 1), (6000, 1500, 0), (3000, 3000, 12)])
def test_select_matches_oracle(n, m, steps, dev):
    from dispu_amd import mesh_sample as S
    from dispu_amd import poisson_cells as PC
    pts = _plane(np.random.default_rng(n + steps), n)
    r_hi = f32(S.hex_radius(1.0, m))
    want = SO.poisson_select(pts, m, r_hi, steps)
    idx, r, count = PC.select(D(pts, dev), m, float(r_hi), steps)
    _check_selection(pts, idx, r, count, m, want, steps)
    if steps == 0:
        assert float(r.item()) == 0.0
    if steps == 0 or m == n:
        assert np.array_equal(N(idx), np.arange(m))


def test_select_ragged_with_per_cloud_m(dev):
    from dispu_amd import poisson_cells as PC
    clouds = _ragged_clouds()
    r_hi = [f32(4.0 * math.sqrt(1.0 / m)) for m in RAGGED_M]
    idx, r, count = PC.select([D(c, dev) for c in clouds], list(RAGGED_M), [float(v) for v in r_hi])
    for c, pts in enumerate(clouds):
        _check_selection(pts, idx[c], r[c], count[c], RAGGED_M[c], SO.poisson_select(pts, RAGGED_M[c], r_hi[c], 12), 12)


# ------------------------------------------------------------------------------------------------------------------ 6. shuffle -------
def test_select_with_shuffle_seed_is_the_oracle_on_the_permuted_cloud(dev):
    from dispu_amd import mesh_sample as S
    from dispu_amd import poisson_cells as PC
    clouds = [_plane(np.random.default_rng(8), 3000), _sphere(np.random.default_rng(9), 1000)]
    ms = [800, 250]
    r_hi = [f32(S.hex_radius(1.0, 800)), f32(S.hex_radius(4 * math.pi, 250))]
    idx, r, count = PC.select([D(c, dev) for c in clouds], ms, [float(v) for v in r_hi], shuffle_seed=7)
    for c, pts in enumerate(clouds):
        perm = np.random.RandomState(7 + c).permutation(pts.shape[0])
        widx, wr, wcount = SO.poisson_select(pts[perm], ms[c], r_hi[c], 12)
        assert np.array_equal(N(idx[c]), np.sort(perm[widx])) and N(idx[c]).dtype == np.int32
        assert N(r[c]).astype(f32).tobytes() == f32(wr).tobytes() and int(count[c].item()) == wcount
    k, cnt = PC.keep(D(clouds[0], dev), 0.02, shuffle_seed=7)
    perm = np.random.RandomState(7).permutation(3000)
    want = np.zeros(3000, bool)
    want[perm] = SO.poisson_keep(clouds[0][perm], f32(0.02))
    assert np.array_equal(N(k).astype(bool), want) and int(cnt.item()) == int(want.sum())


def test_a_line_in_index_order_settles_shuffled_and_never_lies_unshuffled(dev):
    from dispu_amd import _lib
    from dispu_amd import poisson_cells as PC
    n, r = 4096, f32(0.01)
    pts = _line(n, r)
    perm = np.random.RandomState(0).permutation(n)
    want = np.zeros(n, bool)
    want[perm] = SO.poisson_keep(pts[perm], r)
    keep, count, rounds = PC.keep(D(pts, dev), float(r), shuffle_seed=0, return_rounds=True)
    assert np.array_equal(N(keep).astype(bool), want) and int(count.item()) == int(want.sum())
    assert rounds <= 6           # SO.rounds_keep, a snapshot per round, needs 6 here; in-place updates only ever settle a point sooner
    # in index order the chain is as long as the line: the call ends at the round bound at the latest, and then it raises
    try:
        keep, count = PC.keep(D(pts, dev), float(r))
    except RuntimeError as e:
        assert "DISPU_POISSON_MAX_ROUNDS = %d" % _lib.POISSON_MAX_ROUNDS in str(e) and "shuffle_seed" in str(e)
    else:
        _check_keep(pts, r, keep, count)


# ------------------------------------------------------------------------------------------------------------------ 7. run to run ----
def test_two_runs_give_identical_bytes(dev):
    from dispu_amd import poisson_cells as PC
    clouds = [D(c, dev) for c in _ragged_clouds()]
    r_hi = [4.0 * math.sqrt(1.0 / m) for m in RAGGED_M]
    runs = []
    for _ in range(2):
        keep, count = PC.keep(clouds, list(RAGGED_R))
        idx, r, cnt = PC.select(clouds, list(RAGGED_M), r_hi, shuffle_seed=3)
        runs.append([N(t).tobytes() for group in (keep, count, idx, r, cnt) for t in group])
    assert runs[0] == runs[1]


def test_a_non_finite_coordinate_is_refused(dev):
    from dispu_amd import poisson_cells as PC
    pts = _plane(np.random.default_rng(1), 500)
    bad = pts.copy()
    bad[77, 1] = np.nan
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):
        PC.keep([D(pts, dev), D(bad, dev)], 0.05)
    bad[77, 1] = np.inf
    with pytest.raises(ValueError, match="cloud 0 holds a NaN or an infinite coordinate"):
        PC.select([D(bad, dev), D(pts, dev)], 100, 0.1)


# ------------------------------------------------------------------------------------------------------------------ 8. merge ---------
def _sphere_clouds(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        g = rng.standard_normal((n, 3))
        out.append((g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, 3) + rng.uniform(-2, 2, 3)).astype(f32))
    return out


def test_upsample_ragged_with_the_poisson_merge(dev):
    from dispu_amd import poisson_cells as PC
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    gen = Generator(params=OG.init_params(seed=3, bias_scale=0.05, bn_random=True), device=dev)
    clouds = _sphere_clouds([512, 1280], 21)
    outs, st = U.upsample_ragged(gen, clouds, return_stages=True, merge="poisson", merge_seed=5)
    moff, ooff = st["merged_off"], st["out_off"]
    merged = [st["merged"][moff[c]:moff[c + 1]] for c in range(2)]
    r_hi = PC.spacing_r_hi([D(c, dev) for c in clouds], 4)
    idx, r, count = PC.select(merged, [4 * c.shape[0] for c in clouds], r_hi, shuffle_seed=5)
    for c, pc in enumerate(clouds):
        assert outs[c].dtype == f32 and outs[c].shape == (4 * pc.shape[0], 3)
        sel = N(st["sel"][ooff[c]:ooff[c + 1]])
        assert np.array_equal(sel, N(idx[c])) and np.all(np.diff(sel) > 0)
        assert np.array_equal(outs[c], N(merged[c])[sel])                         # every output row is a row of the cloud's merged segment
        mr = f32(N(st["merge_r"][c]))
        assert mr.tobytes() == N(r[c]).astype(f32).tobytes() and int(st["merge_count"][c].item()) == int(count[c].item())
        assert 0.0 < mr < f32(r_hi[c])                                            # the bisection was bracketed
        assert _min_pair_d2(outs[c]) >= f32(mr * mr)
    # the default is untouched
    a = U.upsample_ragged(gen, clouds)
    b = U.upsample_ragged(gen, clouds, merge="fps")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 9. tool ----------
def test_upsample_command_with_the_poisson_merge(dev, tmp_path):
    from dispu_amd import checkpoint as CK
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    sizes = {"a_cloud": 300, "b_cloud": 700}
    for (name, n), pc in zip(sorted(sizes.items()), _sphere_clouds([300, 700], 14)):
        np.savetxt(str(data / "test" / (name + ".xyz")), pc, fmt="%.6f")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data), "--merge", "poisson",
           "--merge_seed", "11"]
    got = []
    for out_dir in (tmp_path / "o1", tmp_path / "o2"):
        r = subprocess.run(cmd + ["--out_folder", str(out_dir)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")
        assert sorted(os.listdir(str(out_dir))) == sorted(n + "_X4.xyz" for n in sizes)
        got.append({n: open(str(out_dir / (n + "_X4.xyz")), "rb").read() for n in sizes})
        for name, n in sizes.items():
            assert np.loadtxt(str(out_dir / (name + "_X4.xyz"))).shape == (4 * n, 3)
    assert got[0] == got[1]


def test_make_dataset_clouds_above_the_old_limit(fandisk, golden_dir, tmp_path, dev):
    """--cells: 4 x 12500 = 50000 candidates, above DISPU_POISSON_MAX_N; the file holds mesh_cloud's points"""
    from dispu_amd import poisson_cells as PC
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    MO.extract_pugan(golden_dir, str(meshes))
    for name in os.listdir(str(meshes)):
        if name != "fandisk.off":
            os.remove(os.path.join(str(meshes), name))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), "clouds", "--mesh_dir", str(meshes), "--out_dir", str(tmp_path / "c"),
           "--num", "12500"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"at most 49152 per cloud" in r.stderr and not (tmp_path / "c").exists()
    r = subprocess.run(cmd + ["--cells"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    pts, _ = PC.mesh_cloud(fandisk, 12500, 4, seed=0)
    want = tmp_path / "want.xyz"
    np.savetxt(str(want), N(pts), fmt="%.6f")
    assert open(str(tmp_path / "c" / "fandisk.xyz"), "rb").read() == open(str(want), "rb").read()
