"""GPU tests of dispu_amd.reconstruct (csrc/signed_distance.hip, csrc/reconstruct.hip) against tests/reconstruct_oracle.py: the device
equals the oracle BIT FOR BIT -- every value of signed_distance, and verts / faces of reconstruct_surface with their order -- so the
geometric assertions of test_reconstruct_oracle.py hold for the device by equality.  Every cloud has at most 2049 points; oracle runs
are shared through lru_cache.

Round trip on the sphere case: the mean P2F distance of the 2048 input points to the device's mesh (dispu_point_to_mesh) against
tests/mesh_oracle.point_to_mesh on the oracle's mesh, within test_mesh_eval_gpu.py's 2e-6.  Both were 0.000711614 (MEAN_P2F below):
the cloud's points lie 0.0007 from the mesh on average, 0.0041 at most, at a voxel of 0.1."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reconstruct_oracle as R  # noqa: E402
import normals_oracle as NO  # noqa: E402
import orient_oracle as OO  # noqa: E402
import mesh_oracle as MO  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue
MEAN_P2F = 0.000711614                                            # sphere case, float64 oracle (printed by the test)


def N(t):
    return t.detach().cpu().numpy()


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return off


# ---- signed_distance ----------------------------------------------------------------------------------------------------------------------

def shell(n, seed):
    """n seeded points with radii in 0.7 .. 1.3"""
    r = np.random.RandomState(seed)
    return (NO.sphere(n, seed=seed + 100).astype(np.float64) * r.uniform(0.7, 1.3, (n, 1))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sd_batch():
    """(queries, points, normals) per pair: a 700-point sphere and a 1300-point torus, each queried at itself and in a shell around it;
    one reference point and three coincident ones (k > m; D == 0 for the queries that sit on them); a lattice queried at its cell
    centres, equidistant from their 8 nearest points; and query counts of 1, 63, 64 and 65 for the partial wave"""
    sph = NO.sphere(700)
    tor, tor_n = OO.torus(1300)
    one = np.float32([[0.25, -0.5, 0.125]])
    three = np.tile(np.float32([[1, 2, 3]]), (3, 1))
    lat = NO.lattice(5)
    centres = NO.lattice(4) + np.float32(0.5)
    pairs = [(np.concatenate([sph, shell(1000, 1)]), sph, sph),
             (np.concatenate([tor, shell(1000, 2) * np.float32(1.2)]), tor, tor_n.astype(np.float32)),
             (shell(63, 3), one, np.float32([[0, 0, 1]])),
             (np.concatenate([three[:2], shell(63, 4) + np.float32([1, 2, 3])]), three, OO.random_units(3, 5)),
             (np.concatenate([centres, lat[:7]]), lat, OO.random_units(len(lat), 6))]
    pairs += [(shell(nq, 10 + nq), sph, sph) for nq in (1, 63, 64, 65)]
    return pairs


@functools.lru_cache(maxsize=None)
def sd_oracle(k, support):
    return [R.signed_distance(q, p, n, k, support) for q, p, n in sd_batch()]


def run_sd(dev, qs, ps, ns, k, support, qoff=None, roff=None, scratch="ok", C_arg=None, null=(), alias=None, scratch_buf=None):
    """the C entry on a packed batch, outputs pre-filled with sentinels -> (rc, out, status); inputs must keep their bits.
    scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the zero-filled one"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    q, p, n = (T(np.concatenate(x).astype(np.float32), dev) for x in (qs, ps, ns))
    good_q, good_r = offsets(qs), offsets(ps)
    qoff = np.ascontiguousarray(good_q if qoff is None else qoff, np.int32)
    roff = np.ascontiguousarray(good_r if roff is None else roff, np.int32)
    full = L.dispu_signed_distance_scratch_bytes(len(qs), C.c_void_p(good_q.ctypes.data), C.c_void_p(good_r.ctypes.data))
    assert full > 0
    buf = torch.zeros((full + 16,), dtype=torch.uint8, device=dev)
    sp, sb = _lib.ptr(buf), full
    if scratch_buf is not None:
        assert scratch in ("ok", "short"), "with scratch_buf only a right or a one-byte-short size can be asked for"
        sp, sb, full = scratch_buf.ptr(), scratch_buf.nbytes, scratch_buf.nbytes
    if scratch == "null":
        sp = C.c_void_p(0)
    elif scratch == "short":
        sb = full - 1
    elif scratch == "misaligned":
        sp = C.c_void_p(buf.data_ptr() + 4)
    out = torch.full((q.shape[0],), 7.0, dtype=torch.float32, device=dev)
    status = torch.full((len(qs),), -7, dtype=torch.int32, device=dev)
    d_qoff, d_roff = T(qoff, dev), T(roff, dev)
    ptrs = dict(qoff=_lib.ptr(d_qoff), roff=_lib.ptr(d_roff), queries=_lib.ptr(q), refs=_lib.ptr(p), normals=_lib.ptr(n), out=_lib.ptr(out),
                status=_lib.ptr(status))
    if alias is not None:
        ptrs["out"] = ptrs[alias]
    for name in null:
        ptrs[name] = C.c_void_p(0)
    before = [N(x).copy() for x in (q, p, n)]
    rc = L.dispu_signed_distance_segments(len(qs) if C_arg is None else C_arg, ptrs["qoff"], C.c_void_p(qoff.ctypes.data), ptrs["roff"],
                                          C.c_void_p(roff.ctypes.data), k, support, ptrs["queries"], ptrs["refs"], ptrs["normals"],
                                          ptrs["out"], ptrs["status"], sp, sb, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert all(same_bits(N(x), b) for x, b in zip((q, p, n), before))           # inputs are only read
    if scratch_buf is not None:
        scratch_buf.inputs = dict(queries=N(q), refs=N(p), normals=N(n), qoff=N(d_qoff), roff=N(d_roff))   # as the call left them
    return rc, N(out), N(status)


@pytest.mark.parametrize("support", [1.0, 1.5, 4.0])
@pytest.mark.parametrize("k", [1, 8, 16, 32])
def test_signed_distance_bits(dev, k, support):
    qs, ps, ns = zip(*sd_batch())
    rc, out, status = run_sd(dev, qs, ps, ns, k, support)
    assert rc == 0 and not status.any()
    want = sd_oracle(k, support)
    o = 0
    for i, w in enumerate(want):
        got = out[o:o + len(w)]
        bad = np.nonzero(got.view(np.uint32) != w.view(np.uint32))[0]
        assert len(bad) == 0, (i, k, support, bad[:5], got[bad[:5]], w[bad[:5]])
        o += len(w)
    assert np.isfinite(out).all()                               # the fallback: f is always defined


def test_signed_distance_fallbacks_by_construction(dev):
    """each way to an all-zero weight sum gives the nearest point's tangent plane, exactly.  At support 1 the k'-th neighbour itself has
    r2 == 1 and weight 0: so has a lone neighbour (k' = 1) and so have equidistant ones"""
    qs, ps, ns = zip(*sd_batch())
    o = offsets(qs)
    _, out, _ = run_sd(dev, qs, ps, ns, 8, 1.0)
    q, p, n = sd_batch()[2]                                     # one reference point: k' = 1
    g = ((q.astype(np.float64) - p[0].astype(np.float64)) * n[0].astype(np.float64))
    assert same_bits(out[o[2]:o[3]], ((g[:, 0] + g[:, 1]) + g[:, 2]).astype(np.float32))
    assert (out[o[3]:o[3] + 2] == 0).all()                      # queries on three coincident points: D == 0, g_0 = 0
    q, p, n = sd_batch()[4]                                     # cell centres: eight neighbours at one distance, r2 == 1 for all
    d2, idx = R.neighbors(q[:64], p, 8)
    assert (d2 == d2[:, :1]).all()
    u = q[:64].astype(np.float64) - p[idx[:, 0]].astype(np.float64)
    n0 = n[idx[:, 0]].astype(np.float64)
    assert same_bits(out[o[4]:o[4] + 64], ((u[:, 0] * n0[:, 0] + u[:, 1] * n0[:, 1]) + u[:, 2] * n0[:, 2]).astype(np.float32))
    _, out1, _ = run_sd(dev, qs, ps, ns, 1, 1.0)                # k = 1 everywhere
    q, p, n = sd_batch()[0]
    _, idx = R.neighbors(q, p, 1)
    u = q.astype(np.float64) - p[idx[:, 0]].astype(np.float64)
    n0 = n[idx[:, 0]].astype(np.float64)
    assert same_bits(out1[:len(q)], ((u[:, 0] * n0[:, 0] + u[:, 1] * n0[:, 1]) + u[:, 2] * n0[:, 2]).astype(np.float32))


def test_signed_distance_python_entry_and_determinism(dev):
    import torch
    from dispu_amd.reconstruct import signed_distance
    qs, ps, ns = zip(*sd_batch())
    dq, dp, dn = ([T(x, dev) for x in xs] for xs in (qs, ps, ns))
    got = signed_distance(dq, dp, dn, k=8, support=1.5)
    again = signed_distance(dq, dp, dn, k=8, support=1.5)
    assert isinstance(got, list) and len(got) == len(qs)
    for g, a, w in zip(got, again, sd_oracle(8, 1.5)):
        assert g.dtype == torch.float32 and same_bits(N(g), w) and same_bits(N(a), w)
    for x, src in zip(dq + dp + dn, qs + ps + ns):
        assert same_bits(N(x), np.ascontiguousarray(src, np.float32))           # inputs are only read
    single = signed_distance(dq[0], dp[0], dn[0])               # tensors in, a tensor out; the defaults are k = 8, support = 1.5
    assert isinstance(single, torch.Tensor) and same_bits(N(single), sd_oracle(8, 1.5)[0])
    q, p, n = dq[0], dp[0], dn[0]
    for bad in (dict(k=0), dict(k=33), dict(k=8.0), dict(support=0.5), dict(support=4.5), dict(support=float("nan")), dict(support="1")):
        with pytest.raises(ValueError):
            signed_distance(q, p, n, **bad)
    poisoned = N(n).copy()
    poisoned[3, 1] = np.nan
    for bad in (n.double(), n[:, :2], n[:-1], n.cpu(), T(poisoned, dev), [n]):
        with pytest.raises(ValueError):
            signed_distance(q, p, bad)
    with pytest.raises(ValueError):
        signed_distance([q], [p], [n, n])
    pts = N(p).copy()
    pts[5, 0] = np.inf
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):      # found by the launch, raised after it
        signed_distance([q, q], [p, T(pts, dev)], [n, n])


def test_signed_distance_abi_refusals_touch_nothing(dev):
    qs, ps, ns = zip(*sd_batch()[:2])
    bent = (np.int32([0, 500, 400]), np.int32([0, 500, 500]), np.int32([1, 500, 800]))
    cases = [dict(k=0), dict(k=33), dict(k=-1), dict(support=0.5), dict(support=4.5), dict(support=float("nan")), dict(C_arg=0), dict(C_arg=-1),
             dict(C_arg=65536), dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"), dict(alias="queries"),
             dict(alias="refs"), dict(alias="normals")]
    cases += [dict(qoff=b) for b in bent] + [dict(roff=b) for b in bent]
    cases += [dict(null=(name,)) for name in ("qoff", "roff", "queries", "refs", "normals", "out", "status")]
    for kw in cases:
        kw.setdefault("k", 8)
        kw.setdefault("support", 1.5)
        rc, out, status = run_sd(dev, qs, ps, ns, **kw)
        assert rc == INVALID and (out == 7).all() and (status == -7).all(), kw
    from dispu_amd import _lib
    L = _lib.lib()
    good = C.c_void_p(offsets(qs).ctypes.data)
    for b in bent:
        assert L.dispu_signed_distance_scratch_bytes(2, C.c_void_p(b.ctypes.data), good) == 0
        assert L.dispu_signed_distance_scratch_bytes(2, good, C.c_void_p(b.ctypes.data)) == 0
    assert L.dispu_signed_distance_scratch_bytes(0, good, good) == 0


# ---- reconstruct_surface ------------------------------------------------------------------------------------------------------------------

def device_mesh(dev, name, **more):
    from dispu_amd.reconstruct import reconstruct_surface
    p, n, kw = R.case_input(name)
    stages = {}
    v, f = reconstruct_surface(T(p, dev), T(n, dev), stages=stages, **dict(kw, **more))
    return N(v), N(f), stages


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reconstruct_equals_the_oracle(dev, name):
    want = R.case_result(name)
    v, f, stages = device_mesh(dev, name)
    assert (stages["voxels"], stages["lattice"]) == (want["nvox"], want["nlat"])
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert f.shape == want["faces"].shape and np.array_equal(f, want["faces"])
    bad = np.nonzero((v.view(np.uint32) != want["verts"].view(np.uint32)).any(axis=1))[0] if v.shape == want["verts"].shape else None
    assert bad is not None and len(bad) == 0, (v.shape, want["verts"].shape, None if bad is None else (bad[:5], v[bad[:5]], want["verts"][bad[:5]]))


def test_reconstruct_is_deterministic_reads_its_inputs_only_and_round_trips(dev):
    import torch
    from dispu_amd import mesh as M
    from dispu_amd.reconstruct import reconstruct_surface
    p, n, kw = R.case_input("sphere")
    dp, dn = T(p, dev), T(n, dev)
    v1, f1 = reconstruct_surface(dp, dn, **kw)
    v2, f2 = reconstruct_surface(dp, dn, **kw)
    assert v1.dtype == torch.float32 and f1.dtype == torch.int32 and v1.device == dp.device
    assert N(v1).tobytes() == N(v2).tobytes() and N(f1).tobytes() == N(f2).tobytes()
    assert same_bits(N(dp), p) and same_bits(N(dn), n)
    want = R.case_result("sphere")
    d, _, _ = M.point_to_mesh(dp, M.Mesh(N(v1), N(f1), dev))
    rd = MO.point_to_mesh(p, want["verts"], want["faces"])[0]
    print("mean P2F: device %.9f, oracle %.9f" % (float(N(d).astype(np.float64).mean()), float(rd.mean())))
    assert abs(float(N(d).astype(np.float64).mean()) - float(rd.mean())) <= 2e-6
    assert abs(float(rd.mean()) - MEAN_P2F) <= 1e-6


def test_reconstruct_python_refusals(dev):
    import torch
    from dispu_amd.reconstruct import reconstruct_surface
    p, n, _ = R.case_input("sphere")
    dp, dn = T(p, dev), T(n, dev)
    for bad in (dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-60), dict(voxel="1"),
                dict(k=0), dict(k=33), dict(support=0.5), dict(support=5), dict(band=0), dict(band=4), dict(band=1.0),
                dict(max_vertices=0), dict(max_vertices=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            reconstruct_surface(dp, dn, **dict(dict(voxel=0.1), **bad))
    poisoned = n.copy()
    poisoned[7, 2] = np.inf
    for bad in (dn.double(), dn[:, :2], dn[:-1], dn.cpu(), T(poisoned, dev), [dn]):
        with pytest.raises(ValueError):
            reconstruct_surface(dp, bad, 0.1)
    for bad in (dp.double(), dp[:0], dp.cpu(), [dp]):
        with pytest.raises(ValueError):
            reconstruct_surface(bad, dn, 0.1)
    with pytest.raises(ValueError, match="voxel"):              # a point at 1000 with h = 1e-4 leaves the index range
        reconstruct_surface(T(np.float32([[1000, 0, 0]]), dev), T(np.float32([[0, 0, 1]]), dev), 1e-4)
    with pytest.raises(ValueError, match="max_vertices"):
        reconstruct_surface(dp, dn, 0.1, max_vertices=100)
    nan = p.copy()
    nan[11, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or an infinite coordinate"):      # found by the launch, raised after it
        reconstruct_surface(T(nan, dev), dn, 0.1)
    edge = np.float32([[(R.BIAS - 1) * 0.5, 0, -(R.BIAS - 1) * 0.5]])           # the last index band 1 admits, on both sides
    up = np.float32([[0, 0, 1]])
    v, f = reconstruct_surface(T(edge, dev), T(up, dev), 0.5)
    want = R.reconstruct(edge, up, 0.5)
    assert same_bits(N(v), want["verts"]) and np.array_equal(N(f), want["faces"])
    with pytest.raises(ValueError, match="voxel"):
        reconstruct_surface(T(edge, dev), T(up, dev), 0.5, band=2)
    v, f = reconstruct_surface(T(np.float32([[0.1, 0.2, 0.3]]), dev), T(np.float32([[0, 0, 0]]), dev), 0.25)    # f == 0 everywhere
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int32


def test_lattice_and_contour_abi_refusals_touch_nothing(dev):
    """NULL, short or misaligned scratch, aliasing outputs, negative and illegal counts at every entry: hipErrorInvalidValue, the
    sentinels in every output (device and host) untouched.  The stages of a small legal run supply the arguments"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    p = T(NO.sphere(200), dev)
    n, h, band = 200, 0.25, 1
    NULL = C.c_void_p(0)

    def i64(m):
        return torch.full((m,), -7, dtype=torch.int64, device=dev)

    def i32(*shape):
        return torch.full(shape, -7, dtype=torch.int32, device=dev)

    def sentinel(*ts):
        torch.cuda.synchronize(dev)
        return all(bool((t == -7).all()) for t in ts)

    def scratch_cases(full):
        buf = torch.zeros((full + 16,), dtype=torch.uint8, device=dev)
        return buf, [(NULL, full), (_lib.ptr(buf), full - 1), (C.c_void_p(buf.data_ptr() + 4), full)]

    # voxels
    full = L.dispu_lattice_voxels_scratch_bytes(n)
    assert full > 0 and L.dispu_lattice_voxels_scratch_bytes(0) == 0 and L.dispu_lattice_voxels_scratch_bytes(-1) == 0
    assert L.dispu_lattice_voxels_scratch_bytes((1 << 24) + 1) == 0
    buf, bent = scratch_cases(full)
    occ, cnt, status = i64(n), C.c_int(-7), C.c_int(-7)
    ok = (n, _lib.ptr(p), h, band, _lib.ptr(occ), C.byref(cnt), C.byref(status), _lib.ptr(buf), full, st)

    def bend(args, **at):
        a = list(args)
        for i, v in at.items():
            a[int(i[1:])] = v
        return a
    calls = [bend(ok, _0=0), bend(ok, _0=-5), bend(ok, _1=NULL), bend(ok, _2=0.0), bend(ok, _2=-1.0),
             bend(ok, _2=float("nan")), bend(ok, _2=float("inf")), bend(ok, _3=0), bend(ok, _3=4), bend(ok, _4=NULL),
             bend(ok, _5=NULL), bend(ok, _6=NULL), bend(ok, _4=_lib.ptr(p))]
    calls += [bend(ok, _7=sp, _8=sb) for sp, sb in bent]
    for a in calls:
        assert L.dispu_lattice_voxels(*a) == INVALID and sentinel(occ) and cnt.value == -7 and status.value == -7
    assert L.dispu_lattice_voxels(*ok) == 0 and status.value == 0 and cnt.value > 0
    nocc = cnt.value

    # dilate
    nk = nocc * 27
    full = L.dispu_lattice_dilate_scratch_bytes(nocc, band)
    assert full > 0 and L.dispu_lattice_dilate_scratch_bytes(0, 1) == 0 and L.dispu_lattice_dilate_scratch_bytes(-1, 1) == 0
    assert L.dispu_lattice_dilate_scratch_bytes(nocc, 0) == 0 and L.dispu_lattice_dilate_scratch_bytes(nocc, 4) == 0
    assert L.dispu_lattice_dilate_scratch_bytes(1 << 24, 3) == 0                # 2^24 * 343 keys: above 2^31 - 1
    buf, bent = scratch_cases(full)
    act, c64 = i64(nk), C.c_longlong(-7)
    ok = (nocc, _lib.ptr(occ), band, _lib.ptr(act), C.byref(c64), _lib.ptr(buf), full, st)
    calls = [bend(ok, _0=0), bend(ok, _0=-3), bend(ok, _1=NULL), bend(ok, _2=0), bend(ok, _2=4), bend(ok, _3=NULL), bend(ok, _4=NULL),
             bend(ok, _3=_lib.ptr(occ))]
    calls += [bend(ok, _5=sp, _6=sb) for sp, sb in bent]
    for a in calls:
        assert L.dispu_lattice_dilate(*a) == INVALID and sentinel(act) and c64.value == -7
    assert L.dispu_lattice_dilate(*ok) == 0 and c64.value >= nocc
    nvox = c64.value

    # corners
    full = L.dispu_lattice_corners_scratch_bytes(nvox)
    assert full > 0 and L.dispu_lattice_corners_scratch_bytes(0) == 0 and L.dispu_lattice_corners_scratch_bytes(-1) == 0
    assert L.dispu_lattice_corners_scratch_bytes(1 << 28) == 0
    buf, bent = scratch_cases(full)
    lat, corner, c64 = i64(8 * nvox), i32(nvox, 8), C.c_longlong(-7)
    ok = (nvox, _lib.ptr(act), _lib.ptr(lat), _lib.ptr(corner), C.byref(c64), _lib.ptr(buf), full, st)
    calls = [bend(ok, _0=0), bend(ok, _0=-3), bend(ok, _1=NULL), bend(ok, _2=NULL), bend(ok, _3=NULL), bend(ok, _4=NULL),
             bend(ok, _2=_lib.ptr(act)), bend(ok, _3=_lib.ptr(act)), bend(ok, _3=_lib.ptr(lat))]
    calls += [bend(ok, _5=sp, _6=sb) for sp, sb in bent]
    for a in calls:
        assert L.dispu_lattice_corners(*a) == INVALID and sentinel(lat, corner) and c64.value == -7
    assert L.dispu_lattice_corners(*ok) == 0 and c64.value > nvox
    nlat = c64.value

    # positions
    pos = torch.full((nlat, 3), -7.0, dtype=torch.float32, device=dev)
    ok = (nlat, _lib.ptr(lat), h, _lib.ptr(pos), st)
    for a in [bend(ok, _0=0), bend(ok, _0=-1), bend(ok, _0=(1 << 24) + 1), bend(ok, _1=NULL), bend(ok, _2=0.0),
              bend(ok, _2=float("nan")), bend(ok, _3=NULL), bend(ok, _3=_lib.ptr(lat))]:
        assert L.dispu_lattice_positions(*a) == INVALID and sentinel(pos)
    assert L.dispu_lattice_positions(*ok) == 0
    from dispu_amd.reconstruct import signed_distance
    f = signed_distance(pos, p, p)

    # count
    full = L.dispu_contour_count_scratch_bytes(nvox, nlat)
    assert full > 0 and L.dispu_contour_count_scratch_bytes(0, nlat) == 0 and L.dispu_contour_count_scratch_bytes(nvox, 0) == 0
    assert L.dispu_contour_count_scratch_bytes(-1, nlat) == 0 and L.dispu_contour_count_scratch_bytes(nvox, (1 << 24) + 1) == 0
    buf, bent = scratch_cases(full)
    num, start, nv, nf = i32(7 * nlat), i32(nvox), C.c_longlong(-7), C.c_longlong(-7)
    ok = (nvox, nlat, _lib.ptr(corner), _lib.ptr(f), _lib.ptr(num), _lib.ptr(start), C.byref(nv), C.byref(nf), _lib.ptr(buf), full, st)
    calls = [bend(ok, _0=0), bend(ok, _0=-2), bend(ok, _1=0), bend(ok, _1=-2)] + [bend(ok, **{"_%d" % i: NULL}) for i in range(2, 8)]
    calls += [bend(ok, _4=_lib.ptr(corner)), bend(ok, _5=_lib.ptr(f)), bend(ok, _5=_lib.ptr(num))]
    calls += [bend(ok, _8=sp, _9=sb) for sp, sb in bent]
    for a in calls:
        assert L.dispu_contour_count(*a) == INVALID and sentinel(num, start) and nv.value == -7 and nf.value == -7
    assert L.dispu_contour_count(*ok) == 0 and nv.value > 0 and nf.value > 0

    # emit
    verts = torch.full((nv.value, 3), -7.0, dtype=torch.float32, device=dev)
    faces = i32(nf.value, 3)
    ok = (nvox, nlat, h, _lib.ptr(lat), _lib.ptr(corner), _lib.ptr(f), _lib.ptr(num), _lib.ptr(start), nv.value, nf.value, _lib.ptr(verts),
          _lib.ptr(faces), st)
    calls = [bend(ok, _0=0), bend(ok, _0=-2), bend(ok, _1=0), bend(ok, _1=-2), bend(ok, _2=0.0), bend(ok, _8=0), bend(ok, _8=-1),
             bend(ok, _8=7 * nlat + 1), bend(ok, _9=0), bend(ok, _9=-1), bend(ok, _9=12 * nvox + 1)]
    calls += [bend(ok, **{"_%d" % i: NULL}) for i in (3, 4, 5, 6, 7, 10, 11)]
    calls += [bend(ok, _10=_lib.ptr(num)), bend(ok, _11=_lib.ptr(corner)), bend(ok, _11=_lib.ptr(verts))]
    for a in calls:
        assert L.dispu_contour_emit(*a) == INVALID and sentinel(verts, faces)
    assert L.dispu_contour_emit(*ok) == 0
    want = R.reconstruct(NO.sphere(200), NO.sphere(200), 0.25)
    torch.cuda.synchronize(dev)
    assert same_bits(N(verts), want["verts"]) and np.array_equal(N(faces), want["faces"])
