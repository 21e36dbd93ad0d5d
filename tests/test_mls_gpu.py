"""GPU tests of dispu_mls_project_segments / dispu_amd.mls.mls_project (csrc/mls_project.hip) against tests/mls_oracle.py: the neighbour
indices bit for bit, one step against the float64 oracle to one fp32 ulp, iterations as chained calls, ragged batches, degenerate,
non-finite and refused input, the Python entry, and tools/upsample.py --denoise_input / --project_output end to end.  Every cloud has at
most 8193 points; an oracle run is shared through lru_cache.

The one-ulp check and its exclusions: a point is selected when the oracle moved it, (l1 - l0) / l2 >= 1e-2 and l1 > 1e-10 l2; selected
points must be the fp32 rounding of the oracle's float64 position or one of its two fp32 neighbours.  The unselected share is capped at
1 % wherever the oracle alone stays below it: at k = 16 and k = 32 it leaves out at most 1 point of any cloud here.  At k = 4 on the
ellipsoid the ORACLE ALONE (no device involved) leaves out 48 of 2049 points (2.3 %) at support 1.5, and more at each of nine other supports tried
from 1 to 4 (three or four weighted points are nearly collinear that often), so no implementation can meet the cap there; that case
asserts everything else and the share it has."""
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
import mls_oracle as O  # noqa: E402
import normals_oracle as NO  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue


def N(t):
    return t.detach().cpu().numpy()


def offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return off


def run_abi(dev, qs, rs, k, support=1.0, iterations=1, want_idx=True, qoff=None, roff=None, scratch="ok", C_arg=None, null=(), alias=None,
            scratch_buf=None):
    """the C entry on a packed batch of pairs, every output pre-filled with a sentinel -> (return code, out, idx, status).
    scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the zero-filled one.
    qoff / roff / C_arg / scratch / null / alias: what a refusal test bends (null: names of pointers passed as NULL; alias: "queries"
    or "refs", the array `out` is made to share)"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    q = torch.from_numpy(np.concatenate(qs).astype(np.float32)).to(dev)
    r = torch.from_numpy(np.concatenate(rs).astype(np.float32)).to(dev)
    good_q, good_r = offsets(qs), offsets(rs)
    qoff = np.ascontiguousarray(good_q if qoff is None else qoff, np.int32)
    roff = np.ascontiguousarray(good_r if roff is None else roff, np.int32)
    nC = len(qs) if C_arg is None else C_arg
    hq, hr = C.c_void_p(qoff.ctypes.data), C.c_void_p(roff.ctypes.data)
    full = L.dispu_mls_project_scratch_bytes(len(qs), C.c_void_p(good_q.ctypes.data), C.c_void_p(good_r.ctypes.data))
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
    total = q.shape[0]
    out = torch.full((total, 3), 7.0, dtype=torch.float32, device=dev)
    idx = torch.full((total, k), -7, dtype=torch.int32, device=dev) if want_idx else None
    status = torch.full((len(qs),), -7, dtype=torch.int32, device=dev)
    d_qoff, d_roff = torch.from_numpy(qoff).to(dev), torch.from_numpy(roff).to(dev)
    ptrs = dict(qoff=_lib.ptr(d_qoff), roff=_lib.ptr(d_roff), queries=_lib.ptr(q), refs=_lib.ptr(r), out=_lib.ptr(out), status=_lib.ptr(status))
    if alias is not None:
        ptrs["out"] = ptrs[alias]
    for name in null:
        ptrs[name] = C.c_void_p(0)
    q0, r0 = N(q).copy(), N(r).copy()
    rc = L.dispu_mls_project_segments(nC, ptrs["qoff"], hq, ptrs["roff"], hr, k, support, iterations, ptrs["queries"], ptrs["refs"],
                                      ptrs["out"], _lib.ptr(idx), ptrs["status"], sp, sb, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert np.array_equal(N(q).view(np.uint32), q0.view(np.uint32)) and np.array_equal(N(r).view(np.uint32), r0.view(np.uint32))   # inputs are only read
    if scratch_buf is not None:
        scratch_buf.inputs = dict(queries=N(q), refs=N(r), qoff=N(d_qoff), roff=N(d_roff))    # as the call left them
    return rc, N(out), (N(idx) if want_idx else None), N(status)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def cloud(name):
    r = np.random.RandomState(0)
    if name == "sphere":
        return NO.sphere(4097)
    if name == "sphere1":                                       # another sample of the same surface: the queries of the size sweep
        return NO.sphere(4097, seed=1)
    if name == "noisy":
        return O.denoise_self()
    if name == "cross_q":
        return O.denoise_cross()[0]
    if name == "cross_r":
        return O.denoise_cross()[1]
    if name == "ellipsoid":
        return NO.far_ellipsoid(2049)
    if name == "plane":
        return NO.noisy_plane(1500)
    if name == "lattice":
        return NO.lattice(17)                                   # 4913 points, massive distance ties
    if name == "coincident":                                    # more duplicates than k, spread over the index range
        p = r.random_sample((1040, 3)).astype(np.float32)
        p[r.permutation(1040)[:40]] = np.float32([0.25, 0.5, 0.75])
        return p
    if name == "clusters":                                      # two clusters 100 apart and 5 isolated points midway
        a = (r.random_sample((2000, 3)) - 0.5).astype(np.float32)
        b = (r.random_sample((2000, 3)) - 0.5).astype(np.float32) + np.float32([100, 0, 0])
        mid = np.float32([50, 0, 0]) + (r.random_sample((5, 3)) - 0.5).astype(np.float32)
        return np.concatenate([a, mid, b])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def neighbours32(qname, nq, rname, m):
    """the oracle's neighbours at k = 32: the first k columns are the neighbours at k (rows beyond min(k, m) padded afresh)"""
    return O.neighbors(cloud(qname)[:nq], cloud(rname)[:m], 32)


def oracle_idx(qname, nq, rname, m, k):
    idx = np.ascontiguousarray(neighbours32(qname, nq, rname, m)[0][:, :k])
    return idx


@functools.lru_cache(maxsize=None)
def oracle_step(qname, rname, k, support):
    q, r = cloud(qname), cloud(rname)
    i32, d32 = neighbours32(qname, len(q), rname, len(r))
    return O.step(q, r, k, support, idx=np.ascontiguousarray(i32[:, :k]), d2=np.ascontiguousarray(d32[:, :k]))


# ---- the search -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 16, 32])
def test_neighbours_at_every_size(dev, k):
    """every reference size against every query size as ONE ragged batch; 4097: 65 cells, so the seed sweep and the pruning are live"""
    pairs = [(nq, m) for m in sorted({1, 2, 3, k, k + 1, 63, 64, 65, 4097}) for nq in (1, 64, 65, 4097)]
    rc, _, idx, status = run_abi(dev, [cloud("sphere1")[:nq] for nq, _ in pairs], [cloud("sphere")[:m] for _, m in pairs], k)
    assert rc == 0 and not status.any()
    o = 0
    for nq, m in pairs:
        assert np.array_equal(idx[o:o + nq], oracle_idx("sphere1", nq, "sphere", m, k)), (nq, m, k)
        o += nq


@pytest.mark.parametrize("k", [4, 16, 32])
def test_neighbours_with_ties_duplicates_and_far_cells(dev, k):
    """lattice: the lower index wins among equal distances; coincident: 40 equal points, more than k; clusters: queries between two far
    clusters, a search that stops at nearby cells fails.  Each as references under sphere queries, and as queries over the sphere"""
    names = ("lattice", "coincident", "clusters")
    pairs = [("sphere", n) for n in names] + [(n, "sphere") for n in names]
    rc, _, idx, status = run_abi(dev, [cloud(a) for a, _ in pairs], [cloud(b) for _, b in pairs], k)
    assert rc == 0 and not status.any()
    o = 0
    for a, b in pairs:
        nq = len(cloud(a))
        want = oracle_idx(a, nq, b, len(cloud(b)), k)
        assert np.array_equal(idx[o:o + nq], want), (a, b, np.nonzero((idx[o:o + nq] != want).any(axis=1))[0][:10])
        o += nq


# ---- one step against float64 -----------------------------------------------------------------------------------------------------------

def check_step(q, out, idx, ref, cap=True):
    """the checks of one pair; ref is the oracle's dict on the same neighbourhoods -> the number of unselected points"""
    assert np.array_equal(idx, ref["idx"])
    q64, o64 = q.astype(np.float64), out.astype(np.float64)
    move = np.linalg.norm(o64 - q64, axis=1)
    print("largest move / sqrt(D): %.4f" % (move / np.maximum(np.sqrt(ref["D"]), 1e-300)).max())
    assert (move <= np.sqrt(ref["D"]) * (1 + 1e-6)).all()       # c is a convex combination of offsets no longer than sqrt(D)
    ok, ev = ref["ok"], ref["evals"]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (ev[:, 1] - ev[:, 0]) / ev[:, 2]
    sel = ok & (gap >= 1e-2) & (ev[:, 1] > 1e-10 * ev[:, 2])
    left = int((~sel).sum())
    r32 = ref["new64"].astype(np.float32)
    near = (out == r32) | (out == np.nextafter(r32, np.float32(-np.inf))) | (out == np.nextafter(r32, np.float32(np.inf)))
    print("unselected %d of %d, selected points off the oracle's rounding: %d, off by more than one ulp: %d" % (
        left, len(q), int((out != r32)[sel].any(axis=1).sum()), int((~near)[sel].any(axis=1).sum())))
    if cap:
        assert left <= 0.01 * len(q), "the gap filter leaves out %d of %d points" % (left, len(q))
    assert near[sel].all()
    assert same_bits(out[~ok], q[~ok])                          # points that stay by rule keep their bits
    return left


@pytest.mark.parametrize("support", [1.0, 1.5])
@pytest.mark.parametrize("qname,rname", [("noisy", "noisy"), ("ellipsoid", "ellipsoid"), ("plane", "plane"), ("cross_q", "cross_r")])
def test_one_step_against_float64(dev, qname, rname, support):
    """ellipsoid: 1 cm of structure at coordinates of 1000 -- moments of raw coordinates would lose it all"""
    rc, out, idx, status = run_abi(dev, [cloud(qname)], [cloud(rname)], 16, support)
    assert rc == 0 and status[0] == 0
    check_step(cloud(qname), out, idx, oracle_step(qname, rname, 16, support))


@pytest.mark.parametrize("k,support", [(4, 1.5), (32, 1.0)])
def test_one_step_at_other_k(dev, k, support):
    """k = 4 at support 1.5 (at support 1 the farthest of four has weight 0 and the plane through the point itself and two others
    moves nothing).  The cap on unselected points holds at k = 32; at k = 4 the oracle alone leaves out 48 of 2049 (module docstring),
    which is asserted as the figure it is"""
    rc, out, idx, status = run_abi(dev, [cloud("ellipsoid")], [cloud("ellipsoid")], k, support)
    assert rc == 0 and status[0] == 0
    left = check_step(cloud("ellipsoid"), out, idx, oracle_step("ellipsoid", "ellipsoid", k, support), cap=k != 4)
    if k == 4:
        assert left == 48


def test_idx_that_is_not_asked_for(dev):
    rc, out, idx, _ = run_abi(dev, [cloud("plane")], [cloud("plane")], 16, want_idx=False)
    rc2, out2, _, _ = run_abi(dev, [cloud("plane")], [cloud("plane")], 16)
    assert rc == 0 and rc2 == 0 and idx is None and same_bits(out, out2)


# ---- iterations, batches ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("qname,rname,support", [("noisy", "noisy", 1.5), ("cross_q", "cross_r", 1.0)])
def test_three_iterations_are_three_chained_calls(dev, qname, rname, support):
    """the surface stays fixed: every iteration searches the ORIGINAL references, in the self case too.  The first step is held to the
    oracle; later steps are not compared to a three-step oracle, because one ulp after step 1 may change a neighbour at step 2"""
    q, r = cloud(qname), cloud(rname)
    rc, out3, idx3, status = run_abi(dev, [q], [r], 16, support, iterations=3)
    assert rc == 0 and status[0] == 0
    cur = q
    for step in range(3):
        rc, cur, idx, status = run_abi(dev, [cur], [r], 16, support)
        assert rc == 0 and status[0] == 0
        if step == 0:
            check_step(q, cur, idx, oracle_step(qname, rname, 16, support))
    assert same_bits(out3, cur) and np.array_equal(idx3, idx)   # idx_out: the last iteration's neighbours
    rc, out2, _, _ = run_abi(dev, [q], [r], 16, support, iterations=2)         # an even count: the other side of the ping-pong
    rc1, one, _, _ = run_abi(dev, [q], [r], 16, support)
    rc2, two, _, _ = run_abi(dev, [one], [r], 16, support)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and same_bits(out2, two)


def test_ragged_batch_equals_each_pair_alone(dev):
    qs = [cloud("noisy")[:n] for n in (1, 65, 4097, 3)]
    rs = [cloud("sphere")[:m] for m in (3, 4097, 65, 1)]
    for iterations in (1, 2):
        rc, out, idx, status = run_abi(dev, qs, rs, 16, 1.5, iterations=iterations)
        rcb, outb, idxb, _ = run_abi(dev, qs, rs, 16, 1.5, iterations=iterations)
        assert rc == 0 and rcb == 0 and not status.any()
        assert out.tobytes() == outb.tobytes() and idx.tobytes() == idxb.tobytes()      # two calls, identical bytes
        o = 0
        for q, r in zip(qs, rs):
            rc1, out1, idx1, _ = run_abi(dev, [q], [r], 16, 1.5, iterations=iterations)
            assert rc1 == 0 and same_bits(out[o:o + len(q)], out1) and np.array_equal(idx[o:o + len(q)], idx1)
            o += len(q)


# ---- degenerate and refused input -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 16])
def test_every_stay_rule(dev, k):
    """the inputs of the CPU test as one batch per support: every query keeps its bits"""
    cases = O.stay_cases()
    for support in sorted({s for _, _, s, _ in cases}):
        mine = [c for c in cases if c[2] == support]
        for iterations in (1, 2):
            rc, out, idx, status = run_abi(dev, [c[0] for c in mine], [c[1] for c in mine], k, support, iterations=iterations)
            assert rc == 0 and not status.any()
            o = 0
            for q, r, _, why in mine:
                assert same_bits(out[o:o + len(q)], q), why
                assert np.array_equal(idx[o:o + len(q)], O.neighbors(q, r, k)[0]), why
                o += len(q)
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])         # the three points that held the query at support 1 are a plane at 2
    rc, out, _, _ = run_abi(dev, [np.float32([[0.2, 0.3, 0.5]])], [tri], k, 2.0)
    assert rc == 0 and np.abs(out - np.float32([[0.2, 0.3, 0.0]])).max() <= 1e-7


@pytest.mark.parametrize("poison", [np.nan, np.inf])
@pytest.mark.parametrize("where", ["queries", "refs"])
def test_non_finite_segment_is_flagged_and_left_alone(dev, poison, where):
    qs = [cloud("noisy")[:300], cloud("plane")[:200].copy(), cloud("ellipsoid")[:129]]
    rs = [cloud("sphere")[:500], cloud("plane")[:400].copy(), cloud("ellipsoid")[:300]]
    (qs if where == "queries" else rs)[1][77, 1] = poison
    for iterations in (1, 3):
        rc, out, idx, status = run_abi(dev, qs, rs, 16, 1.5, iterations=iterations)
        assert rc == 0 and list(status) == [0, 1, 0]
        assert (out[300:500] == 7).all() and (idx[300:500] == -7).all()         # none of its rows is written
        for lo, hi, c in [(0, 300, 0), (500, 629, 2)]:
            _, o1, i1, _ = run_abi(dev, [qs[c]], [rs[c]], 16, 1.5, iterations=iterations)
            assert same_bits(out[lo:hi], o1) and np.array_equal(idx[lo:hi], i1)


def untouched(res):
    _, out, idx, status = res
    return (out == 7).all() and (idx == -7).all() and (status == -7).all()


def test_abi_refusals_touch_nothing(dev):
    qs, rs = [cloud("noisy")[:500], cloud("plane")[:300]], [cloud("sphere")[:400], cloud("plane")[:600]]
    bent = (np.int32([0, 500, 400]), np.int32([0, 500, 500]), np.int32([1, 500, 800]))
    cases = [dict(k=3), dict(k=33), dict(support=0.5), dict(support=4.5), dict(support=float("nan")), dict(support=float("inf")),
             dict(iterations=0), dict(iterations=9), dict(iterations=-1), dict(C_arg=0), dict(C_arg=65536),
             dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"), dict(alias="queries"), dict(alias="refs")]
    cases += [dict(qoff=b) for b in bent] + [dict(roff=b) for b in bent]
    cases += [dict(null=(name,)) for name in ("qoff", "roff", "queries", "refs", "out", "status")]
    for kw in cases:
        kw.setdefault("k", 16)
        res = run_abi(dev, qs, rs, **kw)
        assert res[0] == INVALID and untouched(res), kw
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    good = C.c_void_p(offsets(qs).ctypes.data)
    assert L.dispu_mls_project_scratch_bytes(2, good, good) > 0
    for b in bent:
        bad = C.c_void_p(b.ctypes.data)
        assert L.dispu_mls_project_scratch_bytes(2, bad, good) == 0 and L.dispu_mls_project_scratch_bytes(2, good, bad) == 0
    assert L.dispu_mls_project_scratch_bytes(0, good, good) == 0 and L.dispu_mls_project_scratch_bytes(65536, good, good) == 0
    big = np.int32([0, (1 << 24) + 1])
    one = np.int32([0, 5])
    assert L.dispu_mls_project_scratch_bytes(1, C.c_void_p(big.ctypes.data), C.c_void_p(one.ctypes.data)) == 0   # a segment above 2^24 points
    res = run_abi(dev, qs, rs, 16)                              # the same call, legal
    assert res[0] == 0 and not res[3].any() and not (res[1] == 7).all(axis=1).any()


# ---- the Python entry -------------------------------------------------------------------------------------------------------------------

def test_python_entry(dev):
    import torch
    from dispu_amd.mls import mls_project
    noisy, cq, cr = cloud("noisy"), cloud("cross_q"), cloud("cross_r")
    p, dq, dr = (torch.from_numpy(x).to(dev) for x in (noisy, cq, cr))
    out, idx = mls_project(p, k=16, support=1.5, return_neighbors=True)
    assert out.shape == (4097, 3) and out.dtype == torch.float32 and idx.shape == (4097, 16) and idx.dtype == torch.int32
    assert out.data_ptr() != p.data_ptr() and same_bits(N(p), noisy)
    ref = oracle_step("noisy", "noisy", 16, 1.5)
    assert np.array_equal(N(idx), ref["idx"])
    assert same_bits(N(mls_project(p, p, k=16, support=1.5)), N(out))                           # refs=None is refs=queries
    assert same_bits(N(out), run_abi(dev, [noisy], [noisy], 16, 1.5)[1])
    # the two denoising cases: the device's radial RMS equals the oracle's
    cross = mls_project(dq, dr)                                                                 # k = 16, support = 1.0, one step
    for got, want, before, factor in ((N(out), ref["new32"], noisy, 0.5), (N(cross), oracle_step("cross_q", "cross_r", 16, 1.0)["new32"], cq, 0.25)):
        a, b = O.radial_rms(got), O.radial_rms(want)
        print("radial RMS: input %.6f, device %.9f, oracle %.9f" % (O.radial_rms(before), a, b))
        assert abs(a - b) <= 1e-6 * b and a < factor * O.radial_rms(before)
    # lists: one packed launch sequence, lists out
    lo, li = mls_project([dq, p[:65]], [dr, p], k=8, support=2.0, iterations=2, return_neighbors=True)
    assert isinstance(lo, list) and isinstance(li, list) and lo[0].shape == (8192, 3) and li[1].shape == (65, 8)
    assert same_bits(N(lo[0]), N(mls_project(dq, dr, k=8, support=2.0, iterations=2)))
    assert same_bits(N(lo[1]), N(mls_project(p[:65], p, k=8, support=2.0, iterations=2)))
    self_list = mls_project([p, dr], k=16, support=1.5)
    assert same_bits(N(self_list[0]), N(out)) and self_list[1].shape == (2049, 3)
    for bad in (dict(k=3), dict(k=33), dict(k=16.0), dict(support=0.5), dict(support=float("nan")), dict(support="1"), dict(support=5),
                dict(iterations=0), dict(iterations=9), dict(iterations=1.0)):
        with pytest.raises(ValueError):
            mls_project(p, **bad)
    for bad in (p.double(), p[:, :2], p.reshape(1, -1, 3), p[:0], p.cpu()):
        with pytest.raises(ValueError):
            mls_project(bad)
        with pytest.raises(ValueError):
            mls_project(p, bad)
    poisoned = noisy[:300].copy()
    poisoned[5, 0] = np.inf
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):      # found by the launch, raised after it
        mls_project([p[:100], p[:300]], [p, torch.from_numpy(poisoned).to(dev)])


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------

def test_upsample_tool_denoises_and_projects(dev, tmp_path):
    from dispu_amd import checkpoint as CK
    from oracle import generator as OG
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    np.savetxt(str(data / "test" / "ball.xyz"), O.noisy_sphere(2048, 9, 0.01, 10), fmt="%.6f")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    runs = {"plain": [], "off": ["--denoise_input", "0", "--project_output", "0", "--mls_k", "8", "--mls_support", "2"],
            "mls": ["--denoise_input", "1", "--project_output", "1"], "input": ["--denoise_input", "2", "--mls_support", "1.5"]}
    procs = {name: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for name, extra in runs.items()}
    for name, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    files = {name: open(str(tmp_path / name / "ball_X4.xyz"), "rb").read() for name in runs}
    assert files["off"] == files["plain"]                       # both at 0: the bytes of a run without the flags
    for name in ("mls", "input"):
        rows = np.loadtxt(str(tmp_path / name / "ball_X4.xyz"), ndmin=2)
        assert rows.shape == (4 * 2048, 3) and np.isfinite(rows).all()
        assert files[name] != files["plain"]
