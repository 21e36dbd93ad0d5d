"""GPU tests of dispu_icp_segments / dispu_rigid_apply_segments / dispu_amd.registration (csrc/icp.hip) against tests/icp_oracle.py,
through the C ABI with sentinel-filled outputs: the apply bit for bit, the evaluation (iterations = 0) with exact correspondences, one
step against the float64 oracle, iterations as chained calls, recovery of a known motion, freezing, ragged batches, degenerate,
non-finite and refused input, and the Python entry.  Every cloud has at most 4913 points; the oracle's runs are shared through its
lru_cache.

The bound of one step on T: the kernel and the oracle add the same n terms in different orders, each sum within n * 2^-53 relative of
the exact one; the solve amplifies that by cond(A) (the oracle's); the motion is composed about the target's first point, so an entry of
T scales with the coordinates: 64 * n * 2^-53 * cond(A) * max(1, max |coordinate|), 64 for the constants."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import icp_oracle as O  # noqa: E402
import normals_oracle as NO  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue
INF = float("inf")
OUTS = ("T", "aligned", "corr", "inliers", "rmse", "iters", "flag", "status")


def N(t):
    return t.detach().cpu().numpy()


def offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return off


def run_abi(dev, srcs, tgts, normals=None, init=None, iterations=1, max_distance=INF, tolerance=0.0, want_corr=True, mode=None,
            max_d2=None, qoff=None, roff=None, scratch="ok", C_arg=None, null=(), alias=None, scratch_buf=None):
    """the C entry on a packed batch of pairs, every output pre-filled with a sentinel -> dict(rc and the names of OUTS).
    scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the zero-filled one.
    normals: a list like tgts (plane mode) or None;  init: a list of 4 x 4 arrays or None;  mode / max_d2 / qoff / roff / C_arg /
    scratch / null / alias: what a refusal test bends (null: names of pointers passed as NULL; alias: "source" or "target", the array
    `aligned` is made to share)"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    nc = len(srcs)
    q = torch.from_numpy(np.concatenate(srcs).astype(np.float32)).to(dev)
    r = torch.from_numpy(np.concatenate(tgts).astype(np.float32)).to(dev)
    nr = None if normals is None else torch.from_numpy(np.concatenate(normals).astype(np.float32)).to(dev)
    t0 = None if init is None else torch.from_numpy(np.stack([np.asarray(m, np.float64).reshape(4, 4) for m in init])).to(dev)
    good_q, good_r = offsets(srcs), offsets(tgts)
    qoff = np.ascontiguousarray(good_q if qoff is None else qoff, np.int32)
    roff = np.ascontiguousarray(good_r if roff is None else roff, np.int32)
    hq, hr = C.c_void_p(qoff.ctypes.data), C.c_void_p(roff.ctypes.data)
    full = L.dispu_icp_scratch_bytes(nc, C.c_void_p(good_q.ctypes.data), C.c_void_p(good_r.ctypes.data))
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
    o = dict(T=torch.full((nc, 4, 4), 7.0, dtype=torch.float64, device=dev), aligned=torch.full((total, 3), 7.0, dtype=torch.float32, device=dev),
             corr=torch.full((total,), -7, dtype=torch.int32, device=dev) if want_corr else None,
             inliers=torch.full((nc,), -7, dtype=torch.int32, device=dev), rmse=torch.full((nc,), 7.0, dtype=torch.float64, device=dev),
             iters=torch.full((nc,), -7, dtype=torch.int32, device=dev), flag=torch.full((nc,), -7, dtype=torch.int32, device=dev),
             status=torch.full((nc,), -7, dtype=torch.int32, device=dev))
    d_qoff, d_roff = torch.from_numpy(qoff).to(dev), torch.from_numpy(roff).to(dev)
    ptrs = dict(qoff=_lib.ptr(d_qoff), roff=_lib.ptr(d_roff), source=_lib.ptr(q), target=_lib.ptr(r), normals=_lib.ptr(nr), init=_lib.ptr(t0))
    ptrs.update({name: _lib.ptr(t) for name, t in o.items()})
    if alias is not None:
        ptrs["aligned"] = ptrs[alias]
    for name in null:
        ptrs[name] = C.c_void_p(0)
    q0, r0 = N(q).copy(), N(r).copy()
    if max_d2 is None:
        max_d2 = float(O.max_d2_of(max_distance))
    rc = L.dispu_icp_segments(nc if C_arg is None else C_arg, ptrs["qoff"], hq, ptrs["roff"], hr, (0 if normals is None else 1) if mode is None else mode,
                              iterations, max_d2, tolerance, ptrs["source"], ptrs["target"], ptrs["normals"], ptrs["init"], ptrs["T"],
                              ptrs["aligned"], ptrs["corr"], ptrs["inliers"], ptrs["rmse"], ptrs["iters"], ptrs["flag"], ptrs["status"], sp, sb,
                              _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert np.array_equal(N(q).view(np.uint32), q0.view(np.uint32)) and np.array_equal(N(r).view(np.uint32), r0.view(np.uint32))   # inputs are only read
    if scratch_buf is not None:
        scratch_buf.inputs = dict(queries=N(q), refs=N(r), qoff=N(d_qoff), roff=N(d_roff))    # as the call left them
    res = {name: (N(t) if t is not None else None) for name, t in o.items()}
    res["rc"] = rc
    return res


def same_bytes(a, b, names=OUTS, rows=None, pair=None):
    """every named output of a (its point rows `rows` and pair `pair`, or all of it) equals b's byte for byte"""
    for name in names:
        x = a[name]
        if x is None and b[name] is None:
            continue
        if rows is not None and name in ("aligned", "corr"):
            x = x[rows[0]:rows[1]]
        elif pair is not None and name not in ("aligned", "corr"):
            x = x[pair:pair + 1]
        if np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(b[name]).tobytes():
            return False
    return True


def untouched(res, pair=None, rows=None):
    """the sentinels are still there (for one pair and its point rows, or everywhere)"""
    pr = slice(None) if pair is None else slice(pair, pair + 1)
    rw = slice(None) if rows is None else slice(rows[0], rows[1])
    return ((res["T"][pr] == 7).all() and (res["aligned"][rw] == 7).all() and (res["corr"] is None or (res["corr"][rw] == -7).all())
            and (res["rmse"][pr] == 7).all() and all((res[n][pr] == -7).all() for n in ("inliers", "iters", "flag")))


@functools.lru_cache(maxsize=None)
def cloud(name):
    r = np.random.RandomState(0)
    if name == "sphere":
        return NO.sphere(4097)
    if name == "sphere1":                                       # another sample of the same surface, moved a little: the ragged sources
        return O.apply(O.motion(NO.sphere(4097)), NO.sphere(4097, seed=1))
    if name == "lattice":
        return NO.lattice(17)                                   # 4913 points, massive distance ties
    if name == "coincident":                                    # the coincident cloud of test_mls_gpu.py
        p = r.random_sample((1040, 3)).astype(np.float32)
        p[r.permutation(1040)[:40]] = np.float32([0.25, 0.5, 0.75])
        return p
    if name == "clusters":                                      # the clusters cloud of test_mls_gpu.py
        a = (r.random_sample((2000, 3)) - 0.5).astype(np.float32)
        b = (r.random_sample((2000, 3)) - 0.5).astype(np.float32) + np.float32([100, 0, 0])
        mid = np.float32([50, 0, 0]) + (r.random_sample((5, 3)) - 0.5).astype(np.float32)
        return np.concatenate([a, mid, b])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def unit_normals(name):
    """seeded unit vectors, one per point of the cloud: what the correspondence tests feed plane mode (the sphere's own are its points)"""
    if name in ("sphere", "sphere1"):
        return NO.sphere(4097)
    return NO.sphere(len(cloud(name)), seed=5)


def small_motion():
    return O.motion(NO.sphere(257))


@functools.lru_cache(maxsize=None)
def matched_under_small_motion(a, b):
    """the oracle's nearest points of cloud a under small_motion() in cloud b: one brute-force search shared by modes and distances"""
    return O.match(O.apply(small_motion(), cloud(a)), cloud(b))[:2]


# ---- the apply ---------------------------------------------------------------------------------------------------------------------------

def run_apply(dev, clouds, Ts, off=None, C_arg=None, null=()):
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    p = torch.from_numpy(np.concatenate(clouds).astype(np.float32)).to(dev)
    t = torch.from_numpy(np.stack(Ts).astype(np.float64)).to(dev)
    off = np.ascontiguousarray(offsets(clouds) if off is None else off, np.int32)
    d_off = torch.from_numpy(off).to(dev)
    out = torch.full(tuple(p.shape), 7.0, dtype=torch.float32, device=dev)
    ptrs = dict(off=_lib.ptr(d_off), points=_lib.ptr(p), transform=_lib.ptr(t), out=_lib.ptr(out))
    for name in null:
        ptrs[name] = C.c_void_p(0)
    rc = _lib.lib().dispu_rigid_apply_segments(len(clouds) if C_arg is None else C_arg, ptrs["off"], C.c_void_p(off.ctypes.data), ptrs["points"],
                                               ptrs["transform"], ptrs["out"], _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, N(out)


def test_apply_equals_the_numpy_restatement_bit_for_bit(dev):
    r = np.random.RandomState(3)
    clouds = [(cloud("clusters")[::-1][:n] * np.float32(1.7)).astype(np.float32) for n in (1, 64, 65, 4097)]
    Ts = []
    for i in range(4):                                          # a rotation, a large translation; the last one any matrix at all
        T = O.motion(cloud("sphere")[:50 + i])
        T[:3, 3] += r.standard_normal(3) * 100
        Ts.append(T)
    Ts[3][:3, :] = r.standard_normal((3, 4))
    rc, out = run_apply(dev, clouds, Ts)
    assert rc == 0
    o = 0
    for c, T in zip(clouds, Ts):
        assert out[o:o + len(c)].tobytes() == O.apply(T, c).tobytes()
        o += len(c)
    rc, out = run_apply(dev, clouds, [np.eye(4)] * 4)
    assert rc == 0 and out.tobytes() == np.concatenate(clouds).tobytes()       # the identity returns the input's bits
    for kw in (dict(C_arg=0), dict(C_arg=65536), dict(off=np.int32([0, 1, 65, 64, 4227])), dict(off=np.int32([1, 2, 66, 131, 4228])),
               dict(null=("off",)), dict(null=("points",)), dict(null=("transform",)), dict(null=("out",))):
        rc, out = run_apply(dev, clouds, Ts, **kw)
        assert rc == INVALID and (out == 7).all(), kw


# ---- the evaluation: iterations = 0 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_distance", [INF, 0.1])
@pytest.mark.parametrize("plane", [False, True])
def test_evaluation_at_a_given_init(dev, plane, max_distance):
    """lattice: the lower index wins among equal distances; coincident: 40 equal points; clusters: a search that stops at nearby cells
    fails.  Each as the target under the sphere, and as the source over the sphere, as ONE batch"""
    names = ("lattice", "coincident", "clusters")
    pairs = [("sphere", n) for n in names] + [(n, "sphere") for n in names]
    M = small_motion()
    srcs, tgts = [cloud(a) for a, _ in pairs], [cloud(b) for _, b in pairs]
    nrms = [unit_normals(b) for _, b in pairs] if plane else None
    res = run_abi(dev, srcs, tgts, nrms, init=[M] * len(pairs), iterations=0, max_distance=max_distance)
    assert res["rc"] == 0 and not res["status"].any()
    assert not res["iters"].any() and not res["flag"].any()
    o = 0
    for c, (a, b) in enumerate(pairs):
        want = O.evaluate(M, srcs[c], tgts[c], O.max_d2_of(max_distance), nrms[c] if plane else None, matched_under_small_motion(a, b))
        n = len(srcs[c])
        assert res["T"][c].tobytes() == M.tobytes(), (a, b)
        assert res["aligned"][o:o + n].tobytes() == want["aligned"].tobytes(), (a, b)
        assert np.array_equal(res["corr"][o:o + n], want["corr"]), (a, b, np.nonzero(res["corr"][o:o + n] != want["corr"])[0][:10])
        assert res["inliers"][c] == want["inliers"], (a, b)
        print("%s -> %s: inliers %d, rmse %.17g, oracle %.17g" % (a, b, want["inliers"], res["rmse"][c], want["rmse"]))
        assert abs(res["rmse"][c] - want["rmse"]) <= n * 2.0 ** -53 * want["rmse"], (a, b)
        o += n
    if max_distance == 0.1:
        assert 0 < res["inliers"].sum() < sum(len(s) for s in srcs)             # the cap on the distance is live both ways


def test_corr_that_is_not_asked_for(dev):
    p, nrm, src, _ = O.cap()
    a = run_abi(dev, [src], [p], [nrm], iterations=2)
    b = run_abi(dev, [src], [p], [nrm], iterations=2, want_corr=False)
    assert a["rc"] == 0 and b["rc"] == 0 and b["corr"] is None and same_bytes(a, b, [n for n in OUTS if n != "corr"])


# ---- one step against float64 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("name", ["cap", "far"])
def test_one_step_against_float64(dev, name, plane):
    """far: 2 cm of structure at coordinates of 1000 -- equations about the coordinate origin would lose it all"""
    p, nrm, src, _ = O.cap() if name == "cap" else O.far()
    ref = O.first_step(name, plane)
    res = run_abi(dev, [src], [p], [nrm] if plane else None, iterations=1)
    assert res["rc"] == 0 and res["status"][0] == 0 and res["iters"][0] == 1 and res["flag"][0] == 0
    T = res["T"][0]
    assert np.array_equal(T[3], [0, 0, 0, 1])
    assert res["aligned"].tobytes() == O.apply(T, src).tobytes()               # the device's own T reproduces aligned bit for bit
    n = len(src)
    bound = 64 * n * 2.0 ** -53 * ref["cond"] * max(1.0, float(np.abs(np.concatenate([p, src])).max()))
    print("%s %s: max |T - oracle| %.3g, bound %.3g, cond %.3g" % (name, "plane" if plane else "point", np.abs(T - ref["T"]).max(), bound, ref["cond"]))
    assert np.abs(T - ref["T"]).max() <= bound
    r32 = O.apply64(ref["T"], src).astype(np.float32)
    got = res["aligned"]
    near = (got == r32) | (got == np.nextafter(r32, np.float32(-np.inf))) | (got == np.nextafter(r32, np.float32(np.inf)))
    print("points off the oracle's rounding: %d, off by more than one ulp: %d" % (int((got != r32).any(axis=1).sum()), int((~near).any(axis=1).sum())))
    assert near.all()                                           # every point, no exclusions


# ---- iterations, recovery, freezing, batches ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plane", [False, True])
def test_iterations_are_chained_calls(dev, plane):
    """k iterations at tolerance 0 are k calls of one, each given the transform of the last as init: every output byte for byte (iters
    counts the updates of its own call)"""
    p, nrm, src, _ = O.cap()
    nr = [nrm] if plane else None
    rest = [n for n in OUTS if n != "iters"]
    for k in (3, 2):
        whole = run_abi(dev, [src], [p], nr, iterations=k)
        assert whole["rc"] == 0 and whole["iters"][0] == k and whole["flag"][0] == 0
        T = None
        for _ in range(k):
            one = run_abi(dev, [src], [p], nr, init=T, iterations=1)
            assert one["rc"] == 0 and one["iters"][0] == 1
            T = [one["T"][0]]
        assert same_bytes(whole, one, rest), k


@pytest.mark.parametrize("plane", [False, True])
def test_recovers_the_motion_on_cap(dev, plane):
    p, nrm, src, truth = O.cap()
    ref = O.recovery(plane)
    res = run_abi(dev, [src], [p], [nrm] if plane else None, iterations=8 if plane else 40)
    err = np.abs(res["aligned"].astype(np.float64) - truth).max()
    print("rmse %.3g (oracle %.3g), max |aligned - truth| %.3g" % (res["rmse"][0], ref["rmse"], err))
    assert res["rc"] == 0 and res["status"][0] == 0 and res["flag"][0] == 0 and res["inliers"][0] == len(src)
    assert res["rmse"][0] <= 2 * ref["rmse"] + 1e-7 and err <= 2e-6
    assert np.array_equal(res["corr"], np.arange(0, len(p), 2))                # every point found the point it came from


def test_a_converged_pair_freezes(dev):
    p, nrm, src, _ = O.cap()
    res = run_abi(dev, [src], [p], [nrm], iterations=20, tolerance=1e-6)
    t = int(res["iters"][0])
    assert res["rc"] == 0 and res["flag"][0] == 1 and 0 < t < 20
    assert same_bytes(res, run_abi(dev, [src], [p], [nrm], iterations=t, tolerance=1e-6))
    # in a batch: a pair that starts nearly aligned freezes first, beside one that runs on; neither changes
    early = np.linalg.inv(O.motion(p))
    both = run_abi(dev, [src, src], [p, p], [nrm, nrm], init=[early, np.eye(4)], iterations=20, tolerance=1e-6)
    assert both["rc"] == 0 and list(both["flag"]) == [1, 1] and both["iters"][0] < both["iters"][1] == t
    n = len(src)
    assert same_bytes(both, res, rows=(n, 2 * n), pair=1)
    assert same_bytes(both, run_abi(dev, [src], [p], [nrm], init=[early], iterations=20, tolerance=1e-6), rows=(0, n), pair=0)
    never = run_abi(dev, [src], [p], [nrm], iterations=20, tolerance=0.0)      # tolerance 0 never freezes a pair
    assert never["flag"][0] == 0 and never["iters"][0] == 20


@pytest.mark.parametrize("plane", [False, True])
def test_ragged_batch_equals_each_pair_alone(dev, plane):
    srcs = [cloud("sphere1")[:n] for n in (1, 65, 4097, 3)]
    tgts = [cloud("sphere")[:m] for m in (3, 4097, 65, 1)]
    nrms = [unit_normals("sphere")[:m] for m in (3, 4097, 65, 1)] if plane else None
    a = run_abi(dev, srcs, tgts, nrms, iterations=2)
    b = run_abi(dev, srcs, tgts, nrms, iterations=2)
    assert a["rc"] == 0 and b["rc"] == 0 and not a["status"].any() and same_bytes(a, b)       # two calls, identical bytes
    o = 0
    for c in range(4):
        solo = run_abi(dev, [srcs[c]], [tgts[c]], [nrms[c]] if plane else None, iterations=2)
        assert solo["rc"] == 0 and same_bytes(a, solo, rows=(o, o + len(srcs[c])), pair=c), c
        o += len(srcs[c])


# ---- degenerate, non-finite and refused input --------------------------------------------------------------------------------------------

def test_degenerate_pairs_keep_their_transform(dev):
    for src, tgt, nrm, max_distance, why in O.degenerate_cases():
        for init in (None, [small_motion()]):
            res = run_abi(dev, [src], [tgt], None if nrm is None else [nrm], init=init, iterations=3, max_distance=max_distance)
            T0 = np.eye(4) if init is None else init[0]
            assert res["rc"] == 0 and res["status"][0] == 0 and res["flag"][0] == 2 and res["iters"][0] == 0, why
            assert res["T"][0].tobytes() == T0.tobytes() and res["aligned"].tobytes() == O.apply(T0, src).tobytes(), why
    t, _, s = O.coplanar()                                      # the same coplanar pair point to point is an ordinary problem
    res = run_abi(dev, [s], [t], None, iterations=3)
    assert res["rc"] == 0 and res["flag"][0] == 0 and res["iters"][0] == 3


@pytest.mark.parametrize("poison", [np.nan, np.inf])
@pytest.mark.parametrize("where", ["source", "target"])
def test_non_finite_pair_is_flagged_and_left_alone(dev, poison, where):
    p, nrm, src, _ = O.cap()
    srcs = [src[:300], src[300:500].copy(), cloud("sphere1")[:129]]
    tgts = [p[:500], p[:400].copy(), cloud("sphere")[:300]]
    nrms = [nrm[:500], nrm[:400], unit_normals("sphere")[:300]]
    (srcs if where == "source" else tgts)[1][77, 1] = poison
    for iterations in (1, 3):
        res = run_abi(dev, srcs, tgts, nrms, iterations=iterations)
        assert res["rc"] == 0 and list(res["status"]) == [0, 1, 0]
        assert untouched(res, pair=1, rows=(300, 500))          # none of its rows is written
        for rows, c in [((0, 300), 0), ((500, 629), 2)]:
            solo = run_abi(dev, [srcs[c]], [tgts[c]], [nrms[c]], iterations=iterations)
            assert same_bytes(res, solo, rows=rows, pair=c)


def test_abi_refusals_touch_nothing(dev):
    p, nrm, src, _ = O.cap()
    srcs, tgts, nrms = [src[:500], src[500:800]], [p[:400], p[400:1000]], [nrm[:400], nrm[400:1000]]
    bent = (np.int32([0, 500, 400]), np.int32([0, 500, 500]), np.int32([1, 500, 800]))
    cases = [dict(mode=-1), dict(mode=2), dict(iterations=-1), dict(iterations=129), dict(max_d2=float("nan")), dict(max_d2=-1.0),
             dict(tolerance=float("nan")), dict(tolerance=-1e-9), dict(tolerance=INF), dict(C_arg=0), dict(C_arg=65536),
             dict(scratch="null"), dict(scratch="short"), dict(scratch="misaligned"), dict(alias="source"), dict(alias="target")]
    cases += [dict(qoff=b) for b in bent] + [dict(roff=b) for b in bent]
    cases += [dict(null=(name,)) for name in ("qoff", "roff", "source", "target", "normals", "T", "aligned", "inliers", "rmse", "iters", "flag",
                                              "status")]
    for kw in cases:
        res = run_abi(dev, srcs, tgts, nrms, **kw)
        assert res["rc"] == INVALID and untouched(res) and (res["status"] == -7).all(), kw
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    good = C.c_void_p(offsets(srcs).ctypes.data)
    assert L.dispu_icp_scratch_bytes(2, good, good) > 0
    for b in bent:
        bad = C.c_void_p(b.ctypes.data)
        assert L.dispu_icp_scratch_bytes(2, bad, good) == 0 and L.dispu_icp_scratch_bytes(2, good, bad) == 0
    assert L.dispu_icp_scratch_bytes(0, good, good) == 0 and L.dispu_icp_scratch_bytes(65536, good, good) == 0
    big, one = np.int32([0, (1 << 24) + 1]), np.int32([0, 5])
    assert L.dispu_icp_scratch_bytes(1, C.c_void_p(big.ctypes.data), C.c_void_p(one.ctypes.data)) == 0   # a segment above 2^24 points
    res = run_abi(dev, srcs, tgts, nrms)                        # the same call, legal; NULL normals are legal point to point
    assert res["rc"] == 0 and not res["status"].any() and not (res["aligned"] == 7).all(axis=1).any()
    res = run_abi(dev, srcs, tgts, None, null=("normals", "init", "corr"))
    assert res["rc"] == 0 and not res["status"].any() and (res["iters"] == 1).all()


# ---- the Python entry --------------------------------------------------------------------------------------------------------------------

def test_python_entry(dev):
    import torch
    from dispu_amd.registration import apply_transform, icp
    p, nrm, src, truth = O.cap()
    dp, dn, ds = (torch.from_numpy(x).to(dev) for x in (p, nrm, src))
    r = icp(ds, dp, dn, tolerance=0.0, iterations=8, return_correspondences=True)
    assert r.transform.shape == (4, 4) and r.transform.dtype == torch.float64 and r.transform.is_cuda
    assert r.aligned.shape == (1546, 3) and r.aligned.dtype == torch.float32 and r.correspondences.shape == (1546,)
    assert r.correspondences.dtype == torch.int32 and r.aligned.data_ptr() != ds.data_ptr() and N(ds).tobytes() == src.tobytes()
    assert float(r.fitness) == 1.0 and float(r.rmse) <= 1e-6 and int(r.iterations) == 8 and not bool(r.converged) and not bool(r.degenerate)
    abi = run_abi(dev, [src], [p], [nrm], iterations=8)
    assert N(r.transform).tobytes() == abi["T"][0].tobytes() and N(r.aligned).tobytes() == abi["aligned"].tobytes()
    assert np.array_equal(N(r.correspondences), abi["corr"])
    assert N(apply_transform(ds, r.transform)).tobytes() == N(r.aligned).tobytes()
    d = icp(ds, dp)                                             # the defaults: point to point, 30 iterations, tolerance 1e-6
    assert d.correspondences is None and d.transform.shape == (4, 4) and int(d.iterations) <= 30
    half = icp(ds, dp, max_distance=0.05, iterations=0, return_correspondences=True)
    assert 0.0 < float(half.fitness) < 1.0 and int((N(half.correspondences) >= 0).sum()) == round(float(half.fitness) * 1546)
    assert N(half.transform).tobytes() == np.eye(4).tobytes() and N(half.aligned).tobytes() == src.tobytes()
    # init: a float32 matrix is taken as float64; the returned transform of one call continues the next
    M = torch.from_numpy(small_motion().astype(np.float32)).to(dev)
    a = icp(ds, dp, dn, init=M, iterations=1, tolerance=0.0)
    assert N(a.transform).tobytes() == run_abi(dev, [src], [p], [nrm], init=[N(M).astype(np.float64)], iterations=1)["T"][0].tobytes()
    # lists: one packed launch sequence, lists out, per-pair tensors
    lst = icp([ds, ds[:65]], [dp, dp], [dn, dn], init=[r.transform, M], iterations=2, tolerance=0.0, return_correspondences=True)
    assert isinstance(lst.aligned, list) and isinstance(lst.correspondences, list) and lst.transform.shape == (2, 4, 4)
    assert lst.aligned[1].shape == (65, 3) and lst.fitness.shape == (2,) and lst.converged.dtype == torch.bool
    solo = icp(ds[:65], dp, dn, init=M, iterations=2, tolerance=0.0)
    assert N(lst.transform[1]).tobytes() == N(solo.transform).tobytes() and N(lst.aligned[1]).tobytes() == N(solo.aligned).tobytes()
    stacked = icp([ds, ds[:65]], [dp, dp], [dn, dn], init=torch.stack([r.transform, M.double()]), iterations=2, tolerance=0.0)
    assert N(stacked.transform).tobytes() == N(lst.transform).tobytes()
    outs = apply_transform([ds, ds[:65]], lst.transform)
    assert isinstance(outs, list) and N(outs[0]).tobytes() == N(lst.aligned[0]).tobytes()
    for bad in (dict(iterations=-1), dict(iterations=129), dict(iterations=2.0), dict(max_distance=-1.0), dict(max_distance=float("nan")),
                dict(max_distance="1"), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=INF), dict(init=torch.eye(3, device=dev)),
                dict(init=[torch.eye(4, device=dev)] * 2), dict(init=torch.eye(4, device=dev).long()), dict(target_normals=dn[:100]),
                dict(target_normals=dn.double()), dict(target_normals=[dn])):
        with pytest.raises(ValueError):
            icp(ds, dp, **bad)
    for bad in (dp.double(), dp[:, :2], dp.reshape(1, -1, 3), dp[:0], dp.cpu()):
        with pytest.raises(ValueError):
            icp(bad, dp)
        with pytest.raises(ValueError):
            icp(ds, bad)
    with pytest.raises(ValueError):
        icp(ds, None)
    with pytest.raises(ValueError):
        icp([ds, ds], [dp])
    with pytest.raises(ValueError):
        apply_transform(ds, torch.eye(3, device=dev))
    poisoned = src[:300].copy()
    poisoned[5, 0] = np.inf
    with pytest.raises(ValueError, match="cloud 1 holds a NaN or an infinite coordinate"):      # found by the launch, raised after it
        icp([ds[:100], torch.from_numpy(poisoned).to(dev)], [dp, dp])
