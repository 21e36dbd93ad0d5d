"""GPU tests of dispu_orient_consistent_segments / dispu_amd.normals.orient_consistent (csrc/orient_consistent.hip) against
tests/orient_oracle.py.  Every result is an integer or a sign bit: all comparisons are array_equal, none has a tolerance.  The largest
cloud from a neighbour search has 20 000 points, the deep chains (lists built without a search) up to 274 628; an oracle run is shared
through lru_cache (orient_oracle.expected)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import normals_oracle as NO  # noqa: E402
import orient_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue


def N(t):
    return t.detach().cpu().numpy()


def run_abi(dev, cases, k, vote=0, flags=0, want=("flip", "component", "ncomp"), off=None, scratch="ok", C_arg=None, alias=False,
            drop=None, scratch_buf=None):
    """the C entry on a packed batch of (points, normals, neighbours) triples, every output pre-filled with a sentinel
    -> dict(rc, normal, flip, component, ncomp, status).  scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(),
    .nbytes) in place of the zero-filled one"""
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    pts = torch.from_numpy(np.concatenate([c[0] for c in cases]).astype(np.float32)).to(dev)
    nrm = torch.from_numpy(np.concatenate([c[1] for c in cases]).astype(np.float32)).to(dev)
    nbr = torch.from_numpy(np.concatenate([c[2] for c in cases]).astype(np.int32)).to(dev)
    good = np.zeros(len(cases) + 1, np.int32)
    np.cumsum([len(c[0]) for c in cases], out=good[1:])
    off = good if off is None else np.ascontiguousarray(off, np.int32)
    nC = len(off) - 1 if C_arg is None else C_arg
    total = pts.shape[0]
    hp = C.c_void_p(off.ctypes.data)
    full = L.dispu_orient_consistent_scratch_bytes(len(cases), C.c_void_p(good.ctypes.data), 32)   # what legal arguments need, at most
    assert full > 0
    buf = torch.zeros((full + 16,), dtype=torch.uint8, device=dev)
    if scratch == "ok":
        sp, sb = _lib.ptr(buf), full
    elif scratch == "null":
        sp, sb = C.c_void_p(0), full
    elif scratch == "odd":                                      # not 16-byte aligned
        sp, sb = C.c_void_p(buf.data_ptr() + 4), full
    else:                                                       # one byte short of what this call needs
        sp, sb = _lib.ptr(buf), L.dispu_orient_consistent_scratch_bytes(len(cases), C.c_void_p(good.ctypes.data), k) - 1
    if scratch_buf is not None:
        assert scratch in ("ok", "short"), "with scratch_buf only a right or a one-byte-short size can be asked for"
        sp, sb = scratch_buf.ptr(), scratch_buf.nbytes - (0 if scratch == "ok" else 1)
    out = torch.full((total, 3), 7.0, dtype=torch.float32, device=dev)
    flip = torch.full((total,), 9, dtype=torch.uint8, device=dev) if "flip" in want else None
    comp = torch.full((total,), -7, dtype=torch.int32, device=dev) if "component" in want else None
    ncomp = torch.full((len(cases),), -7, dtype=torch.int32, device=dev) if "ncomp" in want else None
    status = torch.full((len(cases),), -7, dtype=torch.int32, device=dev)
    d_off = torch.from_numpy(off).to(dev)
    args = dict(points=_lib.ptr(pts), normal_in=_lib.ptr(nrm), neighbors=_lib.ptr(nbr), normal_out=_lib.ptr(nrm if alias else out),
                status=_lib.ptr(status), off=_lib.ptr(d_off))
    if drop:
        args[drop] = C.c_void_p(0)
    rc = L.dispu_orient_consistent_segments(nC, args["off"], hp, k, args["points"], args["normal_in"], args["neighbors"], vote, flags,
                                            args["normal_out"], _lib.ptr(flip), _lib.ptr(comp), _lib.ptr(ncomp), args["status"], sp, sb,
                                            None, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    if scratch_buf is not None:
        scratch_buf.inputs = dict(points=N(pts), normal_in=N(nrm), neighbors=N(nbr), off=N(d_off))   # as the call left them
    return dict(rc=rc, normal=N(out), flip=None if flip is None else N(flip), component=None if comp is None else N(comp),
                ncomp=None if ncomp is None else N(ncomp), status=N(status), normal_in=N(nrm))


def assert_equals_oracle(res, lo, hi, c, want):
    assert np.array_equal(res["flip"][lo:hi], want["flip"])
    assert np.array_equal(res["component"][lo:hi], want["component"])
    assert res["ncomp"][c] == want["n_components"]
    assert np.array_equal(res["normal"][lo:hi].view(np.uint32), want["normal"].view(np.uint32))


def check_case(dev, name, vote=0, **kw):
    p, nrm, nbr = O.case(name)
    res = run_abi(dev, [(p, nrm, nbr)], nbr.shape[1], vote=vote, **kw)
    assert res["rc"] == 0 and res["status"][0] == 0, (name, res["rc"], res["status"])
    assert_equals_oracle(res, 0, len(p), 0, O.expected(name, vote))
    return res


@pytest.mark.parametrize("k", O.SMALL_K)
def test_every_small_size(dev, k):
    """n < k: rows padded with -1; n = 1: no edge at all; 63 / 64 / 65: around one wave; 257: above one workgroup"""
    for n in O.SMALL_N:
        check_case(dev, "small_n%d_k%d" % (n, k))


@pytest.mark.parametrize("vote", [0, 1])
@pytest.mark.parametrize("name", ["lattice_plane", "coincident", "zero_normals", "clusters", "helix", "sheet"])
def test_against_the_oracle(dev, name, vote):
    """lattice_plane: every weight ties at 0, (lo, hi) alone decides; coincident: 300 equal points, lists full of duplicates of one place;
    zero_normals: one normal in ten is (0, 0, 0); clusters: 40 components; helix: nearly a path, the deepest trees and the most rounds;
    sheet: 20 000 points, above one workgroup and 2^14, lists with -1 in any column"""
    res = check_case(dev, name, vote)
    if name == "clusters":
        assert res["ncomp"][0] == 40
    if name == "lattice_plane" and vote == 0:
        assert np.array_equal(res["normal"], np.tile(np.float32([0, 0, 1]), (576, 1)))


def test_rounds_ended_by_read_back_give_the_same(dev):
    from dispu_amd import _lib
    for name in ("helix", "clusters"):
        check_case(dev, name, 0, flags=_lib.ORIENT_HOST_ROUNDS)


@pytest.mark.parametrize("name", O.DEEP)
def test_deep_hook_trees(dev, name):
    """one chain of 65 to 274627 links after round one: in the synchronous model (tests/test_orient_oracle.py) launches 2, 3 and 4 of
    the pointer jump work and hand their flag on; 66 points are the last a single launch flattens.  The real launches race and may end
    sooner, so only results are asserted: with the rounds ended on the device and by read-back, twice each.  rising: the chain hooks
    towards the higher index, against the order of the workgroups."""
    from dispu_amd import _lib
    for flags in (0, _lib.ORIENT_HOST_ROUNDS):
        for _ in range(2):
            check_case(dev, name, 0, flags=flags)


def test_outputs_that_are_not_asked_for(dev):
    p, nrm, nbr = O.case("zero_normals")
    res = run_abi(dev, [(p, nrm, nbr)], 8, want=())
    assert res["rc"] == 0 and res["status"][0] == 0 and res["flip"] is None
    assert np.array_equal(res["normal"].view(np.uint32), O.expected("zero_normals")["normal"].view(np.uint32))
    only = run_abi(dev, [(p, nrm, nbr)], 8, want=("component",))
    assert only["rc"] == 0 and np.array_equal(only["component"], O.expected("zero_normals")["component"])


RAGGED = ("small_n1_k16", "coincident", "small_n65_k16", "small_n3_k16", "small_n257_k16")


def test_ragged_batch_equals_each_cloud_alone(dev):
    cases = [O.case(n) for n in RAGGED]
    for vote in (0, 1):
        res = run_abi(dev, cases, 16, vote=vote)
        assert res["rc"] == 0 and not res["status"].any()
        lo = 0
        for c, name in enumerate(RAGGED):
            hi = lo + len(cases[c][0])
            assert_equals_oracle(res, lo, hi, c, O.expected(name, vote))
            lo = hi


def test_two_calls_give_identical_bytes(dev):
    cases = [O.case("helix"), O.case("clusters")]
    cases[1] = (cases[1][0], cases[1][1], np.concatenate([cases[1][2], np.full((1200, 4), -1, np.int32)], axis=1)[:, [0, 8, 1, 2]])
    a, b = run_abi(dev, cases, 4, vote=1), run_abi(dev, cases, 4, vote=1)
    assert a["rc"] == 0 and b["rc"] == 0
    for key in ("normal", "flip", "component", "ncomp", "status"):
        assert a[key].tobytes() == b[key].tobytes()


@pytest.mark.parametrize("what", ["nan", "inf", "index_high", "index_low"])
def test_bad_input_flags_its_cloud_and_leaves_the_others_exact(dev, what):
    import torch
    from dispu_amd.normals import orient_consistent
    names = ("small_n65_k16", "coincident", "small_n257_k16")
    cases = [tuple(np.array(a) for a in O.case(n)) for n in names]
    if what == "nan":
        cases[1][1][77, 1] = np.nan
    elif what == "inf":
        cases[1][1][599, 0] = -np.inf
    elif what == "index_high":
        cases[1][2][5, 3] = 600                                  # n_c itself: the first row of the next cloud in the packed batch
    else:
        cases[1][2][0, 0] = -2
    res = run_abi(dev, cases, 16)
    assert res["rc"] == 0 and list(res["status"]) == [0, 1 if what in ("nan", "inf") else 2, 0]
    assert (res["normal"][65:665] == 7).all() and (res["flip"][65:665] == 9).all() and (res["component"][65:665] == -7).all()
    assert res["ncomp"][1] == -7                                 # none of its outputs is written
    assert_equals_oracle(res, 0, 65, 0, O.expected(names[0]))
    assert_equals_oracle(res, 665, 922, 2, O.expected(names[2]))
    text = "cloud 1 holds a NaN or an infinite normal" if what in ("nan", "inf") else "cloud 1 holds a neighbour index outside"
    with pytest.raises(ValueError, match=text):
        pts, nrm, nbr = [[torch.from_numpy(c[j]).to(dev) for c in cases] for j in range(3)]
        orient_consistent(pts, nrm, k=16, neighbors=nbr)


def untouched(res):
    return ((res["normal"] == 7).all() and (res["flip"] == 9).all() and (res["component"] == -7).all() and (res["ncomp"] == -7).all()
            and (res["status"] == -7).all() and np.array_equal(res["normal_in"].view(np.uint32),
                                                               np.concatenate([O.case(n)[1] for n in RAGGED[1:3]]).view(np.uint32)))


def test_abi_refusals_touch_nothing(dev):
    cases = [O.case(n) for n in RAGGED[1:3]]                    # 600 + 65 points at k = 16
    for kw in (dict(k=3), dict(k=33), dict(scratch="null"), dict(scratch="short"), dict(scratch="odd"), dict(C_arg=65536), dict(C_arg=0),
               dict(off=np.int32([0, 600, 500])), dict(off=np.int32([0, 600, 600])), dict(off=np.int32([1, 600, 665])),
               dict(vote=2), dict(vote=-1), dict(flags=2), dict(alias=True), dict(drop="points"), dict(drop="normal_in"),
               dict(drop="neighbors"), dict(drop="normal_out"), dict(drop="status"), dict(drop="off")):
        res = run_abi(dev, cases, **dict(dict(k=16), **kw))
        assert res["rc"] == INVALID and untouched(res), kw
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L = _lib.lib()
    off = np.int32([0, 600, 665])
    hp = C.c_void_p(off.ctypes.data)
    assert L.dispu_orient_consistent_scratch_bytes(2, hp, 16) > 0
    assert L.dispu_orient_consistent_scratch_bytes(2, hp, 3) == 0 and L.dispu_orient_consistent_scratch_bytes(2, hp, 33) == 0
    assert L.dispu_orient_consistent_scratch_bytes(0, hp, 16) == 0 and L.dispu_orient_consistent_scratch_bytes(65536, hp, 16) == 0
    assert L.dispu_orient_consistent_scratch_bytes(2, None, 16) == 0
    big = np.int32([0, (1 << 24) + 1])
    assert L.dispu_orient_consistent_scratch_bytes(1, C.c_void_p(big.ctypes.data), 16) == 0      # a segment above 2^24 points
    many = (np.arange(9, dtype=np.int64) * (1 << 24)).astype(np.int32)
    assert L.dispu_orient_consistent_scratch_bytes(8, C.c_void_p(many.ctypes.data), 16) == 0     # 2^27 points at k = 16: 2^31 slots
    assert L.dispu_orient_consistent_scratch_bytes(7, C.c_void_p(many.ctypes.data), 16) > 0
    assert run_abi(dev, cases, 16)["rc"] == 0                                                   # the same call, legal


def test_pca_normals_still_refuses_mode_3(dev):
    import torch
    from dispu_amd import _lib
    L = _lib.lib()
    p = torch.from_numpy(NO.sphere(100)).to(dev)
    off = np.int32([0, 100])
    hp = C.c_void_p(off.ctypes.data)
    nb = L.dispu_pca_normals_scratch_bytes(1, hp, 8)
    scratch = torch.zeros((nb,), dtype=torch.uint8, device=dev)
    out = torch.full((100, 3), 7.0, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = L.dispu_pca_normals_segments(1, _lib.ptr(torch.from_numpy(off).to(dev)), hp, 8, _lib.ptr(p), 3, _lib.ptr(p), _lib.ptr(out), None, None,
                                      _lib.ptr(status), _lib.ptr(scratch), nb, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == INVALID and (N(out) == 7).all() and N(status)[0] == -7


def test_python_entry_shapes_and_refusals(dev):
    import torch
    from dispu_amd.normals import estimate_normals, orient_consistent
    p, nrm, nbr = (torch.from_numpy(a).to(dev) for a in O.case("clusters"))
    want0, want1 = O.expected("clusters", 0), O.expected("clusters", 1)
    out = orient_consistent(p, nrm, k=8, neighbors=nbr)
    assert isinstance(out, torch.Tensor) and out.shape == (1200, 3) and np.array_equal(N(out).view(np.uint32), want0["normal"].view(np.uint32))
    out, flip, comp, ncomp = orient_consistent(p, nrm, k=8, neighbors=nbr, vote="majority", return_flips=True, return_components=True)
    assert flip.dtype == torch.uint8 and comp.dtype == torch.int32 and ncomp == 40
    assert np.array_equal(N(flip), want1["flip"]) and np.array_equal(N(comp), want1["component"])
    searched = orient_consistent(p, nrm, k=8)                   # neighbors=None: the lists of the exact search, which the case holds
    assert np.array_equal(N(searched).view(np.uint32), want0["normal"].view(np.uint32))
    q, qn, qb = (torch.from_numpy(a).to(dev) for a in O.case("small_n3_k4"))
    (l0, l1), (f0, f1), (c0, c1), counts = orient_consistent([p, q], [nrm, qn], k=8, neighbors=[nbr, torch.cat([qb, qb], dim=1)],
                                                              return_flips=True, return_components=True)
    assert np.array_equal(N(l0).view(np.uint32), want0["normal"].view(np.uint32)) and counts == [40, 1]
    assert np.array_equal(N(f1), O.expected("small_n3_k4")["flip"]) and not N(c1).any()
    for bad in (dict(k=3), dict(k=33), dict(k=8.0), dict(vote="mst"), dict(vote=0), dict(neighbors=nbr[:, :7]), dict(neighbors=nbr.long()),
                dict(neighbors=nbr.cpu()), dict(neighbors=[nbr]), dict(neighbors=nbr[:100])):
        with pytest.raises(ValueError):
            orient_consistent(p, nrm, **dict(dict(k=8, neighbors=nbr), **bad))
    for bad_p, bad_n in ((p, nrm[:5]), (p, nrm.double()), (p.cpu(), nrm), (p, [nrm]), ([p], nrm), (p[:0], nrm[:0]), (p[:, :2], nrm)):
        with pytest.raises(ValueError):
            orient_consistent(bad_p, bad_n, k=8)
    for bad in (("consistent", ("consistent",)), ("consistent", ("mst",)), ("consistent", None), ("consistent", ("centroid",), 1),
                ("consistent", ("centroid", 1)), ("mst",)):
        with pytest.raises(ValueError):
            estimate_normals(p, orient=bad)


def test_estimate_normals_consistent_on_the_torus(dev):
    """the use the feature is for: a bare x y z torus comes out with every normal outwards; 'centroid' alone leaves the inner half
    of the tube inwards, and as a prior the majority vote mends it"""
    import torch
    from dispu_amd.normals import estimate_normals
    p, true = O.torus(2048, seed=2048)
    t = torch.from_numpy(p).to(dev)
    got, idx = estimate_normals(t, k=12, orient=("consistent",), return_neighbors=True)
    assert ((N(got).astype(np.float64) * true).sum(axis=1) > 0).all()
    plain = N(estimate_normals(t, k=12))
    want = O.orient(p, plain, N(idx), vote=0)                    # the oracle on the kernel's own PCA normals and neighbours
    assert np.array_equal(N(got).view(np.uint32), want["normal"].view(np.uint32)) and want["n_components"] == 1
    cen = N(estimate_normals(t, k=12, orient=("centroid",)))
    assert ((cen.astype(np.float64) * true).sum(axis=1) > 0).mean() < 0.8
    mended = N(estimate_normals(t, k=12, orient=("consistent", ("centroid",))))
    assert ((mended.astype(np.float64) * true).sum(axis=1) > 0).all()
    assert np.array_equal(mended.view(np.uint32), O.orient(p, cen, N(idx), vote=1)["normal"].view(np.uint32))
    both = estimate_normals([t, t[:700]], k=12, orient=("consistent",))
    assert np.array_equal(N(both[0]).view(np.uint32), N(got).view(np.uint32)) and both[1].shape == (700, 3)


def test_upsample_tool_writes_consistent_normals(dev, tmp_path):
    import torch
    from dispu_amd import checkpoint as CK
    from dispu_amd.normals import estimate_normals
    from oracle import generator as OG
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    np.savetxt(str(data / "test" / "ring.xyz"), O.torus(2048, seed=9)[0], fmt="%.6f")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    runs = {"plain": [], "consistent": ["--normals", "pca", "--orient", "consistent", "--normals_k", "12"],
            "prior": ["--normals", "pca", "--orient", "consistent", "--orient_prior", "centroid", "--normals_k", "12"]}
    procs = {name: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for name, extra in runs.items()}
    for name, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    plain = open(str(tmp_path / "plain" / "ring_X4.xyz")).read().splitlines()
    # the tool's own steps in this process: the same checkpoint and input give the same points bit for bit
    from dispu_amd.checkpoint import restore_generator
    from dispu_amd.upsample import upsample_ragged
    _, gen = restore_generator(str(log_dir), device=dev)
    cloud = np.loadtxt(str(data / "test" / "ring.xyz"), ndmin=2).astype(np.float32)
    pred = torch.from_numpy(upsample_ragged(gen, [cloud], 256, 3, 4)[0]).to(dev)
    assert [" ".join("%.6f" % v for v in row) for row in N(pred)] == plain
    for name, orient in (("consistent", ("consistent",)), ("prior", ("consistent", ("centroid",)))):
        rows = open(str(tmp_path / name / "ring_X4.xyz")).read().splitlines()
        assert len(rows) == 4 * 2048 and all(len(r.split(" ")) == 6 for r in rows)
        assert [" ".join(r.split(" ")[:3]) for r in rows] == plain
        want = N(estimate_normals(pred, k=12, orient=orient))
        assert [" ".join(r.split(" ")[3:]) for r in rows] == [" ".join("%.6f" % v for v in row) for row in want]   # the Python call's
