"""CPU side of the mesh sampler: the HDF5 writer, tools/make_dataset.py's argument checks (which fire before the device is touched),
the constants the kernel source mirrors from the header, and a self-check of the yardstick: the parallel-rounds formulation written in
numpy equals the sequential greedy of tests/mesh_sample_oracle.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mesh_sample_oracle as SO  # noqa: E402

TOOL = os.path.join(ROOT, "tools", "make_dataset.py")


def _h5_or_skip():
    from dispu_amd import h5
    try:
        h5.lib()
    except RuntimeError as e:
        pytest.skip(str(e))
    return h5


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64", "uint8"])
def test_h5_write_round_trip(dtype, tmp_path):
    h5 = _h5_or_skip()
    rng = np.random.default_rng(3)
    a = (rng.random((7, 4)) * 200).astype(dtype)
    b = np.arange(5).astype(dtype)
    path = str(tmp_path / "t.h5")
    h5.write(path, {"a": a, "b": b})
    with h5.File(path) as f:
        assert sorted(f.keys()) == ["a", "b"]
        assert f.shape_dtype("a") == ((7, 4), np.dtype(dtype))
        ga, gb = f["a"], f["b"]
    assert ga.dtype == np.dtype(dtype) and np.array_equal(ga, a) and np.array_equal(gb, b)


def test_h5_write_patch_array_and_replace(tmp_path):
    h5 = _h5_or_skip()
    x = np.random.default_rng(0).standard_normal((3, 5, 3)).astype(np.float32)
    path = str(tmp_path / "p.h5")
    h5.write(path, {"old": np.zeros(2, np.int32)})
    h5.write(path, {"poisson_5": x[:, ::-1][:, ::-1], "poisson_2": x[:, :2]})         # a replaced file; a non-contiguous view
    with h5.File(path) as f:
        assert sorted(f.keys()) == ["poisson_2", "poisson_5"]
        assert f["poisson_5"].tobytes() == x.tobytes()
        assert np.array_equal(f["poisson_2"], x[:, :2])
    from dispu_amd import dataset
    inp, gt = dataset.load_patches(path, 2, 5, random=False)
    assert np.array_equal(gt, x) and np.array_equal(inp, x[:, :2])


def test_h5_write_refuses_other_types(tmp_path):
    h5 = _h5_or_skip()
    path = str(tmp_path / "n.h5")
    for bad in (np.zeros(3, np.float16), np.zeros(3, np.complex64), np.float32(1.0), np.zeros(3, ">f4")):
        with pytest.raises(TypeError):
            h5.write(path, {"x": bad})
    assert not os.path.exists(path)


def _run(args):
    return subprocess.run([sys.executable, TOOL] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_tool_refuses_bad_arguments_before_any_device_use(tmp_path):
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    (meshes / "t.off").write_text("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    r = _run(["patches", "--mesh_dir", str(meshes), "--out", str(tmp_path / "o.h5"), "--oversample", "5"])        # k = 5120 > 4096
    assert r.returncode != 0 and b"5120 candidates per patch, at most 4096" in r.stderr
    r = _run(["patches", "--mesh_dir", str(tmp_path / "nowhere"), "--out", str(tmp_path / "o.h5")])
    assert r.returncode != 0 and b"no such directory" in r.stderr
    r = _run(["clouds", "--mesh_dir", str(meshes), "--out_dir", str(tmp_path / "c"), "--num", "0"])
    assert r.returncode != 0 and b"--num must be positive" in r.stderr
    r = _run(["clouds", "--mesh_dir", str(meshes), "--out_dir", str(tmp_path / "c"), "--num", "16384"])           # 65536 candidates
    assert r.returncode != 0 and b"at most 49152 per cloud" in r.stderr
    (tmp_path / "empty").mkdir()
    r = _run(["clouds", "--mesh_dir", str(tmp_path / "empty"), "--out_dir", str(tmp_path / "c"), "--num", "2048"])
    assert r.returncode != 0 and b"no *.off files" in r.stderr
    assert not (tmp_path / "o.h5").exists() and not (tmp_path / "c").exists()


def test_constants_agree():
    """the header and the Python table hold the same limits; the kernel source compiles against the header and holds no copy"""
    from dispu_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dispu_hip.h")).read()
    src = open(os.path.join(ROOT, "dis-pu_amd", "csrc", "poisson_disk.hip")).read()
    for name, val in (("DISPU_POISSON_MAX_N", _lib.POISSON_MAX_N), ("DISPU_POISSON_MAX_ROUNDS", _lib.POISSON_MAX_ROUNDS)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val
        assert not re.search(r"#define %s\b" % name, src) and re.search(r"\b%s\b" % name, src)
    assert _lib.POISSON_MAX_N >= 40960
    tool = open(TOOL).read()
    assert int(re.search(r"KNN_PATCH_MAX_K = (\d+)", tool).group(1)) == _lib.SORT_ROWS_MAX_K == 4096


def test_rounds_formulation_equals_sequential_greedy():
    """2000 points on a plane: the lexicographically first maximal independent set, sequentially and in rounds"""
    rng = np.random.default_rng(11)
    p = np.zeros((2000, 3), np.float32)
    p[:, :2] = rng.random((2000, 2), dtype=np.float32)
    for r in (0.01, 0.03, 0.08, 0.5):
        seq = SO.poisson_keep(p, r)
        par, rounds = SO.rounds_keep(p, r)
        assert np.array_equal(seq, par)
        assert seq[0] and 1 <= rounds <= 2000
        kept = p[seq]
        assert SO.min_pair_d2_f32(kept) >= np.float32(np.float32(r) * np.float32(r)) if len(kept) > 1 else True
    assert SO.poisson_keep(p, 0.0).all() and SO.poisson_keep(p, -1.0).all()
    assert SO.poisson_keep(p, 10.0).sum() == 1


def test_oracle_sampler_is_area_weighted_and_on_the_triangles():
    """the yardstick's own sanity: a zero-area face is never drawn, faces are drawn in proportion to their areas, barycentrics sum to 1"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [1, 1, 0], [0, 3, 0], [3, 3, 0]], np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 4], [1, 5, 2], [2, 6, 7]], np.int32)                 # face 1: three collinear points
    tv = verts[faces].astype(np.float64)
    areas = 0.5 * np.linalg.norm(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]), axis=1)
    assert areas[1] == 0.0
    cum = np.concatenate([[0.0], np.cumsum(areas / areas.sum())])
    pts, face, bary = SO.sample_surface(verts, faces, cum, 3000, seed=5)
    assert not (face == 1).any()
    share = np.bincount(face, minlength=4) / 3000.0
    assert np.abs(share - areas / areas.sum()).max() < 0.03
    assert np.abs(bary.sum(axis=1) - 1.0).max() < 1e-15 and bary.min() >= 0.0
    assert np.abs(pts[:, 2]).max() == 0.0
    a, fa, _ = SO.sample_surface(verts, faces, cum, 100, seed=5)
    assert np.array_equal(a, pts[:100]) and np.array_equal(fa, face[:100])
    b, _, _ = SO.sample_surface(verts, faces, cum, 100, seed=6)
    assert not np.array_equal(a, b)
