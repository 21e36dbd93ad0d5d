"""tools/upsample.py --normals / --orient without a GPU: flag parsing, the six-column reader and writer, refusals before any device work."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "upsample.py")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("upsample_tool_normals", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_leave_the_output_as_it_was(tool):
    a = tool.parse_args([])
    assert (a.normals, a.normals_k, a.orient, a.viewpoint) == ("none", 16, "none", None)


def test_flags_parse(tool):
    a = tool.parse_args(["--normals", "pca", "--normals_k", "32", "--orient", "viewpoint", "--viewpoint", "1", "-2.5", "3e2"])
    assert (a.normals, a.normals_k, a.orient, a.viewpoint) == ("pca", 32, "viewpoint", [1.0, -2.5, 300.0])
    for orient in ("none", "centroid", "input"):
        assert tool.parse_args(["--normals", "pca", "--orient", orient]).orient == orient


@pytest.mark.parametrize("argv", [
    ["--orient", "centroid"],                                              # an orientation without normals
    ["--viewpoint", "0", "0", "1"],
    ["--normals", "pca", "--orient", "viewpoint"],                        # no viewpoint
    ["--normals", "pca", "--viewpoint", "0", "0", "1"],                   # a viewpoint nobody asked for
    ["--normals", "pca", "--orient", "viewpoint", "--viewpoint", "0", "nan", "1"],
    ["--normals", "pca", "--normals_k", "3"],
    ["--normals", "pca", "--normals_k", "33"],
    ["--normals", "svd"],
    ["--normals", "pca", "--orient", "mst"],
])
def test_illegal_flags_are_refused(tool, argv, capsys):
    with pytest.raises(SystemExit) as e:
        tool.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_six_columns_round_trip(tool, tmp_path):
    r = np.random.RandomState(0)
    pts = (r.standard_normal((50, 3)) * 3).astype(np.float32)
    nrm = r.standard_normal((50, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    path = str(tmp_path / "c.xyz")
    tool.save_xyz_normals(path, pts, nrm)
    rows = open(path).read().splitlines()
    assert len(rows) == 50 and all(len(row.split()) == 6 for row in rows)
    assert rows[0] == " ".join("%.6f" % v for v in list(pts[0]) + list(nrm[0]))
    p2, n2 = tool.load_xyz_normals(path)
    assert p2.dtype == np.float32 and n2.dtype == np.float32 and p2.shape == (50, 3) and n2.shape == (50, 3)
    assert np.abs(p2 - pts).max() <= 5.1e-7 * max(1.0, np.abs(pts).max()) and np.abs(n2 - nrm).max() <= 5.1e-7       # %.6f
    tool.save_xyz_normals(str(tmp_path / "d.xyz"), p2, n2)              # what was read is written back unchanged
    assert open(str(tmp_path / "d.xyz")).read() == open(path).read()
    assert np.array_equal(tool.load_xyz(path), p2)                      # load_xyz still takes three columns
    np.savetxt(str(tmp_path / "e.xyz"), np.concatenate([pts, nrm, np.ones((50, 2), np.float32)], axis=1), fmt="%.6f")
    p3, n3 = tool.load_xyz_normals(str(tmp_path / "e.xyz"))             # further columns are ignored
    assert np.array_equal(p3, p2) and np.array_equal(n3, n2)


def test_reader_refuses_three_columns_by_name(tool, tmp_path):
    path = str(tmp_path / "bare.xyz")
    np.savetxt(path, np.zeros((4, 3)), fmt="%.6f")
    with pytest.raises(ValueError, match="bare.xyz.*six columns.*got 3"):
        tool.load_xyz_normals(path)


def test_orient_input_refuses_a_three_column_file_before_the_gpu(tmp_path):
    np.savetxt(str(tmp_path / "a.xyz"), np.zeros((4, 6)), fmt="%.6f")
    np.savetxt(str(tmp_path / "b.xyz"), np.zeros((4, 3)), fmt="%.6f")
    r = subprocess.run([sys.executable, TOOL, "--test_data", str(tmp_path / "*.xyz"), "--log_dir", str(tmp_path), "--normals", "pca",
                        "--orient", "input"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode != 0 and "b.xyz" in out and "six columns" in out and "ROCm" not in out


def test_help_names_the_new_flags():
    r = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0
    for flag in ("--normals", "--normals_k", "--orient", "--viewpoint"):
        assert flag in out


def test_estimate_normals_refuses_bad_input_before_any_launch():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd.normals import estimate_normals
    with pytest.raises(ValueError, match="ROCm device"):
        estimate_normals(torch.zeros(8, 3))
    with pytest.raises(ValueError, match="ROCm device or a list"):
        estimate_normals(np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError, match="at least one cloud"):
        estimate_normals([])
