"""tools/register.py and dispu_amd.registration without a GPU: the defaults, flag parsing, refusals before any device work; and one GPU
test that runs the tool end to end on two sources of the cap."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOL = os.path.join(ROOT, "tools", "register.py")
sys.path.insert(0, HERE)
NEED = ["--target", "t.xyz", "--source", "a.xyz", "--out_folder", "out"]


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("register_tool", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults(tool):
    a = tool.parse_args(NEED)
    assert (a.target, a.source, a.out_folder) == ("t.xyz", ["a.xyz"], "out")
    assert (a.method, a.max_distance, a.iterations, a.tolerance, a.init, a.merge) == ("point", float("inf"), 30, 1e-6, None, False)


def test_flags_parse(tool):
    a = tool.parse_args(["--target", "t.xyz", "--source", "a.xyz", "d/b.xyz", "--out_folder", "o", "--method", "plane", "--max_distance", "0.25",
                         "--iterations", "0", "--tolerance", "0", "--init", "M.txt", "--merge"])
    assert a.source == ["a.xyz", "d/b.xyz"] and (a.method, a.max_distance, a.iterations, a.tolerance, a.init, a.merge) == (
        "plane", 0.25, 0, 0.0, "M.txt", True)
    assert tool.parse_args(NEED + ["--iterations", "128", "--max_distance", "inf"]).iterations == 128
    assert tool.stem("/x/y/scan_01.xyz") == "scan_01"


@pytest.mark.parametrize("argv", [
    ["--source", "a.xyz", "--out_folder", "o"],
    ["--target", "t.xyz", "--out_folder", "o"],
    ["--target", "t.xyz", "--source", "a.xyz"],
    NEED + ["--method", "surface"],
    NEED + ["--iterations", "-1"],
    NEED + ["--iterations", "129"],
    NEED + ["--iterations", "1.5"],
    NEED + ["--max_distance", "-1"],
    NEED + ["--max_distance", "nan"],
    NEED + ["--tolerance", "-1e-3"],
    NEED + ["--tolerance", "inf"],
    NEED + ["--tolerance", "nan"],
    ["--target", "t.xyz", "--source", "a.xyz", "d/a.xyz", "--out_folder", "o"],
])
def test_illegal_flags_are_refused(tool, argv, capsys):
    with pytest.raises(SystemExit) as e:
        tool.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_help_names_the_flags():
    r = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0
    for flag in ("--target", "--source", "--out_folder", "--method", "--max_distance", "--iterations", "--tolerance", "--init", "--merge"):
        assert flag in out


def test_files_are_read_as_stated(tool, tmp_path):
    np.savetxt(str(tmp_path / "c.xyz"), np.arange(12.0).reshape(3, 4))          # a fourth column is ignored
    assert np.array_equal(tool.load_xyz(str(tmp_path / "c.xyz")), np.float32([[0, 1, 2], [4, 5, 6], [8, 9, 10]]))
    np.savetxt(str(tmp_path / "M.txt"), np.eye(4), fmt="%.17g")
    assert np.array_equal(tool.load_init(str(tmp_path / "M.txt")), np.eye(4))
    np.savetxt(str(tmp_path / "bad.txt"), np.eye(3))
    with pytest.raises(SystemExit):
        tool.load_init(str(tmp_path / "bad.txt"))
    np.savetxt(str(tmp_path / "two.xyz"), np.zeros((3, 2)))
    with pytest.raises(SystemExit):
        tool.load_xyz(str(tmp_path / "two.xyz"))


def test_icp_refuses_bad_input_before_any_launch():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import registration as R
    assert (R.ITER_MIN, R.ITER_MAX) == (0, 128)
    assert R.Registration._fields == ("transform", "aligned", "fitness", "rmse", "iterations", "converged", "degenerate", "correspondences")
    with pytest.raises(ValueError, match="ROCm device"):
        R.icp(torch.zeros(8, 3), torch.zeros(9, 3))
    with pytest.raises(ValueError, match="needs a target"):
        R.icp(torch.zeros(8, 3), None)
    with pytest.raises(ValueError, match="ROCm device or two lists"):
        R.icp(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError, match="at least one cloud"):
        R.icp([], [])
    with pytest.raises(ValueError, match="2 query clouds but 1 reference clouds"):
        R.icp([torch.zeros(8, 3), torch.zeros(8, 3)], [torch.zeros(8, 3)])
    with pytest.raises(ValueError, match="target must be one too"):
        R.icp(torch.zeros(8, 3), [torch.zeros(8, 3)])
    with pytest.raises(ValueError, match="ROCm device"):
        R.apply_transform(torch.zeros(8, 3), torch.eye(4))


@pytest.mark.gpu
def test_register_tool_end_to_end(dev, tmp_path):
    import icp_oracle as O
    p, _, src, truth = O.cap()
    np.savetxt(str(tmp_path / "target.xyz"), p, fmt="%.9g")
    np.savetxt(str(tmp_path / "a.xyz"), src, fmt="%.9g")
    second = O.apply(O.motion(p[:100]), src[:700])                              # another pose of a part of the same scan
    np.savetxt(str(tmp_path / "b.xyz"), second, fmt="%.9g")
    out = tmp_path / "out"
    cmd = [sys.executable, TOOL, "--target", str(tmp_path / "target.xyz"), "--source", str(tmp_path / "a.xyz"), str(tmp_path / "b.xyz"),
           "--out_folder", str(out), "--method", "plane", "--iterations", "20", "--merge"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    log = r.stdout.decode(errors="replace")
    assert r.returncode == 0, log
    lines = [ln for ln in log.splitlines() if ln.startswith(("a:", "b:"))]
    assert len(lines) == 2 and all("fitness" in ln and "rmse" in ln and "iterations" in ln for ln in lines), log
    assert lines[0].endswith("converged"), log
    for name, cloud in (("a", src), ("b", second)):
        aligned = np.loadtxt(str(out / (name + "_aligned.xyz")), ndmin=2)
        T = np.loadtxt(str(out / (name + "_transform.txt")), ndmin=2)
        assert aligned.shape == (len(cloud), 3) and T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1])
        again = O.apply(T, np.loadtxt(str(tmp_path / (name + ".xyz")), ndmin=2).astype(np.float32))
        assert np.abs(again.astype(np.float64) - aligned).max() <= 0.5000001e-6  # %.17g round-trips T: the files agree to the %.6f printed
    assert np.abs(np.loadtxt(str(out / "a_aligned.xyz"), ndmin=2) - truth).max() <= 3e-6
    merged = np.loadtxt(str(out / "merged.xyz"), ndmin=2)
    assert merged.shape == (len(p) + len(src) + 700, 3)
    assert np.abs(merged[:len(p)] - p).max() <= 0.5000001e-6
