"""tools/upsample.py --orient consistent / --orient_prior without a GPU: flag parsing, the rules that follow the prior, refusals before any
device work; and the refusals of normals.orient_consistent that need no launch."""
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
    spec = importlib.util.spec_from_file_location("upsample_tool_orient", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults(tool):
    a = tool.parse_args([])
    assert (a.orient, a.orient_prior, a.hint) == ("none", "none", "none")
    assert tool.parse_args(["--normals", "pca", "--orient", "centroid"]).hint == "centroid"


def test_flags_parse(tool):
    a = tool.parse_args(["--normals", "pca", "--orient", "consistent"])
    assert (a.orient, a.orient_prior, a.hint, a.viewpoint) == ("consistent", "none", "none", None)
    for prior in ("none", "centroid", "input"):
        a = tool.parse_args(["--normals", "pca", "--orient", "consistent", "--orient_prior", prior])
        assert (a.orient, a.orient_prior, a.hint) == ("consistent", prior, prior)
    a = tool.parse_args(["--normals", "pca", "--orient", "consistent", "--orient_prior", "viewpoint", "--viewpoint", "0", "0", "9"])
    assert (a.orient_prior, a.hint, a.viewpoint) == ("viewpoint", "viewpoint", [0.0, 0.0, 9.0])


@pytest.mark.parametrize("argv", [
    ["--normals", "pca", "--orient", "mst"],                                                   # still no such name
    ["--normals", "pca", "--orient", "consistent", "--orient_prior", "mst"],
    ["--normals", "pca", "--orient", "consistent", "--orient_prior", "consistent"],
    ["--orient", "consistent"],                                                                # an orientation without normals
    ["--normals", "pca", "--orient_prior", "centroid"],                                        # a prior without --orient consistent
    ["--normals", "pca", "--orient", "centroid", "--orient_prior", "centroid"],
    ["--normals", "pca", "--orient", "consistent", "--orient_prior", "viewpoint"],             # the prior's rule: no viewpoint
    ["--normals", "pca", "--orient", "consistent", "--viewpoint", "0", "0", "1"],              # a viewpoint nobody asked for
    ["--normals", "pca", "--orient", "consistent", "--orient_prior", "centroid", "--viewpoint", "0", "0", "1"],
    ["--normals", "pca", "--orient", "consistent", "--orient_prior", "input", "--attributes", "idw"],   # columns 4-6 twice
])
def test_illegal_flags_are_refused(tool, argv, capsys):
    with pytest.raises(SystemExit) as e:
        tool.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_prior_input_refuses_a_three_column_file_before_the_gpu(tmp_path):
    np.savetxt(str(tmp_path / "a.xyz"), np.zeros((4, 6)), fmt="%.6f")
    np.savetxt(str(tmp_path / "b.xyz"), np.zeros((4, 3)), fmt="%.6f")
    r = subprocess.run([sys.executable, TOOL, "--test_data", str(tmp_path / "*.xyz"), "--log_dir", str(tmp_path), "--normals", "pca",
                        "--orient", "consistent", "--orient_prior", "input"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode != 0 and "b.xyz" in out and "six columns" in out and "ROCm" not in out


def test_help_names_the_new_flags():
    r = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "--orient_prior" in out and "consistent" in out


def test_orient_consistent_refuses_bad_input_before_any_launch():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd.normals import estimate_normals, orient_consistent
    with pytest.raises(ValueError, match="ROCm device"):
        orient_consistent(torch.zeros(8, 3), torch.zeros(8, 3))
    with pytest.raises(ValueError, match="ROCm device or a list"):
        orient_consistent(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError, match="1 .. 65535 clouds"):
        orient_consistent([], [])
    with pytest.raises(ValueError, match="as points is"):
        orient_consistent([torch.zeros(8, 3)], torch.zeros(8, 3))
    with pytest.raises(ValueError, match="ROCm device"):
        estimate_normals(torch.zeros(8, 3), orient=("consistent",))


def test_abi_table_holds_the_new_entries():
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    assert "dispu_orient_consistent_segments" in _lib.SIGNATURES and "dispu_orient_consistent_scratch_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dispu_orient_consistent_segments"][1]) == 18
    off = np.int32([0, 600, 665])
    L = _lib.lib()
    hp = _lib.C.c_void_p(off.ctypes.data)
    assert L.dispu_orient_consistent_scratch_bytes(2, hp, 16) >= 665 * 40
    assert L.dispu_orient_consistent_scratch_bytes(2, hp, 3) == 0
    assert L.dispu_orient_consistent_segments(2, None, hp, 16, None, None, None, 0, 0, None, None, None, None, None, None, 0, None, None) == 1
