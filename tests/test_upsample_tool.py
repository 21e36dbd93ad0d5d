"""CPU side of ragged upsampling: tools/upsample.py's grouping, naming and input checks, and upsample_ragged's refusals, which
fire before anything touches a device (the generator here is None)."""
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
    spec = importlib.util.spec_from_file_location("upsample_tool", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_grouping_keeps_order_and_never_splits(tool):
    rng = np.random.default_rng(0)
    for budget in [1, 100, 1000, 2500, 10 ** 9]:
        sizes = [int(s) for s in rng.integers(1, 2000, 40)]
        groups = tool.group_by_budget(sizes, budget)
        assert [i for g in groups for i in g] == list(range(len(sizes)))
        for g in groups:
            assert g and (len(g) == 1 or sum(sizes[i] for i in g) <= budget)
    assert tool.group_by_budget([5, 5, 5], 10) == [[0, 1], [2]]
    assert tool.group_by_budget([20, 5, 5], 10) == [[0], [1, 2]]
    assert tool.group_by_budget([], 10) == []


def test_output_naming(tool):
    assert tool.output_name("/data/test/camel.xyz", 4) == "camel_X4.xyz"
    assert tool.output_name("chair.v2.xyz", 16) == "chair.v2_X16.xyz"


def test_other_file_types_refused(tool, tmp_path):
    with pytest.raises(ValueError, match=r"bunny\.ply"):
        tool.refuse_unsupported(["a.xyz", "bunny.ply"])
    with pytest.raises(ValueError, match=r"\.pcd"):
        tool.refuse_unsupported(["scan.pcd"])
    tool.refuse_unsupported(["a.xyz", "b.XYZ"])
    (tmp_path / "bunny.ply").write_text("ply\n")
    r = subprocess.run([sys.executable, TOOL, "--test_data", str(tmp_path / "*.ply"), "--log_dir", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and b"only .xyz" in r.stdout


def test_load_xyz_takes_three_columns(tool, tmp_path):
    pts = np.arange(24, dtype=np.float64).reshape(4, 6) / 7
    np.savetxt(str(tmp_path / "n.xyz"), pts)
    got = tool.load_xyz(str(tmp_path / "n.xyz"))
    assert got.dtype == np.float32 and np.array_equal(got, pts.astype(np.float32)[:, :3])


def test_help_without_gpu():
    r = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"--log_dir" in r.stdout and b"--max-points" in r.stdout


def test_upsample_ragged_refuses_bad_input_before_any_launch():
    sys.path.insert(0, ROOT)
    import dispu_amd  # noqa: F401
    from dispu_amd import upsample as U
    ok = np.zeros((300, 3), np.float32)
    with pytest.raises(ValueError, match="at least one cloud"):
        U.upsample_ragged(None, [])
    with pytest.raises(ValueError, match="cloud 1"):
        U.upsample_ragged(None, [ok, np.zeros((300, 2), np.float32)])
    with pytest.raises(ValueError, match="cloud 2"):
        U.upsample_ragged(None, [ok, ok, np.zeros((2, 300, 3), np.float32)])
    with pytest.raises(ValueError, match="cloud 1 has 255 points"):
        U.upsample_ragged(None, [ok, np.zeros((255, 3), np.float32)])
    with pytest.raises(ValueError, match="cloud 0 has 100 points"):
        U.upsample_ragged(None, [np.zeros((100, 3), np.float32)], patch_num_point=128)


def test_segment_offsets():
    sys.path.insert(0, ROOT)
    import dispu_amd  # noqa: F401
    from dispu_amd import upsample as U
    off = U.segment_offsets([3, 1, 4])
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 4, 8]
    with pytest.raises(ValueError, match="2\\^31"):
        U.segment_offsets([2 ** 30, 2 ** 30])
