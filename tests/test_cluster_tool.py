"""tools/upsample.py --keep_clusters without a GPU: the default is off, flag parsing, refusals before any device work."""
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "upsample.py")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("upsample_tool_clusters", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_is_off_and_the_default_command_line_is_untouched(tool):
    a = tool.parse_args([])
    assert (a.keep_clusters, a.cluster_eps, a.cluster_min_points, a.cluster_min_size) == (0, None, 1, 1)
    assert (a.clean_input, a.clean_output, a.denoise_input, a.grid_size) == ("none", "none", 0, None)
    assert tool.parse_args(["--cluster_eps", "0.1"]).keep_clusters == 0          # a radius alone switches nothing on


def test_flags_parse(tool):
    a = tool.parse_args(["--keep_clusters", "2", "--cluster_eps", "0.05", "--cluster_min_points", "10", "--cluster_min_size", "500"])
    assert (a.keep_clusters, a.cluster_eps, a.cluster_min_points, a.cluster_min_size) == (2, 0.05, 10, 500)
    a = tool.parse_args(["--keep_clusters", "32", "--cluster_eps", "1e-3", "--clean_input", "statistical", "--denoise_input", "2"])
    assert (a.keep_clusters, a.cluster_eps, a.clean_input, a.denoise_input) == (32, 1e-3, "statistical", 2)
    assert tool.parse_args(["--keep_clusters", "0"]).cluster_eps is None         # off needs no radius


@pytest.mark.parametrize("argv", [
    ["--keep_clusters", "1"],                                                    # without --cluster_eps
    ["--keep_clusters", "1", "--cluster_eps", "0"],
    ["--keep_clusters", "1", "--cluster_eps", "-0.1"],
    ["--keep_clusters", "1", "--cluster_eps", "nan"],
    ["--keep_clusters", "1", "--cluster_eps", "inf"],
    ["--keep_clusters", "-1", "--cluster_eps", "0.1"],
    ["--keep_clusters", "33", "--cluster_eps", "0.1"],
    ["--keep_clusters", "one", "--cluster_eps", "0.1"],
    ["--keep_clusters", "1", "--cluster_eps", "0.1", "--cluster_min_points", "0"],
    ["--keep_clusters", "1", "--cluster_eps", "0.1", "--cluster_min_size", "0"],
])
def test_illegal_flags_are_refused(tool, argv, capsys):
    with pytest.raises(SystemExit) as e:
        tool.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_help_names_the_new_flags():
    r = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0
    for flag in ("--keep_clusters", "--cluster_eps", "--cluster_min_points", "--cluster_min_size"):
        assert flag in out
