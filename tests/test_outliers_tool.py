"""tools/upsample.py --clean_input / --clean_output without a GPU: the defaults are off, flag parsing, refusals before any device work."""
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
    spec = importlib.util.spec_from_file_location("upsample_tool_outliers", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_are_off(tool):
    a = tool.parse_args([])
    assert (a.clean_input, a.clean_output) == ("none", "none")
    assert (a.outliers_k, a.outliers_std, a.outliers_radius, a.outliers_min) == (16, 2.0, None, 2)


def test_flags_parse(tool):
    a = tool.parse_args(["--clean_input", "statistical", "--clean_output", "radius", "--outliers_k", "31", "--outliers_std", "1.5",
                         "--outliers_radius", "0.05", "--outliers_min", "4"])
    assert (a.clean_input, a.clean_output, a.outliers_k, a.outliers_std, a.outliers_radius, a.outliers_min) == (
        "statistical", "radius", 31, 1.5, 0.05, 4)
    assert tool.parse_args(["--clean_output", "statistical"]).outliers_radius is None       # statistical needs no radius
    assert tool.parse_args(["--clean_input", "none", "--clean_output", "none"]).clean_input == "none"


@pytest.mark.parametrize("argv", [
    ["--clean_input", "radius"],                                           # radius without --outliers_radius
    ["--clean_output", "radius"],
    ["--clean_output", "radius", "--outliers_radius", "0"],
    ["--clean_output", "radius", "--outliers_radius", "-1"],
    ["--clean_output", "radius", "--outliers_radius", "nan"],
    ["--clean_output", "radius", "--outliers_radius", "0.1", "--outliers_min", "0"],
    ["--clean_input", "statistical", "--outliers_k", "0"],
    ["--clean_input", "statistical", "--outliers_k", "32"],
    ["--clean_input", "statistical", "--outliers_std", "inf"],
    ["--clean_input", "statistical", "--outliers_std", "nan"],
    ["--clean_input", "median"],
    ["--clean_output", "yes"],
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
    for flag in ("--clean_input", "--clean_output", "--outliers_k", "--outliers_std", "--outliers_radius", "--outliers_min"):
        assert flag in out


def test_filters_refuse_bad_input_before_any_launch():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import outliers as M
    for fn, kw in ((M.knn_mean_distance, {}), (M.remove_statistical_outliers, {}), (M.radius_neighbor_count, dict(radius=0.1)),
                   (M.remove_radius_outliers, dict(radius=0.1))):
        with pytest.raises(ValueError, match="ROCm device"):
            fn(torch.zeros(8, 3), **kw)
        with pytest.raises(ValueError, match="ROCm device or a list"):
            fn(np.zeros((8, 3), np.float32), **kw)
        with pytest.raises(ValueError, match="at least one cloud"):
            fn([], **kw)
