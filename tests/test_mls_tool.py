"""tools/upsample.py --denoise_input / --project_output and dispu_amd.mls.mls_project without a GPU: the defaults are off, flag parsing,
refusals before any device work."""
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
    spec = importlib.util.spec_from_file_location("upsample_tool_mls", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_are_off(tool):
    a = tool.parse_args([])
    assert (a.denoise_input, a.project_output, a.mls_k, a.mls_support) == (0, 0, 16, 1.0)


def test_flags_parse(tool):
    a = tool.parse_args(["--denoise_input", "2", "--project_output", "8", "--mls_k", "32", "--mls_support", "1.5"])
    assert (a.denoise_input, a.project_output, a.mls_k, a.mls_support) == (2, 8, 32, 1.5)
    a = tool.parse_args(["--denoise_input", "0", "--project_output", "1", "--mls_k", "4", "--mls_support", "4"])
    assert (a.denoise_input, a.project_output, a.mls_k, a.mls_support) == (0, 1, 4, 4.0)


@pytest.mark.parametrize("argv", [
    ["--denoise_input", "-1"],
    ["--denoise_input", "9"],
    ["--project_output", "-1"],
    ["--project_output", "9"],
    ["--denoise_input", "1.5"],
    ["--denoise_input", "1", "--mls_k", "3"],
    ["--denoise_input", "1", "--mls_k", "33"],
    ["--project_output", "1", "--mls_support", "0.5"],
    ["--project_output", "1", "--mls_support", "nan"],
    ["--project_output", "1", "--mls_support", "5"],
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
    for flag in ("--denoise_input", "--project_output", "--mls_k", "--mls_support"):
        assert flag in out


def test_mls_project_refuses_bad_input_before_any_launch():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import mls as M
    with pytest.raises(ValueError, match="ROCm device"):
        M.mls_project(torch.zeros(8, 3))
    with pytest.raises(ValueError, match="ROCm device"):
        M.mls_project(torch.zeros(8, 3), torch.zeros(9, 3))
    with pytest.raises(ValueError, match="ROCm device or a list"):
        M.mls_project(np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError, match="at least one cloud"):
        M.mls_project([])
    with pytest.raises(ValueError, match="at least one cloud"):
        M.mls_project([], [])
    with pytest.raises(ValueError, match="2 query clouds but 1 reference clouds"):
        M.mls_project([torch.zeros(8, 3), torch.zeros(8, 3)], [torch.zeros(8, 3)])
    with pytest.raises(ValueError, match="refs must be one too"):
        M.mls_project(torch.zeros(8, 3), [torch.zeros(8, 3)])
