"""tools/upsample.py --mesh, mesh.save_off and dispu_amd.reconstruct's refusals without a GPU: the default is off, flag parsing, refusals
before any device work, an OFF file that load_off reads back to the same arrays; and one GPU run of the tool whose .off equals the
library call on the cloud the tool wrote."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOL = os.path.join(ROOT, "tools", "upsample.py")
sys.path.insert(0, HERE)
ORIENTED = ["--normals", "pca", "--orient", "consistent"]


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("upsample_tool_mesh", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_is_off(tool):
    a = tool.parse_args([])
    assert (a.mesh, a.mesh_voxel, a.mesh_k, a.mesh_support, a.mesh_band) == ("none", None, 8, 1.5, 1)


def test_flags_parse(tool):
    a = tool.parse_args(ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.05", "--mesh_k", "16", "--mesh_support", "2", "--mesh_band", "2"])
    assert (a.mesh, a.mesh_voxel, a.mesh_k, a.mesh_support, a.mesh_band) == ("off", 0.05, 16, 2.0, 2)
    a = tool.parse_args(["--normals", "pca", "--orient", "centroid", "--mesh", "off", "--mesh_voxel", "1"])
    assert (a.mesh, a.mesh_voxel, a.mesh_k) == ("off", 1.0, 8)


@pytest.mark.parametrize("argv", [
    ["--mesh", "off", "--mesh_voxel", "0.1"],                                   # no normals
    ["--mesh", "off", "--mesh_voxel", "0.1", "--normals", "pca"],               # normals without an orientation
    ORIENTED + ["--mesh", "off"],                                              # no voxel size: there is no automatic one
    ORIENTED + ["--mesh", "ply", "--mesh_voxel", "0.1"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "-1"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "nan"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "inf"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.1", "--mesh_k", "0"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.1", "--mesh_k", "33"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.1", "--mesh_support", "0.5"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.1", "--mesh_support", "nan"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.1", "--mesh_band", "0"],
    ORIENTED + ["--mesh", "off", "--mesh_voxel", "0.1", "--mesh_band", "4"],
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
    for flag in ("--mesh", "--mesh_voxel", "--mesh_k", "--mesh_support", "--mesh_band"):
        assert flag in out


def test_save_off_round_trips(tmp_path):
    import dispu_amd  # noqa: F401
    from dispu_amd import mesh as M
    import reconstruct_oracle as R
    r = R.case_result("far_ellipsoid")                          # coordinates that need all nine digits
    path = str(tmp_path / "m.off")
    M.save_off(path, r["verts"], r["faces"])
    v, f = M.load_off(path)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert v.tobytes() == r["verts"].tobytes() and np.array_equal(f, r["faces"])
    tiny = np.float32([[1e-38, -3.4e38, 1.17549435e-38], [0, -0.0, 1 / 3], [7, 8, 9]])
    M.save_off(path, tiny, np.int64([[0, 1, 2]]))
    v, f = M.load_off(path)
    assert np.array_equal(v, tiny) and f.tolist() == [[0, 1, 2]]
    M.save_off(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))                  # an empty mesh is a legal file
    v, f = M.load_off(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    for bad_v, bad_f in ((tiny[:, :2], [[0, 1, 2]]), (tiny, [[0, 1, 3]]), (tiny, [[0, 1]]), (tiny, np.float32([[0, 1, 2]]))):
        with pytest.raises(ValueError):
            M.save_off(path, bad_v, np.asarray(bad_f))


def test_refusals_before_any_launch():
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import reconstruct as RC
    p = torch.zeros(8, 3)
    with pytest.raises(ValueError, match="ROCm device"):
        RC.reconstruct_surface(p, p, 0.1)
    with pytest.raises(ValueError, match="ROCm device"):
        RC.signed_distance(p, p, p)
    with pytest.raises(ValueError, match="points must be one too"):
        RC.signed_distance(p, [p], [p])
    with pytest.raises(ValueError, match="at least one cloud"):
        RC.signed_distance([], [], [])
    with pytest.raises(ValueError, match="2 query clouds but 1 reference clouds"):
        RC.signed_distance([p, p], [p], [p])
    with pytest.raises(ValueError):
        RC.reconstruct_surface(np.zeros((8, 3), np.float32), p, 0.1)
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True, 1e-60):
        with pytest.raises(ValueError, match="voxel"):
            RC.check_voxel(bad)
    assert RC.check_voxel(0.1) == float(np.float32(0.1)) and RC.check_voxel(2) == 2.0


@pytest.mark.gpu
def test_the_tool_writes_the_mesh_of_the_cloud_it_wrote(dev, tmp_path):
    import torch
    from dispu_amd import checkpoint as CK
    from dispu_amd import mesh as M
    from dispu_amd.reconstruct import reconstruct_surface
    from oracle import generator as OG
    import normals_oracle as NO
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    np.savetxt(str(data / "test" / "ball.xyz"), NO.sphere(2048, seed=9), fmt="%.6f")
    cmd = [sys.executable, TOOL, "--log_dir", str(log_dir), "--data_dir", str(data)] + ORIENTED
    runs = {"plain": [], "mesh": ["--mesh", "off", "--mesh_voxel", "0.15", "--mesh_band", "2", "--mesh_k", "16"]}
    procs = {name: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / name)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for name, extra in runs.items()}
    for name, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["ball_X4.xyz"]       # without the flag: the same files, the same bytes
    assert sorted(os.listdir(str(tmp_path / "mesh"))) == ["ball_X4.off", "ball_X4.xyz"]
    assert open(str(tmp_path / "plain" / "ball_X4.xyz"), "rb").read() == open(str(tmp_path / "mesh" / "ball_X4.xyz"), "rb").read()
    v, f = M.load_off(str(tmp_path / "mesh" / "ball_X4.off"))
    rows = np.loadtxt(str(tmp_path / "mesh" / "ball_X4.xyz"), ndmin=2).astype(np.float32)
    assert rows.shape == (4 * 2048, 6)
    lv, lf = reconstruct_surface(torch.from_numpy(np.ascontiguousarray(rows[:, :3])).to(dev), torch.from_numpy(np.ascontiguousarray(rows[:, 3:])).to(dev),
                                 0.15, k=16, band=2)
    assert len(f) > 0 and v.tobytes() == lv.cpu().numpy().tobytes() and np.array_equal(f, lf.cpu().numpy())
