"""Ragged batches on the GPU: dispu_fps_segments, dispu_knn_patch_segments and dispu_normalize_segments against the single-cloud
entries bit for bit, upsample_ragged against upsample_cloud stage by stage, and tools/upsample.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import generator as OG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def N(t):
    return t.detach().cpu().numpy()


def _cloud(rng, n, dup=False):
    pc = rng.random((n, 3)).astype(np.float32)
    if n > 10:
        pc[10] = pc[3]                                   # a duplicate: ties go to the reference's rule
    if dup and n > 1:
        h = n // 2
        pc[h:] = pc[:n - h]                              # every point of the first half twice
    return pc


def _pack(clouds, dev):
    return torch.from_numpy(np.concatenate(clouds)).to(dev)


# (n, m, duplicates): every FPS tier in one call -- register kernels (n <= 24576, incl. 4097 / 8193 with m < 64),
# region-skipping kernels (4096 < n <= 24576, m >= 64: whole-wave and four-region variants), the streaming kernel (n > 24576)
FPS_CASES = [(1, 1, False), (64, 64, False), (65, 64, True), (65, 1, False), (300, 300, False), (300, 100, True), (2048, 64, False),
             (2048, 682, True), (4097, 1365, False), (4097, 63, False), (8193, 2731, True), (8193, 64, False), (24576, 8192, False),
             (24576, 1, False), (30000, 64, True), (30000, 3, False)]


@pytest.mark.parametrize("arith", [0, 1])
def test_fps_segments_equal_per_cloud(dev, arith):
    from dispu_amd import upsample as U
    from dispu_amd.tf_sampling import farthest_point_sample
    rng = np.random.default_rng(11 + arith)
    clouds = [_cloud(rng, n, d) for n, _, d in FPS_CASES]
    ms = [m for _, m, _ in FPS_CASES]
    off, moff = U.segment_offsets([c.shape[0] for c in clouds]), U.segment_offsets(ms)
    got = N(U.fps_segments(_pack(clouds, dev), off, moff, arith=arith))
    for c, (pc, m) in enumerate(zip(clouds, ms)):
        ref = N(farthest_point_sample(m, torch.from_numpy(pc[None]).to(dev), arith=arith))[0]
        assert np.array_equal(got[moff[c]:moff[c + 1]], ref), (pc.shape[0], m)
    # one segment alone, in each family
    for n, m in [(300, 100), (8193, 2731), (30000, 5)]:
        pc = _cloud(rng, n, True)
        got = N(U.fps_segments(_pack([pc], dev), U.segment_offsets([n]), U.segment_offsets([m]), arith=arith))
        ref = N(farthest_point_sample(m, torch.from_numpy(pc[None]).to(dev), arith=arith))[0]
        assert np.array_equal(got, ref), (n, m)


@pytest.mark.parametrize("k,sizes", [(256, [300, 1000, 2048, 8192, 10000, 256]), (300, [300, 1000, 9000]), (4096, [4096, 10000, 5000])])
def test_knn_patch_segments_equal_per_cloud(dev, k, sizes):
    from dispu_amd import upsample as U
    rng = np.random.default_rng(k)
    clouds = [_cloud(rng, n, dup=(i % 2 == 1)) for i, n in enumerate(sizes)]
    qs = [pc[rng.choice(pc.shape[0], 1 + i % 4, replace=False)] for i, pc in enumerate(clouds)]
    off, qoff = U.segment_offsets(sizes), U.segment_offsets([q.shape[0] for q in qs])
    got = N(U.knn_patch_segments(_pack(clouds, dev), off, _pack(qs, dev), qoff, k))
    assert got.shape == (qoff[-1], k)
    for c, (pc, q) in enumerate(zip(clouds, qs)):
        ref = N(U.knn_patch(torch.from_numpy(pc[None]).to(dev), torch.from_numpy(q[None]).to(dev), k))[0]
        assert np.array_equal(got[qoff[c]:qoff[c + 1]], ref), (pc.shape[0], k)


def test_normalize_segments_equal_per_cloud(dev):
    from dispu_amd import upsample as U
    rng = np.random.default_rng(5)
    sizes = [1, 2, 300, 2048, 5000, 300]
    clouds = [(rng.standard_normal((n, 3)) * rng.uniform(0.1, 10) + rng.uniform(-5, 5, 3)).astype(np.float32) for n in sizes]
    clouds[1][1] = clouds[1][0] + 1.0
    off = U.segment_offsets(sizes)
    out, cen, fur = (N(t) for t in U.normalize_segments(_pack(clouds, dev), off))
    for c, pc in enumerate(clouds):
        o, ce, fu = (N(t) for t in U.normalize_patches(torch.from_numpy(pc[None]).to(dev)))
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)          # the one-point cloud is 0 / 0: NaN, compared by its bits
        assert np.array_equal(bits(out[off[c]:off[c + 1]]), bits(o[0])), c
        assert np.array_equal(bits(cen[c]), bits(ce[0])) and np.array_equal(bits(fur[c]), bits(fu[0])), c


def _sphere_clouds(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        g = rng.standard_normal((n, 3))
        out.append((g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, 3) + rng.uniform(-2, 2, 3)).astype(np.float32))
    return out


def _check_ragged(gen, clouds, **kw):
    from dispu_amd import upsample as U
    outs, st = U.upsample_ragged(gen, clouds, return_stages=True, **kw)
    assert len(outs) == len(clouds)
    rows = dict(cloud_n="off", seeds="seed_off", pidx="seed_off", patches_n="seed_off", fine="seed_off", merged="merged_off",
                sel="out_off")
    for c, pc in enumerate(clouds):
        ref, rst = U.upsample_cloud(gen, pc, return_stages=True, **kw)
        assert outs[c].dtype == np.float32 and outs[c].shape == (int(pc.shape[0] * kw.get("final_ratio", 4)), 3)
        assert np.array_equal(outs[c], ref), c
        for name, o in rows.items():
            off = st[o]
            got = N(st[name][off[c]:off[c + 1]])
            want = N(rst[name])
            want = want.reshape(got.shape) if name in ("cloud_n", "seeds", "pidx", "merged", "sel") else want
            assert np.array_equal(got, want), (c, name)


def test_upsample_ragged_equals_upsample_cloud(dev):
    from dispu_amd.generator import Generator
    gen = Generator(params=OG.init_params(seed=3, bias_scale=0.05, bn_random=True), device=dev)
    _check_ragged(gen, _sphere_clouds([256, 300, 1000, 1024, 2048, 1024, 2500], 8))


def test_upsample_ragged_16x_and_patch_128(dev):
    from dispu_amd.generator import Generator
    gen = Generator(params=OG.init_params(seed=4), device=dev)
    _check_ragged(gen, _sphere_clouds([256, 300, 600], 9), final_ratio=16)
    _check_ragged(gen, _sphere_clouds([128, 300, 700, 300], 10), patch_num_point=128)


def test_upsample_ragged_single_cloud_and_device_input(dev):
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    gen = Generator(params=OG.init_params(seed=5), device=dev)
    (pc,) = _sphere_clouds([1000], 12)
    (out,) = U.upsample_ragged(gen, [pc])
    assert np.array_equal(out, U.upsample_cloud(gen, pc))
    a, b = _sphere_clouds([700, 400], 13)
    outs = U.upsample_ragged(gen, [torch.from_numpy(a).to(dev), b])
    assert np.array_equal(outs[0], U.upsample_cloud(gen, a)) and np.array_equal(outs[1], U.upsample_cloud(gen, b))


def test_upsample_command_end_to_end(dev, tmp_path):
    from dispu_amd import checkpoint as CK
    from dispu_amd import upsample as U
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    clouds = _sphere_clouds([700, 256, 1100], 14)
    names = ["b_cloud", "a_cloud", "c_cloud"]
    for name, pc in zip(names, clouds):
        rows = pc if name != "c_cloud" else np.concatenate([pc, np.ones_like(pc)], axis=1)    # six columns: normals are ignored
        np.savetxt(str(data / "test" / (name + ".xyz")), rows, fmt="%.6f")
    _, gen = CK.restore_generator(str(log_dir), device=dev)
    want = {}
    for name in names:
        pc = np.loadtxt(str(data / "test" / (name + ".xyz"))).astype(np.float32)[:, :3]
        path = str(tmp_path / (name + "_ref.xyz"))
        np.savetxt(path, U.upsample_cloud(gen, pc), fmt="%.6f")
        want[name] = open(path, "rb").read()
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    for extra, out_dir in [([], data / "test" / "output"), (["--max-points", "1", "--out_folder", str(tmp_path / "o2")], tmp_path / "o2")]:
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")
        assert sorted(os.listdir(str(out_dir))) == sorted(n + "_X4.xyz" for n in names)
        for name in names:
            assert open(str(out_dir / (name + "_X4.xyz")), "rb").read() == want[name], (extra, name)
