"""GPU parity of the whole-cloud path (dis-pu_amd/upsample.py vs oracle/upsample.py), stage by stage: seeds and
patch indices exact, normalised patches 1e-6, generator output / merged cloud 1e-5, the final FPS exact on the SAME
merged cloud (a down-sampling of slightly different floats may legitimately pick different near-tie points)."""
import numpy as np
import pytest
import torch

from oracle import generator as OG
from oracle import oracle as O
from oracle import upsample as OU

pytestmark = pytest.mark.gpu


def N(t):
    return t.detach().cpu().numpy()


def merged_from_stages(pc, st):
    """the float32 numpy denormalisation (patch, then cloud: model.py:310-311, :371-372) of the device's own fine cloud with the
    device's own centroids and scales -- normalize_patches again on the stage inputs, which must give the stages back bit for bit."""
    from dispu_amd import upsample as U
    dev = st["fine"].device
    cloud_n, c0, f0 = U.normalize_patches(torch.from_numpy(np.ascontiguousarray(pc, np.float32)[None]).to(dev))
    assert torch.equal(cloud_n, st["cloud_n"])
    patches = st["cloud_n"][0][st["pidx"][0].long()].contiguous()
    pn, pc_c, pc_f = U.normalize_patches(patches)
    assert torch.equal(pn, st["patches_n"])
    fine = N(st["fine"])
    pred = N(pc_c)[:, None, :] + fine * N(pc_f)[:, None, None]
    merged = N(c0)[:, None, :] + pred.reshape(1, -1, 3) * N(f0)[:, None, None]
    assert fine.dtype == np.float32 and merged.dtype == np.float32
    return merged


def test_knn_patch_large_k(dev):
    from dispu_amd import upsample as U
    rng = np.random.default_rng(0)
    for (n, m, k) in [(2048, 24, 256), (1000, 7, 256), (300, 5, 300), (8192, 3, 256), (24576, 12, 256), (10000, 4, 1024)]:   # n > 8192: radix-select kernel
        pc = rng.random((1, n, 3)).astype(np.float32)
        pc[0, 10] = pc[0, 3]                                   # duplicate -> tie resolved by index
        q = pc[:, :m].copy()
        got = N(U.knn_patch(torch.from_numpy(pc).to(dev), torch.from_numpy(q).to(dev), k))
        assert np.array_equal(got[0], OU.extract_knn_patch_idx(q[0], pc[0], k))


def test_config4_16x_with_cd_and_emd(dev):
    """BASELINE configs[3]: 16x upsampling (256 -> 1024 -> 4096, two generator passes, DisPU/model.py:114-118) followed by
    the Chamfer and approxmatch-EMD losses against a 4096-point ground truth, on one GPU."""
    from dispu_amd import loss_utils as LU
    from dispu_amd import synth
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    from oracle import modules as OM
    x, gt = synth.patch_with_gt(1, 256, 4096, seed=21)
    P = OG.init_params(seed=2)
    gen = Generator(params=P, device=dev)
    tx = torch.from_numpy(x).to(dev)
    coarse, fine = U.generator_chain(gen, tx, final_ratio=16)
    assert tuple(fine.shape) == (1, 4096, 3)
    # the chain is two generator calls, the second on the first one's fine cloud
    _, f1_dev = gen(tx)
    c2_dev, f2_dev = gen(f1_dev)
    assert torch.equal(c2_dev, coarse) and torch.equal(f2_dev, fine)
    c1, f1 = OG.generator_forward(P, x)
    c2, f2 = OG.generator_forward(P, f1)
    # pass 1 is bit-exact up to `coarse`; pass 2 starts from fine (1e-5) so its k-NN decisions may flip on near-ties:
    # compare the clouds as point sets through the Chamfer distance, and the losses against the oracle on the GPU cloud
    assert np.abs(N(coarse) - c2).max() < 5e-2
    d1, _, d2, _ = O.nn_distance(N(fine), f2, contract=0)
    assert np.median(d1) < 1e-8 and np.median(d2) < 1e-8
    # pass 2 against the oracle on the device's own pass-1 output: the N = 256 standard at N = 1024
    tap = {}
    c2_own, f2_own = OG.generator_forward(P, N(f1_dev), tap)
    assert np.array_equal(N(coarse), c2_own)
    assert np.array_equal(N(gen._ws[(1, 1024)]["psidx"]).reshape(1, 4096, 16), tap["ps_idx"])
    assert np.abs(N(fine) - f2_own).max() <= 1e-5
    tf, tg = fine.clone(), torch.from_numpy(gt).to(dev)
    cd, emd = float(LU.chamfer(tf, tg)), float(LU.earth_mover(tf, tg))
    assert abs(cd - OM.chamfer(N(tf), gt)) <= 1e-5 * max(1.0, OM.chamfer(N(tf), gt))
    assert abs(emd - OM.earth_mover(N(tf), gt)) <= 1e-5 * OM.earth_mover(N(tf), gt)


def test_config4_at_full_batch_properties(dev):
    """BASELINE configs[3] at the size of SURVEY 8(d): B = 32 patches, 256 -> 1024 -> 4096, CD + EMD against 4096-point ground
    truths.  The oracle's approx_match needs seconds per 4096^2 cloud, so the full batch is checked through size-independent
    properties, and two of the 32 clouds against the oracle:
      * the second generator pass is batch independent (row 5 of the B = 32 run == a B = 1 run on the same input), bit for bit;
      * match: non-negative, every row and column sums to 1 (n == m);  EMD(x, x) is ~0 against EMD(x, y);
      * Chamfer of the batch == the mean of per-cloud Chamfer values computed alone (nn_distance is per cloud);
      * clouds 3 and 30: match_cost / chamfer against the oracle on the same GPU clouds (1e-5)."""
    from dispu_amd import loss_utils as LU
    from dispu_amd import synth
    from dispu_amd import tf_approxmatch as A
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    from dispu_amd.params import init_params
    from oracle import modules as OM
    B = 32
    x, gt = synth.patch_with_gt(B, 256, 4096, seed=1000 * 3)
    gen = Generator(params=init_params(seed=1234), device=dev)
    tx, tg = torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)
    _, fine = U.generator_chain(gen, tx, final_ratio=16)
    assert tuple(fine.shape) == (B, 4096, 3) and torch.isfinite(fine).all()
    _, f1 = gen(tx)
    _, f5 = gen(f1[5:6].clone())
    assert torch.equal(f5[0], fine[5])
    match = A.approx_match(fine, tg)
    assert float(match.min()) >= 0.0
    assert float((match.sum(1) - 1).abs().max()) <= 2e-5 and float((match.sum(2) - 1).abs().max()) <= 2e-5
    cost = A.match_cost(fine, tg, match)
    self_cost = A.match_cost(fine, fine, A.approx_match(fine, fine))
    assert float((self_cost / cost).max()) < 0.05
    emd = float(LU.earth_mover(fine, tg))
    assert abs(emd - float((cost / 4096.0).mean())) <= 1e-6 * emd
    cd = float(LU.chamfer(fine, tg))
    alone = np.mean([float(LU.chamfer(fine[i:i + 1], tg[i:i + 1])) for i in range(B)])
    assert abs(cd - alone) <= 1e-6 * max(1.0, abs(alone))
    for i in (3, 30):
        fi, gi = N(fine[i:i + 1]), gt[i:i + 1]
        assert abs(float(LU.chamfer(fine[i:i + 1], tg[i:i + 1])) - OM.chamfer(fi, gi)) <= 1e-5 * max(1.0, OM.chamfer(fi, gi))
        co = O.match_cost(fi, gi, N(match[i:i + 1]))                       # the oracle's cost of the GPU plan
        assert abs(float(cost[i]) - float(co[0])) <= 1e-5 * float(co[0])


def test_upsample_cloud_stage_parity(dev):
    from dispu_amd import synth
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    rng = np.random.default_rng(1)
    g = rng.standard_normal((1024, 3))
    pc = (g / np.linalg.norm(g, axis=1, keepdims=True) * np.array([1.0, 0.7, 0.4]) + 5.0).astype(np.float32)   # an ellipsoid, off-centre
    P = OG.init_params(seed=3)
    gen = Generator(params=P, device=dev)
    out, st = U.upsample_cloud(gen, pc, return_stages=True)
    want, ws = OU.upsample_cloud(P, pc)
    assert out.shape == (4096, 3) and want.shape == (4096, 3)
    assert np.allclose(N(st["cloud_n"])[0], ws["cloud_n"], atol=2e-6)      # cloud sits at +5: one float32 ulp there is 5e-7
    # FPS / kNN run on the device's own normalised cloud; re-run the oracle ops on exactly that cloud
    cn = N(st["cloud_n"])
    assert np.array_equal(N(st["seeds"]), O.farthest_point_sample(12, cn))
    seeds_xyz = cn[0][N(st["seeds"])[0]]
    assert np.array_equal(N(st["pidx"])[0], OU.extract_knn_patch_idx(seeds_xyz, cn[0], 256))
    pn_want = OU.normalize_point_cloud(cn[0][N(st["pidx"])[0]])[0]
    assert np.allclose(N(st["patches_n"]), pn_want, atol=2e-6)
    c_want, f_want = OG.generator_forward(P, N(st["patches_n"]))
    assert np.abs(N(st["fine"]) - f_want).max() <= 1e-5
    merged = N(st["merged"])
    assert merged.shape == (1, 12 * 1024, 3) and np.array_equal(merged, merged_from_stages(pc, st))
    assert np.array_equal(N(st["sel"]), O.farthest_point_sample(4096, merged))
    assert np.array_equal(out, merged[0][N(st["sel"])[0]])
    # end to end against the independent oracle run: same point set up to float noise unless a near-tie flipped
    d1, _, d2, _ = O.nn_distance(out[None], want[None], contract=0)
    assert np.median(d1) < 1e-9 and np.median(d2) < 1e-9


def test_upsample_cloud_16x_stage_parity(dev):
    """BASELINE configs[3] on a whole cloud: upsample_clouds(final_ratio=16) on 1024 points -> 12 patches, two generator passes
    (256 -> 1024 -> 4096 points per patch), 49152 merged points, FPS to 16384.  Like test_upsample_cloud_stage_parity, every stage
    is checked against the oracle on the device's own input to that stage: seeds and patch indices exact, both generator passes of
    all 12 patches at the N = 256 standard (coarse bit-exact, xyz neighbours index-exact, fine 1e-5), the final FPS exact."""
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    rng = np.random.default_rng(4)
    g = rng.standard_normal((1024, 3))
    pc = (g / np.linalg.norm(g, axis=1, keepdims=True) * np.array([0.5, 1.2, 0.8]) - 3.0).astype(np.float32)   # an ellipsoid, off-centre
    P = OG.init_params(seed=6, bias_scale=0.05, bn_random=True)
    gen = Generator(params=P, device=dev)
    out, st = U.upsample_cloud(gen, pc, final_ratio=16, return_stages=True)
    assert out.shape == (16384, 3)
    cn = N(st["cloud_n"])
    assert np.array_equal(N(st["seeds"]), O.farthest_point_sample(12, cn))
    seeds_xyz = cn[0][N(st["seeds"])[0]]
    assert np.array_equal(N(st["pidx"])[0], OU.extract_knn_patch_idx(seeds_xyz, cn[0], 256))
    pn = N(st["patches_n"])
    assert np.allclose(pn, OU.normalize_point_cloud(cn[0][N(st["pidx"])[0]])[0], atol=2e-6)
    # return_stages keeps the last pass's fine cloud only: run the two passes again, the second must give what the chain gave
    c1, f1 = gen(st["patches_n"])
    c2, f2 = gen(f1)
    assert tuple(f2.shape) == (12, 4096, 3) and torch.equal(f2, st["fine"])
    c1_want, f1_want = OG.generator_forward(P, pn)
    assert np.array_equal(N(c1), c1_want) and np.abs(N(f1) - f1_want).max() <= 1e-5
    tap = {}
    c2_want, f2_want = OG.generator_forward(P, N(f1), tap)
    assert np.array_equal(N(c2), c2_want)
    assert np.array_equal(N(gen._ws[(12, 1024)]["psidx"]).reshape(12, 4096, 16), tap["ps_idx"])
    assert np.abs(N(f2) - f2_want).max() <= 1e-5
    merged = N(st["merged"])
    assert merged.shape == (1, 49152, 3) and np.array_equal(merged, merged_from_stages(pc, st))
    assert np.array_equal(N(st["sel"]), O.farthest_point_sample(16384, merged))
    assert np.array_equal(out, merged[0][N(st["sel"])[0]])


def test_upsample_clouds_batch_equals_single(dev):
    """upsample_clouds: C clouds through ONE launch sequence (FPS over C clouds at once, C * 24 patches in one generator batch)
    == C calls of upsample_cloud, bit for bit (DisPU/model.py:343-381 per cloud)."""
    from dispu_amd import upsample as U
    from dispu_amd.generator import Generator
    rng = np.random.default_rng(8)
    g = rng.standard_normal((3, 1024, 3))
    pcs = (g / np.linalg.norm(g, axis=2, keepdims=True) * rng.uniform(0.5, 1.5, (3, 1, 3)) + rng.uniform(-2, 2, (3, 1, 3))).astype(np.float32)
    gen = Generator(params=OG.init_params(seed=3), device=dev)
    both = N(U.upsample_clouds(gen, pcs))
    assert both.shape == (3, 4096, 3)
    for c in range(3):
        assert np.array_equal(both[c], U.upsample_cloud(gen, pcs[c]))
