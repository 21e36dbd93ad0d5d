"""GPU parity at the HEADLINE size: BASELINE configs[1] exactly as bench.py runs it (B = 32 patches of 256 points,
Xavier weights seed 1234, input seed 1000*2 + rank) -- DisPU/generator.py:31-88 counterpart.

At B = 32 the persistent kernels (ps_local, edge_dense_conv) loop over more than one group per workgroup and the
GEMMs take their interior 128x256 DMA tiles (rm = 32768), grid shapes the B <= 5 tests never reach.  Checked here:
  * a spread of the 32 patches against oracle/generator.py (coarse bit-exact, fine <= 1e-5),
  * batch independence against B = 1 runs (bit-identical),
  * hipGraph replay == eager launch (bit-identical), the way bench.py times the step,
  * the same with non-zero biases / a non-trivial BN fold.
"""
import os

import numpy as np
import pytest
import torch

from oracle import generator as OG

pytestmark = pytest.mark.gpu

BENCH_B, BENCH_N, BENCH_SEED = 32, 256, 1000 * 2 + 0      # bench.py: synth.patches(32, 256, seed=1000*config + rank)
CHECK = (0, 7, 19, 31)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def bench_setup(dev):
    from dispu_amd import synth
    from dispu_amd.generator import Generator
    from dispu_amd.params import init_params
    P = init_params(seed=1234)
    gen = Generator(params=P, device=dev)
    x = synth.patches(BENCH_B, BENCH_N, seed=BENCH_SEED)
    tx = torch.from_numpy(x).to(dev)
    c, f = gen(tx)
    torch.cuda.synchronize()
    return dict(P=P, gen=gen, x=x, tx=tx, c=N(c).copy(), f=N(f).copy())


def test_b32_against_oracle(bench_setup):
    s = bench_setup
    oc, of = OG.generator_forward(s["P"], s["x"][list(CHECK)])
    for j, p in enumerate(CHECK):
        assert np.array_equal(s["c"][p], oc[j]), "coarse of patch %d differs from the oracle (bit-exact expected)" % p
        err = np.abs(s["f"][p] - of[j]).max()
        assert err <= 1e-5, "fine of patch %d off by %g" % (p, err)
    assert np.isfinite(s["f"]).all() and np.isfinite(s["c"]).all()


def test_b32_batch_independence(bench_setup):
    s = bench_setup
    for p in (3, 19, 30):
        c1, f1 = s["gen"](s["tx"][p:p + 1])
        assert np.array_equal(N(c1)[0], s["c"][p]) and np.array_equal(N(f1)[0], s["f"][p]), "patch %d depends on its batch" % p


def test_b32_hipgraph_replay_equals_eager(bench_setup, dev):
    """bench.py's timed region is graph.replay(): the replayed launches must reproduce the eager result bit for bit."""
    s = bench_setup
    gen, tx = s["gen"], s["tx"]
    gen.return_views = True                    # as bench.py: the captured step holds no copy kernels
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gen(tx)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gen(tx)
    ws = gen._ws[(BENCH_B, BENCH_N)]
    for _ in range(3):
        ws["coarse"].zero_()
        ws["fine"].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(N(ws["coarse"]), s["c"]) and np.array_equal(N(ws["fine"]), s["f"])
    gen.return_views = False


def test_b32_biases_and_bn(dev):
    from dispu_amd import synth
    from dispu_amd.generator import Generator
    P = OG.init_params(seed=77, bias_scale=0.05, bn_random=True)
    gen = Generator(params=P, device=dev)
    x = synth.patches(BENCH_B, BENCH_N, seed=4242)
    c, f = gen(torch.from_numpy(x).to(dev))
    c, f = N(c), N(f)
    sel = [5, 26]
    oc, of = OG.generator_forward(P, x[sel])
    for j, p in enumerate(sel):
        assert np.array_equal(c[p], oc[j])
        assert np.abs(f[p] - of[j]).max() <= 1e-5


def test_b64_and_ragged_batches(dev):
    """batches that are not a multiple of the persistent kernels' group count, and a larger one (rm = 65536)."""
    from dispu_amd import synth
    from dispu_amd.generator import Generator
    from dispu_amd.params import init_params
    P = init_params(seed=1234)
    gen = Generator(params=P, device=dev)
    x = synth.patches(64, BENCH_N, seed=99)
    tx = torch.from_numpy(x).to(dev)
    c64, f64 = gen(tx)
    c64, f64 = N(c64).copy(), N(f64).copy()
    for b in (33, 17, 7):
        c, f = gen(tx[:b])
        assert np.array_equal(N(c), c64[:b]) and np.array_equal(N(f), f64[:b]), "B=%d differs from the B=64 rows" % b
    oc, of = OG.generator_forward(P, x[63:64])
    assert np.array_equal(c64[63], oc[0]) and np.abs(f64[63] - of[0]).max() <= 1e-5


def test_split_bf16_gemm_is_fp32_accurate(dev):
    """dispu_linear_bf16x3 (exploratory): three-term bf16 splitting of both operands, six exact partial products per k accumulated
    in fp32 -> as accurate as an fp32 GEMM (compared with float64), though not the same rounding as dispu_linear's fmaf chain."""
    from dispu_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(0)
    M, K, Nn = 512, 2048, 256
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32) * rng.random((M, 1)).astype(np.float32)
    w = (rng.standard_normal((K, Nn)) * 0.03).astype(np.float32)
    b = rng.standard_normal(Nn).astype(np.float32) * 0.1
    r1, r2 = rng.standard_normal((M, Nn)).astype(np.float32), rng.standard_normal((M, Nn)).astype(np.float32)
    tx, tw, tb, t1, t2 = (torch.from_numpy(a).to(dev) for a in (x, w, b, r1, r2))
    planes = torch.empty(3 * K * Nn, dtype=torch.bfloat16, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(L.dispu_bf16x3_split_weights(K, Nn, tw.data_ptr(), Nn, planes.data_ptr(), st), "split")
    # slab-major planes of the wave-specialised kernel: [K / 32][plane][256 cols][4 chunk positions][8], chunk c of column n at
    # position c ^ ((n >> 2) & 3); the three planes add back up to W to 24 bits
    pl = planes.view(K // 32, 3, Nn, 4, 8).float().sum(1)                            # [t][n][position][8]
    pos = (torch.arange(4, device=dev)[None, :] ^ ((torch.arange(Nn, device=dev)[:, None] >> 2) & 3))  # [n][c] -> position
    rec = torch.gather(pl, 2, pos[None, :, :, None].expand(K // 32, Nn, 4, 8)).permute(0, 2, 3, 1).reshape(K, Nn)
    assert float((rec - tw).abs().max()) <= 2.0 ** -22 * float(tw.abs().max())
    y = torch.zeros((M, Nn), device=dev)
    _lib.check(L.dispu_linear_bf16x3(M, K, Nn, tx.data_ptr(), K, planes.data_ptr(), tb.data_ptr(), 1, y.data_ptr(), Nn, t1.data_ptr(), Nn,
                                     t2.data_ptr(), Nn, st), "dispu_linear_bf16x3")
    y32 = torch.zeros((M, Nn), device=dev)
    _lib.check(L.dispu_linear(1, M, K, Nn, tx.data_ptr(), K, 0, tw.data_ptr(), Nn, 0, 0, tb.data_ptr(), 1, y32.data_ptr(), Nn, 0,
                              t1.data_ptr(), Nn, 0, t2.data_ptr(), Nn, 0, st), "dispu_linear")
    want = np.maximum(x.astype(np.float64) @ w.astype(np.float64) + b, 0) + r1 + r2
    scale = (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)).max()
    e3, e32 = np.abs(N(y) - want).max() / scale, np.abs(N(y32) - want).max() / scale
    print("max error / sum|a||b|: split-bf16 %.2e, fp32 MFMA %.2e" % (e3, e32))
    assert e3 <= 4e-7 and e3 <= 4 * e32 + 1e-7


@pytest.mark.parametrize("M,K,Nn", [(256, 2048, 256), (128, 128, 512), (384, 160, 256), (256, 96, 256), (128, 256, 128)])
def test_split_bf16_gemm_shapes(dev, M, K, Nn):
    """Both split-bf16 kernels (wave-specialised: N % 256 == 0, K % 32 == 0, K >= 128; the single-role one otherwise) against float64,
    with and without residuals; planes and kernel are chosen by the same shape rule."""
    from dispu_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(M + K + Nn)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, Nn)) * 0.1).astype(np.float32)
    b = rng.standard_normal(Nn).astype(np.float32)
    r1 = rng.standard_normal((M, Nn)).astype(np.float32)
    tx, tw, tb, t1 = (torch.from_numpy(a).to(dev) for a in (x, w, b, r1))
    planes = torch.empty(3 * K * Nn, dtype=torch.bfloat16, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(L.dispu_bf16x3_split_weights(K, Nn, tw.data_ptr(), Nn, planes.data_ptr(), st), "split")
    scale = (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)).max()
    for act, res in ((1, True), (0, False)):
        y = torch.full((M, Nn + 8), -3.0, device=dev)
        _lib.check(L.dispu_linear_bf16x3(M, K, Nn, tx.data_ptr(), K, planes.data_ptr(), tb.data_ptr(), act, y.data_ptr(), Nn + 8,
                                         t1.data_ptr() if res else None, Nn, None, 0, st), "dispu_linear_bf16x3")
        want = x.astype(np.float64) @ w.astype(np.float64) + b
        want = (np.maximum(want, 0) if act else want) + (r1 if res else 0)
        assert np.abs(N(y)[:, :Nn] - want).max() / scale <= 4e-7
        assert (N(y)[:, Nn:] == -3.0).all()


@pytest.mark.parametrize("M,K,Nn", [(256, 2048, 256), (384, 160, 512)])
def test_split_bf16_streaming_kernel_equals_wave_specialised(dev, M, K, Nn):
    """Round 6's streaming split-bf16 kernel (operands by DMA, all eight waves compute, fragment split pipelined between the MFMAs;
    dispu_debug_x3_kernel(0)) issues the same products in the same order per accumulator as round 4's wave-specialised kernel (the
    default, 1): bit-identical outputs, with residuals and bias."""
    from dispu_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(M + K)
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    w = (rng.standard_normal((K, Nn)) * 0.1).astype(np.float32)
    b = rng.standard_normal(Nn).astype(np.float32)
    r1 = rng.standard_normal((M, Nn)).astype(np.float32)
    tx, tw, tb, t1 = (torch.from_numpy(a).to(dev) for a in (x, w, b, r1))
    planes = torch.empty(3 * K * Nn, dtype=torch.bfloat16, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(L.dispu_bf16x3_split_weights(K, Nn, tw.data_ptr(), Nn, planes.data_ptr(), st), "split")
    ys = {}
    try:
        for which in (1, 0):
            L.dispu_debug_x3_kernel(which)
            y = torch.zeros((M, Nn), device=dev)
            _lib.check(L.dispu_linear_bf16x3(M, K, Nn, tx.data_ptr(), K, planes.data_ptr(), tb.data_ptr(), 1, y.data_ptr(), Nn, t1.data_ptr(), Nn,
                                             None, 0, st), "dispu_linear_bf16x3")
            ys[which] = y
        torch.cuda.synchronize()
    finally:
        L.dispu_debug_x3_kernel(1)
    assert torch.equal(ys[0], ys[1])
    want = np.maximum(x.astype(np.float64) @ w.astype(np.float64) + b, 0) + r1
    scale = (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)).max()
    assert np.abs(N(ys[0]) - want).max() / scale <= 4e-7


def test_generator_split_bf16_mode_within_tolerance(bench_setup, dev):
    """Generator.split_bf16 (exploratory): after_conv through the split-bf16 GEMM.  coarse (decided before the refinement branch)
    stays bit-exact, fine stays within the 1e-5 tolerance against the oracle and within 2e-6 of the strict-fp32 run."""
    from dispu_amd.generator import Generator
    s = bench_setup
    gen = Generator(params=s["P"], device=dev)
    gen.split_bf16 = True
    c, f = gen(s["tx"])
    assert np.array_equal(N(c), s["c"])
    assert np.abs(N(f) - s["f"]).max() <= 2e-6
    oc, of = OG.generator_forward(s["P"], s["x"][[11]])
    assert np.abs(N(f)[11] - of[0]).max() <= 1e-5


def test_two_stream_forward_equals_single_stream(bench_setup, dev):
    """Generator.branches (default on: the non-local cell on a second stream, joined right before the fine head chain) runs the same
    kernels on the same data: coarse and fine bit-identical to the single-stream forward, eagerly and replayed from a hipGraph."""
    from dispu_amd.generator import Generator
    s = bench_setup
    outs = []
    for br in (True, False):
        gen = Generator(params=s["P"], device=dev)
        gen.branches = br
        gen.return_views = True
        c, f = gen(s["tx"])
        torch.cuda.synchronize()
        outs.append((N(c).copy(), N(f).copy()))
        if br:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                gen(s["tx"])
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                c2, f2 = gen(s["tx"])
            c2.zero_(); f2.zero_()
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize()
            outs.append((N(c2).copy(), N(f2).copy()))
    assert Generator(params=s["P"], device=dev).branches                 # the default
    for c, f in outs[1:]:
        assert np.array_equal(c, outs[0][0]) and np.array_equal(f, outs[0][1])
    assert np.array_equal(outs[0][0], s["c"]) and np.array_equal(outs[0][1], s["f"])


@pytest.mark.parametrize("n", [BENCH_N, 1024])
def test_oversize_batches_run_in_chunks(dev, n):
    """Batches above Generator.MAX_POINTS input points (2048 x 256: keeps row * stride products below 2^31) are processed in chunks
    of whole patches; patches are independent, so the result is the unchunked one.  The budget counts points, not patches: with the
    same budget and B, 1024-point patches (the second pass of 16x upsampling) run in more chunks than 256-point ones.  Exercised here
    with tiny budgets of three 1024-point and three 256-point patches."""
    from dispu_amd import synth
    from dispu_amd.generator import Generator
    from dispu_amd.params import init_params
    gen = Generator(params=init_params(seed=1234), device=dev)
    x = torch.from_numpy(synth.patches(7, n, seed=5)).to(dev)
    c7, f7 = gen(x)
    seq = []                                          # the (B, N) of every launch sequence
    ws = gen._workspace
    gen._workspace = lambda b, n_: seq.append((b, n_)) or ws(b, n_)
    chunks = {(BENCH_N, 3 * 1024): [7], (1024, 3 * 1024): [3, 3, 1],
              (BENCH_N, 3 * BENCH_N): [3, 3, 1], (1024, 3 * BENCH_N): [1] * 7}      # a patch above the budget runs alone
    for budget in (3 * 1024, 3 * BENCH_N):
        gen.MAX_POINTS = budget
        del seq[:]
        c, f = gen(x)
        assert seq == [(b, n) for b in chunks[(n, budget)]], budget
        assert torch.equal(c, c7) and torch.equal(f, f7)
    gen.return_views = True
    with pytest.raises(ValueError):
        gen(x)


def test_chain_input_modes_equal_producer_kernels(bench_setup, dev):
    """round 4: the head chains form their own input tiles (dispu_mlp_chain_dup: duplicate_up's rows from the per-source-point product;
    dispu_mlp_chain_sum3: relu(after_conv) + skip + non-local) -- bit-identical to dup_grid + the residual epilogue + dispu_mlp_chain,
    at the bench's size (128-row workgroups) and at B = 1, 3 (64-row workgroups, partial clouds per workgroup)."""
    from dispu_amd.generator import Generator
    s = bench_setup
    old = Generator(params=s["P"], device=dev)
    old.chain_inputs = False
    assert s["gen"].chain_inputs
    for B in (32, 3, 1):
        x = s["tx"][:B].contiguous()
        c0, f0 = old(x)
        c1, f1 = s["gen"](x)
        assert np.array_equal(N(c0), N(c1)) and np.array_equal(N(f0), N(f1)), "B = %d" % B


def test_bench_plain_run_dumps_the_timed_step(bench_setup, tmp_path):
    """`bench.py --steps K --dump-outputs DIR` without --full: the headline fields only, K timed steps, and the clouds of the last
    timed step on disk -- bit-identical to the eager forward of the same seeded patches and weights."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DISPU_BENCH_COLLECTIVES", "DISPU_BENCH_GATHER"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=root, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "one JSON line expected, got %d" % len(lines)
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "points/s" and d["dtype"] == "f32" and d["higher_is_better"] is True and d["metric"].startswith("upsampled points/sec")
    assert abs(d["value"] - BENCH_B * BENCH_N * 4 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("roofline", "cpu_baseline", "alt_split_bf16", "alt_two_in_flight", "ms_per_step_repeats"):
        assert k not in d, "%s belongs to --full" % k
    assert sorted(os.listdir(tmp_path)) == ["coarse.npy", "fine.npy"]
    s = bench_setup
    for name, ref in (("coarse", s["c"]), ("fine", s["f"])):
        a = np.load(str(tmp_path / (name + ".npy")))
        assert a.dtype == np.float32 and a.shape == (BENCH_B, BENCH_N * 4, 3), (name, a.dtype, a.shape)
        assert np.array_equal(a, ref), "%s.npy differs from the eager forward" % name
