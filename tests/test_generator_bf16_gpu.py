"""Generator(dtype="bf16") on the GPU: the local cell's bf16 store alone (dispu_ps_local_bf16, bit for bit against the fp32 kernel's
output rounded), F' and everything upstream inside the generator, after_conv against float64 on the operands it really read, the whole
forward against the CPU reference of tests/generator_bf16_oracle.py, the plumbing around it, and tools/upsample.py --dtype."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import generator_bf16_oracle as BO
from oracle import generator as OG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # hipErrorInvalidValue
CANARY = 0x5A5A
AFT = "refine/PointShuffle/after_conv/"


def N(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16)


def _gen(dev, P, dtype="bf16"):
    from dispu_amd.generator import Generator
    return Generator(params=P, device=dev, dtype=dtype)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone ----
@pytest.mark.parametrize("clouds,n", [(1, 20), (3, 170), (300, 24), (1200, 256)])
def test_ps_local_bf16_abi(dev, clouds, n):
    """dispu_ps_local_bf16 through the C ABI on the inputs of test_generator_gpu.py::test_ps_local_abi_ragged_groups: one chain of groups
    with a ragged tail, ragged groups over several clouds, 900 groups over 256 persistent workgroups (tiles flushed during the next
    group's products, and the drain), and more than 2^18 points (the launch is cut at a cloud boundary and the output base advances in
    2-byte elements).  Every element is the fp32 kernel's, rounded to nearest even; nothing is written behind the result."""
    from dispu_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(clouds * 1000 + n)
    npts = clouds * n
    xyz = torch.from_numpy(rng.random((npts, 3)).astype(np.float32)).to(dev)
    idx = torch.from_numpy(rng.integers(0, n, (npts, 16)).astype(np.int32)).to(dev)
    G = torch.from_numpy(rng.standard_normal((npts, 320)).astype(np.float32)).to(dev)
    A = torch.from_numpy(rng.standard_normal((npts, 128)).astype(np.float32)).to(dev)
    W1 = torch.from_numpy((rng.standard_normal((128, 128)) * 0.1).astype(np.float32)).to(dev)
    b1 = torch.from_numpy((rng.standard_normal(128) * 0.1).astype(np.float32)).to(dev)
    Ww = torch.from_numpy(rng.standard_normal((3, 16)).astype(np.float32)).to(dev)
    bw = torch.from_numpy(rng.standard_normal(16).astype(np.float32)).to(dev)
    sc = torch.from_numpy((1 + 0.1 * rng.standard_normal(16)).astype(np.float32)).to(dev)
    sh = torch.from_numpy((0.1 * rng.standard_normal(16)).astype(np.float32)).to(dev)
    st = _lib.stream_ptr(dev)
    P = lambda t, off=0: t.data_ptr() + 4 * off
    pad = 4096
    out = torch.full((npts * 2048 + pad,), CANARY, dtype=torch.int16, device=dev)             # canary behind the result
    args = lambda k=16, c=128, o=0: (n, k, c, P(idx), P(xyz), P(G, 192), 320, P(A), P(W1), P(b1), P(Ww), P(bw), P(sc), P(sh), out.data_ptr() + o, st)
    _lib.check(L.dispu_ps_local_bf16(npts, *args()), "dispu_ps_local_bf16")
    ref = torch.empty((npts, 2048), device=dev)
    _lib.check(L.dispu_ps_local(npts, n, 16, 128, P(idx), P(xyz), P(G, 192), 320, P(A), P(W1), P(b1), P(Ww), P(bw), P(sc), P(sh), P(ref), st),
               "dispu_ps_local")
    want = ref.bfloat16()
    del ref
    got = out[:npts * 2048].view(npts, 2048)
    assert torch.equal(got, bits(want)), int((got != bits(want)).any(1).nonzero()[0])
    assert bool((out[npts * 2048:] == CANARY).all())
    assert bool((want.float() > 0).any())                                               # not a comparison of zeros
    # argument checks: nothing is launched, nothing is written
    assert L.dispu_ps_local_bf16(0, *args()) == 0
    assert L.dispu_ps_local_bf16(npts, *args(k=8)) == INVALID
    assert L.dispu_ps_local_bf16(npts, *args(c=64)) == INVALID
    assert L.dispu_ps_local_bf16(npts, *args(o=2)) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(got, bits(want))


# ------------------------------------------------------------------------------------- 2. F' inside the generator ----
@pytest.fixture(scope="module")
def b32(dev):
    """both modes at the bench's shape (32 patches of 256 points), on biased weights and a folded BatchNorm"""
    from dispu_amd import synth
    P = OG.init_params(seed=77, bias_scale=0.05, bn_random=True)
    tx = torch.from_numpy(synth.patches(32, 256, seed=4242)).to(dev)
    res = {"tx": tx, "P": P}
    for dt in ("f32", "bf16"):
        gen = _gen(dev, P, dt)
        c, f = gen(tx)
        torch.cuda.synchronize()
        res[dt] = dict(gen=gen, c=N(c).copy(), f=N(f).copy(), ws=gen._ws[(32, 256)])
    return res


def test_fp_is_the_fp32_tensor_rounded(b32):
    a, b = b32["f32"], b32["bf16"]
    assert b["ws"]["fp"].dtype == torch.bfloat16 and tuple(b["ws"]["fp"].shape) == (32 * 1024, 2048)
    assert torch.equal(bits(b["ws"]["fp"]), bits(a["ws"]["fp"].bfloat16()))
    assert np.array_equal(a["c"], b["c"])
    assert torch.equal(a["ws"]["psidx"], b["ws"]["psidx"])
    assert not np.array_equal(a["f"], b["f"])                 # the mode does change the one product


# ------------------------------------------------------------------------------------------ 3. aft against float64 ----
def _aft_operands(dev, B, n):
    from dispu_amd import synth
    P = OG.init_params(seed=7, bias_scale=0.05, bn_random=True)
    x = torch.from_numpy(synth.patches(B, n, seed=11)).to(dev)
    g16, g32 = _gen(dev, P, "bf16"), _gen(dev, P, "f32")
    g16(x)
    g32(x)
    torch.cuda.synchronize()
    return P, g16, g16._ws[(B, n)], g32._ws[(B, n)]


@pytest.mark.parametrize("B,n", [(1, 256), (1, 288), (2, 250)])      # rm = 2000: the generic bf16 kernel and the add3 residual path
def test_aft_against_float64(dev, B, n):
    """relu(x^.w^ + b) in float64 on the operands after_conv really read: the stored bf16 F' and the packed weight image.  Bound per
    element: 2e-6 (|x^|.|w^|) + 1e-6 (1 + |z|), tests/test_train_bf16_gpu.py's for these kernels (fp32 accumulation of 2048 exact
    bf16 x bf16 products).  Against the UNROUNDED operands each factor's RNE error is at most 2^-8, so the products differ by at most
    2^-7 (1 + 2^-9) |x||w| each, summed."""
    P, g16, ws, ws32 = _aft_operands(dev, B, n)
    rm = B * n * 4
    W = P[AFT + "weights"].astype(np.float32)
    what = N(g16._aft_bt.float()).T                                               # [2048, 256]: what the streaming kernel multiplies with
    assert np.array_equal(what, BO.bf16_round(W))
    xhat = N(ws["fp"].float()).astype(np.float64)
    x = N(ws32["fp"]).astype(np.float64)
    assert np.array_equal(xhat.astype(np.float32), BO.bf16_round(N(ws32["fp"])))
    b = P[AFT + "biases"].astype(np.float64)
    w64 = what.astype(np.float64)
    p_hat = xhat @ w64
    z = np.maximum(p_hat + b, 0.0)
    mag = np.abs(xhat) @ np.abs(w64)
    slack = 2e-6 * mag + 1e-6 * (1 + np.abs(z))
    aft = N(ws["aft"]).astype(np.float64)
    worst = float((np.abs(aft - z) / slack).max())
    print("aft (%d, %d): worst |aft - z| / bound = %.3f" % (B, n, worst))
    assert np.all(np.abs(aft - z) <= slack)
    p = x @ W.astype(np.float64)
    bound = 2.0 ** -7 * (1 + 2.0 ** -9) * (np.abs(x) @ np.abs(W.astype(np.float64))) + slack
    print("aft (%d, %d): worst |x^.w^ - x.w| / bound = %.3f" % (B, n, float((np.abs(p_hat - p) / bound).max())))
    assert np.all(np.abs(p_hat - p) <= bound)
    if rm % 128 == 0:
        assert "sum" not in ws                     # the fine chain's loader forms (aft + skip) + nl
    else:
        assert torch.equal(ws["sum"], (ws["aft"] + ws["skip"]) + ws["nl"])


def test_stream_and_generic_kernel_agree(dev):
    """after_conv's two kernels on the same bf16 F' (the (1, 256) case): the streaming kernel on the packed weight image and the generic
    bf16 kernel on the fp32 weight round the same operands and add in the same order -- bit-identical."""
    from dispu_amd import _lib
    L = _lib.lib()
    P, g16, ws, _ = _aft_operands(dev, 1, 256)
    st = _lib.stream_ptr(dev)
    p = lambda t: t.data_ptr()
    w, b = g16.P[AFT + "weights"], g16.P[AFT + "biases"]
    y1, y2 = torch.zeros((1024, 256), device=dev), torch.zeros((1024, 256), device=dev)
    _lib.check(L.dispu_linear_bf16_stream(1024, 2048, 256, p(ws["fp"]), 2048, 1, p(g16._aft_bt), 2048, p(b), 1, p(y1), 256, 0, 1, 0, st), "stream")
    _lib.check(L.dispu_linear_bf16s(1, 1024, 2048, 256, p(ws["fp"]), 2048, 0, p(w), 256, 0, 0, p(b), 1, p(y2), 256, 0, None, 0, 0, 1, st), "bf16s")
    assert torch.equal(y1, y2) and torch.equal(y1, ws["aft"]) and bool((y1 > 0).any())


# ----------------------------------------------------------------------------- 4. end to end against the reference ----
def test_end_to_end_against_the_rounded_oracle(dev, monkeypatch):
    worst = 0.0
    for name, P, x in BO.cases():
        with monkeypatch.context() as m:
            BO.patch(m)
            oc, of = OG.generator_forward(P, x)
        c, f = _gen(dev, P)(torch.from_numpy(x).to(dev))
        assert np.array_equal(N(c), oc), name                       # bit for bit, as in fp32
        err = float(np.abs(N(f) - of).max())
        print("fine %s: max |gpu - reference| = %.3e (tolerance %.3e, recorded reference spread %.3e)" % (name, err, BO.FINE_TOL, BO.REF_SPREAD))
        worst = max(worst, err)
    assert worst <= BO.FINE_TOL


# -------------------------------------------------------------------------------------------------- 5. plumbing ----
def test_second_load_params_replaces_the_weight_image(dev):
    from dispu_amd import synth
    PA, PB = OG.init_params(seed=3, bias_scale=0.05), OG.init_params(seed=4, bias_scale=0.05)
    x = torch.from_numpy(synth.patches(2, 256, seed=21)).to(dev)
    gen = _gen(dev, PA)
    fa = N(gen(x)[1]).copy()
    gen.load_params(PB)
    c, f = gen(x)
    cb, fb = _gen(dev, PB)(x)
    assert torch.equal(c, cb) and torch.equal(f, fb)
    assert not np.array_equal(fa, N(f))


def test_chunking_fine_out_branches_and_repeat(dev):
    from dispu_amd import synth
    P = OG.init_params(seed=9, bias_scale=0.05, bn_random=True)
    x = torch.from_numpy(synth.patches(3, 256, seed=22)).to(dev)
    gen = _gen(dev, P)
    c0, f0 = gen(x)
    c1, f1 = gen(x)
    assert torch.equal(c0, c1) and torch.equal(f0, f1)                       # two runs
    small = _gen(dev, P)
    small.MAX_POINTS = 512                                                     # chunks of 2 + 1 patches
    c2, f2 = small(x)
    assert sorted(k for k in small._ws if isinstance(k[0], int)) == [(1, 256), (2, 256)]
    assert torch.equal(c0, c2) and torch.equal(f0, f2)
    buf = torch.zeros((3, 1024, 3), device=dev)
    gen.fine_out = buf
    _, f3 = gen(x)
    gen.fine_out = None
    assert torch.equal(buf, f0) and torch.equal(f3, f0)
    one = _gen(dev, P)
    one.branches = False
    c4, f4 = one(x)
    assert torch.equal(c0, c4) and torch.equal(f0, f4)
    # the producer-kernel twins of the head chains: (aft + skip) + nl by dispu_add3 instead of the fine chain's loader
    for attr in ("chain_inputs", "fused_heads"):
        twin = _gen(dev, P)
        setattr(twin, attr, False)
        c5, f5 = twin(x)
        assert "sum" in twin._ws[(3, 256)], attr
        assert torch.equal(c0, c5) and torch.equal(f0, f5), attr


def test_profile_labels(dev):
    from dispu_amd import synth
    P = OG.init_params(seed=9)
    for B, n, label in [(1, 256, "linear_bf16_stream[1024x2048x256]"), (2, 250, "linear_bf16s[2000x2048x256]")]:
        gen = _gen(dev, P)
        gen.profile = []
        gen(torch.from_numpy(synth.patches(B, n, seed=23)).to(dev))
        torch.cuda.synchronize()
        names = [p[0] for p in gen.profile]
        assert "ps_local_bf16" in names and label in names and "ps_local" not in names
        assert ("add3" in names) == (B * n * 4 % 128 != 0)
        from test_generator_gpu import _labels_follow_path
        path = gen.path(B, n)
        assert (path.local, path.after, path.add3) == ("bf16", {256: "bf16_stream", 250: "bf16s"}[n], n == 250)
        _labels_follow_path(names, path)


def test_b32_hipgraph_replay_equals_eager(b32, dev):
    s = b32["bf16"]
    gen, tx = s["gen"], b32["tx"]
    gen.return_views = True
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gen(tx)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gen(tx)
    ws = s["ws"]
    for _ in range(3):
        ws["coarse"].zero_()
        ws["fine"].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(N(ws["coarse"]), s["c"]) and np.array_equal(N(ws["fine"]), s["f"])
    gen.return_views = False


def test_value_errors(dev):
    from dispu_amd import synth
    from dispu_amd.generator import Generator
    P = OG.init_params(seed=9)
    with pytest.raises(ValueError, match="dtype"):
        Generator(params=P, device=dev, dtype="fp16")
    with pytest.raises(ValueError, match=r"Trainer\(dtype"):
        Generator(params=P, device=dev, dtype="bf16", is_training=True)
    x = torch.from_numpy(synth.patches(1, 256, seed=24)).to(dev)
    gen = _gen(dev, P)
    gen.split_bf16 = True
    with pytest.raises(ValueError, match="split_bf16"):
        gen(x)
    gen.split_bf16 = False
    gen.fused_local = False
    with pytest.raises(ValueError, match="fused_local"):
        gen(x)
    gen.fused_local = True
    gen(x)


# ------------------------------------------------------------------------------------------------------ 6. tool ----
def test_upsample_command_dtype(dev, tmp_path):
    """tools/upsample.py --dtype bf16 writes what upsample_ragged gives with a bf16 generator; --dtype f32 writes, byte for byte, what a
    run without the flag writes.  (The three runs go side by side.)"""
    from dispu_amd import checkpoint as CK
    from dispu_amd import upsample as U
    log_dir, data = tmp_path / "log", tmp_path / "data"
    (data / "test").mkdir(parents=True)
    log_dir.mkdir()
    CK.save_generator_params(str(log_dir / "model"), OG.init_params(seed=6, bias_scale=0.05), step=3)
    rng = np.random.default_rng(15)
    names, clouds = ["a_cloud", "b_cloud"], []
    for name, npt in zip(names, [300, 520]):
        v = rng.standard_normal((npt, 3))
        pc = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        np.savetxt(str(data / "test" / (name + ".xyz")), pc, fmt="%.6f")
        clouds.append(np.loadtxt(str(data / "test" / (name + ".xyz"))).astype(np.float32)[:, :3])
    _, gen = CK.restore_generator(str(log_dir), device=dev, dtype="bf16")
    assert gen.dtype == "bf16"
    want = {}
    for name, pred in zip(names, U.upsample_ragged(gen, clouds)):
        path = str(tmp_path / (name + "_ref.xyz"))
        U.save_xyz(path, pred)
        want[name] = open(path, "rb").read()
    cmd = [sys.executable, os.path.join(ROOT, "tools", "upsample.py"), "--log_dir", str(log_dir), "--data_dir", str(data)]
    runs = {"default": [], "f32": ["--dtype", "f32"], "bf16": ["--dtype", "bf16"]}
    procs = {k: subprocess.Popen(cmd + extra + ["--out_folder", str(tmp_path / k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for k, extra in runs.items()}
    for k, pr in procs.items():
        out, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, out.decode(errors="replace")
    read = lambda k, name: open(str(tmp_path / k / (name + "_X4.xyz")), "rb").read()
    for name in names:
        assert read("bf16", name) == want[name], name
        assert read("f32", name) == read("default", name), name
        assert read("f32", name) != read("bf16", name), name
