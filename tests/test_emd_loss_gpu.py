"""The EMD term of the training loss on the GPU (`10.0 * earth_mover(fine, gt, radius)`, DisPU/model.py:77), layer by layer:
dispu_approx_match_levels_ws + dispu_emd_loss_grad alone through the C ABI, dispu_pu_loss_finalize_e, and the Trainer with
TrainOpts.use_emd (loss head, the step without the term, tape, one epoch of tools/train.py).

Reference: tests/emd_oracle.py (float64 numpy, held to the C oracle and to a float64 autograd by tests/test_emd_oracle.py) as sums
over the `match` that dispu_approx_match_ws wrote for the same clouds in the same arith mode -- never an independently run auction:
single plan entries are ill-conditioned against 1-ulp exp differences, the sums over ONE plan are not.

Bounds: values 1e-5 relative; gradients 1e-5 of max |reference| (the project's rule, as check_loss_head of
tests/test_train_loss_gpu.py).  Inputs of the kernel cases: synth.patches as in test_approx_match_and_cost.

Measured on an MI355X (each test prints its own figures as `[measured]` lines), relative to the bound's scale:
  kernel alone (7 shapes x 2 arith modes)  cost 3.0e-8 .. 9.2e-8 against float64 and 0 .. 9.2e-8 against dispu_match_cost_ws; dpred
                            1.1e-7 .. 3.6e-7; radius NULL 6e-8 .. 3.6e-7; the scratch of levels_ws byte-identical to
                            approx_match_ws's and two runs bit-identical in every case
  pred on a gt point        both pairs carry match 1.0000; their rows' |dpred| 0 and 1.8e-34; dpred 1.9e-7, cost 3.3e-8
  finalize entry            every output <= 4.5e-7 (the largest: dis_fine_emd at b = 1500); pu_loss bit-equal to the fp32 restatement in all 32 cases
  loss head with the term   dis_fine_emd 1.1e-8 .. 1.0e-7, pu_loss <= 4.3e-8, dfine 1.8e-7 .. 3.5e-7, no row left out; the term's
                            gradient is 7e-6 .. 3.5e-5 of max |dfine| at emd_w = 10 and 0.81 / 0.88 of it at emd_w = 1e6
  dfine increment           (emd_w = 1e6) 3.8e-7 at weight_fine = 0.01, 4.1e-7 at 1.0; the composed value 0 .. 7.5e-8
  step without the term     terms, loss_vals, workspace keys and launch sequence identical; dfine: 146 of 6144 entries differ from the
                            Trainer without the field, 136 of 6144 between two runs of one unchanged Trainer (max 1.5e-5 of 59)
  taped vs eager            parameters after one Adam step: max 1.5e-3, 99 % quantile <= 1.9e-9 (f32 and bf16)"""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emd_oracle as EO  # noqa: E402
import uniform_oracle as UO  # noqa: E402

from oracle import generator as OG  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "train.py")
F32 = np.float32
INVALID = 1                     # hipErrorInvalidValue
CONTRACT, PINNED_EXP = 1, 2
SENT = -12345.0

_KEEP = []


def dv(a, dev, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del _KEEP[:]


def p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(0)


def N_(t):
    return t.detach().cpu().numpy()


def close(a, ref, rel, what=""):
    ref = np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(np.asarray(a, np.float64) - ref).max()
    print("[measured] %s: max err %.3e of scale %.3e = %.2e (bound %.0e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e > %.0e)" % (what, err, scale, err / scale, rel)


def each_close(a, ref, rel, what=""):
    """every entry relative to ITS reference (values: one cost per cloud)."""
    a, ref = np.asarray(a, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    err = np.abs(a / ref - 1.0).max()
    print("[measured] %s: worst rel err %.2e (bound %.0e)" % (what, err, rel))
    assert err <= rel, "%s: rel %.2e > %.0e (%s vs %s)" % (what, err, rel, a, ref)


def scalar_close(a, ref, rel, what=""):
    err = abs(float(a) - float(ref))
    print("[measured] %s: %.9g vs %.9g, rel err %.2e (bound %.0e)" % (what, float(a), float(ref), err / max(abs(float(ref)), 1e-300), rel))
    assert err <= rel * abs(float(ref)), "%s: %.9g vs %.9g" % (what, float(a), float(ref))


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


class Guarded(object):
    """a device buffer of `n` floats with `g` guard floats on either side; `fill` goes into the body (default: the sentinel)."""

    def __init__(self, dev, n, fill=None, g=64):
        self.n, self.g = n, g
        self.t = torch.full((n + 2 * g,), SENT, dtype=torch.float32, device=dev)
        if isinstance(fill, np.ndarray):
            self.t[g:g + n] = torch.from_numpy(np.ascontiguousarray(fill, F32).reshape(-1)).to(dev)
        elif fill is not None:
            self.t[g:g + n] = fill
        _KEEP.append(self.t)

    def ptr(self):
        return p(self.t, self.g)

    def body(self):
        return N_(self.t[self.g:self.g + self.n])

    def guards_intact(self):
        a = N_(self.t)
        return bool((a[:self.g] == SENT).all() and (a[self.g + self.n:] == SENT).all())

    def untouched(self):
        return bool((N_(self.t) == SENT).all())


def pattern(shape, scale):
    """a known non-zero start of dpred, of the gradient's own magnitude (its rounding stays far below the bound)."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((((i * 7) % 13) - 6) / 6.0 * scale).astype(F32).reshape(shape)


@functools.lru_cache(maxsize=None)
def clouds(b, n, m):
    from dispu_amd import synth
    if min(n, m) < 8:                 # the patch synthesiser normalises by the max radius: undefined for a single point
        rng = np.random.default_rng(n * 1000 + m)
        return rng.random((b, n, 3), dtype=F32), rng.random((b, m, 3), dtype=F32)
    return synth.patches(b, n, seed=n), synth.patches(b, m, seed=m + 1)


def radii(b):
    return np.linspace(0.5, 2.0, b).astype(F32) if b > 1 else np.array([0.5], F32)


def run_fused(dev, L, x1, x2, arith, radius, coef, start):
    """dispu_approx_match_ws (-> match, the scratch it leaves), dispu_approx_match_levels_ws into a second scratch, then
    dispu_emd_loss_grad on THAT scratch; every buffer guarded.  -> dict(match, temp_full, temp_levels, cost, dpred, scratch)"""
    lib, st = L.lib(), L.stream_ptr(dev)
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    t1, t2 = dv(x1, dev), dv(x2, dev)
    nt = lib.dispu_approx_match_scratch_bytes(b, n, m)
    assert nt % 4 == 0
    match = Guarded(dev, b * n * m)
    ta, tb = Guarded(dev, nt // 4), Guarded(dev, nt // 4)
    L.check(lib.dispu_approx_match_ws(b, n, m, p(t1), p(t2), match.ptr(), ta.ptr(), nt, arith, st), "approx_match_ws")
    L.check(lib.dispu_approx_match_levels_ws(b, n, m, p(t1), p(t2), tb.ptr(), nt, arith, st), "approx_match_levels_ws")
    ns = lib.dispu_emd_loss_grad_scratch_bytes(b, n, m)
    assert ns % 4 == 0 and ns > 0
    cost, dpred, sc = Guarded(dev, b), Guarded(dev, b * n * 3, fill=start), Guarded(dev, ns // 4)
    r = dv(radius, dev) if radius is not None else None
    L.check(lib.dispu_emd_loss_grad(b, n, m, p(t1), p(t2), tb.ptr(), p(r), coef, cost.ptr(), dpred.ptr(), sc.ptr(), ns, arith, st),
            "emd_loss_grad")
    torch.cuda.synchronize()
    for buf, name in ((match, "match"), (ta, "temp"), (tb, "temp (levels)"), (cost, "cost"), (dpred, "dpred"), (sc, "scratch")):
        assert buf.guards_intact(), "%s: written outside the buffer" % name
    return dict(match=match.body().reshape(b, m, n), temp_full=ta.body(), temp_levels=tb.body(), cost=cost.body(),
                dpred=dpred.body().reshape(b, n, 3), scratch=sc.body(), t1=t1, t2=t2)


# ------------------------------------------------------------------------------------- dispu_emd_loss_grad alone ----
KERNEL_SHAPES = [(2, 256, 256),      # one row block, several partner tiles
                 (1, 1024, 1024),    # the Trainer's own shape
                 (2, 300, 200), (2, 200, 300),   # tails, multiL / multiR != 1
                 (2, 129, 127),      # short tails on both sides
                 (3, 1, 5),          # a single point
                 (1, 1025, 1023)]    # either side of a block edge


@pytest.mark.parametrize("arith", [CONTRACT, CONTRACT | PINNED_EXP], ids=["hwexp", "pinned"])
@pytest.mark.parametrize("b,n,m", KERNEL_SHAPES, ids=["%dx%dx%d" % s for s in KERNEL_SHAPES])
def test_emd_loss_grad_kernel(dev, L, b, n, m, arith):
    """cost against float64 sums over the device's own match and against dispu_match_cost_ws on it; the accumulated gradient against
    float64; guards; the scratch of levels_ws byte-identical to the one approx_match_ws leaves; two runs bit-identical."""
    x1, x2 = clouds(b, n, m)
    radius, coef = radii(b), 10.0 * 0.5 / (b * m)
    first = run_fused(dev, L, x1, x2, arith, radius, coef, np.zeros((b, n, 3), F32))
    assert np.array_equal(first["temp_levels"].view(np.uint32), first["temp_full"].view(np.uint32)), "levels_ws leaves another scratch"
    ref = EO.emd_value_grad(x1, x2, first["match"], None)
    want = (coef / radius.astype(np.float64))[:, None, None] * ref["grad1"]
    assert np.abs(want).max() > 0 and ref["cost"].min() > 0
    start = pattern((b, n, 3), np.abs(want).max())
    out = run_fused(dev, L, x1, x2, arith, radius, coef, start)
    each_close(out["cost"], ref["cost"], 1e-5, "emd cost (%d, %d, %d) arith %d vs float64" % (b, n, m, arith))
    lib, st = L.lib(), L.stream_ptr(dev)
    mc = torch.empty((b,), dtype=torch.float32, device=dev)
    msc = torch.empty((max(lib.dispu_match_cost_scratch_bytes(b, n, m) // 4, 1),), dtype=torch.float32, device=dev)
    L.check(lib.dispu_match_cost_ws(b, n, m, p(out["t1"]), p(out["t2"]), p(dv(out["match"], dev)), p(mc), p(msc), arith & CONTRACT, st),
            "match_cost_ws")
    each_close(out["cost"], N_(mc), 1e-5, "emd cost (%d, %d, %d) arith %d vs dispu_match_cost_ws" % (b, n, m, arith))
    close(out["dpred"].astype(np.float64) - start.astype(np.float64), want, 1e-5, "emd dpred (%d, %d, %d) arith %d, accumulated" % (b, n, m, arith))
    # the gradient without the start, and the raw cost, do not depend on what dpred held: run to run bit-identical
    again = run_fused(dev, L, x1, x2, arith, radius, coef, start)
    for k in ("cost", "dpred", "scratch", "temp_levels"):
        assert np.array_equal(out[k].view(np.uint32), again[k].view(np.uint32)), "%s differs run to run" % k
    assert np.array_equal(first["cost"].view(np.uint32), out["cost"].view(np.uint32))
    # radius = NULL: the factor is coef
    bare = run_fused(dev, L, x1, x2, arith, None, coef, np.zeros((b, n, 3), F32))
    close(bare["dpred"], coef * ref["grad1"], 1e-5, "emd dpred (%d, %d, %d) arith %d, radius NULL" % (b, n, m, arith))
    assert np.array_equal(bare["cost"].view(np.uint32), out["cost"].view(np.uint32))


def test_prediction_on_a_ground_truth_point(dev, L):
    """pred[k] == gt[l] bit for bit in two places: d2 = 0 there, the pair's direction is 0 * rsqrt(1e-20) = 0 -- finite, and what the
    oracle's clamp rule gives."""
    x1, x2 = (a.copy() for a in clouds(2, 200, 200))
    x1[0, 5], x1[1, 150] = x2[0, 9], x2[1, 150]
    radius, coef = radii(2), 0.01
    out = run_fused(dev, L, x1, x2, CONTRACT, radius, coef, np.zeros((2, 200, 3), F32))
    assert np.isfinite(out["dpred"]).all() and np.isfinite(out["cost"]).all()
    assert out["match"][0, 9, 5] > 0 and out["match"][1, 150, 150] > 0, "the coincident pairs carry no mass: the clamp is not exercised"
    ref = EO.emd_value_grad(x1, x2, out["match"], None)
    want = (coef / radius.astype(np.float64))[:, None, None] * ref["grad1"]
    print("[measured] coincident pairs: match %.4f, %.4f; their rows' |dpred| %.3e, %.3e of max %.3e" %
          (out["match"][0, 9, 5], out["match"][1, 150, 150], np.abs(out["dpred"][0, 5]).max(), np.abs(out["dpred"][1, 150]).max(), np.abs(want).max()))
    close(out["dpred"], want, 1e-5, "coincident points dpred")
    each_close(out["cost"], ref["cost"], 1e-5, "coincident points cost")


def test_emd_entries_refuse_invalid_arguments(dev, L):
    lib, st = L.lib(), L.stream_ptr(dev)
    b, n, m = 2, 300, 200
    x1, x2 = (dv(a, dev) for a in clouds(b, n, m))
    nt, ns = lib.dispu_approx_match_scratch_bytes(b, n, m), lib.dispu_emd_loss_grad_scratch_bytes(b, n, m)
    temp, sc, cost, dp = Guarded(dev, nt // 4), Guarded(dev, ns // 4), Guarded(dev, b), Guarded(dev, b * n * 3)
    rad = dv(radii(b), dev)

    def levels(b_=b, n_=n, m_=m, t=temp.ptr(), nb=nt):
        return lib.dispu_approx_match_levels_ws(b_, n_, m_, p(x1), p(x2), t, nb, CONTRACT, st)

    def fused(b_=b, n_=n, m_=m, a1=p(x1), a2=p(x2), t=temp.ptr(), c=cost.ptr(), d=dp.ptr(), s=sc.ptr(), nb=ns):
        return lib.dispu_emd_loss_grad(b_, n_, m_, a1, a2, t, p(rad), 0.5, c, d, s, nb, CONTRACT, st)
    assert levels(t=None) == INVALID and levels(nb=nt - 4) == INVALID and levels(nb=0) == INVALID
    assert levels(b_=-1) == INVALID and levels(n_=0) == INVALID and levels(m_=0) == INVALID and levels(b_=65536) == INVALID
    assert levels(b_=0) == 0 and levels(b_=0, t=None, nb=0) == 0
    assert fused(t=None) == INVALID and fused(nb=ns - 4) == INVALID and fused(nb=0) == INVALID and fused(s=None) == INVALID
    assert fused(c=None) == INVALID and fused(d=None) == INVALID and fused(a1=None) == INVALID and fused(a2=None) == INVALID
    assert fused(b_=-1) == INVALID and fused(n_=0) == INVALID and fused(m_=-2) == INVALID
    assert fused(b_=0) == 0 and fused(b_=0, t=None, s=None, nb=0) == 0
    torch.cuda.synchronize()
    for buf, name in ((temp, "temp"), (sc, "scratch"), (cost, "cost"), (dp, "dpred")):
        assert buf.untouched(), "a refused (or empty) call wrote to %s" % name
    fin = lambda cd=p(sc.t), rep=None, nrep=0, up=None, nl=0, nu=0, ec=p(sc.t), b_=2, m_=8, out=p(sc.t, 16): \
        lib.dispu_pu_loss_finalize_e(cd, rep, nrep, 0.5, 1.0, up, nl, nu, 10.0, ec, p(rad), b_, m_, 10.0, out, st)
    assert fin(cd=None) == INVALID and fin(out=None) == INVALID and fin(ec=None) == INVALID and fin(b_=0) == INVALID and fin(m_=0) == INVALID
    assert fin(rep=p(sc.t), nrep=0) == INVALID and fin(up=p(sc.t), nl=0, nu=5) == INVALID and fin(up=p(sc.t), nl=9, nu=5) == INVALID
    assert fin(up=p(sc.t), nl=5, nu=0) == INVALID
    torch.cuda.synchronize()
    assert sc.untouched(), "a refused finalize wrote to its buffers"


# ---------------------------------------------------------------------------------------- dispu_pu_loss_finalize_e ----
def run_finalize_e(dev, L, cd, rep, nrep, wf, rep_w, upart, nl, nu, uniform_w, cost, radius, b, m, emd_w):
    """as the trainer calls it: cd = loss_vals[0:2], out = loss_vals + 2 (9 floats, guards follow) -> out[0..6]"""
    lv = Guarded(dev, 9, g=8)
    lv.t[lv.g:lv.g + 2] = torch.from_numpy(np.asarray(cd, F32)).to(dev)
    L.check(L.lib().dispu_pu_loss_finalize_e(lv.ptr(), p(rep), nrep, wf, rep_w, p(upart), nl, nu, uniform_w, p(cost), p(radius), b, m, emd_w,
                                             p(lv.t, lv.g + 2), L.stream_ptr(dev)), "pu_loss_finalize_e")
    torch.cuda.synchronize()
    body = lv.body()
    assert lv.guards_intact(), "pu_loss_finalize_e wrote past out[6]"
    assert np.array_equal(body[:2], np.asarray(cd, F32)), "cd[0..1] did not survive the aliased call"
    return body[2:9]


@pytest.mark.parametrize("b", [1, 2, 28, 1500])
def test_pu_loss_finalize_e(dev, L, b):
    rng = np.random.default_rng(300 + b)
    nrep, nl, nu, m = 2048, 5, 51, 1024
    rep = rng.uniform(0.0, 4e-3, nrep).astype(F32)
    upart = rng.uniform(0.0, 0.5, nl * nu).astype(F32)
    cost = rng.uniform(20.0, 60.0, b).astype(F32)
    radius = rng.uniform(0.5, 2.0, b).astype(F32)
    trep = dv(np.concatenate([rep, np.full(64, 1e6, F32)]), dev)          # anything read past the end would show
    tup = dv(np.concatenate([upart, np.full(64, 1e6, F32)]), dev)
    tc, tr = dv(np.concatenate([cost, np.full(64, 1e9, F32)]), dev), dv(np.concatenate([radius, np.full(64, 1e-9, F32)]), dev)
    for wf in (0.01, 1.0):
        for with_rep in (True, False):
            for with_u in (True, False):
                cd = rng.uniform(1e-3, 5e-2, 2).astype(F32)
                r, n = (trep, nrep) if with_rep else (None, 0)
                out = run_finalize_e(dev, L, cd, r, n, wf, 0.5, tup if with_u else None, nl, nu, 10.0, tc, tr, b, m, 10.0)
                ref = EO.pu_loss_terms_e(cd[0], cd[1], rep if with_rep else None, n, F32(wf), 0.5, upart if with_u else None, 10.0,
                                         cost, radius, m, 10.0)
                what = "finalize_e out[%%d] b=%d wf=%g rep=%s uniform=%s" % (b, wf, with_rep, with_u)
                for j in (0, 1, 2, 3, 5, 6):
                    if ref[j] == 0.0:
                        assert out[j] == 0.0, (j, out[j])
                    else:
                        scalar_close(out[j], ref[j], 1e-5, what % j)
                assert out[4] == F32(wf)
                # pu_loss IS the stated fp32 expression of the entry's own outputs: ((c + wf (f + e)) + r) [+ u]
                pu = EO.pu_loss_f32(out[0], out[1], out[6], out[2], out[5] if with_u else None, wf)
                assert F32(pu).tobytes() == F32(out[3]).tobytes(), (pu, out[3])
                # without the uniform partials the first five outputs at emd_w = 0 are dispu_pu_loss_finalize's, bit for bit
                if not with_u:
                    zero = run_finalize_e(dev, L, cd, r, n, wf, 0.5, None, 0, 0, 0.0, tc, tr, b, m, 0.0)
                    plain = Guarded(dev, 8, g=8)
                    plain.t[plain.g:plain.g + 2] = torch.from_numpy(cd).to(dev)
                    L.check(L.lib().dispu_pu_loss_finalize(plain.ptr(), p(r), n, wf, 0.5, p(plain.t, plain.g + 2), L.stream_ptr(dev)), "pu_loss_finalize")
                    torch.cuda.synchronize()
                    assert np.array_equal(zero[:5].view(np.uint32), plain.body()[2:7].view(np.uint32)) and zero[5] == 0.0 and zero[6] == 0.0
    # radius = NULL is radius 1
    cd = np.array([0.01, 0.02], F32)
    out = run_finalize_e(dev, L, cd, None, 0, 1.0, 0.5, None, 0, 0, 0.0, tc, None, b, m, 10.0)
    scalar_close(out[6], EO.emd_value(cost, None, m, 10.0), 1e-5, "finalize_e, radius NULL, b=%d" % b)


# ------------------------------------------------------------------------------------------------- the Trainer ----
FIRST_EPOCH, LAST_STAGE = 5, 35          # weight_fine 0.01 (its first-epoch value) and 1.0


def make_trainer(dev, epoch, opts=None, dtype="f32", **flags):
    from dispu_amd.train import Trainer, TrainOpts
    if opts is None:
        opts = TrainOpts()
        opts.use_emd = True
        for k, v in flags.items():
            setattr(opts, k, v)
    tr = Trainer(opts=opts, params=OG.init_params(seed=1234, bias_scale=0.05, bn_random=True), device=dev, dtype=dtype)
    tr.epoch = epoch
    return tr


def loss_head(dev, tr, B, N, seed):
    from dispu_amd import synth
    x, gt = synth.patch_with_gt(B, N, 4 * N, seed=seed)
    radius = np.random.default_rng(1000 + seed).uniform(0.5, 2.0, B).astype(F32)
    tr.zero_grad()
    tr.forward(dv(x, dev))
    terms = tr.loss_backward(dv(gt, dev), dv(radius, dev))
    torch.cuda.synchronize()                    # read dfine BEFORE backward(), which adds it into dcoarse
    return gt, radius, terms


def device_match(dev, fine, gt):
    """the plan of (fine, gt) as dispu_approx_match_ws writes it in the Trainer's arith mode: the same 21 auction launches on the same
    inputs as the Trainer's levels_ws call (run-to-run identical, test_emd_loss_grad_kernel), then the assembly."""
    from dispu_amd.tf_approxmatch import approx_match
    return N_(approx_match(dv(fine, dev), dv(gt, dev)))


def check_emd_loss_head(dev, tr, B, N, gt, radius, terms, what):
    """float64 Chamfer + repulsion (the reference test_loss_head builds from loss_oracle) [+ uniform] + EMD on the device's own match,
    at the device's own fine cloud; then the composed loss_utils.earth_mover and its autograd on the same cloud."""
    import test_train_loss_gpu as TL
    from dispu_amd import loss_utils as LU
    from dispu_amd.train import weight_fine
    ws = tr._ws[(B, N)]
    wf, ew = weight_fine(tr.epoch), float(tr.opts.emd_w)
    uniform = bool(tr.opts.use_uniform)
    ref = TL.loss_head_reference(ws, gt, radius, wf, tr.opts.use_repulse, float(tr.opts.repulsion_w))
    del TL._KEEP[:]
    fine = N_(ws["fine"]).reshape(B, -1, 3)
    M = fine.shape[1]
    emd = EO.emd_value_grad(fine, gt, device_match(dev, fine, gt), radius, ew, wf)
    each_close(N_(ws["emd_cost"]), emd["cost"], 1e-5, "%s raw cost per cloud" % what)
    want = dict(dis_coarse_cd=ref["terms"][0], dis_fine_cd=ref["terms"][1], repulsion_loss=ref["terms"][2], dis_fine_emd=emd["value"],
                pu_loss=ref["terms"][3] + wf * emd["value"])
    dfine, skip = ref["dfine"] + emd["grad"], ref["skip"]
    if uniform:
        uw = float(tr.opts.uniform_w)
        lv = UO.host_levels(M)
        seeds = O.farthest_point_sample(lv["npoint"], fine, contract=CONTRACT)
        new_xyz = O.gather_point(fine, seeds)
        slots = [O.query_ball_point(r, ns, fine, new_xyz, contract=CONTRACT)[0] for r, ns in zip(lv["r"], lv["ns"])]
        res = UO.uniform_value_grad(fine, slots, scale=uw)
        want.update(uniform_loss=uw * res["value"], pu_loss=want["pu_loss"] + uw * res["value"])
        dfine, skip = dfine + res["grad"], skip | UO.near_tie_rows(res, slots, (B, M), 1e-5)
    assert float(terms["weight_fine"]) == wf and set(terms) == set(want) | {"weight_fine"}
    for k, r in want.items():
        if r == 0.0:
            assert float(terms[k]) == 0.0, k
        else:
            scalar_close(float(terms[k]), r, 1e-5, "%s %s" % (what, k))
    assert want["dis_fine_emd"] > 0
    print("[measured] %s: %d of %d dfine rows left out (Chamfer / repulsion / uniform branch ties); EMD share of max |dfine| %.2e" %
          (what, int(skip.sum()), skip.size, np.abs(emd["grad"]).max() / np.abs(dfine).max()))
    assert skip.sum() <= 1e-3 * skip.size
    got = N_(ws["dfine"]).reshape(B, M, 3).astype(np.float64)
    keep = ~skip
    err = np.abs(got - dfine)[keep].max()
    print("[measured] %s dfine: max err %.3e of scale %.3e = %.2e (bound 1e-05)" % (what, err, np.abs(dfine).max(), err / np.abs(dfine).max()))
    assert err <= 1e-5 * np.abs(dfine).max()
    # the composed form: emd_w * loss_utils.earth_mover(fine, gt, radius) and its autograd (weighted by weight_fine like the term)
    x = dv(fine, dev).requires_grad_(True)
    v = ew * LU.earth_mover(x, dv(gt, dev), radius=dv(radius, dev))
    (g,) = torch.autograd.grad(wf * v, x)
    scalar_close(float(terms["dis_fine_emd"]), float(v.detach()), 1e-5, "%s dis_fine_emd vs emd_w * loss_utils.earth_mover" % what)
    close(N_(g), emd["grad"], 1e-5, "%s autograd of the composed term vs float64" % what)


SEEDS = {FIRST_EPOCH: 75, LAST_STAGE: 62}   # patches on which loss_head_reference (the existing float64 Chamfer + repulsion reference) finds
                                            # no repulsion row within 1e-5 of a branch, judged on the reference alone (it refuses more than 2)


@pytest.mark.parametrize("epoch,use_repulse,use_uniform", [(FIRST_EPOCH, True, False), (LAST_STAGE, True, False), (LAST_STAGE, False, False),
                                                           (FIRST_EPOCH, False, True), (LAST_STAGE, True, True)])
def test_loss_head_with_emd(dev, epoch, use_repulse, use_uniform):
    B, N = 2, 256
    tr = make_trainer(dev, epoch, use_repulse=use_repulse, use_uniform=use_uniform)
    gt, radius, terms = loss_head(dev, tr, B, N, seed=SEEDS[epoch])
    check_emd_loss_head(dev, tr, B, N, gt, radius, terms, "emd loss head epoch %d repulse=%s uniform=%s" % (epoch, use_repulse, use_uniform))


@pytest.mark.parametrize("epoch", [FIRST_EPOCH, LAST_STAGE])
def test_dfine_increment_is_the_composed_terms_gradient(dev, epoch):
    """dfine with the term minus dfine without it (the same forward, the loss head once more with use_emd = False) against the
    autograd of weight_fine * emd_w * loss_utils.earth_mover(fine, gt, radius), 1e-5 of its largest entry.

    At emd_w = 10 this difference cannot be resolved in the fp32 buffer the term is accumulated into: the term's gradient is 2e-5 ..
    4e-5 of max |dfine| (printed by test_loss_head_with_emd: 2.8e-3 against 80 at weight_fine = 1), so the bound, 1e-5 of ITS largest
    entry = 2.8e-8, lies below half an ulp of the entries it is added to (ulp(80) = 7.6e-6), and the two runs' Chamfer atomics differ
    by more than that as well (measured: max |difference - autograd| 3.2e-5 = 1.1e-2 of the term's scale).  The term is linear in
    emd_w, so the increment is taken at emd_w = 1e6, where it is the larger part of dfine and fp32 resolves it: everything the Trainer
    does to the term (coef = emd_w * weight_fine / (B * M), radius, the accumulation behind the Chamfer gradient) is in it."""
    from dispu_amd import loss_utils as LU
    from dispu_amd.train import weight_fine
    B, N, ew = 2, 256, 1e6
    tr = make_trainer(dev, epoch, emd_w=ew)
    gt, radius, terms = loss_head(dev, tr, B, N, seed=SEEDS[epoch])
    ws, wf = tr._ws[(B, N)], weight_fine(epoch)
    check_emd_loss_head(dev, tr, B, N, gt, radius, terms, "emd loss head epoch %d, emd_w = 1e6" % epoch)      # float64, the term now dominant
    on = N_(ws["dfine"]).reshape(B, -1, 3).astype(np.float64)
    tr.opts.use_emd = False
    off_terms = tr.loss_backward(dv(gt, dev), dv(radius, dev))
    torch.cuda.synchronize()
    off = N_(ws["dfine"]).reshape(B, -1, 3).astype(np.float64)
    tr.opts.use_emd = True
    assert "dis_fine_emd" not in off_terms and float(off_terms["dis_fine_cd"]) == float(terms["dis_fine_cd"])
    x = dv(N_(ws["fine"]).reshape(B, -1, 3), dev).requires_grad_(True)
    v = ew * LU.earth_mover(x, dv(gt, dev), radius=dv(radius, dev))
    (g,) = torch.autograd.grad(wf * v, x)
    what = "epoch %d, emd_w = 1e6" % epoch
    scalar_close(float(terms["dis_fine_emd"]), float(v.detach()), 1e-5, "%s dis_fine_emd vs emd_w * loss_utils.earth_mover" % what)
    scalar_close(float(terms["pu_loss"]), float(off_terms["pu_loss"]) + wf * float(v.detach()), 1e-5, "%s pu_loss vs the step without + wf * term" % what)
    print("[measured] %s: max |increment| %.3e, max |dfine without the term| %.3e" % (what, np.abs(on - off).max(), np.abs(off).max()))
    close(on - off, N_(g).astype(np.float64), 1e-5, "%s dfine increment vs the composed term's autograd" % what)


def test_emd_weight_scales_the_term_only(dev):
    tr = make_trainer(dev, LAST_STAGE, emd_w=2.5)
    gt, radius, terms = loss_head(dev, tr, 2, 256, seed=62)
    check_emd_loss_head(dev, tr, 2, 256, gt, radius, terms, "emd loss head, emd_w = 2.5")
    tr10 = make_trainer(dev, LAST_STAGE)
    _, _, t10 = loss_head(dev, tr10, 2, 256, seed=62)
    scalar_close(float(t10["dis_fine_emd"]), 4.0 * float(terms["dis_fine_emd"]), 1e-5, "emd_w 10 vs 2.5")
    assert float(t10["dis_fine_cd"]) == float(terms["dis_fine_cd"]) and float(t10["repulsion_loss"]) == float(terms["repulsion_loss"])


def _launch_signature(tr, gt, radius):
    """the launches of one more loss_backward on the current forward, as a launch tape records them: (entry, every non-pointer
    argument) in submission order (pointers differ from Trainer to Trainer, nothing else may)."""
    from dispu_amd import _lib
    _lib.tape_begin()
    try:
        tr.loss_backward(gt, radius)
    finally:
        tape = _lib.tape_end()
    torch.cuda.synchronize()
    return [(name, tuple(a.value for a in cargs if not isinstance(a, C.c_void_p))) for _, cargs, name in tape.calls]


def test_emd_off_is_the_step_without_the_field(dev):
    """use_emd = False against a Trainer whose options do not have the field at all: the same launches with the same scalar arguments
    in the same order, loss terms and loss_vals bit-identical, no EMD entry in the terms, the same workspace keys (no new buffer).

    dfine: bit-identity cannot be asked of it, with or without this term -- the Chamfer and repulsion gradients are accumulated with
    float atomics (chamfer_grad_kernel, repulsion_loss_grad_kernel) and two runs of ONE unchanged Trainer already differ in ~2 % of
    the entries (tests/test_uniform_loss_gpu.py:test_uniform_off_is_the_step_without_the_field measured 142 of 6144; both figures are
    printed below).  The launch sequence IS identical, so dfine is held to what a re-ordered fp32 sum allows: every entry within
    (k - 1) 2^-23 of the largest |entry| for the at most k = 32 contributions a row collects."""
    from dispu_amd.generator import _Opts
    from dispu_amd.train import TrainOpts

    class OldOpts(_Opts):                      # the training-side options as they were before the EMD term
        base_lr_g, beta, lr_decay, decay_step, lr_decay_rate, lr_clip, use_repulse, repulsion_w = 0.001, 0.9, True, 30, 0.7, 1e-6, True, 1.0
        use_uniform, uniform_w = False, 10.0
    assert not hasattr(OldOpts(), "use_emd") and TrainOpts.use_emd is False and TrainOpts.emd_w == 10.0
    outs = []
    for opts in (OldOpts(), OldOpts(), None):
        tr = make_trainer(dev, 25, opts=opts, use_emd=False)
        gt, radius, terms = loss_head(dev, tr, 2, 256, seed=61)
        ws = tr._ws[(2, 256)]
        assert "dis_fine_emd" not in terms and not any(k.startswith("emd") for k in ws)
        out = ({k: float(v) for k, v in terms.items()}, N_(ws["dfine"]).copy(), N_(ws["loss_vals"]).copy(), sorted(ws))
        outs.append(out + (_launch_signature(tr, dv(gt, dev), dv(radius, dev)),))
    old, old2, new = outs
    assert old[0] == new[0]
    assert np.array_equal(old[2].view(np.uint32), new[2].view(np.uint32))
    assert old[3] == new[3], "the workspace gained or lost a buffer with use_emd = False"
    assert len(new[4]) > 8 and old[4] == new[4], "the launch sequence changed with use_emd = False"
    assert not any("emd" in name or "levels" in name or name == "dispu_pu_loss_finalize_e" for name, _ in new[4])
    top = float(np.abs(old[1]).max())
    for what, a, b in (("one unchanged Trainer, run to run", old[1], old2[1]), ("without the field vs use_emd = False", old[1], new[1])):
        same = a.view(np.uint32) == b.view(np.uint32)
        print("[measured] dfine, %s: %d of %d entries differ, max |diff| %.3e of max |dfine| %.3e" %
              (what, int((~same).sum()), same.size, float(np.abs(a - b).max()), top))
    assert float(np.abs(old[1] - new[1]).max()) <= 31 * 2.0 ** -23 * top


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_taped_step_equals_eager_step_with_emd(dev, dtype):
    """train_step_taped == train_step with the term on (the tolerances of test_taped_steps_equal_eager_steps): parameters after one
    Adam step; the tape's key holds use_emd and emd_w."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer, TrainOpts
    P = OG.init_params(seed=22, bias_scale=0.05, bn_random=True)
    B = 4
    rs = torch.ones(B, device=dev)
    e, g = Trainer(TrainOpts(), params=P, device=dev, dtype=dtype), Trainer(TrainOpts(), params=P, device=dev, dtype=dtype)
    for t in (e, g):
        t.opts.use_emd, t.epoch = True, 20
    gtol = 2e-5 if dtype == "f32" else 2e-3
    for i in range(3):
        if i == 2:
            e.opts.emd_w = g.opts.emd_w = 2.5            # a new key: a new tape
        x, gt = synth.patch_with_gt(B, 256, 1024, seed=40 + i)
        for name in ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var"):
            getattr(g, name).copy_(getattr(e, name))
        g.adam_t, g.global_step = e.adam_t, e.global_step
        xs, gs = dv(x, dev), dv(gt, dev)
        te = e.train_step(xs, gs, rs)
        tg = g.train_step_taped(xs, gs, rs)
        torch.cuda.synchronize()
        assert "dis_fine_emd" in te and "dis_fine_emd" in tg and float(te["dis_fine_emd"]) > 0
        assert te["dis_fine_emd"].dtype == torch.float32 and te["pu_loss"].dtype == torch.float32       # the loss stays fp32
        floor = 4e-7 * float(e.flat_g.abs().max())
        for k in e.G:
            scale = float(e.G[k].abs().max()) + 1e-12
            assert float((g.G[k] - e.G[k]).abs().max()) <= gtol * scale + floor + 2e-6, (i, k)
        for k in te:
            a, b = float(te[k]), float(tg[k])
            assert abs(a - b) <= (1e-5 if dtype == "f32" else 1e-2) * max(1.0, abs(a)), (i, k, a, b)
        diff = N_((g.flat_p - e.flat_p).abs())
        print("[measured] taped vs eager with emd (%s) step %d: params max %.2e q99 %.2e; dis_fine_emd %.6g" %
              (dtype, i, diff.max(), np.quantile(diff, 0.99), float(te["dis_fine_emd"])))
        assert diff.max() <= 2.5e-3 and np.quantile(diff, 0.99) <= (2e-5 if dtype == "f32" else 1e-3)
    assert len(g._tapes) == 2
    assert sorted(k[6:8] for k in g._tapes) == [(True, 2.5), (True, 10.0)]


def test_train_tool_epoch_with_the_emd_flag(tmp_path, dev):
    """tools/train.py --use_emd true in a fresh process on the committed 4-patch HDF5 file (B = 1 -> 3 steps): the epoch's line in
    log_train.txt ends in a finite, positive dis_fine_emd column, args.txt names the flags, a checkpoint is written."""
    from dispu_amd import checkpoint as CK, h5
    h5.lib()
    data = tmp_path / "data"
    data.mkdir()
    shutil.copy(os.path.join(ROOT, "tests", "golden", "patches_small.h5"), str(data / "PUGAN_poisson_256_poisson_1024.h5"))
    log_dir = str(tmp_path / "log")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, TOOL, "--data_dir", str(data), "--log_dir", log_dir, "--batch_size", "1",
                        "--epoch_per_save", "1", "--seed", "3", "--training_epoch", "1", "--use_emd", "true"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    lines = [l for l in open(os.path.join(log_dir, "log_train.txt")).read().splitlines() if l.startswith("epoch ")]
    assert len(lines) == 1 and lines[0] in out
    m = re.fullmatch(r"epoch 0001 g_loss=(\d+\.\d+)  coarse_cd=\S+  coarse_hd=\S+  fine_cd=(\d+\.\d+) fine_hd=\S+  time=\S+  dis_fine_emd=(\d+\.\d+)",
                     lines[0])
    assert m, lines[0]
    g_loss, fine_cd, emd = (float(v) for v in m.groups())
    print("[measured] train tool with --use_emd true: g_loss %.6f fine_cd %.6f dis_fine_emd %.6f" % (g_loss, fine_cd, emd))
    assert np.isfinite(emd) and emd > 0 and g_loss > 0.01 * emd            # weight_fine is 0.01 in the first epoch
    args = open(os.path.join(log_dir, "args.txt")).read().splitlines()
    assert "use_emd: True" in args and "emd_w: 10.0" in args and args == sorted(args)
    assert CK.pre_load_checkpoint(log_dir)[0] == 1 and os.path.exists(os.path.join(log_dir, "model-1.index"))
