"""The uniform term of the training loss on the GPU (Common/loss_utils.py:238-267, DisPU/model.py:86), layer by layer:
dispu_uniform_loss_grad alone through the C ABI, hand-built clouds, dispu_pu_loss_finalize_u, loss_utils.get_uniform_loss, and the
Trainer with TrainOpts.use_uniform (loss head, tape, one fit epoch).

References: tests/uniform_oracle.py (float64 numpy, held to an autograd restatement of the reference's graph at 1e-8 by
tests/test_uniform_oracle.py) on seeds and ball-query slots of the project's CPU oracle (oracle/oracle.py), which the device's own
seeds and slots must equal bit for bit.

Bounds: value partials and values 1e-5 relative; gradients 1e-5 of max |reference| (the project's rule, as check_loss_head of
tests/test_train_loss_gpu.py).  Rows touched by a slot whose float64 partner gap is below 1e-5 may be left out (an fp32 evaluation
may legitimately take the other partner there); they must be at most 0.1 % of the rows and are 0 on these inputs.

Inputs of the random cases: loss_oracle.jittered_pair.

Measured on an MI355X (each test prints its own figures as `[measured]` lines), relative to the bound's scale:
  kernel alone              partials 6.3e-8 .. 2.7e-7, value 1.9e-8 .. 1.8e-7, dpcd 1.6e-7 .. 4.4e-7; seeds, slots and counts equal
                            to the oracle's and to dispu_query_ball's in every case; smallest partner gap 2.3e-4: no row left out
  constructed cases         dpcd 3.3e-8 (exact tie), 1.7e-7 (full / nearly full balls); lone seed and coincident points exact zeros
  get_uniform_loss          value 4.0e-8, autograd 1.5e-7; against the composed ops 1.9e-7 / 2.3e-7
  loss head with the term   uniform_loss 7e-9 .. 1.6e-7, dfine 2.1e-7 .. 4.5e-7, no row left out
  taped vs eager            parameters after one Adam step: max 1.7e-3, 99 % quantile 1e-9"""
import ctypes as C
import functools
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_oracle as LO  # noqa: E402
import uniform_oracle as UO  # noqa: E402

from oracle import generator as OG  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID = 1                     # hipErrorInvalidValue
CONTRACT = 1
TIE = 1e-5
SENT = -12345.0
ISENT = -777

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


def close(a, ref, rel, what="", keep=None):
    ref = np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    d = np.abs(np.asarray(a, np.float64) - ref)
    err = (d[keep] if keep is not None else d).max()
    print("[measured] %s: max err %.3e of scale %.3e = %.2e (bound %.0e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e > %.0e)" % (what, err, scale, err / scale, rel)


def scalar_close(a, ref, rel, what=""):
    err = abs(float(a) - float(ref))
    print("[measured] %s: %.9g vs %.9g, rel err %.2e (bound %.0e)" % (what, float(a), float(ref), err / max(abs(float(ref)), 1e-300), rel))
    assert err <= rel * abs(float(ref)), "%s: %.9g vs %.9g" % (what, float(a), float(ref))


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


class Guarded(object):
    """a device buffer of `n` 4-byte elements with `g` guard elements on either side; `fill` goes into the body."""

    def __init__(self, dev, n, fill=None, g=64, dtype=torch.float32):
        self.n, self.g = n, g
        self.sent = SENT if dtype == torch.float32 else ISENT
        self.t = torch.full((n + 2 * g,), self.sent, dtype=dtype, device=dev)
        if isinstance(fill, np.ndarray):
            self.t[g:g + n] = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).to(dev).to(dtype)
        elif fill is not None:
            self.t[g:g + n] = fill
        _KEEP.append(self.t)

    def ptr(self):
        return p(self.t, self.g)

    def body(self):
        return N_(self.t[self.g:self.g + self.n])

    def guards_intact(self):
        a = N_(self.t)
        return bool((a[:self.g] == self.sent).all() and (a[self.g + self.n:] == self.sent).all())


class Tables(object):
    """hand-built host tables of dispu_uniform_loss_grad: ns [L] int32, levels [L][4] float32 = r | e | value factor | gradient factor."""

    def __init__(self, npoint, ns, r, e, vfac, gfac):
        L_ = len(ns)
        self.nlevels, self.npoint, self.ns_list, self.slots = L_, npoint, list(ns), sum(ns)
        self.ns = (C.c_int * L_)(*ns)
        self.levels = (C.c_float * (4 * L_))(*[v for row in zip(r, e, vfac, gfac) for v in row])


def run_kernel(dev, L, pcd, seeds, tab, prefill=None, slots=True, arith=CONTRACT):
    """one dispu_uniform_loss_grad launch on guarded buffers -> dict(partial [L, balls], dpcd | None (prefill: the buffer's start; None:
    dpcd = NULL), idx [per level [B, S, ns]] | None, cnt [L, B, S] | None); every guard is checked."""
    B, n, _ = pcd.shape
    S, Lv = tab.npoint, tab.nlevels
    balls = B * S
    part = Guarded(dev, Lv * balls)
    dp = Guarded(dev, B * n * 3, fill=np.asarray(prefill, F32)) if prefill is not None else None
    gi = Guarded(dev, balls * tab.slots, fill=ISENT, dtype=torch.int32) if slots else None
    gc = Guarded(dev, Lv * balls, dtype=torch.int32) if slots else None
    x, s = dv(pcd, dev), dv(seeds, dev, torch.int32)
    L.check(L.lib().dispu_uniform_loss_grad(B, n, S, Lv, C.addressof(tab.ns), C.addressof(tab.levels), p(x), p(s), part.ptr(),
                                            dp.ptr() if dp else None, gi.ptr() if gi else None, gc.ptr() if gc else None, arith,
                                            L.stream_ptr(dev)), "uniform_loss_grad")
    torch.cuda.synchronize()
    for buf, name in ((part, "partial"), (dp, "dpcd"), (gi, "idx_out"), (gc, "cnt_out")):
        assert buf is None or buf.guards_intact(), "%s: written outside the buffer" % name
    out = dict(partial=part.body().reshape(Lv, balls), dpcd=dp.body().reshape(B, n, 3) if dp else None, idx=None, cnt=None)
    if slots:
        flat, off, out["idx"] = gi.body(), 0, []
        for ns in tab.ns_list:
            out["idx"].append(flat[off:off + balls * ns].reshape(B, S, ns))
            off += balls * ns
        out["cnt"] = gc.body().reshape(Lv, B, S)
    return out


def pattern(shape, scale):
    """a known non-zero start of dpcd, of the gradient's own magnitude (its rounding stays far below the bound)."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((((i * 7) % 13) - 6) / 6.0 * scale).astype(F32).reshape(shape)


@functools.lru_cache(maxsize=None)
def cloud(B, N, seed):
    return LO.jittered_pair(B, N, N, seed)[1]


@functools.lru_cache(maxsize=None)
def host_reference(B, N, percentages, seed, scale):
    """pcd, host levels, the oracle's seeds / slots / counts, and the float64 value and gradient on them (computed once per case)."""
    pcd = cloud(B, N, seed)
    lv = UO.host_levels(N, list(percentages))
    seeds = O.farthest_point_sample(lv["npoint"], pcd, contract=CONTRACT)
    new_xyz = O.gather_point(pcd, seeds)
    slots, cnts = [], []
    for r, ns in zip(lv["r"], lv["ns"]):
        idx, cnt = O.query_ball_point(r, ns, pcd, new_xyz, contract=CONTRACT)
        slots.append(idx)
        cnts.append(cnt)
    res = UO.uniform_value_grad(pcd, slots, list(percentages), scale=scale)
    return pcd, lv, seeds, slots, cnts, res


# ------------------------------------------------------------------------------- dispu_uniform_loss_grad alone ----
KERNEL_CASES = [(1, 40, (0.05, 0.2)), (3, 100, (0.03, 0.05, 0.12)), (2, 333, (0.01, 0.02, 0.04, 0.1)), (1, 2500, (0.004, 0.02)),
                (2, 1024, tuple(UO.DEFAULT_PERCENTAGES))]


@pytest.mark.parametrize("B,N,percentages", KERNEL_CASES, ids=["%dx%dxL%d" % (b, n, len(q)) for b, n, q in KERNEL_CASES])
def test_uniform_loss_grad_kernel(dev, L, B, N, percentages):
    """seeds (dispu_fps) equal the oracle's; idx_out / cnt_out equal the ball-query oracle AND dispu_query_ball bit for bit; partials,
    value and the accumulated gradient against float64; dpcd = NULL writes nothing but the partials (the same ones)."""
    from dispu_amd import loss_utils as LU
    from dispu_amd.tf_grouping import query_ball_point
    from dispu_amd.tf_sampling import farthest_point_sample, gather_point
    scale = 2.5
    pcd, lv, seeds, slots, cnts, res = host_reference(B, N, percentages, 300 + N, scale)
    tab = LU.UniformTables(B, N, list(percentages), scale=scale)
    assert tab.npoint == lv["npoint"] and tab.ns_list == lv["ns"]
    x = dv(pcd, dev)
    dseeds = farthest_point_sample(tab.npoint, x)
    assert np.array_equal(N_(dseeds), seeds), "dispu_fps seeds differ from the oracle's"
    start = pattern(pcd.shape, np.abs(res["grad"]).max())
    out = run_kernel(dev, L, pcd, seeds, tab, prefill=start)
    new_xyz = gather_point(x, dseeds)
    for l, (r, ns) in enumerate(zip(lv["r"], lv["ns"])):
        assert np.array_equal(out["idx"][l], slots[l]), "level %d: slots differ from the ball-query oracle" % l
        assert np.array_equal(out["cnt"][l], cnts[l]), "level %d: counts differ from the ball-query oracle" % l
        di, dc = query_ball_point(r, ns, x, new_xyz)
        assert np.array_equal(out["idx"][l], N_(di)) and np.array_equal(out["cnt"][l], N_(dc)), "level %d: differs from dispu_query_ball" % l
    padded = sum(int((c < ns).sum()) for c, ns in zip(cnts, lv["ns"]))
    print("[measured] uniform kernel (%d, %d, L=%d): %d of %d balls padded, ns %s" % (B, N, len(percentages), padded, len(percentages) * B * tab.npoint, lv["ns"]))
    for l in range(len(percentages)):
        close(out["partial"][l], res["partial"][l], 1e-5, "uniform partial level %d (%d, %d)" % (l, B, N))
    scalar_close(out["partial"].astype(np.float64).mean(), res["value"], 1e-5, "uniform value (%d, %d)" % (B, N))
    skip = UO.near_tie_rows(res, slots, (B, N), TIE)
    print("[measured] uniform kernel (%d, %d): %d of %d rows left out (partner gap < %.0e); smallest gap %.2e" %
          (B, N, int(skip.sum()), skip.size, TIE, min(float(g.min()) for g in res["gap"])))
    assert skip.sum() <= 1e-3 * skip.size
    assert np.abs(res["grad"]).max() > 0
    close(out["dpcd"].astype(np.float64) - start.astype(np.float64), res["grad"], 1e-5, "uniform dpcd (%d, %d), accumulated" % (B, N), keep=~skip)
    # value only: dpcd = idx_out = cnt_out = NULL
    only = run_kernel(dev, L, pcd, seeds, tab, prefill=None, slots=False)
    assert np.array_equal(only["partial"], out["partial"]), "the value-only launch gives other partials"


# ------------------------------------------------------------------------------------------- constructed cases ----
def grid_points(n, spacing):
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(64, 3)[:n].astype(np.float64)
    return (g * spacing).astype(F32)[None]


def run_constructed(dev, L, pcd, seeds, ns, r, e, prefill_scale=1.0):
    """value factor 1, gradient factor 1 per level -> (device outputs, float64 reference on the expected slots of the caller)"""
    tab = Tables(seeds.shape[1], ns, r, e, [1.0] * len(ns), [1.0] * len(ns))
    start = pattern(pcd.shape, prefill_scale)
    return tab, start, run_kernel(dev, L, pcd, seeds, tab, prefill=start)


def constructed_reference(pcd, slots, ns, e, S):
    B = pcd.shape[0]
    Lv = len(ns)
    # uniform_value_grad's factors: partial = w / ns * sum q, k = scale w / (L B S ns): w = ns and scale = L B S make both 1
    return UO.uniform_value_grad(pcd, slots, scale=float(Lv * B * S), levels=dict(ns=list(ns), e=list(e), w=[float(k) for k in ns]))


def test_seed_alone_in_its_ball(dev, L):
    """every slot is the seed: value ns (1e-4 - e)^2 / (e + 1e-8) per ball, the gradient exactly zero (dpcd keeps its bits)."""
    pcd = grid_points(27, 1.0)
    seeds = np.array([[0, 13, 26]], np.int32)
    ns, e = [4, 7], [0.05, 0.11]
    tab, start, out = run_constructed(dev, L, pcd, seeds, ns, [0.1, 0.4], e)
    for l in range(2):
        assert np.array_equal(out["idx"][l], np.repeat(seeds[..., None], ns[l], -1)) and (out["cnt"][l] == 1).all()
        want = ns[l] * (1e-4 - e[l]) ** 2 / (e[l] + 1e-8)
        for s in range(3):
            scalar_close(out["partial"][l, s], want, 1e-5, "lonely seed level %d ball %d" % (l, s))
    assert np.array_equal(out["dpcd"], start), "a ball of one point moved the gradient"


def test_coincident_points(dev, L):
    """two distinct indices with equal coordinates: finite results, no gradient between them."""
    pcd = np.array([[[0.5, -0.25, 0.125], [0.5, -0.25, 0.125], [3, 3, 3], [-3, 3, 3]]], F32)
    seeds = np.array([[0]], np.int32)
    ns, e = [3], [0.07]
    tab, start, out = run_constructed(dev, L, pcd, seeds, ns, [0.1], e)
    assert out["idx"][0].tolist() == [[[0, 1, 0]]] and out["cnt"][0].tolist() == [[2]]
    assert np.isfinite(out["partial"]).all() and np.isfinite(out["dpcd"]).all()
    scalar_close(out["partial"][0, 0], 3 * (1e-4 - e[0]) ** 2 / (e[0] + 1e-8), 1e-5, "coincident points")
    assert np.array_equal(out["dpcd"], start), "coincident points pushed each other"


def test_exact_tie_takes_the_earlier_slot(dev, L):
    """-a, 0, +a on a line, exactly representable: the middle member's two partners tie and the earlier slot wins; the gradient says
    which was taken (row 0 gets two contributions, row 2 one)."""
    a = 0.25
    pcd = np.array([[[-a, 0, 0], [0, 0, 0], [a, 0, 0], [9, 9, 9]]], F32)
    seeds = np.array([[1]], np.int32)
    ns, e = [3], [0.1]
    tab, start, out = run_constructed(dev, L, pcd, seeds, ns, [0.5], e, prefill_scale=0.0)
    assert out["idx"][0].tolist() == [[[0, 1, 2]]] and out["cnt"][0].tolist() == [[3]]
    ref = constructed_reference(pcd, [np.array([[[0, 1, 2]]])], ns, e, 1)
    assert ref["partner"][0].tolist() == [[[1, 0, 1]]] and ref["gap"][0][0, 0, 1] == 0.0
    u = np.sqrt(a * a + 1e-8)
    f = (u - e[0]) / ((e[0] + 1e-8) * u) * 2 * a
    assert np.allclose(ref["grad"][0, :3, 0], [-2 * f, f, f], rtol=1e-12)
    close(out["dpcd"], ref["grad"], 1e-5, "collinear tie dpcd")
    assert out["dpcd"][0, 0, 0] < 0 < out["dpcd"][0, 2, 0] and abs(out["dpcd"][0, 0, 0]) > 1.5 * abs(out["dpcd"][0, 2, 0])
    close(out["partial"][0], ref["partial"][0], 1e-5, "collinear tie partial")


def test_full_and_nearly_full_balls(dev, L):
    """four points inside the radius: a ball of 3 slots is cut after the first three in index order, one of 4 is exactly full
    (cnt == ns), one of 5 has cnt == ns - 1 and repeats the first hit once."""
    rng = np.random.default_rng(3)
    pcd = (grid_points(40, 1.0) + 0.0).copy()
    inside = [5, 11, 17, 30]
    pcd[0, inside] = (np.array([2.0, 2.0, 2.0]) + rng.uniform(-0.05, 0.05, (4, 3))).astype(F32)
    seeds = np.array([[17]], np.int32)
    ns, e = [3, 4, 5], [0.03, 0.04, 0.05]
    tab, start, out = run_constructed(dev, L, pcd, seeds, ns, [0.3, 0.3, 0.3], e, prefill_scale=0.5)
    want = [[5, 11, 17], [5, 11, 17, 30], [5, 11, 17, 30, 5]]
    for l in range(3):
        assert out["idx"][l].tolist() == [[want[l]]], l
    assert out["cnt"][:, 0, 0].tolist() == [3, 4, 4]
    ref = constructed_reference(pcd, [np.array([[w]]) for w in want], ns, e, 1)
    for l in range(3):
        close(out["partial"][l], ref["partial"][l], 1e-5, "full / nearly full balls, level %d" % l)
    close(out["dpcd"].astype(np.float64) - start, ref["grad"], 1e-5, "full / nearly full balls dpcd")


def test_uniform_entries_refuse_invalid_arguments(dev, L):
    lib, st = L.lib(), L.stream_ptr(dev)
    f = torch.full((4096,), SENT, dtype=torch.float32, device=dev)
    i = torch.full((4096,), ISENT, dtype=torch.int32, device=dev)
    x = torch.rand((2, 100, 3), device=dev)
    s = torch.zeros((2, 5), dtype=torch.int32, device=dev)
    ns, lev = (C.c_int * 8)(*[4] * 8), (C.c_float * 32)(*[0.1] * 32)
    NS, LEV, X, S_, F, I = C.addressof(ns), C.addressof(lev), p(x), p(s), p(f), p(i)

    def call(b=2, n=100, npoint=5, nl=2, ns_=NS, lev_=LEV, x_=X, s_=S_, part=F, dp=p(f, 1024), io=I, co=p(i, 2048)):
        return lib.dispu_uniform_loss_grad(b, n, npoint, nl, ns_, lev_, x_, s_, part, dp, io, co, CONTRACT, st)
    assert call(b=-1) == INVALID and call(n=0) == INVALID and call(npoint=0) == INVALID and call(npoint=-3) == INVALID
    assert call(nl=0) == INVALID and call(nl=9) == INVALID and call(nl=-1) == INVALID
    assert call(ns_=None) == INVALID and call(lev_=None) == INVALID and call(x_=None) == INVALID and call(s_=None) == INVALID
    assert call(part=None) == INVALID
    for bad in (1, 0, -2, 65, 101):                           # outside 2..min(64, n)
        one = (C.c_int * 8)(4, bad, 4, 4, 4, 4, 4, 4)
        assert call(ns_=C.addressof(one)) == INVALID, bad
    small = (C.c_int * 8)(*[4] * 8)
    assert call(n=3, ns_=C.addressof(small)) == INVALID       # ns = 4 > n = 3
    assert call(b=0) == 0
    assert call(b=0, nl=9) == INVALID                         # an empty batch is still validated
    # dispu_pu_loss_finalize_u
    fin = lambda cd=F, rep=None, nrep=0, up=F, nl=5, nu=51, out=p(f, 8): lib.dispu_pu_loss_finalize_u(cd, rep, nrep, 0.5, 1.0, up, nl, nu, 10.0, out, st)
    assert fin(cd=None) == INVALID and fin(out=None) == INVALID and fin(up=None) == INVALID
    assert fin(nl=0) == INVALID and fin(nl=9) == INVALID and fin(nu=0) == INVALID and fin(nu=-1) == INVALID
    assert fin(rep=F, nrep=0) == INVALID and fin(rep=F, nrep=-5) == INVALID
    torch.cuda.synchronize()
    assert bool((f == SENT).all()) and bool((i == ISENT).all()), "a refused call wrote to its buffers"


# ---------------------------------------------------------------------------------------- dispu_pu_loss_finalize_u ----
def run_finalize_u(dev, L, cd, rep, nrep, wf, rep_w, upart, nl, nu, uniform_w):
    """as the trainer calls it: cd = loss_vals[0:2], out = loss_vals + 2 (8 floats, guards follow) -> out[0..5]"""
    lv = Guarded(dev, 8, g=8)
    lv.t[lv.g:lv.g + 2] = torch.from_numpy(np.asarray(cd, F32)).to(dev)
    L.check(L.lib().dispu_pu_loss_finalize_u(lv.ptr(), p(rep), nrep, wf, rep_w, p(upart), nl, nu, uniform_w, p(lv.t, lv.g + 2),
                                             L.stream_ptr(dev)), "pu_loss_finalize_u")
    torch.cuda.synchronize()
    body = lv.body()
    assert lv.guards_intact(), "pu_loss_finalize_u wrote past out[5]"
    assert np.array_equal(body[:2], np.asarray(cd, F32)), "cd[0..1] did not survive the aliased call"
    return body[2:8]


@pytest.mark.parametrize("nu", [1, 51, 408, 1025])
@pytest.mark.parametrize("nl", [1, 5, 8])
def test_pu_loss_finalize_u(dev, L, nl, nu):
    rng = np.random.default_rng(100 * nl + nu)
    nrep = 2048
    rep = rng.uniform(0.0, 4e-3, nrep).astype(F32)
    upart = rng.uniform(0.0, 0.5, nl * nu).astype(F32)
    trep = dv(np.concatenate([rep, np.full(64, 1e6, F32)]), dev)          # anything read past the end would show
    tup = dv(np.concatenate([upart, np.full(64, 1e6, F32)]), dev)
    for wf in (0.01, 1.0):
        for with_rep in (True, False):
            cd = rng.uniform(1e-3, 5e-2, 2).astype(F32)
            r, n = (trep, nrep) if with_rep else (None, 0)
            out = run_finalize_u(dev, L, cd, r, n, wf, 0.5, tup, nl, nu, 10.0)
            ref = UO.pu_loss_terms_u(cd[0], cd[1], rep if with_rep else None, n, F32(wf), 0.5, upart, 10.0)
            for j in (0, 1, 2, 3, 5):
                if ref[j] == 0.0:
                    assert out[j] == 0.0
                else:
                    scalar_close(out[j], ref[j], 1e-5, "finalize_u out[%d] L=%d nu=%d wf=%g rep=%s" % (j, nl, nu, wf, with_rep))
            assert out[4] == F32(wf)
            # uniform_w = 0: the first five outputs are dispu_pu_loss_finalize's, bit for bit
            zero = run_finalize_u(dev, L, cd, r, n, wf, 0.5, tup, nl, nu, 0.0)
            plain = Guarded(dev, 8, g=8)
            plain.t[plain.g:plain.g + 2] = torch.from_numpy(cd).to(dev)
            L.check(L.lib().dispu_pu_loss_finalize(plain.ptr(), p(r), n, wf, 0.5, p(plain.t, plain.g + 2), L.stream_ptr(dev)), "pu_loss_finalize")
            torch.cuda.synchronize()
            assert np.array_equal(zero[:5].view(np.uint32), plain.body()[2:7].view(np.uint32)) and zero[5] == 0.0


# ------------------------------------------------------------------------------------ loss_utils.get_uniform_loss ----
def _composed():
    spec = importlib.util.spec_from_file_location("uniform_bench", os.path.join(ROOT, "tools", "uniform_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.composed_uniform_loss


def test_get_uniform_loss(dev):
    """value and torch.autograd.grad against the oracle at (2, 1024), and against the path composed from the existing Python ops
    (query_ball_point, group_point, differences, torch.sort)."""
    from dispu_amd import loss_utils as LU
    B, N = 2, 1024
    pcd, lv, seeds, slots, cnts, res = host_reference(B, N, tuple(UO.DEFAULT_PERCENTAGES), 300 + N, 1.0)
    x = dv(pcd, dev).requires_grad_(True)
    v = LU.get_uniform_loss(x)
    assert v.dim() == 0 and v.dtype == torch.float32
    (g,) = torch.autograd.grad(3.0 * v, x)
    scalar_close(float(v.detach()), res["value"], 1e-5, "get_uniform_loss value")
    skip = UO.near_tie_rows(res, slots, (B, N), TIE)
    assert skip.sum() <= 1e-3 * skip.size
    close(N_(g), 3.0 * res["grad"], 1e-5, "get_uniform_loss autograd", keep=~skip)
    x2 = dv(pcd, dev).requires_grad_(True)
    vc = _composed()(x2)
    (gc,) = torch.autograd.grad(3.0 * vc, x2)
    scalar_close(float(v.detach()), float(vc.detach()), 1e-5, "get_uniform_loss vs composed ops, value")
    close(N_(g), N_(gc).astype(np.float64), 1e-5, "get_uniform_loss vs composed ops, gradient", keep=~skip)
    # other percentages / radius reach the kernel
    v2 = LU.get_uniform_loss(x.detach(), [0.01, 0.03], radius=1.5)
    lv2 = UO.host_levels(N, [0.01, 0.03], 1.5)
    new_xyz = O.gather_point(pcd, seeds)
    s2 = [O.query_ball_point(r, ns, pcd, new_xyz, contract=CONTRACT)[0] for r, ns in zip(lv2["r"], lv2["ns"])]
    scalar_close(float(v2), UO.uniform_value_grad(pcd, s2, [0.01, 0.03], radius=1.5)["value"], 1e-5, "get_uniform_loss, radius 1.5")
    with pytest.raises(ValueError, match="at least k columns"):
        LU.get_uniform_loss(torch.zeros((1, 64, 3), device=dev))


# ------------------------------------------------------------------------------------------------- the Trainer ----
def make_trainer(dev, epoch, use_uniform=True, uniform_w=10.0, opts=None, dtype="f32"):
    from dispu_amd.train import Trainer, TrainOpts
    if opts is None:
        opts = TrainOpts()
        opts.use_uniform, opts.uniform_w = use_uniform, uniform_w
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


def check_uniform_loss_head(tr, B, N, gt, radius, terms, what):
    """float64 Chamfer + repulsion (the reference test_loss_head builds from loss_oracle) + uniform, at the device's own fine cloud."""
    import test_train_loss_gpu as TL
    from dispu_amd.train import weight_fine
    ws = tr._ws[(B, N)]
    wf, uw = weight_fine(tr.epoch), float(tr.opts.uniform_w)
    ref = TL.loss_head_reference(ws, gt, radius, wf, tr.opts.use_repulse, float(tr.opts.repulsion_w))
    del TL._KEEP[:]
    fine = N_(ws["fine"]).reshape(B, -1, 3)
    M = fine.shape[1]
    lv = UO.host_levels(M)
    seeds = O.farthest_point_sample(lv["npoint"], fine, contract=CONTRACT)
    assert np.array_equal(N_(ws["useeds"]), seeds), "the trainer's seeds differ from the oracle's"
    new_xyz = O.gather_point(fine, seeds)
    slots = [O.query_ball_point(r, ns, fine, new_xyz, contract=CONTRACT)[0] for r, ns in zip(lv["r"], lv["ns"])]
    res = UO.uniform_value_grad(fine, slots, scale=uw)
    want = dict(dis_coarse_cd=ref["terms"][0], dis_fine_cd=ref["terms"][1], repulsion_loss=ref["terms"][2],
                uniform_loss=uw * res["value"], pu_loss=ref["terms"][3] + uw * res["value"])
    assert float(terms["weight_fine"]) == wf and set(terms) == set(want) | {"weight_fine"}
    for k, r in want.items():
        scalar_close(float(terms[k]), r, 1e-5, "%s %s" % (what, k))
    assert want["uniform_loss"] > 0
    close(N_(ws["dcoarse"]).reshape(B, M, 3), ref["dcoarse"], 1e-5, "%s dcoarse" % what)
    skip = ref["skip"] | UO.near_tie_rows(res, slots, (B, M), TIE)
    print("[measured] %s: %d of %d dfine rows left out; uniform share of max |dfine| %.2e" %
          (what, int(skip.sum()), skip.size, np.abs(res["grad"]).max() / np.abs(ref["dfine"] + res["grad"]).max()))
    assert skip.sum() <= 1e-3 * skip.size
    close(N_(ws["dfine"]).reshape(B, M, 3), ref["dfine"] + res["grad"], 1e-5, "%s dfine" % what, keep=~skip)
    return want


@pytest.mark.parametrize("epoch,B,N", [(25, 2, 256), (35, 3, 256)])
def test_loss_head_with_uniform(dev, epoch, B, N):
    tr = make_trainer(dev, epoch)
    gt, radius, terms = loss_head(dev, tr, B, N, seed=50 + B)
    check_uniform_loss_head(tr, B, N, gt, radius, terms, "uniform loss head epoch %d B=%d" % (epoch, B))


def test_loss_head_uniform_weight(dev):
    """uniform_w = 2.5 scales the term (and its gradient) and nothing else."""
    tr = make_trainer(dev, 35, uniform_w=2.5)
    gt, radius, terms = loss_head(dev, tr, 2, 256, seed=62)
    a = check_uniform_loss_head(tr, 2, 256, gt, radius, terms, "uniform loss head, uniform_w = 2.5")
    tr10 = make_trainer(dev, 35)
    _, _, t10 = loss_head(dev, tr10, 2, 256, seed=62)
    scalar_close(float(t10["uniform_loss"]), 4.0 * float(terms["uniform_loss"]), 1e-5, "uniform_w 10 vs 2.5")
    assert float(t10["dis_fine_cd"]) == float(terms["dis_fine_cd"]) and float(t10["repulsion_loss"]) == float(terms["repulsion_loss"])
    assert a["uniform_loss"] > 0


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


def test_uniform_off_is_the_step_without_the_field(dev):
    """use_uniform = False against a Trainer whose options do not have the field at all: the same launches with the same scalar
    arguments in the same order, loss terms and loss_vals bit-identical, no uniform entry in the terms, no uniform buffers.

    dfine: bit-identity cannot be asked of it -- the Chamfer and repulsion gradients are accumulated with float atomics
    (chamfer_grad_kernel, repulsion_loss_grad_kernel) and two runs of ONE unchanged Trainer already differ (measured on an MI355X:
    142 of 6144 entries run to run, 123 between the two Trainers compared here, max |diff| 2.7e-5 at max |dfine| 59; both figures are
    printed below).  It is held to what a re-ordered fp32 sum allows: every entry within (k - 1) 2^-23 of the largest |entry| for
    the at most k = 32 contributions a row collects (20 repulsion slots + its own terms + the gt points that chose it)."""
    from dispu_amd.generator import _Opts
    from dispu_amd.train import TrainOpts

    class OldOpts(_Opts):                      # the training-side options as they were before the uniform term
        base_lr_g, beta, lr_decay, decay_step, lr_decay_rate, lr_clip, use_repulse, repulsion_w = 0.001, 0.9, True, 30, 0.7, 1e-6, True, 1.0
    assert not hasattr(OldOpts(), "use_uniform") and TrainOpts.use_uniform is False and TrainOpts.uniform_w == 10.0
    outs = []
    for opts in (OldOpts(), OldOpts(), None):
        tr = make_trainer(dev, 25, use_uniform=False, opts=opts)
        gt, radius, terms = loss_head(dev, tr, 2, 256, seed=61)
        ws = tr._ws[(2, 256)]
        assert "uniform_loss" not in terms and "utabs" not in ws
        out = ({k: float(v) for k, v in terms.items()}, N_(ws["dfine"]).copy(), N_(ws["loss_vals"]).copy())
        outs.append(out + (_launch_signature(tr, dv(gt, dev), dv(radius, dev)),))
    old, old2, new = outs
    assert old[0] == new[0]
    assert np.array_equal(old[2].view(np.uint32), new[2].view(np.uint32))
    assert len(new[3]) > 8 and old[3] == new[3], "the launch sequence changed with use_uniform = False"
    assert not any("uniform" in name or name == "dispu_pu_loss_finalize_u" for name, _ in new[3])
    top = float(np.abs(old[1]).max())
    for what, a, b in (("one unchanged Trainer, run to run", old[1], old2[1]), ("without the field vs use_uniform = False", old[1], new[1])):
        same = a.view(np.uint32) == b.view(np.uint32)
        print("[measured] dfine, %s: %d of %d entries differ, max |diff| %.3e of max |dfine| %.3e" %
              (what, int((~same).sum()), same.size, float(np.abs(a - b).max()), top))
    assert float(np.abs(old[1] - new[1]).max()) <= 31 * 2.0 ** -23 * top


def test_uniform_refuses_small_patches(dev):
    from dispu_amd import synth
    tr = make_trainer(dev, 25)
    x, gt = synth.patch_with_gt(2, 64, 256, seed=3)
    args = (dv(x, dev), dv(gt, dev), torch.ones(2, device=dev))
    for step in (tr.train_step, tr.train_step_taped):
        with pytest.raises(ValueError, match=r"at least 125 .* got 64 \(256 fine points\)"):
            step(*args)
    tr.forward(args[0])
    with pytest.raises(ValueError, match="at least 500 fine points"):
        tr.loss_backward(args[1], args[2])
    assert tr.global_step == 0 and not tr._tapes


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_taped_step_equals_eager_step_with_uniform(dev, dtype):
    """train_step_taped == train_step with the term on (the tolerances of test_taped_steps_equal_eager_steps); the tape's key holds
    use_uniform and uniform_w, and the recorded host tables stay alive in the workspace."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer, TrainOpts
    P = OG.init_params(seed=22, bias_scale=0.05, bn_random=True)
    B = 4
    rs = torch.ones(B, device=dev)
    mk = lambda: TrainOpts()
    e, g = Trainer(mk(), params=P, device=dev, dtype=dtype), Trainer(mk(), params=P, device=dev, dtype=dtype)
    for t in (e, g):
        t.opts.use_uniform, t.epoch = True, 20
    gtol = 2e-5 if dtype == "f32" else 2e-3
    for i in range(3):
        if i == 2:
            e.opts.uniform_w = g.opts.uniform_w = 2.5            # a new key: a new tape
        x, gt = synth.patch_with_gt(B, 256, 1024, seed=40 + i)
        for name in ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var"):
            getattr(g, name).copy_(getattr(e, name))
        g.adam_t, g.global_step = e.adam_t, e.global_step
        xs, gs = dv(x, dev), dv(gt, dev)
        te = e.train_step(xs, gs, rs)
        tg = g.train_step_taped(xs, gs, rs)
        torch.cuda.synchronize()
        assert "uniform_loss" in te and "uniform_loss" in tg and float(te["uniform_loss"]) > 0
        floor = 4e-7 * float(e.flat_g.abs().max())
        for k in e.G:
            scale = float(e.G[k].abs().max()) + 1e-12
            assert float((g.G[k] - e.G[k]).abs().max()) <= gtol * scale + floor + 2e-6, (i, k)
        for k in te:
            a, b = float(te[k]), float(tg[k])
            assert abs(a - b) <= (1e-5 if dtype == "f32" else 1e-2) * max(1.0, abs(a)), (i, k, a, b)
        diff = N_((g.flat_p - e.flat_p).abs())
        print("[measured] taped vs eager with uniform (%s) step %d: params max %.2e q99 %.2e; uniform_loss %.6g" %
              (dtype, i, diff.max(), np.quantile(diff, 0.99), float(te["uniform_loss"])))
        assert diff.max() <= 2.5e-3 and np.quantile(diff, 0.99) <= (2e-5 if dtype == "f32" else 1e-3)
    assert len(g._tapes) == 2
    assert sorted(k[4:6] for k in g._tapes) == [(True, 2.5), (True, 10.0)]
    assert sorted(g._ws[(B, 256)]["utabs"]) == [2.5, 10.0]


def test_fit_epoch_logs_the_uniform_term(tmp_path, dev):
    """one fit epoch on synthetic patches with the term on: every step's pu_loss is the sum of its four terms, and the epoch's g_loss
    (log_train.txt) is the mean of those."""
    from dispu_amd import dataset, params, synth, train
    _, gt = synth.patch_with_gt(12, 256, 1024, seed=21)
    fetcher = dataset.DeviceFetcher(gt, gt, 4, patch_num_point=256, device=dev, seed=5)
    opts = train.TrainOpts()
    opts.batch_size, opts.training_epoch, opts.epoch_per_save, opts.use_uniform = 4, 1, 1, True
    tr = train.Trainer(opts, params.init_params(seed=7), device=dev)
    steps, inner = [], tr.train_step

    def step(x, g, r):
        terms = inner(x, g, r)
        steps.append({k: float(v) for k, v in terms.items()})
        return terms
    tr.train_step = step
    recs = train.fit(tr, fetcher, opts, str(tmp_path / "log"))
    assert len(recs) == 1 and len(steps) == recs[0]["steps"] == 2
    for s in steps:
        assert s["uniform_loss"] > 0
        total = s["dis_coarse_cd"] + s["weight_fine"] * s["dis_fine_cd"] + s["repulsion_loss"] + s["uniform_loss"]
        assert abs(s["pu_loss"] - total) <= 1e-5 * total
    mean = float(np.mean([s["pu_loss"] for s in steps]))
    without = float(np.mean([s["pu_loss"] - s["uniform_loss"] for s in steps]))
    assert abs(recs[0]["g_loss"] - mean) <= 1e-5 * mean and recs[0]["g_loss"] > without
    line = [l for l in open(str(tmp_path / "log" / "log_train.txt")).read().splitlines() if l.startswith("epoch 0001")]
    assert len(line) == 1 and abs(float(re.search(r"g_loss=(\d+\.\d+)", line[0]).group(1)) - mean) <= 1e-5 * mean
    args = open(str(tmp_path / "log" / "args.txt")).read().splitlines()
    assert "use_uniform: True" in args and "uniform_w: 10.0" in args and args == sorted(args)
