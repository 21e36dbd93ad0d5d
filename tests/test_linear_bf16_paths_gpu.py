"""The bf16-product GEMMs (csrc/linear_bf16.hip) in each of the three block tiles gb_launch can pick -- 128 x 32 (N <= 32), 64 x 64 and
128 x 128 (at least 512 tiles of 128 x 128 over the batch), as reported by dispu_linear_bf16_plan -- in the NN and NT layouts:
dispu_linear_bf16, dispu_linear_bf16s (bf16-stored X / Y) and dispu_linear_bf16_masked, with M and N past a tile edge, K in
{1, 7, 63, 64, 65, 129} (around GB_KALIGN = 64 and both slab depths, 64 and 32), R1 / R2 / both, a mask over a prefix and over all of
the columns, operands with odd row strides, outputs between sentinel columns and guard rows.

Reference and bound are those of test_train_bf16_gpu.py::test_linear_bf16_vs_float64_of_rounded_operands: the float64 product of the
bf16-rounded operands, |got - z| <= 2e-6 (|x| . |w|) + 1e-6 (1 + |z|).  A bf16-stored Y is the fp32 result rounded once, bit for bit,
and a bf16-stored X gives what the fp32-stored X does (the kernel rounds it the same way).
The 128 x 128 tile is reached at small cost with batch 8, M = N = 1000 (8 x 8 x 8 = 512 tiles); the masked entry needs batch 1 and gets
there with 4097 x 1921 (33 x 16 tiles).

The TN products (dispu_linear_tn_bf16*) are not forced into 128 x 128 here: their split plan keeps tiles x splits near 256 - 1024 on
the 64 x 64 / 128 x 32 tiling, so they never select that tile at any K x N this model has.  tests/test_tn_paths_gpu.py runs them on
every tile their plan can reach (128 x 128 included: one- and two-tile outputs over >= 130817 rows, or 512 tiles without a split).

[measured] worst |got - z| / bound over all cases: 0.061 (dispu_linear_bf16, 128 x 128 tile, NN, K = 65, R1).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (1, 7, 63, 64, 65, 129)
# tile code -> (batch, M, N): M and N one past a tile where the tile allows it
SHAPES = {128032: (1, 129, 29), 64064: (1, 65, 65), 128128: (8, 1000, 1000)}
MASKED_SHAPES = {128032: (1, 129, 29), 64064: (1, 65, 65), 128128: (1, 4097, 1921)}
GUARD, SENT = 1, -77.0
WORST = {"f": 0.0}


def r16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy().astype(np.float64)


class Buf(object):
    """[batch][rows (+ guards)][ld] device buffer holding `data` [batch, rows, cols] at column offset `c0`, the rest `fill`"""

    def __init__(self, dev, batch, rows, cols, ld, c0=0, guard=0, data=None, fill=np.nan, extra=5, dtype=torch.float32):
        self.batch, self.rows, self.cols, self.ld, self.c0, self.guard = batch, rows, cols, ld, c0, guard
        self.stride = (rows + 2 * guard) * ld + extra
        h = np.full(batch * self.stride + 8, fill, np.float32)
        if data is not None:
            for z in range(batch):
                np.lib.stride_tricks.as_strided(h[z * self.stride + guard * ld + c0:], shape=(rows, cols), strides=(4 * ld, 4))[...] = data[z]
        self.fill = fill
        self.t = torch.from_numpy(h).to(dev).to(dtype)
        self.esize = self.t.element_size()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.esize * (self.guard * self.ld + self.c0))

    def read(self):
        """(data [batch, rows, cols] as stored, everything else still the fill value)"""
        h = self.t.float().cpu().numpy()
        out = np.empty((self.batch, self.rows, self.cols), np.float32)
        for z in range(self.batch):
            v = np.lib.stride_tricks.as_strided(h[z * self.stride + self.guard * self.ld + self.c0:], shape=(self.rows, self.cols),
                                                strides=(4 * self.ld, 4))
            out[z] = v
            v[...] = self.fill
        return out, bool((h == np.float32(self.fill)).all())


def make(dev, code, K, transb, shapes=SHAPES):
    batch, M, N = shapes[code]
    rng = np.random.default_rng([code, K, transb, M])
    x = rng.standard_normal((batch, M, K), dtype=np.float32)
    w = (rng.standard_normal((batch, N, K) if transb else (batch, K, N)) * 0.1).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    r1, r2 = rng.standard_normal((batch, M, N), dtype=np.float32), rng.standard_normal((batch, M, N), dtype=np.float32)
    wr, wc = w.shape[1:]
    d = dict(batch=batch, M=M, N=N, K=K, transb=transb, x=x, w=w, bias=bias, r1=r1, r2=r2,
             X=Buf(dev, batch, M, K, K + 3, c0=1, data=x), W=Buf(dev, batch, wr, wc, wc + 1, data=w),
             B=torch.from_numpy(bias).to(dev), R1=Buf(dev, batch, M, N, N + 1, data=r1), R2=Buf(dev, batch, M, N, N + 2, data=r2, extra=7))
    xr, w64 = r16(x), r16(w)
    wl = np.swapaxes(w64, 1, 2) if transb else w64
    d["prod"] = np.matmul(xr, wl)
    d["absprod"] = np.matmul(np.abs(xr), np.abs(wl))
    return d


def reference(d, bias, act, res, mask=None, mcols=0):
    z = d["prod"] + (d["bias"] if bias else 0)
    if act:
        z = np.maximum(z, 0)
    if res & 1:
        z = z + d["r1"]
    if res & 2:
        z = z + d["r2"]
    if mask is not None and mcols > 0:
        z[:, :, :mcols] = np.where(mask[None, :, :mcols] > 0, z[:, :, :mcols], 0.0)
    return z, 2e-6 * d["absprod"] + 1e-6 * (1 + np.abs(z))


def held(got, z, bound, what):
    err = np.abs(got.astype(np.float64) - z)
    frac = float((err / bound).max())
    WORST["f"] = max(WORST["f"], frac)
    print("[measured] %s: worst |got - z| / bound = %.3f (so far %.3f)" % (what, frac, WORST["f"]))
    assert (err <= bound).all(), "%s: %.3g x the bound" % (what, frac)


def ybuf(dev, d, dtype=torch.float32):
    return Buf(dev, d["batch"], d["M"], d["N"], d["N"] + 5, c0=2, guard=GUARD, fill=SENT, dtype=dtype)


def common(d):
    return (d["batch"], d["M"], d["K"], d["N"])


@pytest.mark.parametrize("transb", [0, 1])
@pytest.mark.parametrize("code", list(SHAPES))
def test_linear_bf16_tile(dev, code, transb):
    from dispu_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    for i, K in enumerate(KS):
        d = make(dev, code, K, transb)
        assert L.dispu_linear_bf16_plan(d["batch"], d["M"], d["N"], 1) == code
        res, act, bias = (0, 1, 2, 3, 1, 3)[i], i % 2, i != 2
        Y = ybuf(dev, d)
        _lib.check(L.dispu_linear_bf16(*common(d), d["X"].ptr(), d["X"].ld, d["X"].stride, d["W"].ptr(), d["W"].ld, d["W"].stride, transb,
                                       C.c_void_p(d["B"].data_ptr()) if bias else None, act, Y.ptr(), Y.ld, Y.stride,
                                       d["R1"].ptr() if res & 1 else None, d["R1"].ld, d["R1"].stride,
                                       d["R2"].ptr() if res & 2 else None, d["R2"].ld, d["R2"].stride, st), "dispu_linear_bf16")
        got, clean = Y.read()
        z, bound = reference(d, bias, act, res)
        held(got, z, bound, "bf16 %d transb %d K %d res %d" % (code, transb, K, res))
        assert clean, "wrote outside the output"


@pytest.mark.parametrize("transb", [0, 1])
@pytest.mark.parametrize("code", list(SHAPES))
def test_linear_bf16s_tile(dev, code, transb):
    """bf16-stored X: the same operands the fp32-storage kernel rounds to, held to the same bound; bf16-stored Y: that result rounded once"""
    from dispu_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    for K in KS:
        d = make(dev, code, K, transb)
        Xb = Buf(dev, d["batch"], d["M"], K, K + 3, c0=1, data=d["x"], dtype=torch.bfloat16)
        outs = {}
        for xb, yb, res in ((1, 0, 1), (1, 0, 0), (1, 1, 0), (0, 1, 0)):                # (R1 must be NULL when Y is bf16)
            X = Xb if xb else d["X"]
            Y = ybuf(dev, d, torch.bfloat16 if yb else torch.float32)
            _lib.check(L.dispu_linear_bf16s(*common(d), X.ptr(), X.ld, X.stride, d["W"].ptr(), d["W"].ld, d["W"].stride, transb,
                                            C.c_void_p(d["B"].data_ptr()), 1, Y.ptr(), Y.ld, Y.stride, d["R1"].ptr() if res else None,
                                            d["R1"].ld, d["R1"].stride, xb | (4 * yb), st), "dispu_linear_bf16s")
            outs[(xb, yb, res)], clean = Y.read()
            assert clean, "wrote outside the output"
        for res in (1, 0):
            z, bound = reference(d, 1, 1, res)
            held(outs[(1, 0, res)], z, bound, "bf16s X stored %d transb %d K %d res %d" % (code, transb, K, res))
        want = torch.from_numpy(outs[(1, 0, 0)]).bfloat16().float().numpy()
        assert np.array_equal(outs[(1, 1, 0)], want)                    # a bf16 Y is the fp32 result rounded once (nearest even)
        assert np.array_equal(outs[(0, 1, 0)], want)                    # a stored-bf16 X is the rounding the kernel applies itself


@pytest.mark.parametrize("transb", [0, 1])
@pytest.mark.parametrize("code", list(MASKED_SHAPES))
def test_linear_bf16_masked_tile(dev, code, transb):
    from dispu_amd import _lib
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    for K in KS:
        d = make(dev, code, K, transb, MASKED_SHAPES)
        M, N = d["M"], d["N"]
        assert L.dispu_linear_bf16_plan(1, M, N, 1) == code
        rng = np.random.default_rng(K)
        mk = np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32)
        mk[rng.random((M, N)) < 0.05] = -1.0
        Mk = Buf(dev, 1, M, N, N + 3, data=mk[None])
        for mcols in (N - 5, N):
            Y = ybuf(dev, d)
            _lib.check(L.dispu_linear_bf16_masked(1, M, K, N, d["X"].ptr(), d["X"].ld, 0, d["W"].ptr(), d["W"].ld, 0, transb,
                                                  C.c_void_p(d["B"].data_ptr()), 0, Y.ptr(), Y.ld, 0, d["R1"].ptr(), d["R1"].ld, 0,
                                                  Mk.ptr(), Mk.ld, mcols, st), "dispu_linear_bf16_masked")
            got, clean = Y.read()
            z, bound = reference(d, 1, 0, 1, mk, mcols)
            assert not got[0][:, :mcols][mk[:, :mcols] <= 0].any()          # masked entries are exactly zero
            held(got, z, bound, "bf16 masked %d transb %d K %d mcols %d" % (code, transb, K, mcols))
            assert clean, "wrote outside the output"
