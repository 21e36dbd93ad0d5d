"""The training attention kernels ALONE through the C ABI (csrc/attention_train.hip: dispu_attention_fwd_lse, dispu_attention_bwd) against
tests/attention_train_oracle.py (numpy float64 from the explicit formulas, held to float64 autograd by tests/test_attention_train_oracle.py),
on every path the launch code takes.  tests/test_train_fused_gpu.py visits them with m == nk, compact operands and benign inputs.

Paths.  The entries pick the workgroup shape separately: forward and dQ by ft_split(b, m), dK|dV by ft_split(b, nk); ft_block remaps
workgroups to clouds when b % 8 == 0; the loader has three prologues (1, 2, >= 3 stages) and the 4-tile stage of the split shape four
tail sizes.  `path()` restates the rule and every case asserts the path its comment claims; nothing is instrumented.
  (b, m, nk)        forward / dQ (stream the nk keys)           dK|dV (streams the m queries)
  (257, 128, 32)    128 columns, no remap, 1 stage              split, no remap, one full stage of 4 tiles
  (64, 512, 64)     128 columns, remap, 2 stages                split, remap, 4 full stages
  (64, 96, 512)     split, remap, 4 full stages                 128 columns, remap, 3 stages
  (257, 32, 128)    split, no remap, one full stage             128 columns, no remap, 1 stage
  (3, 160, 160)     split, 2 stages, tail of 1                  same
  (2, 192, 192)     split, 2 stages, tail of 2                  same
  (1, 352, 352)     split, 3 stages, tail of 3                  same
  (5, 64, 288)      split, 3 stages, tail of 1                  split, one stage of 2 tiles
  (8, 64, 64)       split, remap, one stage of 2 tiles: waves 2 and 3 never get a tile (maximum -inf, sum 0 in the combine)
  (2, 32, 64)       split, one stage of 2 tiles                 split, one stage of 1 tile: three idle waves
  (64, 512, 96)     128 columns, remap, 3 stages                split, remap, 4 full stages
  (64, 64, 512)     split, remap, 4 full stages                 128 columns, remap, 2 stages
so each of the three kernels runs in both workgroup shapes with 1, 2 and 3 or more stages, with and without the remap.

Layouts.  Every shape runs once as the trainer calls it (ld == 64, K|V and dK|dV interleaved at 128) and once with every operand
strided and offset: Q 68, O 72, dO 80, dQ 72, K 72, V 84, dK 68, dV 88, each window at its own multiple of 4 floats.  Every output is a
train_ops_oracle.Strided / Guarded pre-filled with a sentinel: after the calls every element of every window is written, every column
outside a window and every guard is intact, and every input holds the bits that were uploaded.

Inputs (attention_train_oracle's builders).  Cloud c's V and dO carry their own powers of two and EVERY comparison is per cloud, against
that cloud's own largest float64 entry: a wrong cloud offset or a cloud served twice cannot hide behind another cloud's magnitude.

Bounds.  benign, ascending, descending, one_hot, equal_keys, zero_q: the project's 1e-5 of the cloud's largest entry for O, D, dQ, dK,
dV and 1e-5 max(1, max |lse2|) for lse2 (the float32 restatement of the algorithm sits near 1e-6 there, test_attention_train_oracle.py).
equal_keys makes dQ analytically zero: it is held to 1e-5 of the terms that cancel in it.  k_offset and big_logits, where the exponent
arithmetic of P = 2^(s2 - lse2) is ill-conditioned: per output and per cloud max(1e-5, 2 x the error of recompute_f32 on the same
inputs), both against float64; the factor 2 is for the MFMA's sequential accumulation and for v_exp_f32 / v_log_f32 not being correctly
rounded.  Every comparison prints its worst cloud before it asserts (pytest -s).

Determinism: two calls at (64, 512, 64) and (64, 96, 512) give the same bits in all six outputs.  Refusals: every pointer operand of both
entries NULL, one float off 16-byte alignment and under a stride that is no multiple of 4; m % 32, nk % 32, d != 64, b < 0, m <= 0,
nk <= 0; NULL lse2 and dvec; each returns hipErrorInvalidValue and leaves every output holding its sentinel; b == 0 returns 0 and
writes nothing.

Found by test_ill_conditioned_inputs and fixed with it: fa_train_bwd_dkv_kernel formed its logits as Q[q][d] * (K[k][d] * scale2) while
the forward, whose lse2 it subtracts, and the dQ kernel form (Q[q][d] * scale2) * K[k][d].  The two roundings differ by about eps32 |s2|,
and P = 2^(s2 - lse2) turned that into an error of dK and dV that the row's lse2 does not share: cloud by cloud dK and dV were up to
5.7 x as far from float64 as the restatement (dV at big_logits * 8: 2.1e-5 against 6.1e-6) while O, D and dQ sat at 1.0 - 1.8 x, and six of
the eight cases missed the bound on dK.  Now the loader waves store the Q tile times scale2, the logits are the forward's own products,
dK leaves the kernel times ln 2 = scale / scale2, and dK and dV follow the restatement like the rest (at most 1.7 x); the two backward
launches take the time they took (243 us at 32 x 1024 x 1024, 80 us at 8).

Measured on an MI355X, worst cloud of any shape, as a fraction of the cloud's largest float64 entry (bound 1e-5):
                 O        lse2     D        dQ       dK       dV
  benign         1.5e-6   4.2e-7   3.1e-6   2.1e-6   2.4e-6   1.7e-6
  ascending      1.9e-6   1.8e-7   1.6e-6   2.5e-6   1.4e-6   1.3e-6
  descending     1.5e-6   2.0e-7   1.3e-6   3.6e-6   1.1e-6   1.1e-6
  one_hot        3.4e-7   8.5e-8   4.0e-7   1.2e-6   2.3e-6   3.4e-7
  equal_keys     4.9e-7   3.5e-7   4.1e-7   1.8e-7   6.3e-7   8.1e-7      (dQ: of the terms that cancel)
  zero_q         6.3e-7   1.1e-7   4.6e-7   8.0e-7   0        6.1e-7      lse2 - log2 nk: 0 where nk is a power of two, else below one ulp
The ill-conditioned sets, kernel / float32 restatement / float32 three-op path (torch on the CPU, the trainer's flash_attn = False
arithmetic), worst cloud; the asserted bound is max(1e-5, twice the restatement's error of the same cloud):
  (64, 512, 64)  wide forward and dQ, split dK|dV
    k_offset, max |s2| 70     O 5.0e-6 / 5.0e-6 / 6.0e-6   dQ 9.0e-6 / 8.4e-6 / 5.7e-6   dK 3.6e-6 / 3.6e-6 / 3.7e-6   dV 2.9e-6 / 2.9e-6 / 2.1e-6
    k_offset, max |s2| 280    O 1.9e-5 / 1.9e-5 / 2.4e-5   dQ 3.4e-5 / 3.8e-5 / 2.1e-5   dK 1.2e-5 / 1.2e-5 / 1.5e-5   dV 1.1e-5 / 1.1e-5 / 9.7e-6
    big_logits * 4.5 (157)    O 9.7e-6 / 9.7e-6 / 7.7e-6   dQ 9.2e-6 / 9.2e-6 / 1.1e-5   dK 7.8e-6 / 7.8e-6 / 7.2e-6   dV 3.4e-6 / 3.4e-6 / 1.8e-6
    big_logits * 8 (480)      O 2.4e-5 / 2.4e-5 / 2.3e-5   dQ 3.4e-5 / 3.4e-5 / 4.1e-5   dK 2.5e-5 / 2.5e-5 / 2.9e-5   dV 6.1e-6 / 6.1e-6 / 5.0e-6
  (64, 96, 512)  split forward and dQ, wide dK|dV, every operand strided
    k_offset, max |s2| 70     O 7.5e-6 / 7.5e-6 / 6.7e-6   dQ 2.0e-5 / 1.5e-5 / 1.0e-5   dK 5.2e-6 / 5.1e-6 / 1.0e-5   dV 5.5e-6 / 5.5e-6 / 4.5e-6
    k_offset, max |s2| 280    O 2.1e-5 / 2.1e-5 / 2.0e-5   dQ 4.1e-5 / 8.1e-5 / 3.6e-5   dK 2.4e-5 / 2.4e-5 / 2.3e-5   dV 2.3e-5 / 2.3e-5 / 1.7e-5
    big_logits * 4.5 (175)    O 9.6e-6 / 9.5e-6 / 8.0e-6   dQ 1.5e-5 / 1.5e-5 / 1.6e-5   dK 1.5e-5 / 1.5e-5 / 1.5e-5   dV 5.5e-6 / 5.6e-6 / 5.8e-6
    big_logits * 8 (512)      O 2.3e-5 / 2.3e-5 / 2.2e-5   dQ 5.1e-5 / 5.1e-5 / 5.0e-5   dK 5.1e-5 / 5.1e-5 / 5.0e-5   dV 1.4e-5 / 1.4e-5 / 1.8e-5
  D follows O (1.7e-5 / 2.9e-5 at 480 / 512); lse2 stays below 5e-7 of max(1, max |lse2|) everywhere.  Cloud by cloud the kernel is at most
  1.85 x the restatement in any output above the 1e-5 floor.  The recomputation costs about eps32 max |s2| (1.2e-7 x 280 = 3.3e-5), as
  the three-op path does: neither arithmetic is better conditioned than the other.

Mutations (arithmetic only, on a scratch build) and the tests of this file that fail under each, all others passing:
  alpha = 1 in fa_train_fwd_kernel                       every case in which a wave meets a second tile: 16 of test_paths_and_layouts, the
                                                         ascending and one_hot cases of those 8 shapes (descending, where the maximum never
                                                         moves, rightly passes), all 8 of test_ill_conditioned_inputs
  wsc[li] for wsc[w * 32 + li] in the split combine      every case whose forward is split: 18 of test_paths_and_layouts, 27 of test_inputs
                                                         (ascending, descending, one_hot), the 4 split-forward cases of
                                                         test_ill_conditioned_inputs, test_refusals_write_nothing's final valid call
  no final multiplier in the wide dK store               every case whose dK|dV is wide, (64, 96, 512), (257, 32, 128), (64, 64, 512): 6 of
                                                         test_paths_and_layouts, 12 of test_inputs (zero_q has dK == 0), 4 ill-conditioned
  lse2 and D swapped in load_stat of the dK|dV loader    95 of 96: everything that runs the backward
  Dq = dsum (one half-wave) in fa_train_bwd_dq_kernel    93 of 96: everything but the two determinism cases
  logits of dK|dV as Q * (K * scale2), as they were      6 of test_ill_conditioned_inputs: k_offset280, big_logits4.5, big_logits8 at both
                                                         shapes, on dK; no other test of the suite notices"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_train_oracle as AO  # noqa: E402
import train_ops_oracle as TO  # noqa: E402
from train_ops_oracle import F32, INVALID, SENT, Guarded, Strided, close, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 0.125
NAMES = ("O", "lse2", "D", "dQ", "dK", "dV")


@pytest.fixture(autouse=True)
def _release():
    yield
    TO.release()


@pytest.fixture(scope="module")
def L():
    from dispu_amd import _lib
    return _lib


def path(b, rows, streamed):
    """(split, remap, stages, tiles in the last stage beyond full ones) of a kernel that owns `rows` columns per cloud and streams
    `streamed` rows in 32-row tiles.  The first line is ft_split, restated."""
    split = rows % 128 != 0 or b * (rows // 128) < 256
    per_stage, tiles = (4 if split else 1), streamed // 32
    return split, b % 8 == 0, -(-tiles // per_stage), tiles % per_stage


S, W = True, False          # split (32 columns, 4 tiles per stage) / wide (128 columns, 1 tile per stage)
SHAPES = [
    # (b, m, nk), path of forward and dQ, path of dK|dV: (split, remap, stages, tail)
    ((257, 128, 32), (W, False, 1, 0), (S, False, 1, 0)),     # wide without the remap (ft_block's identity branch), one stage | one full split stage
    ((64, 512, 64), (W, True, 2, 0), (S, True, 4, 0)),        # wide, two stages: the prologue's second load, no third | four full split stages
    ((64, 96, 512), (S, True, 4, 0), (W, True, 3, 0)),        # four full split stages | wide, three stages: the loop's own load
    ((257, 32, 128), (S, False, 1, 0), (W, False, 1, 0)),     # one full split stage, no remap | wide without the remap, one stage
    ((3, 160, 160), (S, False, 2, 1), (S, False, 2, 1)),      # a tail of one tile behind a full stage
    ((2, 192, 192), (S, False, 2, 2), (S, False, 2, 2)),      # a tail of two
    ((1, 352, 352), (S, False, 3, 3), (S, False, 3, 3)),      # three stages, a tail of three; a single cloud
    ((5, 64, 288), (S, False, 3, 1), (S, False, 1, 2)),       # three stages with a tail of one | one stage of two tiles
    ((8, 64, 64), (S, True, 1, 2), (S, True, 1, 2)),          # waves 2 and 3 of the split workgroup never get a tile, with the remap
    ((2, 32, 64), (S, False, 1, 2), (S, False, 1, 1)),        # ... and three idle waves in dK|dV, one column block per cloud
    ((64, 512, 96), (W, True, 3, 0), (S, True, 4, 0)),        # the wide forward and dQ with three stages
    ((64, 64, 512), (S, True, 4, 0), (W, True, 2, 0)),        # the wide dK|dV with two
]
SHAPE_IDS = ["x".join(str(v) for v in s[0]) for s in SHAPES]
ILL_SHAPES = [(64, 512, 64), (64, 96, 512)]     # between them every kernel in both workgroup shapes: wide fwd / dQ + split dK|dV, and the reverse


def test_every_case_takes_the_path_it_claims():
    seen = set()
    for (b, m, nk), fwd, dkv in SHAPES:
        assert m % 32 == 0 and nk % 32 == 0 and b * m * nk <= 3.2e6
        assert path(b, m, nk) == fwd, (b, m, nk, path(b, m, nk))
        assert path(b, nk, m) == dkv, (b, m, nk, path(b, nk, m))
        seen |= {("q",) + fwd, ("k",) + dkv}
    for who in "qk":        # both workgroup shapes with and without the remap, and 1, 2 and >= 3 stages of each
        assert {(s, r) for w, s, r, _, _ in seen if w == who} == {(S, True), (S, False), (W, True), (W, False)}
        for split in (S, W):
            assert {min(n, 3) for w, s, _, n, _ in seen if w == who and s == split} == {1, 2, 3}
    assert {t for w, s, _, n, t in seen if w == "q" and s == S} == {0, 1, 2, 3}
    assert {(n, t) for w, s, _, n, t in seen if s == S and n > 1 and t} >= {(2, 1), (2, 2), (3, 3), (3, 1)}     # partial tails behind full stages
    assert all(path(*s)[0] != path(s[0], s[2], s[1])[0] for s in ILL_SHAPES)


@functools.lru_cache(maxsize=2)
def case(kind, b, m, nk):
    """inputs and float64 reference of a case, computed once and shared by the tests that use it (never modified)."""
    q, k, v, do = AO.build(kind, b, m, nk)
    O, lse2 = AO.forward(q, k, v, SCALE)
    dQ, dK, dV, Dv = AO.backward(q, k, v, do, SCALE)
    for a in (q, k, v, do, O, lse2, dQ, dK, dV, Dv):
        a.setflags(write=False)
    return (q, k, v, do), dict(O=O, lse2=lse2, D=Dv, dQ=dQ, dK=dK, dV=dV)


def written(a, what):
    a = np.asarray(a)
    assert np.isfinite(a).all(), what + ": not finite"
    assert not (a == F32(SENT)).any(), "%s: %d elements of its window were never written" % (what, int((a == F32(SENT)).sum()))


class Launch(object):
    """buffers of one forward + backward call pair in one of the two layouts, and the two calls."""

    def __init__(self, dev, b, m, nk, q, k, v, do, strided):
        self.dev, self.b, self.m, self.nk = dev, b, m, nk
        rq, rk = b * m, b * nk
        if strided:
            self.sq, self.so = Strided(dev, rq, 64, 68, 4, q), Strided(dev, rq, 64, 72, 8)
            self.sdo, self.sdq = Strided(dev, rq, 64, 80, 12, do), Strided(dev, rq, 64, 72, 4)
            self.sk, self.sv = Strided(dev, rk, 64, 72, 4, k), Strided(dev, rk, 64, 84, 16, v)
            self.sdk, self.sdv = Strided(dev, rk, 64, 68, 0), Strided(dev, rk, 64, 88, 20)
            self.K, self.V = (self.sk.ptr(), 72), (self.sv.ptr(), 84)
            self.dK, self.dV = (self.sdk.ptr(), 68), (self.sdv.ptr(), 88)
            self.inputs, self.kv_out = [self.sq, self.sk, self.sv, self.sdo], [self.sdk, self.sdv]
        else:       # the trainer's: compact rows, K|V one 128-wide buffer, dK|dV another
            self.sq, self.so = Strided(dev, rq, 64, 64, 0, q), Strided(dev, rq, 64, 64, 0)
            self.sdo, self.sdq = Strided(dev, rq, 64, 64, 0, do), Strided(dev, rq, 64, 64, 0)
            self.skv = Strided(dev, rk, 128, 128, 0, np.concatenate([k.reshape(rk, 64), v.reshape(rk, 64)], 1))
            self.sdkv = Strided(dev, rk, 128, 128, 0)
            self.K, self.V = (self.skv.ptr(), 128), (self.skv.G.ptr(64), 128)
            self.dK, self.dV = (self.sdkv.ptr(), 128), (self.sdkv.G.ptr(64), 128)
            self.inputs, self.kv_out = [self.sq, self.skv, self.sdo], [self.sdkv]
        self.strided = strided
        self.glse, self.gd = Guarded(dev, rq), Guarded(dev, rq)

    def forward(self, L, **kw):
        a = dict(b=self.b, m=self.m, nk=self.nk, d=64, Q=self.sq.ptr(), ldq=self.sq.ld, K=self.K[0], ldk=self.K[1], V=self.V[0], ldv=self.V[1],
                 scale=SCALE, O=self.so.ptr(), ldo=self.so.ld, lse2=self.glse.ptr())
        a.update(kw)
        rc = L.lib().dispu_attention_fwd_lse(a["b"], a["m"], a["nk"], a["d"], a["Q"], a["ldq"], a["K"], a["ldk"], a["V"], a["ldv"], a["scale"],
                                             a["O"], a["ldo"], a["lse2"], L.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def backward(self, L, **kw):
        a = dict(b=self.b, m=self.m, nk=self.nk, d=64, Q=self.sq.ptr(), ldq=self.sq.ld, K=self.K[0], ldk=self.K[1], V=self.V[0], ldv=self.V[1],
                 scale=SCALE, O=self.so.ptr(), ldo=self.so.ld, lse2=self.glse.ptr(), dO=self.sdo.ptr(), lddo=self.sdo.ld, dQ=self.sdq.ptr(),
                 lddq=self.sdq.ld, dK=self.dK[0], lddk=self.dK[1], dV=self.dV[0], lddv=self.dV[1], dvec=self.gd.ptr())
        a.update(kw)
        rc = L.lib().dispu_attention_bwd(a["b"], a["m"], a["nk"], a["d"], a["Q"], a["ldq"], a["K"], a["ldk"], a["V"], a["ldv"], a["scale"], a["O"],
                                         a["ldo"], a["lse2"], a["dO"], a["lddo"], a["dQ"], a["lddq"], a["dK"], a["lddk"], a["dV"], a["lddv"],
                                         a["dvec"], L.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def outputs_untouched(self, forward_too=True):
        outs = [self.sdq, self.gd] + self.kv_out + ([self.so, self.glse] if forward_too else [])
        return all(o.untouched() if isinstance(o, Strided) else (o.guards_intact() and same_bits(o.body(), np.full(o.n, SENT, F32))) for o in outs)

    def run(self, L, what):
        """both calls and every check that does not need a reference -> dict of the six outputs, [b, ...]."""
        b, m, nk = self.b, self.m, self.nk
        L.check(self.forward(L), "attention_fwd_lse")
        assert self.outputs_untouched(forward_too=False), what + ": the forward wrote a backward output"
        O_bits, lse_bits = self.so.full().copy(), self.glse.body().copy()
        written(self.so.data(), what + " O")
        written(lse_bits, what + " lse2")
        assert self.so.rest_untouched() and self.glse.guards_intact(), what + ": the forward wrote outside O or lse2"
        assert all(s.untouched() for s in self.inputs), what + ": the forward changed an input"
        L.check(self.backward(L), "attention_bwd")
        assert all(s.untouched() for s in self.inputs), what + ": the backward changed an input"
        assert same_bits(self.so.full(), O_bits) and same_bits(self.glse.body(), lse_bits) and self.glse.guards_intact(), what + ": the backward changed O or lse2"
        assert self.sdq.rest_untouched() and self.gd.guards_intact() and all(s.rest_untouched() for s in self.kv_out), what + ": the backward wrote outside a window"
        if self.strided:
            dk, dv_ = self.sdk.data(), self.sdv.data()
        else:
            dk, dv_ = self.sdkv.data()[:, :64], self.sdkv.data()[:, 64:]
        got = dict(O=self.so.data().reshape(b, m, 64), lse2=lse_bits.reshape(b, m), D=self.gd.body().reshape(b, m),
                   dQ=self.sdq.data().reshape(b, m, 64), dK=dk.reshape(b, nk, 64), dV=dv_.reshape(b, nk, 64))
        for n in NAMES:
            written(got[n], "%s %s" % (what, n))
        return got


def hold(got, ref, bound, what, floor=None):
    """per cloud: max |got - ref| <= bound (a number or [b]) x the cloud's own largest |ref| (not below floor [b]); the worst cloud is
    printed before anything is asserted."""
    e = AO.cloud_errors(got, ref, floor)
    bound = np.broadcast_to(np.asarray(bound, np.float64), e.shape)
    w = int((e / bound).argmax())
    print("[measured] %s: worst cloud %d of %d: %.2e of its largest entry (bound %.1e)" % (what, w, e.size, e[w], bound[w]))
    assert (e <= bound).all(), "%s: %d clouds beyond the bound, cloud %d at %.2e (bound %.1e)" % (what, int((e > bound).sum()), w, e[w], bound[w])
    return float(e.max())


def lse_floor(ref):
    """lse2 is compared against max(1, max |lse2|) of its cloud."""
    return np.ones(ref.shape[0])


def compare(got, ref, what, bounds=None, dq_floor=None):
    for n in NAMES:
        hold(got[n], ref[n], 1e-5 if bounds is None else bounds[n], "%s %s" % (what, n),
             lse_floor(ref[n]) if n == "lse2" else dq_floor if n == "dQ" else None)


# ------------------------------------------------------------------------------------- every path, both layouts ----
@pytest.mark.parametrize("strided", [False, True], ids=["trainer", "strided"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_paths_and_layouts(dev, L, shape, strided):
    b, m, nk = shape[0]
    (q, k, v, do), ref = case("benign", b, m, nk)
    what = "benign %dx%dx%d %s" % (b, m, nk, "strided" if strided else "trainer")
    compare(Launch(dev, b, m, nk, q, k, v, do, strided).run(L, what), ref, what)


# ----------------------------------------------------------------------------------- inputs that stress the softmax ----
@pytest.mark.parametrize("kind", AO.WELL[1:])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_inputs(dev, L, shape, kind):
    """the layout alternates with the case, so each kind meets both."""
    b, m, nk = shape[0]
    (q, k, v, do), ref = case(kind, b, m, nk)
    strided = (SHAPES.index(shape) + AO.WELL.index(kind)) % 2 == 1
    what = "%s %dx%dx%d %s" % (kind, b, m, nk, "strided" if strided else "trainer")
    got = Launch(dev, b, m, nk, q, k, v, do, strided).run(L, what)
    compare(got, ref, what, dq_floor=AO.dq_cancelled(q, k, v, do, SCALE) if kind == "equal_keys" else None)
    if kind == "zero_q":
        # every logit is zero: lse2 = log2 nk to an ulp, every query of a cloud gets the same O by the same operations, dK = 0 exactly
        want = np.log2(nk)
        print("[measured] %s: lse2 - log2 nk within %.2e (one ulp is %.2e)" % (what, np.abs(got["lse2"] - want).max(), np.spacing(F32(want))))
        assert np.abs(got["lse2"].astype(np.float64) - want).max() <= np.spacing(F32(want))
        assert all(same_bits(got["O"][c], np.broadcast_to(got["O"][c, :1], (m, 64))) for c in range(b)), what + ": O differs between queries of a cloud"
        hold(got["O"][:, 0], v.astype(np.float64).mean(1), 1e-5, what + " O vs the column mean of V")
        close(got["lse2"], np.full((b, m), want), 1e-5, what + " lse2 vs log2 nk")
        assert not got["dK"].any(), what + ": dK must be exactly zero"


@pytest.mark.parametrize("kind", AO.ILL)
@pytest.mark.parametrize("shape", ILL_SHAPES, ids=["x".join(str(v) for v in s) for s in ILL_SHAPES])
def test_ill_conditioned_inputs(dev, L, shape, kind):
    """max(1e-5, twice the float32 restatement's own error), per output and per cloud; the three-op float32 error is printed beside it."""
    b, m, nk = shape
    (q, k, v, do), ref = case(kind, b, m, nk)
    what = "%s %dx%dx%d max |s2| %.0f" % (kind, b, m, nk, AO.s2_max(q, k, SCALE))
    r, t = AO.recompute_f32(q, k, v, do, SCALE), AO.three_op_f32(q, k, v, do, SCALE)
    bounds, rest = {}, {}
    for n in NAMES:
        fl = lse_floor(ref[n]) if n == "lse2" else None
        er = rest[n] = AO.cloud_errors(r[n], ref[n], fl)
        bounds[n] = np.maximum(1e-5, 2.0 * er)
        print("[measured] %s %s: restatement %.2e%s" % (what, n, er.max(), ", three-op float32 %.2e" % AO.cloud_errors(t[n], ref[n]).max() if n in t else ""))
    got = Launch(dev, b, m, nk, q, k, v, do, ILL_SHAPES.index(shape) == 1).run(L, what)
    for n in NAMES:
        ek = AO.cloud_errors(got[n], ref[n], lse_floor(ref[n]) if n == "lse2" else None)
        print("[measured] %s %s: kernel %.2e (restatement %.2e) over the clouds; cloud by cloud the kernel is at most %.2f x the restatement" % (
            what, n, ek.max(), rest[n].max(), (ek / np.maximum(rest[n], 1e-300)).max()))
    compare(got, ref, what, bounds)


# ------------------------------------------------------------------------------------------------- determinism ----
@pytest.mark.parametrize("shape", ILL_SHAPES, ids=["x".join(str(v) for v in s) for s in ILL_SHAPES])
def test_two_calls_give_the_same_bits(dev, L, shape):
    """no float atomics and a fixed combine order: all six outputs, in both workgroup shapes of every kernel."""
    b, m, nk = shape
    (q, k, v, do), _ = case("benign", b, m, nk)
    one = Launch(dev, b, m, nk, q, k, v, do, False).run(L, "first call")
    two = Launch(dev, b, m, nk, q, k, v, do, False).run(L, "second call")
    for n in NAMES:
        assert same_bits(one[n], two[n]), "%s differs between two calls" % n


# --------------------------------------------------------------------------------------------------- refusals ----
def test_refusals_write_nothing(dev, L):
    """every refused call returns hipErrorInvalidValue and leaves every output holding its sentinel.  The buffers are sized for
    (2, 64, 96) and no refused call names a larger shape."""
    b, m, nk = 2, 64, 96
    (q, k, v, do), ref = case("benign", b, m, nk)
    la = Launch(dev, b, m, nk, q, k, v, do, True)
    odd = {"Q": la.sq.G.ptr(5), "K": la.sk.G.ptr(5), "V": la.sv.G.ptr(17), "O": la.so.G.ptr(9), "dO": la.sdo.G.ptr(13), "dQ": la.sdq.G.ptr(5),
           "dK": la.sdk.G.ptr(1), "dV": la.sdv.G.ptr(21)}                     # each window's pointer, one float on
    lds = {"Q": "ldq", "K": "ldk", "V": "ldv", "O": "ldo", "dO": "lddo", "dQ": "lddq", "dK": "lddk", "dV": "lddv"}
    shapes = [dict(m=48), dict(m=33), dict(nk=48), dict(nk=95), dict(d=32), dict(d=128), dict(d=0), dict(b=-1), dict(m=0), dict(m=-32), dict(nk=0),
              dict(nk=-32)]
    calls = 0
    for fn, ptrs, nulls in [(la.forward, ("Q", "K", "V", "O"), ("lse2",)), (la.backward, ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"), ("lse2", "dvec"))]:
        bad = list(shapes) + [{n: None} for n in ptrs + nulls] + [{n: odd[n]} for n in ptrs]
        for n in ptrs:
            base = dict(Q=68, K=72, V=84, O=72, dO=80, dQ=72, dK=68, dV=88)[n]
            bad += [{lds[n]: base + 1}, {lds[n]: base + 2}, {lds[n]: base - 1}]
        for kw in bad:
            assert fn(L, **kw) == INVALID, "%s(%s) was not refused" % (fn.__name__, kw)
            calls += 1
        assert la.outputs_untouched() and all(s.untouched() for s in la.inputs), fn.__name__ + ": a refused call wrote"
        assert fn(L, b=0) == 0                                           # nothing to do
        assert la.outputs_untouched() and all(s.untouched() for s in la.inputs), fn.__name__ + ": b == 0 wrote"
    assert calls == 2 * len(shapes) + (4 + 1 + 4 + 12) + (8 + 2 + 8 + 24)
    compare(la.run(L, "the same arguments, valid"), ref, "after the refusals")      # the base arguments are valid: the refusals were the overrides'
