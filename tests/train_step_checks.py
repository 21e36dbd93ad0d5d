"""The end-to-end checks of one training step against oracle/train_oracle.py (float64 torch autograd), for any batch [B, N, 3]
Trainer.forward accepts.  tests/test_train_gpu.py applies them at (2, 256), tests/test_train_shapes_gpu.py at the shapes where
dis-pu_amd/train.py takes another path, tests/test_train_shapes.py (CPU) applies the same measures to the oracle run in float32
against itself in float64, which is how the inputs of the shape cases were chosen.

Bounds (the project's, the same at every shape): forward, moving statistics and the tapped intermediates 1e-5 of each tensor's
scale; loss terms 2e-5; activation gradients row-wise, median <= 1e-5 and at most 1 % of rows above 1e-3 (an fp32 forward takes
another ReLU / max / arg-min branch than float64 at near-ties, which changes single ROWS by O(1), see tests/test_train_gpu.py);
parameter gradients relative L2 <= 3e-3 and relative max <= 2e-2; the first Adam update within 2e-2 * lr where |g| > 1e-3 max|g|.
The forward is continuous: its checks have no row allowance.

A plain helper module (like tests/train_ops_oracle.py): no test lives here."""
import numpy as np
import torch

from oracle import generator as OG
from oracle import train_oracle as T

DEAD = "refine/PointShuffle/weight_net/wconv0/biases"      # a bias in front of BatchNorm: its gradient is identically 0
WATCH = ("dc1", "dc2", "dc3", "dc4", "coarse", "fine", "fine_feat")
DC_COLS = {1: (360, 456), 2: (240, 360), 3: (120, 240), 4: (0, 120)}      # columns of dense block d in the 480-wide feature buffer
ROW_MEDIAN, ROW_OFF, ROW_SHARE = 1e-5, 1e-3, 0.01
# (B, N, synth seed) of the shape cases: the smallest batches that reach each path of dis-pu_amd/train.py (the table in
# tests/test_train_shapes_gpu.py); every seed is the first one tests/test_train_shapes.py accepts for its shape
SHAPE_CASES = ((2, 24, 2), (2, 40, 1), (4, 64, 4), (1, 128, 1), (1, 512, 4), (1, 1024, 7), (68, 64, 1))
GRAD_L2, GRAD_MAX = 3e-3, 2e-2


def N_(t):
    return t.detach().cpu().numpy()


def close(a, ref, rel, what=""):
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(np.asarray(a, np.float64) - ref).max()
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)
    return err / scale


# ------------------------------------------------------------------------------------------------- the reference ----
_ORACLE = {}


def oracle_step(B, N, seed):
    """One oracle evaluation of the step on synth.patch_with_gt(B, N, 4N, seed) with radii linspace(1, 1.3, B), the parameters
    init_params(1234, bias_scale=0.05, bn_random=True) and epoch 0, in the oracle's current precision (T.DT).  Computed once per
    process and shared: callers must not modify what they get."""
    key = (B, N, seed, T.DT)
    if key not in _ORACLE:
        from dispu_amd import synth
        P = OG.init_params(seed=1234, bias_scale=0.05, bn_random=True)
        x, gt = synth.patch_with_gt(B, N, 4 * N, seed=seed)
        radius = np.linspace(1.0, 1.3, B).astype(np.float32)
        act, taps = {}, {}
        loss, terms, grads, bn, (coarse, fine) = T.loss_and_grads(P, x, gt, radius, epoch=0, act_grads=act, fwd_taps=taps)
        _ORACLE[key] = dict(P=P, x=x, gt=gt, radius=radius,
                            ref=dict(loss=loss, terms=terms, grads=grads, bn=bn, coarse=coarse, fine=fine, act=act, taps=taps))
    return _ORACLE[key]


# --------------------------------------------------------------------------------------------------- the measures ----
def row_errors(h, r):
    return np.linalg.norm(h - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-30)


def rowwise(pairs):
    """{name: (have, ref)} of [rows, C] arrays -> {name: (median row error, share of rows above 1e-3, rows, indices of those rows)}"""
    out = {}
    for k, (h, r) in pairs.items():
        e = row_errors(np.asarray(h, np.float64), np.asarray(r, np.float64))
        out[k] = (float(np.median(e)), float((e > ROW_OFF).mean()), e.shape[0], np.nonzero(e > ROW_OFF)[0])
    return out


def grad_measures(got, ref):
    """-> {name: (relative L2, relative max)} over every parameter gradient but the dead bias"""
    out = {}
    for k, r in ref.items():
        if k == DEAD:
            continue
        g = np.asarray(got[k], np.float64)
        out[k] = (float(np.linalg.norm(g - r) / np.linalg.norm(r)), float(np.abs(g - r).max() / np.abs(r).max()))
    return out


def activation_pairs(B, N, have, act, agg):
    """the seven watched activation gradients as {name: (have, ref)} row matrices: dc1..dc4 [B*N, .], coarse / fine [B*4N, 3] and
    fine_feat [B*4N, 256].  have["fine_feat"] is the gradient ALREADY masked by relu'(agg), as the backward leaves it in `dagg`; the
    reference's gets the same mask, from `agg`, the forward values of the side under test."""
    rn, rm = B * N, B * 4 * N
    pairs = {k: (np.asarray(have[k], np.float64).reshape(rn if k.startswith("dc") else rm, -1),
                 np.asarray(act[k], np.float64).reshape(rn if k.startswith("dc") else rm, -1)) for k in WATCH}
    h, r = pairs["fine_feat"]
    pairs["fine_feat"] = (h, r * (np.asarray(agg).reshape(rm, 256) > 0))
    return pairs


def float32_proxy(B, N, seed, set_dt):
    """The oracle in float32 against itself in float64 on one case: how far rounding alone moves the checked quantities, with no
    device involved.  set_dt(dtype) sets oracle.train_oracle.DT (a test passes a monkeypatch).
    -> (most flagged rows of a watched tensor, worst share of flagged rows, worst relative L2 of a parameter gradient)"""
    set_dt(torch.float64)
    r64 = oracle_step(B, N, seed)["ref"]
    set_dt(torch.float32)
    r32 = oracle_step(B, N, seed)["ref"]
    mask = r32["taps"]["fine_feat"] > 0
    have = dict(r32["act"], fine_feat=r32["act"]["fine_feat"] * mask)
    m = rowwise(activation_pairs(B, N, have, r64["act"], r32["taps"]["fine_feat"]))
    g = grad_measures(r32["grads"], r64["grads"])
    return max(len(v[3]) for v in m.values()), max(v[1] for v in m.values()), max(v[0] for v in g.values())


# ------------------------------------------------------------------------------------------------ the device step ----
def run_step(dev, B, N, seed, dtype="f32"):
    """oracle_step(B, N, seed) and ONE fresh Trainer on it: zero_grad, forward, loss_backward, backward."""
    from dispu_amd.train import Trainer
    o = oracle_step(B, N, seed)
    tr = Trainer(params=o["P"], device=dev, dtype=dtype)
    dx, dgt, dr = (torch.from_numpy(np.ascontiguousarray(o[k])).to(dev) for k in ("x", "gt", "radius"))
    tr.zero_grad()
    c, f = tr.forward(dx)
    t = tr.loss_backward(dgt, dr)
    tr.backward()
    torch.cuda.synchronize()
    return dict(o, tr=tr, c=N_(c), f=N_(f), t=t, dev_inputs=(dx, dgt, dr))


def check_training_forward(step, B, N):
    ref, tr = step["ref"], step["tr"]
    assert step["c"].shape == (B, 4 * N, 3) and step["f"].shape == (B, 4 * N, 3)
    close(step["c"], ref["coarse"], 1e-5, "coarse")
    close(step["f"], ref["fine"], 1e-5, "fine")
    close(N_(tr.moving_mean), ref["bn"]["moving_mean"], 1e-5, "moving_mean")
    close(N_(tr.moving_var), ref["bn"]["moving_variance"], 1e-5, "moving_variance")


def check_intermediates(step, B, N):
    """the forward values the oracle taps, stage by stage: the 480-wide dense-block features, duplicate_up's output and
    PointShuffle2's output (relu(aggregation)).  -> {name: error / scale}"""
    ws, taps = step["tr"]._ws[(B, N)], step["ref"]["taps"]
    rn, rm = B * N, B * 4 * N
    return {name: close(N_(ws[buf]), taps[name].reshape(rows, c), 1e-5, "%s (workspace %r)" % (name, buf))
            for name, buf, rows, c in (("feat480", "feat", rn, 480), ("up128", "up128", rm, 128), ("fine_feat", "agg", rm, 256))}


def check_loss_terms(step, B, N):
    t, ref = step["t"], step["ref"]
    for k in ("dis_coarse_cd", "dis_fine_cd", "repulsion_loss"):
        assert abs(float(t[k]) - ref["terms"][k]) <= 2e-5 * max(abs(ref["terms"][k]), 1e-3), (k, float(t[k]), ref["terms"][k])
    assert abs(float(t["pu_loss"]) - ref["loss"]) <= 2e-5 * abs(ref["loss"]), (float(t["pu_loss"]), ref["loss"])


def check_activation_gradients_rowwise(step, B, N):
    """-> (worst median row error, worst share of rows above 1e-3) over the seven watched tensors"""
    ws, act = step["tr"]._ws[(B, N)], step["ref"]["act"]
    dfeat = N_(ws["dfeat"])
    have = {"dc%d" % d: dfeat[:, a:b] for d, (a, b) in DC_COLS.items()}
    have.update(coarse=N_(ws["dcoarse"]), fine=N_(ws["dfine"]), fine_feat=N_(ws["dagg"]))
    m = rowwise(activation_pairs(B, N, have, act, N_(ws["agg"])))
    for k, (med, share, rows, off) in m.items():
        assert med <= ROW_MEDIAN, (k, med)
        assert share <= ROW_SHARE, (k, "%d of %d rows" % (len(off), rows), off[:10])
    return max(v[0] for v in m.values()), max(v[1] for v in m.values())


def check_gradients(step, B, N):
    """-> worst relative L2 over the parameter gradients"""
    got, ref = step["tr"].grads(), step["ref"]["grads"]
    assert set(got) == set(ref)
    assert np.abs(got[DEAD]).max() <= 1e-4 * np.abs(ref[DEAD.replace("biases", "weights")]).max()   # fp32 cancellation residue
    m = grad_measures(got, ref)
    bad = {k: v for k, v in m.items() if v[0] > GRAD_L2 or v[1] > GRAD_MAX}
    assert not bad, "gradient mismatch (rel L2, rel max): %s" % bad
    return max(v[0] for v in m.values())


def check_train_step_matches_oracle_adam(step, B, N, dev):
    """a fresh Trainer.train_step == oracle loss_and_grads + adam_step (first step, t = 1)."""
    from dispu_amd.train import Trainer
    P, ref = step["P"], step["ref"]
    tr = Trainer(params=P, device=dev)
    tr.train_step(*step["dev_inputs"])
    torch.cuda.synchronize()
    newP = T.adam_step(P, ref["grads"], {}, 1e-3)
    got = tr.params()
    # the first Adam step moves every coordinate by ~lr * sign(g): compare where |g| is not negligible
    for k, g in ref["grads"].items():
        if k.endswith("weight_net/wconv0/biases"):
            continue          # true gradient is 0 (bias in front of BN): Adam normalises pure rounding noise there
        big = np.abs(g) > 1e-3 * np.abs(g).max()
        if not big.any():
            continue
        upd, upd_ref = got[k].astype(np.float64) - P[k], newP[k] - P[k]
        assert np.abs(upd - upd_ref)[big].max() <= 2e-2 * 1e-3, k
    assert tr.adam_t == 1 and tr.global_step == 1


# ------------------------------------------------------------------------------------------- which path a step took ----
class RecordingLib(object):
    """What _lib.tape_lib() returns, seen through a recorder: every C entry called through it is appended to `names`, then runs
    as usual.  A test installs it with monkeypatch.setattr(_lib, "tape_lib", lambda: rec); the library itself is untouched."""

    def __init__(self, real):
        self._real = real
        self.names = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call

    def count(self, name):
        return self.names.count(name)

    def launches(self):
        """the recorded calls a launch tape would hold (the rule of _lib._TapeLib: int-returning, no size or plan query)"""
        from dispu_amd import _lib
        return [n for n in self.names if n not in _lib._NO_TAPE and "scratch" not in n and getattr(_lib.lib(), n).restype is _lib._i]


def recording(monkeypatch):
    from dispu_amd import _lib
    rec = RecordingLib(_lib.tape_lib())
    monkeypatch.setattr(_lib, "tape_lib", lambda: rec)
    return rec
