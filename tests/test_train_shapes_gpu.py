"""The training step against the float64 oracle (oracle/train_oracle.py) at every kind of batch Trainer.forward accepts, not only
(2, 256): dis-pu_amd/train.py switches code paths on B and N, and the single-kernel suites cannot see the trainer's glue on those
paths -- offsets into the 480-wide feature buffer, leading dimensions, which buffer a branch reads, a scratch buffer sized by
another shape, an accumulator zero-filled for one shape and used at the next.

Each case is the smallest batch that reaches its path; each must PROVE it took that path (test_step_takes_the_path_it_was_chosen_for,
from the C entries a recording proxy around _lib.tape_lib() sees), then passes the checks of tests/train_step_checks.py with the
bounds of tests/test_train_gpu.py, unchanged.  The synth seeds are the ones tests/test_train_shapes.py accepts (the float32 oracle
against the float64 one: at most half the row allowance), so that the 1 % row allowance cannot hide a failure.

    (B, N, seed)     what only it reaches
    (2, 24, 2)       smallest legal N (17 of 24 points are neighbours); 96-row clouds under the 64-row tiles of the head chains;
                     rm = B * 4N = 192, no multiple of 128: after_conv through _lin, no split-K; attention at 3 tiles of 32
    (2, 40, 1)       160-row clouds, rm = 320: the other remainder of the 64- and 128-row tilings
    (4, 64, 4)       split-K with nsp = 8 at rm = 1024, four clouds
    (1, 128, 1)      B = 1: BatchNorm statistics of one cloud, a single entry in every batched launch
    (1, 512, 4)      N > 256: the forward without the fused stem (layer0 alone, k-NN + edge_dense_conv + a prep product per block)
    (1, 1024, 7)     4N = 4096, the accepted maximum
    (68, 64, 1)      rm = 17408 > 16384: defer_side off, after_conv through _lin on the large side (the slowest oracle evaluation)

Measured on an MI355X in one run (nothing in the tests is tuned to these; -s prints them; the last digit moves with the float atomics):
    (B, N)       intermediates, error / scale        activation gradients, row-wise           parameter gradients
                 feat480   up128     fine_feat       worst median   rows above 1e-3, worst    worst rel L2   worst rel max
    (2, 24)      6.1e-07   7.0e-07   2.6e-06         7.4e-07        0                         3.5e-06        3.4e-06
    (2, 40)      6.0e-07   5.4e-07   1.9e-06         7.5e-07        0                         1.9e-06        3.5e-06
    (4, 64)      5.6e-07   7.6e-07   2.1e-06         9.7e-07        0                         2.7e-06        7.0e-06
    (1, 128)     4.3e-07   6.3e-07   2.3e-06         9.9e-07        0                         2.6e-06        3.0e-06
    (1, 512)     6.1e-07   6.4e-07   3.5e-06         1.4e-06        0                         3.9e-06        5.0e-06
    (1, 1024)    6.4e-07   6.7e-07   2.8e-06         1.5e-06        0.10 % (1 of 1024)        1.5e-05        2.0e-05
    (68, 64)     6.9e-07   8.1e-07   2.4e-06         9.2e-07        0.34 % (15 of 4352)       3.8e-05        1.3e-04
    bounds       1e-05     1e-05     1e-05           1e-05          1 %                       3e-03          2e-02

The flagged rows of (1, 1024) and (68, 64) are single rows scattered over the clouds and tensors (at (68, 64): 15, 11, 8 and 1 of the
4352 rows of dc1..dc4, 1 - 2 of the 17408 rows of coarse, fine and fine_feat), every other row agrees to ~1e-6: branch flips at
near-ties, as at (2, 256).  One trainer changing shapes: flat_g within 4e-08 - 2e-07 of its largest entry of a fresh trainer's.
bf16 against f32 at (1, 512) and (2, 40): gradient cosine 1.000000, relative L2 3e-06 and 4e-06 -- every dense product of these small batches lies under
Trainer.bf16_min_macs and stays fp32, what differs is the bf16 storage of the local cell's pair tensors and the products reading them, in the refine branch whose
gradients carry weight_fine = 0.01 at epoch 0.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_checks as K  # noqa: E402

from oracle import generator as OG  # noqa: E402

pytestmark = pytest.mark.gpu

NO_SPLITK = ((2, 24), (2, 40), (68, 64))          # rm % 128 != 0, or rm > 16384


@pytest.fixture(scope="module", params=K.SHAPE_CASES, ids=lambda c: "%d-%d-seed%d" % c)
def case(request, dev):
    """one oracle evaluation and one fresh f32 Trainer per case (K.run_step), with the C entries the step called"""
    B, N, seed = request.param
    with pytest.MonkeyPatch.context() as mp:
        rec = K.recording(mp)
        step = K.run_step(dev, B, N, seed)
    return dict(step, B=B, N=N, seed=seed, calls=rec)


def test_step_takes_the_path_it_was_chosen_for(case):
    """A shape that silently falls onto the common path tests nothing."""
    B, N, rec, tr = case["B"], case["N"], case["calls"], case["tr"]
    if N > 256:
        assert rec.count("dispu_stem_block") == 0
        assert rec.count("dispu_knn_feat_strided") == 4 and rec.count("dispu_edge_dense_conv") == 4 and rec.count("dispu_linear_small_k") == 1
    else:
        assert rec.count("dispu_stem_block") == 4
        assert rec.count("dispu_knn_feat_strided") == 0 and rec.count("dispu_edge_dense_conv") == 0 and rec.count("dispu_linear_small_k") == 0
    assert (rec.count("dispu_linear_splitk_finish") == 0) == ((B, N) in NO_SPLITK)
    assert (tr.defer_side is False) == ((B, N) == (68, 64))
    assert rec.count("dispu_attention_fwd_lse") == 1 and rec.count("dispu_attention_bwd") == 1
    # ... and Trainer.path states the same, without a device
    path = tr.path(B, N)
    assert path.stem == (rec.count("dispu_stem_block") == 4)
    assert path.after_split == (0 if rec.count("dispu_linear_splitk_finish") == 0 else 8) and (path.after_split == 0) == ((B, N) in NO_SPLITK)
    assert path.defer_side is tr.defer_side
    assert path.attention == "flash" and path.local_bwd == "pair" and rec.count("dispu_ps_local_grad") == 0
    assert path.split_skip and rec.count("dispu_ps_skip_max_grad") == 1


def test_training_forward(case):
    K.check_training_forward(case, case["B"], case["N"])


def test_forward_intermediates(case):
    m = K.check_intermediates(case, case["B"], case["N"])
    print("[measured] (%d, %d) forward intermediates, error / scale (bound 1e-05): %s"
          % (case["B"], case["N"], ", ".join("%s %.1e" % kv for kv in m.items())))


def test_loss_terms(case):
    K.check_loss_terms(case, case["B"], case["N"])


def test_activation_gradients_rowwise(case):
    try:
        med, share = K.check_activation_gradients_rowwise(case, case["B"], case["N"])
    finally:
        ws = case["tr"]._ws[(case["B"], case["N"])]
        have = {"dc%d" % d: K.N_(ws["dfeat"])[:, a:b] for d, (a, b) in K.DC_COLS.items()}
        have.update(coarse=K.N_(ws["dcoarse"]), fine=K.N_(ws["dfine"]), fine_feat=K.N_(ws["dagg"]))
        m = K.rowwise(K.activation_pairs(case["B"], case["N"], have, case["ref"]["act"], K.N_(ws["agg"])))
        print("[measured] (%d, %d) activation gradients: worst median row error %.1e (bound 1e-05), worst share of rows above 1e-3 "
              "%.2f %% (bound 1 %%); flagged rows per tensor: %s" % (case["B"], case["N"], max(v[0] for v in m.values()),
                                                                    100 * max(v[1] for v in m.values()),
                                                                    {k: "%d/%d" % (len(v[3]), v[2]) for k, v in m.items() if len(v[3])}))


def test_gradients(case):
    m = K.grad_measures(case["tr"].grads(), case["ref"]["grads"])
    print("[measured] (%d, %d) parameter gradients: worst rel L2 %.1e (bound 3e-03), worst rel max %.1e (bound 2e-02)"
          % (case["B"], case["N"], max(v[0] for v in m.values()), max(v[1] for v in m.values())))
    K.check_gradients(case, case["B"], case["N"])


def test_train_step_matches_oracle_adam(case, dev):
    K.check_train_step_matches_oracle_adam(case, case["B"], case["N"], dev)


# ------------------------------------------------------------------------------------ one trainer, changing shapes ----
def _pass(tr, xs, gs, rs):
    tr.zero_grad()
    tr.forward(xs)
    terms = {k: float(v) for k, v in tr.loss_backward(gs, rs).items()}
    tr.backward()
    torch.cuda.synchronize()
    return terms


def test_one_trainer_changing_shapes(dev):
    """One Trainer runs (4, 64), (1, 512), (2, 24), (4, 64): a scratch buffer sized by a larger shape is reused by a smaller one and
    the other way round, the last pass returns to a cached workspace whose accumulators were zero-filled "for exactly ONE backward()"
    after the trainer has been elsewhere.  After every pass its gradients, loss terms and moving statistics equal those of a fresh
    Trainer that ran only that shape from the same parameters and moving statistics: flat_g within 1e-5 of its largest entry (only the
    float atomics differ, the bound of test_second_backward_on_one_forward), loss terms within 1e-5 * max(1, |a|), moving statistics
    rtol 1e-5 / atol 1e-6 (the bounds of test_taped_steps_equal_eager_steps)."""
    from dispu_amd import synth
    from dispu_amd.train import Trainer
    P = OG.init_params(seed=1234, bias_scale=0.05, bn_random=True)
    tr = Trainer(params=P, device=dev)
    for i, (B, N, seed) in enumerate(((4, 64, 4), (1, 512, 4), (2, 24, 2), (4, 64, 4))):
        x, gt = synth.patch_with_gt(B, N, 4 * N, seed=seed)
        xs, gs = torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)
        rs = torch.from_numpy(np.linspace(1.0, 1.3, B).astype(np.float32)).to(dev)
        fresh = Trainer(params=P, device=dev)
        for name in ("flat_p", "moving_mean", "moving_var"):
            getattr(fresh, name).copy_(getattr(tr, name))
        want = _pass(fresh, xs, gs, rs)
        got = _pass(tr, xs, gs, rs)
        scale = float(fresh.flat_g.abs().max())
        err = float((tr.flat_g - fresh.flat_g).abs().max())
        print("[measured] pass %d at (%d, %d): flat_g differs by %.1e of its largest entry (bound 1e-05)" % (i, B, N, err / scale))
        assert scale > 0 and err <= 1e-5 * scale, (i, B, N, err, scale)
        for k, a in want.items():
            assert np.isfinite(a) and abs(got[k] - a) <= 1e-5 * max(1.0, abs(a)), (i, B, N, k, got[k], a)
        assert np.allclose(K.N_(tr.moving_mean), K.N_(fresh.moving_mean), rtol=1e-5, atol=1e-6), (i, B, N)
        assert np.allclose(K.N_(tr.moving_var), K.N_(fresh.moving_var), rtol=1e-5, atol=1e-6), (i, B, N)
    assert set(tr._ws) == {(4, 64), (1, 512), (2, 24)}


# ---------------------------------------------------------------------------------------------- bf16 at other shapes ----
@pytest.mark.parametrize("B,N,seed", [(1, 512, 4), (2, 40, 1)])
def test_bf16_step_at_other_shapes(dev, B, N, seed, monkeypatch):
    """Trainer(dtype="bf16") against the f32 trainer at the same shape, under the criteria of tests/test_train_bf16_gpu.py
    (test_bf16_step_forward_and_loss, test_bf16_step_gradient_direction), unchanged; in addition the bf16 loss terms lie within 2 % of
    the float64 oracle's.  At (2, 40) most products fall under bf16_min_macs and stay fp32: the mixed dispatch is what that case runs
    (asserted: the bf16 step calls bf16 entries AND dispu_linear, the f32 step no bf16 entry)."""
    rec = K.recording(monkeypatch)
    a = K.run_step(dev, B, N, seed)
    assert not [n for n in rec.names if "bf16" in n]
    del rec.names[:]
    b = K.run_step(dev, B, N, seed, dtype="bf16")
    assert [n for n in rec.names if "bf16" in n] and rec.count("dispu_linear")
    assert np.isfinite(b["f"]).all()
    assert np.abs(b["c"] - a["c"]).max() <= 2e-2 and np.abs(b["f"] - a["f"]).max() <= 3e-2
    assert np.median(np.abs(b["f"] - a["f"])) <= 2e-3
    ref = dict(a["ref"]["terms"], pu_loss=a["ref"]["loss"])
    for k in ("dis_coarse_cd", "dis_fine_cd", "pu_loss"):
        fa, fb = float(a["t"][k]), float(b["t"][k])
        assert abs(fb - fa) <= 2e-2 * abs(fa), (k, fa, fb)
        assert abs(fb - ref[k]) <= 2e-2 * abs(ref[k]), (k, ref[k], fb)
    ga, gb = K.N_(a["tr"].flat_g).astype(np.float64), K.N_(b["tr"].flat_g).astype(np.float64)
    cos = float(ga @ gb / (np.linalg.norm(ga) * np.linalg.norm(gb)))
    print("[measured] (%d, %d) bf16 vs fp32 gradient: cosine %.6f (bound 0.97), relative L2 %.1e"
          % (B, N, cos, np.linalg.norm(ga - gb) / np.linalg.norm(ga)))
    assert cos >= 0.97, cos
