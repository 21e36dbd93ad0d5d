"""The train phase on the GPU (DisPU/model.py:181-303): train.fit over dataset.DeviceFetcher against a hand-written loop over
the same fetcher and train_step, its artefacts (log_train.txt, args.txt, model-<epoch> + `checkpoint`), resuming, both step
functions, and tools/train.py as a fresh child process on the committed HDF5 fixture.

What fit is held to, per step of the epoch: the batch it consumed is bit-equal to the hand loop's (the sampler is deterministic),
and its trainer's state after the step agrees with the hand loop's train_step on that batch FROM THE STATE FIT HAD BEFORE IT.
Run-to-run a step differs by float-atomics rounding only, so the bounds are those tests/test_checkpoint_gpu.py uses for a resumed
trajectory (parameters: max 2.5e-3, 99.9 % quantile 2e-5, mean 1e-6; moving statistics rtol 1e-5; loss terms 1e-4 relative), at
the default learning rate.  The Adam moments have the gradients' scale, not the learning rate's: all but the 0.1 % of entries
must agree to that same 1e-4, relative to the largest moment.  The hand loop is re-seated on fit's state before every step because
two free-running trajectories of train_step do not stay within such bounds over five steps: where a gradient entry is ~0 its
rounding decides the sign of a full lr-sized Adam move, and the later steps amplify that."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "train.py")
LINE = re.compile(r"^epoch (\d{4}) g_loss=(-?\d+\.\d{9})  coarse_cd=(-?\d+\.\d{9})  coarse_hd=(-?\d+\.\d{9})  fine_cd=(-?\d+\.\d{9}) fine_hd=(-?\d+\.\d{9})  time=\d+\.\d{4}$")
STATE = ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var")


def N(t):
    return t.detach().cpu().numpy()


def _setup(dev, seed=7, batch=4, n=24):
    from dispu_amd import dataset, params, synth, train
    _, gt = synth.patch_with_gt(n, 256, 1024, seed=21)
    fetcher = dataset.DeviceFetcher(gt, gt, batch, patch_num_point=256, device=dev, seed=5)
    opts = train.TrainOpts()
    opts.batch_size, opts.training_epoch, opts.epoch_per_save = batch, 2, 1
    trainer = train.Trainer(opts, params.init_params(seed=seed), device=dev)
    return trainer, fetcher, opts


def _log_lines(log_dir):
    return [LINE.match(l) for l in open(os.path.join(log_dir, "log_train.txt")).read().splitlines() if LINE.match(l)]


def _state(t):
    return dict((k, getattr(t, k).clone()) for k in STATE), t.adam_t


def _record_steps(trainer, name):
    """wrap trainer.<name> (train_step / train_step_taped): every call leaves (state before, batch, loss terms, state after)."""
    steps, inner = [], getattr(trainer, name)

    def step(x, gt, radius):
        before, batch = _state(trainer), tuple(v.clone() for v in (x, gt, radius))
        terms = inner(x, gt, radius)
        steps.append((before, batch, dict((k, float(v)) for k, v in terms.items()), _state(trainer)))
        return terms
    setattr(trainer, name, step)
    return steps


def _hand_loop_agrees(steps, b, fb):
    """the hand-written loop (fb.next_batch + b.train_step), re-seated on the recorded state before every step (module docstring)"""
    for i, (before, batch, terms, after) in enumerate(steps):
        mine = fb.next_batch()
        assert all(torch.equal(u, v) for u, v in zip(mine, batch)), "batch %d differs" % i
        for k in STATE:
            getattr(b, k).copy_(before[0][k])
        b.adam_t = before[1]
        tb = b.train_step(*mine)
        torch.cuda.synchronize()
        diff = np.abs(N(b.flat_p) - N(after[0]["flat_p"]))
        print("step %d params: max %.3e q99.9 %.3e mean %.3e" % (i + 1, diff.max(), np.quantile(diff, 0.999), diff.mean()))
        assert diff.max() <= 2.5e-3 and np.quantile(diff, 0.999) <= 2e-5 and diff.mean() <= 1e-6, (i, diff.max(), np.quantile(diff, 0.999), diff.mean())
        for k in ("flat_m", "flat_v"):
            d, top = np.abs(N(getattr(b, k)) - N(after[0][k])), float(np.abs(N(after[0][k])).max())
            assert np.quantile(d, 0.999) <= 1e-4 * max(1.0, top), (i, k, np.quantile(d, 0.999), top)
        for k in ("moving_mean", "moving_var"):
            assert np.allclose(N(getattr(b, k)), N(after[0][k]), rtol=1e-5, atol=1e-7), (i, k)
        for k in terms:
            assert abs(float(tb[k]) - terms[k]) <= 1e-4 * max(1.0, abs(terms[k])), (i, k)
        assert b.adam_t == after[1] == i + 1


def test_fit_artefacts_and_hand_loop(tmp_path, dev):
    from dispu_amd import checkpoint as CK, train
    log_dir = str(tmp_path / "log")
    a, fa, opts = _setup(dev)
    recs = train.fit(a, fa, opts, log_dir)
    assert [r["epoch"] for r in recs] == [1, 2] and all(r["steps"] == 5 for r in recs) and a.epoch == 2 and a.global_step == 10
    assert fa.epoch == 2 and not N(fa.status).any()
    lines = _log_lines(log_dir)
    assert len(lines) == 2 and [int(m.group(1)) for m in lines] == [1, 2]
    for m, r in zip(lines, recs):
        got = [float(m.group(i)) for i in range(2, 7)]
        want = [r["g_loss"], r["coarse_cd"], r["coarse_hd"], r["fine_cd"], r["fine_hd"]]
        assert np.allclose(got, want, rtol=0, atol=1e-9) and all(np.isfinite(want)) and min(want) > 0
    args = open(os.path.join(log_dir, "args.txt")).read().splitlines()
    assert args == sorted(args) and "batch_size: 4" in args and "epoch_per_save: 1" in args and "base_lr_g: 0.001" in args
    # a checkpoint only where fine_cd improved; the state file names the latest one
    improved = recs[1]["fine_cd"] < recs[0]["fine_cd"]
    assert recs[0]["saved"] is not None and (recs[1]["saved"] is not None) == improved
    assert os.path.exists(os.path.join(log_dir, "model-1.index")) and os.path.exists(os.path.join(log_dir, "model-2.index")) == improved
    assert CK.pre_load_checkpoint(log_dir)[0] == (2 if improved else 1)

    # epoch 1 against a hand-written loop over the same fetcher and train_step
    a, fa, opts = _setup(dev)
    opts.training_epoch = 1
    steps = _record_steps(a, "train_step")
    recs = train.fit(a, fa, opts, str(tmp_path / "one"))
    assert len(steps) == 5 and a.adam_t == 5 and a.global_step == 5 and a.epoch == 1
    # the epoch's log values are the means of the steps' terms
    for key, term in (("g_loss", "pu_loss"), ("coarse_cd", "dis_coarse_cd"), ("fine_cd", "dis_fine_cd")):
        mean = float(np.mean([s[2][term] for s in steps]))
        assert abs(recs[0][key] - mean) <= 1e-5 * max(1.0, abs(mean)), key
    b, fb, _ = _setup(dev)
    _hand_loop_agrees(steps, b, fb)
    # ... whose last step leaves the state fit left: parameters, both moments, BN statistics (same bounds, checked in the loop above
    # against steps[-1]'s state after, which IS fit's final state)
    assert all(torch.equal(getattr(a, k), steps[-1][3][0][k]) for k in STATE)


def test_fit_restore_resumes_at_the_saved_epoch(tmp_path, dev):
    from dispu_amd import checkpoint as CK, params, train
    log_dir = str(tmp_path / "log")
    a, fa, opts = _setup(dev)
    opts.training_epoch, opts.decay_step = 1, 1           # the learning rate decays with every epoch: a resumed run must pick it up
    train.fit(a, fa, opts, log_dir)
    saved = CK.pre_load_checkpoint(log_dir)[0]
    assert saved == 1
    # a trainer with other weights: everything comes from the checkpoint; training_epoch == saved epoch -> no epoch runs
    b = train.Trainer(opts, params.init_params(seed=99), device=dev)
    fb = _setup(dev)[1]
    assert train.fit(b, fb, opts, log_dir, restore=True) == []
    assert b.epoch == a.epoch == 1 and b.adam_t == a.adam_t and torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m)
    # the fresh fetcher was brought to the restored epoch: the permutation (and with it every draw) of the uninterrupted run
    assert fb.epoch == fa.epoch == 1 and torch.equal(fb.perm, fa.perm) and fb.batch_idx == 0
    assert train.weight_fine(b.epoch) == train.weight_fine(a.epoch)
    assert train.learning_rate(opts, b.epoch) == train.learning_rate(opts, a.epoch) == pytest.approx(0.001 * 0.7)
    opts.training_epoch = 2
    recs = train.fit(b, fb, opts, log_dir, restore=True)
    assert [r["epoch"] for r in recs] == [2] and b.epoch == 2 and recs[0]["saved"] is not None       # best starts at infinity again
    assert fb.epoch == 2
    assert [int(m.group(1)) for m in _log_lines(log_dir)] == [1, 2]                                   # appended, not overwritten
    assert CK.pre_load_checkpoint(log_dir)[0] == 2


def test_fit_taped_step_function(tmp_path, dev):
    """fit(train_step_fn="taped"): every taped step of the epoch against the eager train_step on the same batch from the same state."""
    from dispu_amd import train
    a, fa, opts = _setup(dev)
    opts.training_epoch = 1
    steps = _record_steps(a, "train_step_taped")
    recs = train.fit(a, fa, opts, str(tmp_path / "taped"), train_step_fn="taped")
    assert len(steps) == 5 and len(a._tapes) == 1 and recs[0]["steps"] == 5 and a.adam_t == 5
    b, fb, _ = _setup(dev)
    _hand_loop_agrees(steps, b, fb)
    assert len(b._tapes) == 0


def _run_tool(argv):
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, TOOL] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_train_tool_child_process(tmp_path, dev):
    """tools/train.py in a fresh process on the committed 4-patch HDF5 file: B = 1 -> 3 steps per epoch."""
    from dispu_amd import checkpoint as CK, h5
    h5.lib()
    data = tmp_path / "data"
    data.mkdir()
    shutil.copy(os.path.join(ROOT, "tests", "golden", "patches_small.h5"), str(data / "PUGAN_poisson_256_poisson_1024.h5"))
    log_dir = str(tmp_path / "log")
    common = ["--data_dir", str(data), "--log_dir", log_dir, "--batch_size", "1", "--epoch_per_save", "1", "--seed", "3"]
    r = _run_tool(common + ["--training_epoch", "2"])
    out = r.stdout.decode()
    assert r.returncode == 0, out
    lines = _log_lines(log_dir)
    assert [int(m.group(1)) for m in lines] == [1, 2] and "train_dataset: 4" in out
    args = open(os.path.join(log_dir, "args.txt")).read().splitlines()
    assert args == sorted(args) and "batch_size: 1" in args and "sampler: device" in args and "training_epoch: 2" in args
    improved = float(lines[1].group(5)) < float(lines[0].group(5))
    assert CK.pre_load_checkpoint(log_dir)[0] == (2 if improved else 1) and os.path.exists(os.path.join(log_dir, "model-1.index"))
    # resume with the taped step and the host sampler
    r = _run_tool(common + ["--training_epoch", "3", "--restore", "--tape", "--sampler", "host"])
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert [int(m.group(1)) for m in _log_lines(log_dir)][:2] == [1, 2] and len(_log_lines(log_dir)) == (3 if improved else 4)
