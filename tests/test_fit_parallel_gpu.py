"""train.fit_parallel on the GPU: two `gloo` ranks sharing the test box's one GPU (the transport tests/test_distributed_gpu.py uses
for every N > 1 path; real runs use nccl == RCCL, one GPU per rank, through the same calls).  The setup is that of
tests/test_train_phase_gpu.py: 24 synthetic patches 256 -> 1024, GLOBAL batch 4 (2 per rank), 2 epochs of 5 steps.

ONE spawn (module fixture) runs the loop, the checks that need both ranks in lock-step, and a restored run; the tests read its report:
  (i)   every rank's batches are bit-equal to its rows of an unsharded DeviceFetcher(batch 4);
  (ii)  after every step flat_p / flat_m / flat_v and the BN moving statistics are bit-identical across the ranks;
  (iii) every recorded step, re-seated on the state before it and re-run by train_step on the same shard, in lock-step on both ranks
        (the step all-reduces), agrees within the bounds tests/test_train_phase_gpu.py uses and justifies (two evaluations of a step
        differ by float-atomics rounding): parameters max 2.5e-3, 99.9 % quantile 2e-5, mean 1e-6; moments 1e-4 of the largest;
        statistics rtol 1e-5; loss terms 1e-4;
  (iv)  one log_train.txt whose loss / CD columns are the mean over ranks and steps of the recorded terms and whose HD columns are the
        mean over steps of the max over ranks of each rank's train._hausdorff_terms (1e-5 relative); checkpoints written once;
  (v)   a fresh two-rank run with restore=True resumes at the saved epoch with rank-identical parameters bit-equal to the checkpoint
        and the fetcher at the restored epoch's permutation, and appends to the log;
  (vi)  tools/train.py under torch.distributed.run --nproc-per-node 2 on the committed HDF5 fixture."""
import hashlib
import os
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "train.py")
LINE = re.compile(r"^epoch (\d{4}) g_loss=(-?\d+\.\d{9})  coarse_cd=(-?\d+\.\d{9})  coarse_hd=(-?\d+\.\d{9})  fine_cd=(-?\d+\.\d{9}) fine_hd=(-?\d+\.\d{9})  time=\d+\.\d{4}$")
STATE = ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var")
B_GLOBAL, EPOCHS, STEPS = 4, 2, 5


def N(t):
    return t.detach().cpu().numpy()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _state(t):
    return dict((k, getattr(t, k).clone()) for k in STATE), t.adam_t, t.epoch


def _digest(t):
    h = hashlib.sha1()
    for k in STATE:
        h.update(N(getattr(t, k)).tobytes())
    return h.hexdigest()


def _hand_step_failures(i, b, before, batch, terms, after):
    """one recorded step re-run by b.train_step from the state before it: the bounds of the module docstring, (iii)"""
    for k in STATE:
        getattr(b, k).copy_(before[0][k])
    b.adam_t, b.epoch = before[1], before[2]
    tb = b.train_step(*batch)
    torch.cuda.synchronize()
    bad = []
    diff = np.abs(N(b.flat_p) - N(after[0]["flat_p"]))
    fig = "step %d params: max %.3e q99.9 %.3e mean %.3e" % (i + 1, diff.max(), np.quantile(diff, 0.999), diff.mean())
    if not (diff.max() <= 2.5e-3 and np.quantile(diff, 0.999) <= 2e-5 and diff.mean() <= 1e-6):
        bad.append(fig)
    for k in ("flat_m", "flat_v"):
        d, top = np.abs(N(getattr(b, k)) - N(after[0][k])), float(np.abs(N(after[0][k])).max())
        if not np.quantile(d, 0.999) <= 1e-4 * max(1.0, top):
            bad.append("step %d %s: q99.9 %.3e, largest %.3e" % (i + 1, k, np.quantile(d, 0.999), top))
    for k in ("moving_mean", "moving_var"):
        if not np.allclose(N(getattr(b, k)), N(after[0][k]), rtol=1e-5, atol=1e-7):
            bad.append("step %d %s" % (i + 1, k))
    for k in terms:
        if not abs(float(tb[k]) - terms[k]) <= 1e-4 * max(1.0, abs(terms[k])):
            bad.append("step %d term %s: %r vs %r" % (i + 1, k, float(tb[k]), terms[k]))
    if b.adam_t != after[1]:
        bad.append("step %d adam_t %d vs %d" % (i + 1, b.adam_t, after[1]))
    return fig, bad


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rep = {}
    try:
        from dispu_amd import checkpoint as CK, dataset, params, synth, train
        dev = torch.device("cuda:0")
        log_dir = os.path.join(tmp, "log")
        _, gt = synth.patch_with_gt(24, 256, 1024, seed=21)

        def fetcher(shard=(rank, world)):
            return dataset.DeviceFetcher(gt, gt, B_GLOBAL, patch_num_point=256, device=dev, seed=5, shard=shard)

        opts = train.TrainOpts()
        opts.batch_size, opts.training_epoch, opts.epoch_per_save = B_GLOBAL, EPOCHS, 1
        a, fa = train.Trainer(opts, params.init_params(seed=7), device=dev), fetcher()

        steps, perms, inner = [], {}, a.train_step

        def step(x, g, radius):
            perms[fa.epoch] = fa.perm.clone()
            before, batch = _state(a), tuple(v.clone() for v in (x, g, radius))
            terms = inner(x, g, radius)
            hd = train._hausdorff_terms(a, x, g, radius)
            steps.append((before, batch, dict((k, float(v)) for k, v in terms.items()), _state(a), [float(h) for h in hd], _digest(a)))
            return terms
        a.train_step = step
        saves = []

        def save_fn(d, t, e):
            saves.append(e)
            return CK.save_train_state(d, t, e)

        recs = train.fit_parallel(a, fa, opts, log_dir, save_fn=save_fn)
        rep["recs"] = [{k: v for k, v in r.items() if k != "seconds"} for r in recs]
        rep["saves"], rep["epoch"], rep["global_step"], rep["fetcher_epoch"] = saves, a.epoch, a.global_step, fa.epoch
        rep["status"] = N(fa.status).tolist()
        rep["terms"] = [s[2] for s in steps]
        rep["hd"] = [s[4] for s in steps]
        rep["digests"] = [s[5] for s in steps]
        rep["final_is_last_step"] = all(torch.equal(getattr(a, k), steps[-1][3][0][k]) for k in STATE)

        # (i) this rank's batches against its rows of the unsharded fetcher's
        fu, lo, shard_ok = fetcher(shard=None), rank * (B_GLOBAL // world), []
        for i, s in enumerate(steps):
            full = fu.next_batch()
            shard_ok.append(all(torch.equal(u[lo:lo + B_GLOBAL // world], v) for u, v in zip(full, s[1])))
            if i % STEPS == STEPS - 1:
                fu.reset()
        rep["shard_ok"] = shard_ok
        rep["shard_rows"] = [int(s[1][0].shape[0]) for s in steps]

        # (iii) the hand loop, in lock-step on both ranks (train_step all-reduces over the two of them)
        b, fb = train.Trainer(opts, params.init_params(seed=7), device=dev), fetcher()
        figs, bad = [], []
        for i, (before, batch, terms, after, _, _) in enumerate(steps):
            mine = fb.next_batch()
            if not all(torch.equal(u, v) for u, v in zip(mine, batch)):
                bad.append("batch %d differs" % i)
            fig, more = _hand_step_failures(i, b, before, mine, terms, after)
            figs.append(fig)
            bad += more
            if i % STEPS == STEPS - 1:
                fb.reset()
        rep["hand_figures"], rep["hand_failures"] = figs, bad

        # (v) a fresh run restores: first up to the saved epoch itself (no epoch runs), then one epoch more
        saved, prefix = CK.pre_load_checkpoint(log_dir)
        c, fc = train.Trainer(opts, params.init_params(seed=99), device=dev), fetcher()
        opts.training_epoch = saved
        rep["restore_noop"] = train.fit_parallel(c, fc, opts, log_dir, restore=True, save_fn=save_fn)
        want = CK.load_generator_params(prefix)
        rep["restored"] = dict(saved=saved, epoch=c.epoch, adam_t=c.adam_t, digest=_digest(c), fetcher_epoch=fc.epoch, batch_idx=fc.batch_idx,
                               params_equal=all(np.array_equal(N(c.P[k]), np.asarray(want[k], np.float32).reshape(N(c.P[k]).shape))
                                                for k in c.names),
                               perm_equal=bool(saved in perms and torch.equal(fc.perm, perms[saved])) if saved < EPOCHS else
                               bool(torch.equal(fc.perm, fa.perm)))
        opts.training_epoch = saved + 1
        more = train.fit_parallel(c, fc, opts, log_dir, restore=True, save_fn=save_fn)
        rep["resumed"] = dict(epochs=[r["epoch"] for r in more], saved=[r["saved"] is not None for r in more], epoch=c.epoch,
                              fetcher_epoch=fc.epoch, digest=_digest(c), saves=list(saves))
        q.put((rank, rep))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fit_parallel_gpu"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, tmp, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=600))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return tmp, [r[1] for r in sorted(res, key=lambda r: r[0])]


def _log_lines(log_dir):
    return [LINE.match(l) for l in open(os.path.join(log_dir, "log_train.txt")).read().splitlines() if LINE.match(l)]


def test_shards_are_rows_of_the_unsharded_batches(run):
    _, res = run
    for r in res:
        assert len(r["shard_ok"]) == EPOCHS * STEPS and all(r["shard_ok"]), r["shard_ok"]
        assert r["shard_rows"] == [B_GLOBAL // 2] * (EPOCHS * STEPS)
        assert r["status"] == [0, 0]


def test_replicas_stay_bit_identical_after_every_step(run):
    _, res = run
    assert len(res[0]["digests"]) == EPOCHS * STEPS and res[0]["digests"] == res[1]["digests"]
    assert len(set(res[0]["digests"])) == EPOCHS * STEPS          # ... and the state did move with every step
    assert all(r["final_is_last_step"] for r in res)
    assert all((r["epoch"], r["global_step"], r["fetcher_epoch"]) == (EPOCHS, EPOCHS * STEPS, EPOCHS) for r in res)


def test_every_step_agrees_with_a_hand_loop(run):
    _, res = run
    for rank, r in enumerate(res):
        print("rank %d\n  %s" % (rank, "\n  ".join(r["hand_figures"])))
        assert len(r["hand_figures"]) == EPOCHS * STEPS and r["hand_failures"] == [], r["hand_failures"]


def test_artefacts_one_log_global_values_checkpoints_once(run):
    tmp, res = run
    log_dir = os.path.join(tmp, "log")
    assert [f for f in os.listdir(tmp)] == ["log"] and os.path.isfile(os.path.join(log_dir, "log_train.txt"))
    assert res[0]["recs"] == res[1]["recs"] and [r["epoch"] for r in res[0]["recs"]] == [1, 2]
    lines = _log_lines(log_dir)
    text = open(os.path.join(log_dir, "log_train.txt")).read().splitlines()
    assert text[0] == "train_dataset: 24" and [int(m.group(1)) for m in lines][:2] == [1, 2]
    for e in range(EPOCHS):
        sl = slice(e * STEPS, (e + 1) * STEPS)
        want = [np.mean([[r["terms"][i][k] for r in res] for i in range(e * STEPS, (e + 1) * STEPS)])
                for k in ("pu_loss", "dis_coarse_cd", "dis_fine_cd")]
        hd = np.array([r["hd"][sl] for r in res], np.float64)                     # [rank, step, coarse / fine]
        want_hd = hd.max(axis=0).mean(axis=0)
        want = [want[0], want[1], want_hd[0], want[2], want_hd[1]]
        got_log = [float(lines[e].group(i)) for i in range(2, 7)]
        got_rec = [res[0]["recs"][e][k] for k in ("g_loss", "coarse_cd", "coarse_hd", "fine_cd", "fine_hd")]
        print("epoch %d logged %s expected %s" % (e + 1, got_log, want))
        for g, r, w in zip(got_log, got_rec, want):
            assert np.isfinite(w) and w > 0
            assert abs(r - w) <= 1e-5 * abs(w) and abs(g - w) <= 1e-5 * abs(w) + 1e-9, (e, g, r, w)
    # checkpoints: epoch 1 always, epoch 2 where fine_cd improved -- written by rank 0 alone, once each
    improved = res[0]["recs"][1]["fine_cd"] < res[0]["recs"][0]["fine_cd"]
    first_run = [1, 2] if improved else [1]
    assert res[0]["saves"][:len(first_run)] == first_run and res[1]["saves"] == [] and res[1]["resumed"]["saves"] == []
    assert [r["saved"] is not None for r in res[1]["recs"]] == [True, improved]
    assert os.path.exists(os.path.join(log_dir, "model-1.index")) and os.path.exists(os.path.join(log_dir, "model-2.index"))
    args = open(os.path.join(log_dir, "args.txt")).read().splitlines()
    assert args == sorted(args) and "batch_size: 4" in args


def test_restore_resumes_at_the_saved_epoch_on_both_ranks(run):
    tmp, res = run
    improved = res[0]["recs"][1]["fine_cd"] < res[0]["recs"][0]["fine_cd"]
    saved = 2 if improved else 1
    for r in res:
        assert r["restore_noop"] == []
        v = r["restored"]
        assert v["saved"] == saved and v["epoch"] == saved and v["adam_t"] == saved * STEPS
        assert v["params_equal"] and v["perm_equal"] and v["fetcher_epoch"] == saved and v["batch_idx"] == 0
        assert r["resumed"]["epochs"] == [saved + 1] and r["resumed"]["saved"] == [True]       # best starts at infinity again
        assert r["resumed"]["epoch"] == saved + 1 and r["resumed"]["fetcher_epoch"] == saved + 1
    assert res[0]["restored"]["digest"] == res[1]["restored"]["digest"]
    assert res[0]["resumed"]["digest"] == res[1]["resumed"]["digest"] != res[0]["restored"]["digest"]
    if improved:                                          # restored after the last epoch: the state the first run ended in
        assert res[0]["restored"]["digest"] == res[0]["digests"][-1]
    else:
        assert res[0]["restored"]["digest"] == res[0]["digests"][STEPS - 1]
    assert [int(m.group(1)) for m in _log_lines(os.path.join(tmp, "log"))] == [1, 2, saved + 1]     # appended, not overwritten
    assert res[0]["resumed"]["saves"][-1] == saved + 1


def test_train_tool_under_the_launcher(tmp_path, dev):
    """tools/train.py as torch.distributed.run starts it, two ranks over gloo on the committed 4-patch HDF5 file: global batch 2 ->
    one step per epoch."""
    from dispu_amd import checkpoint as CK, h5
    h5.lib()
    data = tmp_path / "data"
    data.mkdir()
    shutil.copy(os.path.join(ROOT, "tests", "golden", "patches_small.h5"), str(data / "PUGAN_poisson_256_poisson_1024.h5"))
    log_dir = str(tmp_path / "log")
    env = dict(os.environ, DISPU_TRAIN_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), TOOL, "--data_dir", str(data), "--log_dir", log_dir,
           "--batch_size", "2", "--epoch_per_save", "1", "--seed", "3", "--training_epoch", "2"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    epoch_lines = [l for l in out.splitlines() if LINE.match(l)]
    assert [int(LINE.match(l).group(1)) for l in epoch_lines] == [1, 2], out          # from ONE rank: every epoch line once
    assert out.count("train_dataset: 4") == 1 and out.count("checkpoints in") == 1
    lines = _log_lines(log_dir)
    assert [m.group(0) for m in lines] == epoch_lines
    improved = float(lines[1].group(5)) < float(lines[0].group(5))
    assert CK.pre_load_checkpoint(log_dir)[0] == (2 if improved else 1)
    found = sorted(f for f in os.listdir(log_dir) if f.startswith("model-") and f.endswith(".index"))
    assert found == (["model-1.index", "model-2.index"] if improved else ["model-1.index"])
    assert "batch_size: 2" in open(os.path.join(log_dir, "args.txt")).read().splitlines()
