"""The data-parallel train loop (train.fit_parallel) without a GPU: its control flow at world 1 on stubs (steps per epoch, log
lines, save rule, restore start, step-function choice), and two `gloo` ranks on CPU whose meter rows are known functions of
(rank, epoch, step): the logged values are the mean / max over ranks per step, then the mean over steps; rank 0 alone writes the
log and calls save_fn; both ranks return the same records; the three refusals; a sampler status flag set on rank 1 raises on
both ranks.  The two-rank scenarios share ONE spawn (module fixture)."""
import os
import re
import socket
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "train.py")
LINE = re.compile(r"^epoch (\d{4}) g_loss=(-?\d+\.\d{9})  coarse_cd=(-?\d+\.\d{9})  coarse_hd=(-?\d+\.\d{9})  fine_cd=(-?\d+\.\d{9}) fine_hd=(-?\d+\.\d{9})  time=\d+\.\d{4}$")
KEYS = ("g_loss", "coarse_cd", "coarse_hd", "fine_cd", "fine_hd")


class StubFetcher(object):
    def __init__(self, length, batch_size, shard=None, flag_in_epoch=None):
        self.length, self.batch_size, self.shard = length, batch_size, shard
        self.batches, self.resets, self.epoch, self.flag_in_epoch = 0, 0, 0, flag_in_epoch

    def __len__(self):
        return self.length

    def reset(self):
        self.resets += 1
        self.epoch += 1

    def next_batch(self):
        self.batches += 1
        return "x", "gt", "radius"

    def status_flags(self):
        return (1, 0) if self.flag_in_epoch is not None and self.epoch == self.flag_in_epoch else (0, 0)


class StubTrainer(object):
    """fine_cd of epoch e (constant within it) comes from a list; counts steps and remembers the epoch each ran in."""
    device, pg = "cpu", None

    def __init__(self, fine_cd):
        self.fine_cd, self.epoch, self.steps, self.taped, self.last = fine_cd, 0, [], 0, None

    def train_step(self, x, gt, radius):
        assert (x, gt, radius) == ("x", "gt", "radius")
        self.steps.append(self.epoch)
        f = self.fine_cd[self.epoch]
        self.last = {"pu_loss": 10.0 + f, "dis_coarse_cd": 2.0, "dis_fine_cd": f}
        return self.last

    def train_step_taped(self, x, gt, radius):
        self.taped += 1
        return self.train_step(x, gt, radius)


def _meter(trainer, x, gt, radius, row):
    """the stub of dispu_step_meters: the step's terms and fixed Hausdorff values into the table row it is handed"""
    assert (x, gt, radius) == ("x", "gt", "radius") and tuple(row.shape) == (5,) and row.dtype == torch.float32
    t = trainer.last
    row.copy_(torch.tensor([t["pu_loss"], t["dis_coarse_cd"], 3.0, t["dis_fine_cd"], 4.0]))


def _fit(tmp_path, fine_cd, epochs, per_save, restore_epoch=None, length=24, batch=4, step_fn="eager", fetcher=None):
    from dispu_amd import train
    saves, fetcher, trainer = [], fetcher or StubFetcher(length, batch), StubTrainer(fine_cd)
    opts = types.SimpleNamespace(batch_size=batch, training_epoch=epochs, epoch_per_save=per_save)

    def restore_fn(log_dir, t):
        t.epoch = restore_epoch
        return restore_epoch

    recs = train.fit_parallel(trainer, fetcher, opts, str(tmp_path), restore=restore_epoch is not None, train_step_fn=step_fn,
                              save_fn=lambda d, t, e: saves.append((e, t.epoch)) or "model-%d" % e, restore_fn=restore_fn, meter_fn=_meter)
    return recs, saves, fetcher, trainer


# ------------------------------------------------------------------------------------------------------- world 1 ----
def test_world1_steps_log_lines_and_save_rule(tmp_path):
    assert not dist.is_initialized()
    fine = [5.0, 4.0, 4.5, 4.0, 3.0, 4.0, 9.0, 1.0]
    recs, saves, fetcher, trainer = _fit(tmp_path, fine, epochs=8, per_save=2)
    assert fetcher.batches == 8 * 5 and fetcher.resets == 8 and trainer.steps == [e for e in range(8) for _ in range(5)]
    assert [r["epoch"] for r in recs] == list(range(1, 9)) and all(r["steps"] == 5 for r in recs)
    # epoch % 2 == 0 AND strictly below the best SAVED so far: 2 (4.0), not 4 (ties), not 6 (worse), 8 (1.0)
    assert saves == [(2, 2), (8, 8)]
    assert [r["saved"] for r in recs] == [None, "model-2", None, None, None, None, None, "model-8"]
    assert [r["fine_cd"] for r in recs] == fine and all(r["coarse_hd"] == 3.0 and r["fine_hd"] == 4.0 for r in recs)
    lines = open(os.path.join(str(tmp_path), "log_train.txt")).read().splitlines()
    assert lines[0] == "train_dataset: 24" and len(lines) == 9 and all(LINE.match(l) for l in lines[1:])
    assert lines[1].startswith("epoch 0001 g_loss=15.000000000  coarse_cd=2.000000000  coarse_hd=3.000000000  fine_cd=5.000000000 fine_hd=4.000000000  time=")
    assert open(os.path.join(str(tmp_path), "args.txt")).read() == "batch_size: 4\nepoch_per_save: 2\ntraining_epoch: 8\n"


def test_world1_restore_start_and_log_mode(tmp_path):
    recs, _, _, _ = _fit(tmp_path, [1.0] * 10, epochs=3, per_save=1)
    assert len(recs) == 3
    recs, saves, fetcher, trainer = _fit(tmp_path, [1.0] * 10, epochs=7, per_save=1, restore_epoch=3)
    assert [r["epoch"] for r in recs] == [4, 5, 6, 7] and trainer.steps[0] == 3 and fetcher.batches == 4 * 5
    assert fetcher.resets == 3 + 4 and fetcher.epoch == 7           # three resets to reach the restored epoch, then one per epoch
    assert [e for e, _ in saves] == [4]                              # best starts at infinity after a restore
    lines = [l for l in open(os.path.join(str(tmp_path), "log_train.txt")).read().splitlines() if LINE.match(l)]
    assert [int(l[6:10]) for l in lines] == [1, 2, 3, 4, 5, 6, 7]   # 'a' mode keeps the first run's lines
    recs, _, _, _ = _fit(tmp_path, [1.0] * 10, epochs=3, per_save=1, restore_epoch=5)
    assert recs == []


def test_world1_step_function_choice_and_refusals(tmp_path):
    _, _, _, trainer = _fit(tmp_path, [1.0] * 3, epochs=1, per_save=1, step_fn="taped")
    assert trainer.taped == 5
    _, _, _, trainer = _fit(tmp_path, [1.0] * 3, epochs=1, per_save=1)
    assert trainer.taped == 0 and len(trainer.steps) == 5
    with pytest.raises(ValueError):
        _fit(tmp_path, [1.0] * 3, epochs=1, per_save=1, step_fn="graphed")
    with pytest.raises(ValueError, match="positive"):
        _fit(tmp_path, [1.0] * 3, epochs=1, per_save=1, batch=0)


def test_world1_status_flag_raises(tmp_path):
    with pytest.raises(RuntimeError, match="sampler"):
        _fit(tmp_path, [1.0] * 4, epochs=3, per_save=1, fetcher=StubFetcher(24, 4, flag_in_epoch=1))


def test_reduce_meter_tables():
    """mean over ranks for loss / CD, max over ranks for the Hausdorff columns, PER STEP, then the mean over steps: the max of the
    means would be wrong (rank 1 wins step 0, rank 0 wins step 1)."""
    from dispu_amd import train
    r0 = [[1.0, 2.0, 10.0, 4.0, 1.0], [3.0, 2.0, 30.0, 8.0, 7.0]]
    r1 = [[5.0, 6.0, 20.0, 0.0, 5.0], [7.0, 2.0, 10.0, 4.0, 3.0]]
    got = train.reduce_meter_tables(np.array([np.ravel(r0), np.ravel(r1)], np.float32), 2)
    assert got == [(3.0 + 5.0) / 2, (4.0 + 2.0) / 2, (20.0 + 30.0) / 2, (2.0 + 6.0) / 2, (5.0 + 7.0) / 2]
    assert train.reduce_meter_tables(np.zeros((2, 0), np.float32), 0) == [0.0] * 5


def test_device_fetcher_shard_refused_before_device_work():
    from dispu_amd import dataset
    gt = np.zeros((8, 64, 3), np.float32)
    with pytest.raises(ValueError, match="divide"):
        dataset.DeviceFetcher(gt, gt, 5, patch_num_point=32, device="cpu", shard=(0, 2))
    with pytest.raises(ValueError, match="rank"):
        dataset.DeviceFetcher(gt, gt, 4, patch_num_point=32, device="cpu", shard=(2, 2))


def test_tool_refuses_host_sampler_and_ragged_batch_under_a_launcher(tmp_path):
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for argv, word in ((["--sampler", "host", "--batch_size", "4"], "--sampler host"), (["--batch_size", "5"], "divide")):
        r = subprocess.run([sys.executable, TOOL, "--data_dir", str(tmp_path)] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                           timeout=120)
        assert r.returncode != 0 and word in r.stderr.decode(), r.stderr.decode()


# ------------------------------------------------------------------------------------------------ two gloo ranks ----
EPOCHS, STEPS = 3, 5
FINE = [5.0, 3.0, 4.0]


def known_row(rank, epoch, s):
    """exactly representable in float32; rank 1 holds the larger coarse HD on even steps, rank 0 on odd ones"""
    return [10.0 + rank + s + epoch, 2.0 + 0.5 * rank, 3.0 + s + (rank if s % 2 == 0 else 1 - rank) * 2.0, FINE[epoch] + 0.25 * rank,
            4.0 + (5.0 * rank if s == 2 else 0.0)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dispu_amd import train
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        opts = types.SimpleNamespace(batch_size=4, training_epoch=EPOCHS, epoch_per_save=1)

        def meter(trainer, x, gt, radius, row):
            row.copy_(torch.tensor(known_row(rank, trainer.epoch, len(trainer.steps) - 1 - STEPS * trainer.epoch)))

        def run(log_dir, trainer=None, fetcher=None, o=opts, group=None, **kw):
            saves, lines = [], []
            trainer = trainer or StubTrainer(FINE)
            fetcher = fetcher or StubFetcher(24, 4, shard=(rank, world))
            recs = train.fit_parallel(trainer, fetcher, o, os.path.join(tmp, log_dir), group=group, meter_fn=meter,
                                      save_fn=lambda d, t, e: saves.append(e) or "model-%d" % e, log=lines.append, **kw)
            return recs, saves, lines, trainer, fetcher

        # ---- known rows
        recs, saves, lines, trainer, fetcher = run("known")
        out["known"] = dict(recs=[{k: v for k, v in r.items() if k != "seconds"} for r in recs], saves=saves, lines=lines,
                            steps=len(trainer.steps), batches=fetcher.batches, resets=fetcher.resets, epoch=trainer.epoch,
                            seconds=[r["seconds"] for r in recs])
        # ---- the loop over a group of its own (the trainer reduces over the same one)
        other = dist.new_group([0, 1])
        t = StubTrainer(FINE)
        t.pg = other
        recs, saves, _, _, _ = run("group", trainer=t, group=other)
        out["group"] = (len(recs), saves)
        # ---- refusals, each before the first step (no collective is entered: a rank that did not refuse would hang the test)
        refused = {}
        cases = {
            "batch": dict(o=types.SimpleNamespace(batch_size=5, training_epoch=1, epoch_per_save=1)),
            "no_shard": dict(fetcher=StubFetcher(24, 4)),
            "wrong_shard": dict(fetcher=StubFetcher(24, 4, shard=(1 - rank, world))),
            "trainer_group": dict(trainer=t),                                  # reduces over `other`, the loop runs on the default group
            "loop_group": dict(group=other),                                    # a trainer on the default group, the loop on `other`
        }
        for name, kw in cases.items():
            tr = kw.get("trainer") or StubTrainer(FINE)
            kw["trainer"] = tr
            before = len(tr.steps)
            try:
                run("refused_" + name, **kw)
                refused[name] = "ran"
            except ValueError as e:
                refused[name] = "ValueError" if len(tr.steps) == before else "ValueError after a step"
        out["refused"] = refused
        # ---- a status flag on rank 1 in the second epoch
        t0 = time.time()
        f = StubFetcher(24, 4, shard=(rank, world), flag_in_epoch=1 if rank == 1 else None)
        tr = StubTrainer(FINE)
        try:
            run("flag", trainer=tr, fetcher=f)
            out["flag"] = ("ran", None, tr.epoch, time.time() - t0)
        except RuntimeError as e:
            out["flag"] = ("RuntimeError", str(e), tr.epoch, time.time() - t0)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fit_parallel"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, tmp, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=180))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return tmp, [r[1] for r in sorted(res, key=lambda r: r[0])]


def _expected(epoch):
    rows = np.array([[known_row(r, epoch, s) for s in range(STEPS)] for r in range(2)], np.float64)       # [rank, step, 5]
    per_step = rows.mean(axis=0)
    per_step[:, [2, 4]] = rows[:, :, [2, 4]].max(axis=0)
    return per_step.mean(axis=0)


def test_two_ranks_logged_values_are_mean_and_max_over_ranks_then_mean_over_steps(two_ranks):
    tmp, res = two_ranks
    recs = res[0]["known"]["recs"]
    assert [r["epoch"] for r in recs] == [1, 2, 3] and all(r["steps"] == STEPS for r in recs)
    for e, r in enumerate(recs):
        want = _expected(e)
        assert np.allclose([r[k] for k in KEYS], want, rtol=1e-12, atol=0), (e, r, want)
    # the maximum is taken per step: the max over ranks of each rank's epoch mean is smaller
    rows = np.array([[known_row(r, 0, s) for s in range(STEPS)] for r in range(2)])
    assert recs[0]["coarse_hd"] > rows[:, :, 2].mean(axis=1).max() + 0.5
    lines = [LINE.match(l) for l in open(os.path.join(tmp, "known", "log_train.txt")).read().splitlines()[1:]]
    assert len(lines) == EPOCHS and all(lines)
    for m, r in zip(lines, recs):
        assert np.allclose([float(m.group(i)) for i in range(2, 7)], [r[k] for k in KEYS], rtol=0, atol=1e-9)


def test_two_ranks_rank0_alone_writes_and_saves(two_ranks):
    tmp, res = two_ranks
    assert sorted(os.listdir(os.path.join(tmp, "known"))) == ["args.txt", "log_train.txt"]
    text = open(os.path.join(tmp, "known", "log_train.txt")).read().splitlines()
    assert text[0] == "train_dataset: 24" and len(text) == 1 + EPOCHS                # one writer: no doubled or interleaved lines
    assert res[0]["known"]["lines"] == text and res[1]["known"]["lines"] == []       # `log` is rank 0's
    # fine_cd (mean over ranks) 5.125, 3.125, 4.125 with epoch_per_save 1: epochs 1 and 2 save, on rank 0 only
    assert res[0]["known"]["saves"] == [1, 2] and res[1]["known"]["saves"] == []
    for r in res:                                                                      # every rank ran every step and every reset
        k = r["known"]
        assert (k["steps"], k["batches"], k["resets"], k["epoch"]) == (EPOCHS * STEPS, EPOCHS * STEPS, EPOCHS, EPOCHS)


def test_two_ranks_return_identical_records(two_ranks):
    _, res = two_ranks
    assert res[0]["known"]["recs"] == res[1]["known"]["recs"]                         # `saved` included: rank 0's value reaches rank 1
    assert [r["saved"] for r in res[1]["known"]["recs"]] == ["model-1", "model-2", None]
    assert all(s > 0 for r in res for s in r["known"]["seconds"])
    assert res[0]["group"] == (EPOCHS, [1, 2]) and res[1]["group"] == (EPOCHS, [])   # the loop over an explicit group


def test_two_ranks_refusals(two_ranks):
    _, res = two_ranks
    for r in res:
        assert r["refused"] == dict.fromkeys(("batch", "no_shard", "wrong_shard", "trainer_group", "loop_group"), "ValueError"), r["refused"]


def test_two_ranks_status_flag_on_rank1_raises_on_both(two_ranks):
    _, res = two_ranks
    (k0, m0, e0, s0), (k1, m1, e1, s1) = res[0]["flag"], res[1]["flag"]
    assert k0 == k1 == "RuntimeError" and m0 == m1 and "(1, 1, 0)" in m0, (m0, m1)
    assert e0 == e1 == 1                                   # the first epoch completed, the flagged one raised on both ranks
    assert s0 < 60 and s1 < 60
