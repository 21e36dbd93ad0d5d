"""train.fit_parallel with the EMD term on (TrainOpts.use_emd): two `gloo` ranks sharing the test box's one GPU, the transport and
setup of tests/test_fit_parallel_gpu.py (12 synthetic patches 256 -> 1024, GLOBAL batch 4 = 2 per rank, one epoch of 2 steps).
ONE spawn; the test reads its report: every step of every rank reports a positive dis_fine_emd that is part of its pu_loss inside
the weight_fine parenthesis, the replicas stay bit-identical, and the epoch's dis_fine_emd (the record and the last column of the
line in log_train.txt) is the mean over ranks and steps of the ranks' values, like g_loss."""
import hashlib
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("flat_p", "flat_m", "flat_v", "moving_mean", "moving_var")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _digest(t):
    h = hashlib.sha1()
    for k in STATE:
        h.update(getattr(t, k).detach().cpu().numpy().tobytes())
    return h.hexdigest()


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dispu_amd import dataset, params, synth, train
        dev = torch.device("cuda:0")
        _, gt = synth.patch_with_gt(12, 256, 1024, seed=21)
        fa = dataset.DeviceFetcher(gt, gt, 4, patch_num_point=256, device=dev, seed=5, shard=(rank, world))
        opts = train.TrainOpts()
        opts.batch_size, opts.training_epoch, opts.epoch_per_save, opts.use_emd = 4, 1, 1, True
        a = train.Trainer(opts, params.init_params(seed=7), device=dev)
        steps, inner = [], a.train_step

        def step(x, g, radius):
            terms = inner(x, g, radius)
            steps.append((dict((k, float(v)) for k, v in terms.items()), _digest(a), int(x.shape[0])))
            return terms
        a.train_step = step
        recs = train.fit_parallel(a, fa, opts, os.path.join(tmp, "log"))
        q.put((rank, dict(recs=[{k: v for k, v in r.items() if k != "seconds"} for r in recs], terms=[s[0] for s in steps],
                          digests=[s[1] for s in steps], rows=[s[2] for s in steps])))
    finally:
        dist.destroy_process_group()


def test_fit_parallel_with_the_emd_term(dev, tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=300))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    reps = [r[1] for r in sorted(res, key=lambda r: r[0])]
    assert all(len(r["terms"]) == 2 and r["rows"] == [2, 2] for r in reps)
    assert reps[0]["digests"] == reps[1]["digests"], "the replicas drifted apart"
    for r in reps:
        for s in r["terms"]:
            assert s["dis_fine_emd"] > 0 and "uniform_loss" not in s
            total = s["dis_coarse_cd"] + s["weight_fine"] * (s["dis_fine_cd"] + s["dis_fine_emd"]) + s["repulsion_loss"]
            assert abs(s["pu_loss"] - total) <= 1e-5 * total
    mean = float(np.mean([s["pu_loss"] for r in reps for s in r["terms"]]))
    # per step the mean of the two ranks' values, then the mean over steps (train.reduce_meter_tables), in float64
    emd = float(np.mean([np.mean([r["terms"][i]["dis_fine_emd"] for r in reps]) for i in range(2)]))
    assert reps[0]["terms"][0]["dis_fine_emd"] != reps[1]["terms"][0]["dis_fine_emd"], "the ranks saw the same shard"
    rec = reps[0]["recs"][0]
    assert reps[1]["recs"][0]["dis_fine_emd"] == rec["dis_fine_emd"]
    print("[measured] fit_parallel with emd: g_loss %.6f (mean pu_loss %.6f), dis_fine_emd %.6f (mean over ranks %.6f)" %
          (rec["g_loss"], mean, rec["dis_fine_emd"], emd))
    assert abs(rec["g_loss"] - mean) <= 1e-5 * mean and abs(rec["dis_fine_emd"] - emd) <= 1e-5 * emd
    line = [l for l in open(str(tmp_path / "log" / "log_train.txt")).read().splitlines() if l.startswith("epoch 0001")]
    assert len(line) == 1 and abs(float(re.search(r"g_loss=(\d+\.\d+)", line[0]).group(1)) - mean) <= 1e-5 * mean
    logged = re.search(r"  dis_fine_emd=(\d+\.\d+)$", line[0])
    assert logged and np.isfinite(float(logged.group(1))) and abs(float(logged.group(1)) - emd) <= 1e-5 * emd
