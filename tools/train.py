#!/usr/bin/env python3
"""Command line of the reference's train phase, `dis-pu.py --phase train` (DisPU/model.py:181-303): read
<data_dir>/PUGAN_poisson_<P>_poisson_<4P>.h5, train the generator for --training_epoch epochs (dis-pu_amd/train.py:fit) and leave
log_train.txt, args.txt and the `model-<epoch>` checkpoints (+ the `checkpoint` state file) in --log_dir; --restore resumes from the
latest checkpoint there.  Flags and defaults are those of DisPU/configs.py that the train phase reads; --seed, --dtype, --sampler and
--tape are this project's own.  Under `python -m torch.distributed.run --nproc-per-node N tools/train.py ...` it is one of N data-parallel
ranks (train.py:fit_parallel): --batch_size stays the global batch, rank r trains on device LOCAL_RANK over RCCL (DISPU_TRAIN_BACKEND=gloo
lets ranks share devices), rank 0 alone prints and writes the artefacts.  `--sampler device` (default) draws every batch on the GPU in one launch (dataset.DeviceFetcher);
`--sampler host` is dataset.Fetcher, which repeats the reference's numpy draw sequence (np.random.seed(--seed))."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def str2bool(x):
    """true / false in any letter case; anything else is a usage error."""
    v = x.lower()
    if v not in ("true", "false"):
        raise argparse.ArgumentTypeError("expected true or false, got %r" % x)
    return v == "true"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Train the Dis-PU generator (the reference's --phase train).")
    ap.add_argument("--log_dir", default="log", help="log_train.txt, args.txt and checkpoints go here")
    ap.add_argument("--data_dir", default="data", help="holds PUGAN_poisson_<P>_poisson_<4P>.h5")
    ap.add_argument("--augment", type=str2bool, default=True, help="jitter / z rotation / scale augmentation")
    ap.add_argument("--restore", action="store_true", help="resume from the latest checkpoint of --log_dir")
    ap.add_argument("--training_epoch", type=int, default=401)
    ap.add_argument("--batch_size", type=int, default=28)
    ap.add_argument("--random", type=str2bool, default=True, help="sub-sample the input from the ground truth (non-uniform)")
    ap.add_argument("--jitter_sigma", type=float, default=0.01, help="jitter augmentation")
    ap.add_argument("--jitter_max", type=float, default=0.03, help="jitter augmentation")
    ap.add_argument("--up_ratio", type=int, default=4, help="4 only")
    ap.add_argument("--patch_num_point", type=int, default=256)
    ap.add_argument("--base_lr_g", type=float, default=0.001)
    ap.add_argument("--beta", type=float, default=0.9)
    ap.add_argument("--lr_decay", type=str2bool, default=True)
    ap.add_argument("--decay_step", type=int, default=30)
    ap.add_argument("--lr_decay_rate", type=float, default=0.7)
    ap.add_argument("--lr_clip", type=float, default=1e-6)
    ap.add_argument("--epoch_per_save", type=int, default=20)
    ap.add_argument("--use_repulse", type=str2bool, default=True)
    ap.add_argument("--repulsion_w", type=float, default=1.0, help="repulsion_weight")
    ap.add_argument("--use_uniform", type=str2bool, default=False, help="add uniform_w * get_uniform_loss(fine) to the loss (model.py:86)")
    ap.add_argument("--uniform_w", type=float, default=10.0, help="uniform_weight")
    ap.add_argument("--use_emd", type=str2bool, default=False, help="add weight_fine * emd_w * earth_mover(fine, gt, radius) to the loss (model.py:77)")
    ap.add_argument("--emd_w", type=float, default=10.0, help="the factor in front of earth_mover (model.py:77)")
    ap.add_argument("--visulize", type=str2bool, default=False, help="not supported (refused when true)")
    ap.add_argument("--seed", type=int, default=0, help="initial weights, the epoch permutations and every batch draw")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32", help="Trainer arithmetic")
    ap.add_argument("--sampler", choices=("device", "host"), default="device", help="device: one launch per batch; host: numpy draws")
    ap.add_argument("--tape", action="store_true", help="replay the step from a launch tape (Trainer.train_step_taped)")
    return ap.parse_args(argv)


def refuse_unsupported(a):
    """ValueError naming the first option value the train phase cannot honour."""
    if a.up_ratio != 4:
        raise ValueError("--up_ratio %d: the shipped generator graph is built for up_ratio 4" % a.up_ratio)
    if a.visulize:
        raise ValueError("--visulize true: the reference's matplotlib three-view plots are not available")
    if a.batch_size <= 0 or a.training_epoch < 0 or a.epoch_per_save <= 0 or a.patch_num_point <= 0:
        raise ValueError("--batch_size, --epoch_per_save and --patch_num_point must be positive, --training_epoch non-negative")
    if a.use_uniform and a.patch_num_point * a.up_ratio < 500:
        raise ValueError("--use_uniform true needs at least 500 fine points (two slots in the smallest ball): --patch_num_point >= 125, "
                         "got %d" % a.patch_num_point)
    if a.augment and not a.jitter_max > 0:
        raise ValueError("--jitter_max must be positive (the reference asserts clip > 0)")


def data_file(a):
    """dataset.py:85."""
    return os.path.join(a.data_dir, "PUGAN_poisson_%d_poisson_%d.h5" % (a.patch_num_point, a.patch_num_point * a.up_ratio))


def main(argv=None):
    a = parse_args(argv)
    try:
        refuse_unsupported(a)
    except ValueError as e:
        sys.exit(str(e))
    # started by `python -m torch.distributed.run --nproc-per-node N tools/train.py ...`: one data-parallel rank of N
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world > 1 and a.sampler == "host":
        sys.exit("--sampler host draws whole batches from numpy's global state and cannot be sharded: use --sampler device with "
                 "%d ranks" % world)
    if world > 1 and a.batch_size % world:
        sys.exit("--batch_size %d (the global batch) does not divide over %d ranks" % (a.batch_size, world))
    path = data_file(a)
    if not os.path.isfile(path):
        sys.exit("no training data at %s" % path)

    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import dataset, params, train

    if not torch.cuda.is_available():
        sys.exit("no ROCm device")
    if world == 1:
        dev = torch.device("cuda:0")
    else:
        # DISPU_TRAIN_BACKEND=gloo lets a box with fewer GPUs than ranks run the N > 1 loop (ranks share devices, collectives are
        # staged through the host); real runs use nccl == RCCL, one GPU per rank
        import torch.distributed as dist
        backend = os.environ.get("DISPU_TRAIN_BACKEND", "nccl")
        ndev = torch.cuda.device_count()
        if backend == "nccl" and local >= ndev:
            sys.exit("LOCAL_RANK %d but only %d visible GPUs" % (local, ndev))
        dev = torch.device("cuda", local % ndev)
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    try:
        say = print if rank == 0 else (lambda *args: None)
        P, G = a.patch_num_point, a.patch_num_point * a.up_ratio
        inp, gt = dataset.load_patches(path, P, G, random=a.random)
        kw = dict(batch_size=a.batch_size, patch_num_point=P, augment=a.augment, random=a.random, jitter_sigma=a.jitter_sigma,
                  jitter_max=a.jitter_max, device=dev)
        if a.sampler == "device":
            fetcher = dataset.DeviceFetcher(inp, gt, seed=a.seed, shard=(rank, world) if world > 1 else None, **kw)
        else:
            np.random.seed(a.seed)
            fetcher = dataset.Fetcher(inp, gt, **kw)
        opts = train.TrainOpts()
        for k, v in vars(a).items():
            setattr(opts, k, v)
        trainer = train.Trainer(opts, params.init_params(seed=a.seed), device=dev, dtype=a.dtype)
        loop = train.fit_parallel if world > 1 else train.fit
        recs = loop(trainer, fetcher, opts, a.log_dir, restore=a.restore, train_step_fn="taped" if a.tape else "eager", log=say)
        say("%d epochs, %d checkpoints in %s" % (len(recs), sum(r["saved"] is not None for r in recs), a.log_dir))
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
