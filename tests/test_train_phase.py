"""Train phase without a GPU: the host Philox twin against Random123's known answers, tools/train.py's argument handling, the
log / args.txt formats of DisPU/model.py:198-222 and the epoch loop's control flow (steps per epoch, save rule, restore start)
on a stub trainer and a stub fetcher."""
import importlib.util
import os
import re
import subprocess
import sys
import types

import pytest

import sampler_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "train.py")


def _tool():
    spec = importlib.util.spec_from_file_location("train_tool", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ Philox twin ----
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_twin_known_answers(counter, key, want):
    assert SO.philox4x32_10(counter, key) == want


def test_philox_block_layout():
    """counter = (block number, stream, position, epoch), key = the seed's two halves."""
    assert SO.block((0xa4093822 | (0x299f31d0 << 32)), 0x03707344, 0x13198a2e, stream=0x85a308d3, number=0x243f6a88) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    assert SO.u01(0xffffffff) == 1.0 - 2.0 ** -24 and SO.u01(0xff) == 0.0


# ----------------------------------------------------------------------------------------------------- the tool ----
def test_tool_help_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    for flag in ("--log_dir", "--data_dir", "--augment", "--restore", "--training_epoch", "--batch_size", "--random", "--jitter_sigma",
                 "--jitter_max", "--up_ratio", "--patch_num_point", "--base_lr_g", "--beta", "--lr_decay", "--decay_step",
                 "--lr_decay_rate", "--lr_clip", "--epoch_per_save", "--use_repulse", "--repulsion_w", "--seed", "--dtype", "--sampler",
                 "--tape"):
        assert flag in out, flag


def test_tool_defaults_are_the_reference_settings():
    a = _tool().parse_args([])
    assert (a.log_dir, a.data_dir, a.augment, a.restore, a.training_epoch, a.batch_size, a.random) == ("log", "data", True, False, 401, 28, True)
    assert (a.jitter_sigma, a.jitter_max, a.up_ratio, a.patch_num_point) == (0.01, 0.03, 4, 256)
    assert (a.base_lr_g, a.beta, a.lr_decay, a.decay_step, a.lr_decay_rate, a.lr_clip) == (0.001, 0.9, True, 30, 0.7, 1e-6)
    assert (a.epoch_per_save, a.use_repulse, a.repulsion_w) == (20, True, 1.0)
    assert (a.seed, a.dtype, a.sampler, a.tape) == (0, "f32", "device", False)
    assert _tool().data_file(a) == os.path.join("data", "PUGAN_poisson_256_poisson_1024.h5")
    assert _tool().parse_args(["--augment", "False", "--lr_decay", "false"]).augment is False
    assert _tool().parse_args(["--augment", "TRUE"]).augment is True
    for bad in ("t", "rue", "", "1", "yes"):             # only true / false are values of a boolean flag
        with pytest.raises(SystemExit):
            _tool().parse_args(["--augment", bad])


@pytest.mark.parametrize("argv,word", [(["--up_ratio", "2"], "up_ratio"), (["--visulize", "true"], "visulize"),
                                       (["--batch_size", "0"], "batch_size"), (["--jitter_max", "0"], "jitter_max")])
def test_tool_refuses_unsupported_values(argv, word, tmp_path):
    tool = _tool()
    with pytest.raises(ValueError, match=word):
        tool.refuse_unsupported(tool.parse_args(argv))
    r = subprocess.run([sys.executable, TOOL, "--data_dir", str(tmp_path)] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and word in r.stderr.decode()


def test_tool_refuses_bad_choices_and_missing_data(tmp_path):
    for argv in (["--dtype", "fp8"], ["--sampler", "thread"]):
        r = subprocess.run([sys.executable, TOOL] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2
    r = subprocess.run([sys.executable, TOOL, "--data_dir", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and "PUGAN_poisson_256_poisson_1024.h5" in r.stderr.decode()


# --------------------------------------------------------------------------------------------------- formatters ----
def test_log_line_and_args_formats():
    from dispu_amd import train
    line = train.format_log_line(7, 1.5, 0.25, 12.0, 0.125, 3.0, 90.0)
    assert line == "epoch 0007 g_loss=1.500000000  coarse_cd=0.250000000  coarse_hd=12.000000000  fine_cd=0.125000000 fine_hd=3.000000000  time=1.5000"
    assert train.LOG_FORMAT == "epoch %04d g_loss=%.9f  coarse_cd=%.9f  coarse_hd=%.9f  fine_cd=%.9f fine_hd=%.9f  time=%.4f"
    ns = types.SimpleNamespace(log_dir="log", batch_size=28, augment=True, base_lr_g=0.001)
    assert train.format_args(ns) == "augment: True\nbase_lr_g: 0.001\nbatch_size: 28\nlog_dir: log\n"
    assert train.steps_per_epoch(24, 4) == 5 and train.steps_per_epoch(24000, 28) == 856 and train.steps_per_epoch(10, 4) == 1


# ----------------------------------------------------------------------------------------------------- the loop ----
class StubFetcher(object):
    def __init__(self, length, batch_size):
        self.length, self.batch_size = length, batch_size
        self.batches, self.resets = 0, 0

    def __len__(self):
        return self.length

    def reset(self):
        self.resets += 1

    def next_batch(self):
        self.batches += 1
        return "x", "gt", "radius"


class StubTrainer(object):
    """fine_cd of epoch e (constant within it) comes from a list; counts steps and remembers the epoch each ran in."""

    def __init__(self, fine_cd):
        self.fine_cd, self.epoch, self.steps, self.taped = fine_cd, 0, [], 0

    def train_step(self, x, gt, radius):
        assert (x, gt, radius) == ("x", "gt", "radius")
        self.steps.append(self.epoch)
        f = self.fine_cd[self.epoch]
        return {"pu_loss": 10.0 + f, "dis_coarse_cd": 2.0, "dis_fine_cd": f, "repulsion_loss": 0.0, "weight_fine": 0.01}

    def train_step_taped(self, x, gt, radius):
        self.taped += 1
        return self.train_step(x, gt, radius)


def _fit(tmp_path, fine_cd, epochs, per_save, restore_epoch=None, length=24, batch=4, step_fn="eager"):
    from dispu_amd import train
    saves, fetcher, trainer = [], StubFetcher(length, batch), StubTrainer(fine_cd)
    opts = types.SimpleNamespace(batch_size=batch, training_epoch=epochs, epoch_per_save=per_save)

    def restore_fn(log_dir, t):
        t.epoch = restore_epoch
        return restore_epoch

    recs = train.fit(trainer, fetcher, opts, str(tmp_path), restore=restore_epoch is not None, train_step_fn=step_fn,
                     save_fn=lambda d, t, e: saves.append((e, t.epoch)) or "model-%d" % e, restore_fn=restore_fn,
                     hd_fn=lambda t, x, gt, r: (3.0, 4.0))
    return recs, saves, fetcher, trainer


LINE = re.compile(r"^epoch \d{4} g_loss=-?\d+\.\d{9}  coarse_cd=-?\d+\.\d{9}  coarse_hd=-?\d+\.\d{9}  fine_cd=-?\d+\.\d{9} fine_hd=-?\d+\.\d{9}  time=\d+\.\d{4}$")


def test_loop_steps_and_save_rule(tmp_path):
    # epochs 1..6 (numbered after the increment); fine_cd indexed by the epoch the steps RAN in (0..5)
    fine = [5.0, 4.0, 4.5, 3.0, 3.0, 2.0]
    recs, saves, fetcher, trainer = _fit(tmp_path, fine, epochs=6, per_save=2)
    assert fetcher.batches == 6 * 5 and fetcher.resets == 6 and trainer.steps == [e for e in range(6) for _ in range(5)]
    assert [r["epoch"] for r in recs] == [1, 2, 3, 4, 5, 6] and all(r["steps"] == 5 for r in recs)
    # saved only where epoch % 2 == 0 AND strictly better than the best SAVED so far: epoch 2 (4.0), epoch 4 (3.0), epoch 6 (2.0)
    assert saves == [(2, 2), (4, 4), (6, 6)]
    fine = [5.0, 4.0, 4.5, 4.0, 3.0, 4.0, 9.0, 1.0]
    recs, saves, _, _ = _fit(tmp_path, fine, epochs=8, per_save=2)
    assert [e for e, _ in saves] == [2, 8]           # epoch 4 ties the best (not strictly better), epoch 6 is worse, odd epochs never save
    assert [r["saved"] for r in recs] == [None, "model-2", None, None, None, None, None, "model-8"]
    lines = open(os.path.join(str(tmp_path), "log_train.txt")).read().splitlines()
    assert len([l for l in lines if LINE.match(l)]) == 8
    assert lines[1].startswith("epoch 0001 g_loss=15.000000000  coarse_cd=2.000000000  coarse_hd=3.000000000  fine_cd=5.000000000 fine_hd=4.000000000  time=")
    assert open(os.path.join(str(tmp_path), "args.txt")).read() == "batch_size: 4\nepoch_per_save: 2\ntraining_epoch: 8\n"


def test_loop_restore_start_epoch_and_log_mode(tmp_path):
    recs, saves, fetcher, trainer = _fit(tmp_path, [1.0] * 10, epochs=3, per_save=1)
    assert len(recs) == 3
    recs, saves, fetcher, trainer = _fit(tmp_path, [1.0] * 10, epochs=7, per_save=1, restore_epoch=3)
    assert [r["epoch"] for r in recs] == [4, 5, 6, 7] and trainer.steps[0] == 3 and fetcher.batches == 4 * 5
    assert [e for e, _ in saves] == [4]              # best starts at infinity after a restore, as in the reference
    lines = [l for l in open(os.path.join(str(tmp_path), "log_train.txt")).read().splitlines() if LINE.match(l)]
    assert [int(l[6:10]) for l in lines] == [1, 2, 3, 4, 5, 6, 7]         # 'a' mode keeps the first run's lines
    recs, _, _, _ = _fit(tmp_path, [1.0] * 10, epochs=3, per_save=1, restore_epoch=5)
    assert recs == []                                 # range(5, 3) is empty


def test_loop_restore_advances_an_epoch_counting_fetcher(tmp_path):
    from dispu_amd import train

    class Counting(StubFetcher):
        epoch = 0

        def reset(self):
            StubFetcher.reset(self)
            self.epoch += 1

    f, t = Counting(24, 4), StubTrainer([1.0] * 10)
    opts = types.SimpleNamespace(batch_size=4, training_epoch=5, epoch_per_save=1)

    def restore_fn(log_dir, tr):
        tr.epoch = 3
        return 3

    seen = []
    train.fit(t, f, opts, str(tmp_path), restore=True, save_fn=lambda d, tr, e: seen.append((e, f.epoch)) or "m", restore_fn=restore_fn,
              hd_fn=lambda tr, x, gt, r: (3.0, 4.0))
    assert f.resets == 3 + 2 and f.epoch == 5 and seen[0] == (4, 4)      # three resets to reach epoch 3, then one per epoch run


def test_sampler_limits_agree_between_header_and_kernel():
    """DISPU_SAMPLER_MAX_ROUNDS / DISPU_SAMPLER_MAX_G are written in the public header only: the kernel source uses them under these
    names and holds no value of its own (it compiles against the header through csrc/common.h)."""
    pat = re.compile(r"^#define (DISPU_SAMPLER_MAX_\w+) (\d+)", re.M)
    hdr = dict(pat.findall(open(os.path.join(ROOT, "include", "dispu_hip.h")).read()))
    src = open(os.path.join(ROOT, "dis-pu_amd", "csrc", "batch_sampler.hip")).read()
    common = open(os.path.join(ROOT, "dis-pu_amd", "csrc", "common.h")).read()
    assert set(hdr) == {"DISPU_SAMPLER_MAX_ROUNDS", "DISPU_SAMPLER_MAX_G"} and all(int(v) > 0 for v in hdr.values())
    assert not pat.findall(src) and not pat.findall(common) and 'include/dispu_hip.h"' in common
    assert all(re.search(r"\b%s\b" % name, src) for name in hdr)


def test_loop_step_function_choice(tmp_path):
    _, _, _, trainer = _fit(tmp_path, [1.0] * 3, epochs=1, per_save=1, step_fn="taped")
    assert trainer.taped == 5
    with pytest.raises(ValueError):
        _fit(tmp_path, [1.0] * 3, epochs=1, per_save=1, step_fn="graphed")


def test_fit_refuses_a_process_group(tmp_path, monkeypatch):
    import torch.distributed as dist
    from dispu_amd import train
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        train.fit(object(), object(), object(), str(tmp_path))


def test_device_fetcher_refuses_before_any_device_work():
    """P > G (and a random=False input of the wrong size) raise in the constructor, before anything touches a device."""
    import numpy as np
    from dispu_amd import dataset
    gt = np.zeros((4, 64, 3), np.float32)
    with pytest.raises(ValueError, match="distinct"):
        dataset.DeviceFetcher(gt, gt, 2, patch_num_point=65, device="cpu")
    with pytest.raises(ValueError, match="random=False"):
        dataset.DeviceFetcher(gt, gt, 2, patch_num_point=32, random=False, device="cpu")
