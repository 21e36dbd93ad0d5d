"""CPU tests of dis-pu_amd/poisson_cells.py: what is refused before the device is touched, the index map of shuffle_seed, the r_hi
arithmetic, and the constants the module shares with include/dispu_hip.h.  No compute call is made here."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeDeviceTensor(torch.Tensor):
    """a host tensor that claims to live on a device: passes the checks that come before any launch, never reaches one"""
    is_cuda = True


def _fake(n):
    return torch.zeros((n, 3)).as_subclass(_FakeDeviceTensor)


def test_refusals_need_no_device():
    from dispu_amd import poisson_cells as PC
    for bad in (torch.zeros(8, 3), [torch.zeros(8, 3)]):
        with pytest.raises(ValueError, match="must live on a ROCm device"):
            PC.keep(bad, 0.1)
        with pytest.raises(ValueError, match="must live on a ROCm device"):
            PC.select(bad, 2, 0.1)
    with pytest.raises(ValueError, match="a float32 .n, 3. tensor"):
        PC.keep(np.zeros((8, 3), np.float32), 0.1)
    with pytest.raises(ValueError, match="at least one cloud"):
        PC.keep([], 0.1)
    for shape in ((8,), (8, 2), (2, 8, 3)):
        with pytest.raises(ValueError, match="expected an .n, 3. tensor"):
            PC.keep(torch.zeros(shape).as_subclass(_FakeDeviceTensor), 0.1)
    with pytest.raises(ValueError, match="expected 1 .. 2\\^24"):
        PC.keep(_fake(0), 0.1)
    with pytest.raises(ValueError, match="must be float32"):
        PC.keep(torch.zeros((8, 3), dtype=torch.float64).as_subclass(_FakeDeviceTensor), 0.1)
    # radii, m: the wrong number, the wrong kind
    with pytest.raises(ValueError, match="radius: one value per cloud \\(2\\), got 3"):
        PC.keep([_fake(8), _fake(9)], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="radius must be finite"):
        PC.keep(_fake(8), float("inf"))
    with pytest.raises(ValueError, match="r_hi: one value per cloud \\(1\\), got 2"):
        PC.select(_fake(8), 2, [0.1, 0.2])
    with pytest.raises(ValueError, match="m: one value per cloud \\(2\\), got 1"):
        PC.select([_fake(8), _fake(9)], [2], 0.1)
    with pytest.raises(ValueError, match="m must be integers"):
        PC.select(_fake(8), 2.5, 0.1)
    with pytest.raises(ValueError, match="cannot select 9 of 8 points \\(cloud 0\\)"):
        PC.select(_fake(8), 9, 0.1)
    with pytest.raises(ValueError, match="cannot select 10 of 9 points \\(cloud 1\\)"):
        PC.select([_fake(8), _fake(9)], [8, 10], 0.1)
    with pytest.raises(ValueError, match="cannot select 0 of 8"):
        PC.select(_fake(8), 0, 0.1)
    for steps in (-1, 1.5, None):
        with pytest.raises(ValueError, match="steps must be an integer >= 0"):
            PC.select(_fake(8), 2, 0.1, steps=steps)
    for seed in (1.5, "7", True):
        with pytest.raises(ValueError, match="shuffle_seed must be None or an integer"):
            PC.keep(_fake(8), 0.1, shuffle_seed=seed)
        with pytest.raises(ValueError, match="shuffle_seed must be None or an integer"):
            PC.select(_fake(8), 2, 0.1, shuffle_seed=seed)


def test_upsample_ragged_refuses_an_unknown_merge():
    from dispu_amd import upsample as U
    with pytest.raises(ValueError, match="merge must be 'fps' or 'poisson'"):
        U.upsample_ragged(None, [np.zeros((256, 3), np.float32)], merge="random")


def test_shuffle_index_map_is_a_pure_function_and_inverts_the_permutation():
    from dispu_amd import poisson_cells as PC
    rng = np.random.default_rng(3)
    for seed, c, n in ((0, 0, 1), (7, 0, 2), (7, 3, 1000), (2 ** 31, 5, 257), (-4, 1, 64)):
        perm = PC.shuffle_permutation(seed, c, n)
        assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(n))
        assert np.array_equal(perm, PC.shuffle_permutation(seed, c, n))                                  # no hidden state
        if 0 <= seed + c < 2 ** 32:
            assert np.array_equal(perm, np.random.RandomState(seed + c).permutation(n))                  # the documented stream
        assert np.array_equal(PC.shuffle_permutation(seed, c + 1, n), PC.shuffle_permutation(seed + 1, c, n))
        # per-point values: what position j of the permuted cloud holds is input point perm[j]'s
        values = rng.integers(0, 255, n).astype(np.uint8)
        assert np.array_equal(PC.unshuffle_flags(values[perm], perm), values)
        # indices: a subset of the permuted cloud names the same points of the input, ascending there
        pick = np.sort(rng.choice(n, size=max(1, n // 3), replace=False)).astype(np.int32)
        back = PC.unshuffle_indices(pick, perm)
        assert back.dtype == np.int32 and np.all(np.diff(back) > 0)
        pts = rng.random((n, 3))
        assert np.array_equal(np.sort(pts[perm][pick], axis=0), np.sort(pts[back], axis=0))
        assert set(back.tolist()) == set(perm[pick].tolist())


def test_spacing_r_hi_arithmetic():
    from dispu_amd import poisson_cells as PC
    assert PC.spacing_from_mean_nn(0.5, 4) == 0.5
    assert PC.spacing_from_mean_nn(0.5, 16) == 0.25
    assert PC.spacing_from_mean_nn(0.03, 4) == 2.0 * 0.03 / math.sqrt(4.0)
    assert PC.spacing_from_mean_nn(0.0, 4) == 0.0
    with pytest.raises(ValueError, match="final_ratio must be positive"):
        PC.spacing_from_mean_nn(0.1, 0)


def test_constants_match_the_header():
    from dispu_amd import _lib
    from dispu_amd import poisson_cells as PC
    text = open(os.path.join(ROOT, "include", "dispu_hip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define DISPU_(\w+) (\d+)\s*$", text, flags=re.M)}
    assert defines["POISSON_CELLS_NONFINITE"] == _lib.POISSON_CELLS_NONFINITE == PC.STATUS_NONFINITE == 4
    assert defines["POISSON_MAX_ROUNDS"] == _lib.POISSON_MAX_ROUNDS == PC.MAX_ROUNDS
    assert (PC.STATUS_NOT_SETTLED, PC.STATUS_SHORT) == (1, 2)                     # bits 0 and 1, as dispu_poisson_disk_select's
    for name in ("dispu_poisson_cells_scratch_bytes", "dispu_poisson_cells_keep", "dispu_poisson_cells_select"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, text)


def test_c_entries_refuse_what_the_shims_refuse():
    """no device is needed: every refusal comes before the first launch"""
    import ctypes
    from dispu_amd import _lib
    L = _lib.lib()
    assert L.dispu_poisson_cells_scratch_bytes(0, 10) == 0 and L.dispu_poisson_cells_scratch_bytes(65536, 10 ** 6) == 0
    assert L.dispu_poisson_cells_scratch_bytes(3, 2) == 0 and L.dispu_poisson_cells_scratch_bytes(1, 2 ** 31) == 0
    small, large = L.dispu_poisson_cells_scratch_bytes(1, 1000), L.dispu_poisson_cells_scratch_bytes(2, 100000)
    assert 0 < small < large
    off = (ctypes.c_int * 3)(0, 5, 9)
    moff_bad = (ctypes.c_int * 3)(0, 6, 8)               # 6 of 5
    one = ctypes.c_void_p(16)                            # non-null, aligned, never dereferenced: the refusals come first
    V = ctypes.cast
    p = lambda a: V(a, ctypes.c_void_p)
    assert L.dispu_poisson_cells_keep(2, p(off), p(off), one, one, one, one, None, one, 0, one, None) != 0        # scratch too small
    assert L.dispu_poisson_cells_keep(2, p(off), p(off), None, one, one, one, None, one, large, one, None) != 0   # no points
    assert L.dispu_poisson_cells_keep(0, p(off), p(off), one, one, one, one, None, one, large, one, None) != 0    # no segment
    bad = (ctypes.c_int * 3)(0, 5, 5)                    # an empty segment
    assert L.dispu_poisson_cells_keep(2, p(bad), p(bad), one, one, one, one, None, one, large, one, None) != 0
    assert L.dispu_poisson_cells_select(2, p(off), p(moff_bad), p(off), p(moff_bad), 12, one, one, one, one, one, None, one, large, one,
                                        None) != 0
    assert L.dispu_poisson_cells_select(2, p(off), p(off), p(off), p(off), -1, one, one, one, one, one, None, one, large, one, None) != 0
