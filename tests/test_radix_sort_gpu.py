"""GPU test of the device-wide stable radix sort alone (dispu_radix_sort_pairs, csrc/radix_sort.hip) against
np.argsort(kind="stable"): keys and payload exact.  Sizes around the tile and the one-workgroup scan, every pass count the bits give
(0 extra bits in a pass, a pass of one bit, all eight passes), key sets where stability decides every position, and once 2049 tiles, where
the scan of the digit table gives every thread of its one-workgroup tier two sums."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048
SIZES = (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 100003)
BITS = (1, 8, 9, 33, 64)
HIGH = 0xA5 << 56            # bits above `bits` must be equal in all keys: once zero, once this


def _key_sets(n, bits, rng):
    mask = np.uint64((1 << bits) - 1)
    rnd = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    rnd &= mask
    asc = np.sort(rnd)
    sets = {"random": rnd, "four_values": rng.integers(0, 4, n, dtype=np.uint64) & mask, "all_equal": np.full(n, 3, np.uint64) & mask,
            "sorted": asc, "reversed": asc[::-1].copy()}
    if bits <= 56:
        sets["random_high_bits_set"] = rnd | np.uint64(HIGH)
    return sets


def _sort(dev, keys, vals, bits, scratch_buf=None):
    """scratch_buf: the caller's own scratch (tests/scratch_contract.py: .ptr(), .nbytes) in place of the uninitialised one"""
    import torch
    from dispu_amd import _lib
    L = _lib.lib()
    n = keys.shape[0]
    assert _lib.RADIX_TILE == TILE
    k = torch.from_numpy(keys.view(np.int64)).to(dev)
    v = torch.from_numpy(vals.view(np.int32)).to(dev)
    ko, vo = torch.empty_like(k), torch.empty_like(v)
    nbytes = L.dispu_radix_sort_scratch_bytes(n)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    sp = _lib.ptr(scratch)
    if scratch_buf is not None:
        sp, nbytes = scratch_buf.ptr(), scratch_buf.nbytes
    _lib.check(L.dispu_radix_sort_pairs(n, bits, _lib.ptr(k), _lib.ptr(v), _lib.ptr(ko), _lib.ptr(vo), sp, nbytes,
                                        _lib.stream_ptr(dev)), "dispu_radix_sort_pairs")
    torch.cuda.synchronize()
    if scratch_buf is not None:
        scratch_buf.inputs = dict(keys=k.cpu().numpy().view(np.uint64), vals=v.cpu().numpy().view(np.uint32))   # as the call left them
    assert np.array_equal(k.cpu().numpy().view(np.uint64), keys) and np.array_equal(v.cpu().numpy().view(np.uint32), vals), "inputs were written"
    return ko.cpu().numpy().view(np.uint64), vo.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", SIZES)
def test_radix_sort_pairs_is_the_stable_argsort(dev, n, bits):
    rng = np.random.default_rng(1000 * bits + n)
    vals = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5BD1E995)       # distinct: a swap of equal keys shows
    for name, keys in _key_sets(n, bits, rng).items():
        order = np.argsort(keys, kind="stable")
        ko, vo = _sort(dev, keys, vals, bits)
        assert np.array_equal(ko, keys[order]), "%s: keys" % name
        assert np.array_equal(vo, vals[order]), "%s: payload (stability)" % name


BIG = TILE * TILE + 1         # 2049 tiles: the digit table [256][2049] has 257 scan chunks, so scan_sums_kernel's threads scan two sums each


@pytest.mark.parametrize("bits", (8, 17))
@pytest.mark.parametrize("name", ("random", "four_values"))
def test_more_than_2048_tiles(dev, name, bits):
    """the sorter's own scan tier past one sum per thread (tests/test_second_trips.py restates the threshold): one pass, and three
    passes whose last has one bit"""
    rng = np.random.default_rng(1000 * bits + BIG)
    vals = (np.arange(BIG, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5BD1E995)
    keys = _key_sets(BIG, bits, rng)[name]
    order = np.argsort(keys, kind="stable")
    ko, vo = _sort(dev, keys, vals, bits)                                       # also asserts that the inputs were only read
    assert np.array_equal(ko, keys[order]), "%s: keys" % name
    assert np.array_equal(vo, vals[order]), "%s: payload (stability)" % name


def test_zero_bits_copies_and_two_runs_agree(dev):
    rng = np.random.default_rng(5)
    n = 5 * TILE + 3
    keys = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    vals = np.arange(n, dtype=np.uint32)
    ko, vo = _sort(dev, np.full(n, 7, np.uint64), vals, 0)
    assert np.array_equal(ko, np.full(n, 7, np.uint64)) and np.array_equal(vo, vals)
    a, b = _sort(dev, keys, vals, 40), _sort(dev, keys, vals, 40)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sorter_refuses_bad_arguments(dev):
    import torch
    from dispu_amd import _lib
    L = _lib.lib()
    k = torch.zeros(8, dtype=torch.int64, device=dev)
    v = torch.zeros(8, dtype=torch.int32, device=dev)
    s = torch.empty(L.dispu_radix_sort_scratch_bytes(8), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    assert L.dispu_radix_sort_pairs(8, 65, _lib.ptr(k), _lib.ptr(v), _lib.ptr(k.clone()), _lib.ptr(v.clone()), _lib.ptr(s), s.numel(), st) != 0
    assert L.dispu_radix_sort_pairs(8, 8, _lib.ptr(k), _lib.ptr(v), _lib.ptr(k), _lib.ptr(v), _lib.ptr(s), s.numel(), st) != 0      # aliased
    assert L.dispu_radix_sort_pairs(8, 8, _lib.ptr(k), _lib.ptr(v), _lib.ptr(k.clone()), _lib.ptr(v.clone()), _lib.ptr(s), 16, st) != 0
    assert L.dispu_radix_sort_pairs(1 << 31, 8, _lib.ptr(k), _lib.ptr(v), _lib.ptr(k.clone()), _lib.ptr(v.clone()), _lib.ptr(s), s.numel(), st) != 0
    assert L.dispu_radix_sort_scratch_bytes(1 << 31) == 0 and L.dispu_radix_sort_scratch_bytes(0) == 0
    torch.cuda.synchronize()
