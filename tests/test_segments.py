"""dis-pu_amd/segments.py, the packed ragged batch of the whole-cloud operations: the device-free helpers on the CPU, and the class
Packed (whose clouds must live on a device) on the GPU with the clouds that reach each of its refusals."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    sys.path.insert(0, ROOT)
    import dispu_amd  # noqa: F401
    from dispu_amd import segments
    return segments


def test_offsets(S):
    from dispu_amd import upsample as U
    off = S.offsets([3, 1, 4])
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 4, 8]
    assert S.offsets([]).tolist() == [0]
    assert S.offsets([2 ** 31 - 1]).tolist() == [0, 2 ** 31 - 1]
    with pytest.raises(ValueError, match=re.escape("a packed batch holds at most 2^31 - 1 rows, got 2147483648")):
        S.offsets([2 ** 30, 2 ** 30])
    assert U.segment_offsets is S.offsets                       # the name tests and tools call


def test_check_int_range(S):
    assert S.check_int_range(4, 4, 32, "k") == 4 and S.check_int_range(np.int64(32), 4, 32, "k") == 32
    assert type(S.check_int_range(np.int32(7), 4, 32, "k")) is int
    for bad, shown in ((True, "True"), (3.0, "3.0"), (3, "3"), (33, "33"), ("8", "'8'"), (None, "None")):
        with pytest.raises(ValueError, match="^" + re.escape("k must be an integer in 4 .. 32, got %s" % shown) + "$"):
            S.check_int_range(bad, 4, 32, "k")
    with pytest.raises(ValueError, match="^" + re.escape("cap must be an integer in 1 .. 31, got 0") + "$"):
        S.check_int_range(0, 1, 31, "cap")
    assert S.is_int(5) and S.is_int(np.int16(5)) and not S.is_int(False) and not S.is_int(5.0) and not S.is_int(np.float32(5))


def test_split(S):
    import torch
    t = torch.arange(24).reshape(8, 3)
    off = S.offsets([3, 1, 4])
    parts = S.split(t, off, False)
    assert [p.tolist() for p in parts] == [t[0:3].tolist(), t[3:4].tolist(), t[4:8].tolist()]
    assert torch.equal(S.split(t, S.offsets([8]), True), t)
    # the compaction case: fewer rows than the batch had, under a second offset table (int64, as it comes back from the device)
    kept, new_off = t[:5], np.int64([0, 2, 2, 5])
    parts = S.split(kept, new_off, False)
    assert [p.shape[0] for p in parts] == [2, 0, 3] and torch.equal(parts[2], t[2:5])
    assert torch.equal(S.split(kept, np.int64([0, 5]), True), kept)
    assert S.split(t[:0], np.int64([0, 0]), True).shape == (0, 3)


def test_check_cloud_without_a_device(S):
    import torch
    for bad, text in ((np.zeros((5, 3), np.float32), "cloud 0: expected a float32 [n, 3] tensor on a ROCm device, got ndarray"),
                      (torch.zeros((5, 3)), "cloud 0 must live on a ROCm device (dis-pu_amd has no CPU path)")):
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            S.check_cloud(bad, "cloud 0")
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            S.Packed([bad], "test")
    with pytest.raises(ValueError, match="^" + re.escape("points must be a float32 [n, 3] tensor on a ROCm device or a list of them, got int") + "$"):
        S.Packed(3, "test")
    with pytest.raises(ValueError, match="^test needs at least one cloud$"):
        S.Packed([], "test")
    with pytest.raises(ValueError, match="^at most 65535 clouds per call, got 65536$"):
        S.Packed([None] * 65536, "test")


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[1], [64, 65, 1]], ids=["one_point", "cell_edge_and_one_point"])
def test_packed(S, dev, sizes):
    import torch
    g = torch.Generator(device="cpu").manual_seed(len(sizes))
    clouds = [torch.rand((n, 3), generator=g).to(dev) for n in sizes]
    b = S.Packed(clouds[0] if len(sizes) == 1 else clouds, "test", words=3)
    assert b.single == (len(sizes) == 1) and b.C == len(sizes) and b.total == sum(sizes) and b.dev == clouds[0].device
    assert b.off.dtype == np.int32 and b.off.tolist() == S.offsets(sizes).tolist()
    b.pack()
    assert b.cloud.is_contiguous() and torch.equal(b.cloud, torch.cat(clouds))
    assert b.d_off.dtype == torch.int32 and b.d_off.cpu().tolist() == b.off.tolist()
    assert b.status.dtype == torch.int32 and b.status.cpu().tolist() == [0] * len(sizes)
    rows = [torch.full((n,), c, dtype=torch.int32, device=dev) for c, n in enumerate(sizes)]
    packed = b.pack_like(rows)
    assert packed.shape == (sum(sizes),) and packed.is_contiguous()
    back = b.split(packed)
    if b.single:
        assert torch.equal(back, rows[0]) and torch.equal(b.split(b.cloud), clouds[0])
    else:
        assert len(back) == len(sizes) and all(torch.equal(x, y) for x, y in zip(back, rows))
        assert all(torch.equal(x, y) for x, y in zip(b.split(b.cloud), clouds))
    assert b.scratch(16, "dispu_x").shape == (16,) and b.scratch(16, "dispu_x").dtype == torch.uint8
    with pytest.raises(ValueError, match="^dispu_x refuses these clouds$"):
        b.scratch(0, "dispu_x")
    b.refuse_non_finite()
    b.status[-1] = 1
    with pytest.raises(ValueError, match="^cloud %d holds a NaN or an infinite coordinate$" % (len(sizes) - 1)):
        b.refuse_non_finite()
    b.refuse_non_finite(torch.zeros(len(sizes), dtype=torch.int32))           # a status of the caller's own, as read back after a compaction
    b.limit(2 ** 31 // sum(sizes) - 1)
    with pytest.raises(ValueError, match="^" + re.escape("a packed batch holds at most 2^31 - 1 neighbour slots, got %d points at k = 7" % sum(sizes)) + "$"):
        b.limit(2 ** 31 // sum(sizes) + 1, unit="neighbour slots", tail=" at k = 7")
    b2 = S.Packed(clouds, "test")
    b2.pack(status=False)
    assert b2.status is None and not b2.single


@pytest.mark.gpu
def test_packed_refusals(S, dev):
    import torch
    ok = torch.zeros((64, 3), device=dev)
    for bad, text in ((torch.zeros((0, 3), device=dev), "cloud 1 has 0 points, expected 1 .. 2^24"),
                      (torch.zeros((5, 2), device=dev), "cloud 1: expected an [n, 3] tensor, got shape (5, 2)"),
                      (torch.zeros((5, 3), dtype=torch.float64, device=dev), "cloud 1 must be float32, got torch.float64"),
                      (torch.zeros((5, 3)), "cloud 1 must live on a ROCm device (dis-pu_amd has no CPU path)"),
                      (torch.zeros((1, 3), device=dev).expand((1 << 24) + 1, 3), "cloud 1 has 16777217 points, expected 1 .. 2^24")):
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            S.Packed([ok, bad], "test")
    with pytest.raises(ValueError, match="^" + re.escape("refs of cloud 0 has 0 points, expected 1 .. 2^24") + "$"):
        S.Packed(torch.zeros((0, 3), device=dev), "test", label="refs of cloud %d")
    full = torch.zeros((1, 3), device=dev).expand(1 << 24, 3)                # 43 x 2^24 points x 3 words >= 2^31, and no memory behind them
    with pytest.raises(ValueError, match="^" + re.escape("a packed batch holds at most 2^31 - 1 output words, got 721420288 points") + "$"):
        S.Packed([full] * 43, "test", words=3)
    assert S.Packed([full] * 42, "test", words=3).total == 42 << 24
