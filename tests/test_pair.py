"""segments.Pair, the one pairing check of the operators that search one batch of clouds from another (knn_cross, transfer_attributes,
mls_project, signed_distance): the refusals that need no device, in their order and with each caller's argument name, on the CPU; the
int32 row bound of either side on the GPU, with clouds that have no memory behind them."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("knn_cross", "transfer_attributes", "mls_project", "signed_distance")


@pytest.fixture(scope="module")
def calls():
    """entry point -> (the call given its first two arguments, what it calls the second)"""
    sys.path.insert(0, ROOT)
    import dispu_amd  # noqa: F401
    from dispu_amd import attributes as A, mls as M, reconstruct as R
    return {"knn_cross": (lambda q, r: A.knn_cross(q, r, 3), "refs"),
            "transfer_attributes": (lambda q, r: A.transfer_attributes(q, r, labels=None, features=None), "refs"),
            "mls_project": (lambda q, r: M.mls_project(q, r, k=4), "refs"),
            "signed_distance": (lambda q, r: R.signed_distance(q, r, None), "points")}


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_in_order_without_a_device(calls, entry):
    import torch
    call, name = calls[entry]
    a, b = torch.zeros((8, 3)), torch.zeros((9, 3))
    with pytest.raises(ValueError, match="^%s: queries is a tensor, so %s must be one too, got list$" % (entry, name)):
        call(a, [b])
    with pytest.raises(ValueError, match="^2 query clouds but 1 reference clouds$"):
        call([a, b], [b])
    with pytest.raises(ValueError, match="^%s needs at least one cloud$" % entry):
        call([], [])
    for q, r in ((a, b), ([a, b], [b, a])):                   # well formed, so the clouds themselves are looked at: queries first
        with pytest.raises(ValueError, match="^queries of cloud 0 must live on a ROCm device"):
            call(q, r)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_row_bound_on_either_side(calls, dev, entry):
    import torch
    call, _ = calls[entry]
    full = torch.zeros((1, 3), device=dev).expand(1 << 24, 3)             # 128 x 2^24 = 2^31 rows, and no memory behind them
    one = torch.zeros((1, 3), device=dev)
    held = torch.cuda.memory_allocated(dev)
    with pytest.raises(ValueError, match=r"at most 2\^31 - 1 query points, got 2147483648$"):
        call([full] * 128, [one] * 128)
    with pytest.raises(ValueError, match=r"at most 2\^31 - 1 reference points, got 2147483648$"):
        call([one] * 128, [full] * 128)
    assert torch.cuda.memory_allocated(dev) == held                       # refused before anything was packed


@pytest.mark.gpu
def test_largest_batch_passes(dev):
    import torch
    from dispu_amd import segments as S
    full = torch.zeros((1, 3), device=dev).expand(1 << 24, 3)
    one = torch.zeros((1, 3), device=dev)
    for q, r, name in (([full] * 127, [one] * 127, "refs"), ([one] * 127, [full] * 127, "points")):
        b = S.Pair(q, r, "test", name=name)                               # the constructor alone: nothing is packed
        assert (b.C, b.queries.total, b.refs.total) == (127, len(q) * q[0].shape[0], len(r) * r[0].shape[0])
        assert b.nq == b.queries.total and not b.single and b.refs is not b.queries
    b = S.Pair([full] * 127, None, "test")                                # a batch against itself: one Packed
    assert b.refs is b.queries and b.refs.total == (1 << 31) - (1 << 24)
