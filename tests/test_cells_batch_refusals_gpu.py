"""Every C entry over a packed batch in 64-point cells (normals, orientation, the outlier filters, the cross-cloud search) refuses the
same illegal host offsets with hipErrorInvalidValue, before any launch: they all go through cells_batch_check (csrc/morton_cells.hip).
The offsets that decide are the host ones, so a segment of 2^24 + 1 points needs no memory; the device buffers are those of a legal
batch of 5 + 3 points, pre-filled with sentinels that a refused call must leave alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INVALID = 1                                                     # hipErrorInvalidValue
K = 4
BAD = {"C = 1, an empty segment": (1, [0, 0]), "does not start at 0": (1, [1, 5]), "shrinks": (2, [0, 5, 3]),
       "a segment of 2^24 + 1 points": (1, [0, (1 << 24) + 1])}


@pytest.mark.parametrize("name", sorted(BAD))
def test_every_entry_refuses_bad_host_offsets(dev, name):
    import torch
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    nC, off = BAD[name][0], np.int32(BAD[name][1])
    good = np.int32([0, 5, 8])
    bad, ok = C.c_void_p(off.ctypes.data), C.c_void_p(good.ctypes.data)

    assert L.dispu_pca_normals_scratch_bytes(nC, bad, K) == 0 and L.dispu_orient_consistent_scratch_bytes(nC, bad, K) == 0
    assert L.dispu_knn_mean_dist_scratch_bytes(nC, bad, K) == 0 and L.dispu_radius_count_scratch_bytes(nC, bad) == 0
    assert L.dispu_compact_scratch_bytes(nC, bad) == 0
    assert L.dispu_knn_cross_scratch_bytes(nC, bad, ok) == 0 and L.dispu_knn_cross_scratch_bytes(nC, ok, bad) == 0

    nb = max(L.dispu_pca_normals_scratch_bytes(2, ok, K), L.dispu_orient_consistent_scratch_bytes(2, ok, K),
             L.dispu_compact_scratch_bytes(2, ok), L.dispu_knn_cross_scratch_bytes(2, ok, ok))
    assert nb > 0
    g = torch.Generator(device="cpu").manual_seed(1)
    cloud = torch.rand((8, 3), generator=g).to(dev)
    d_off = torch.from_numpy(good).to(dev)
    scratch = torch.zeros((nb,), dtype=torch.uint8, device=dev)
    f = torch.full((8, 3), 7.0, dtype=torch.float32, device=dev)             # float outputs: normals, mean distances, features, d2
    i = torch.full((8, K), -7, dtype=torch.int32, device=dev)                # int outputs: neighbours, counts, indices, labels, offsets
    d = torch.full((2, 3), 7.0, dtype=torch.float64, device=dev)             # the statistics
    b = torch.full((8,), 9, dtype=torch.uint8, device=dev)                   # the flip bytes
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    nbr = torch.full((8, K), -1, dtype=torch.int32, device=dev)
    rcs = {
        "pca_normals": L.dispu_pca_normals_segments(nC, p(d_off), bad, K, p(cloud), 0, None, p(f), None, p(i), p(status), p(scratch), nb, st),
        "orient_consistent": L.dispu_orient_consistent_segments(nC, p(d_off), bad, K, p(cloud), p(cloud), p(nbr), 0, 0, p(f), p(b), p(i), p(i),
                                                                p(status), p(scratch), nb, None, st),
        "knn_mean_dist": L.dispu_knn_mean_dist_segments(nC, p(d_off), bad, K, p(cloud), p(f), p(status), p(scratch), nb, st),
        "radius_count": L.dispu_radius_count_segments(nC, p(d_off), bad, 0.5, 2, p(cloud), p(i), p(status), p(scratch), nb, st),
        "outlier_threshold": L.dispu_outlier_threshold_segments(nC, p(d_off), bad, p(cloud), p(nbr), 2.0, p(d), st),
        "compact": L.dispu_compact_segments(nC, p(d_off), bad, p(cloud), 0, p(nbr), None, 0, None, p(f), p(i), p(i), p(scratch), nb, st),
        "knn_cross, queries": L.dispu_knn_cross_segments(nC, p(d_off), bad, p(d_off), ok, K, p(cloud), p(cloud), p(i), p(f), p(status),
                                                         p(scratch), nb, st),
        "knn_cross, refs": L.dispu_knn_cross_segments(nC, p(d_off), ok, p(d_off), bad, K, p(cloud), p(cloud), p(i), p(f), p(status),
                                                      p(scratch), nb, st),
        "transfer, queries": L.dispu_transfer_attributes_segments(nC, p(d_off), bad, p(d_off), ok, K, 0, p(cloud), p(cloud), 3, p(cloud), p(f),
                                                                  p(nbr), p(i), p(status), p(scratch), nb, st),
        "transfer, refs": L.dispu_transfer_attributes_segments(nC, p(d_off), ok, p(d_off), bad, K, 0, p(cloud), p(cloud), 3, p(cloud), p(f),
                                                               p(nbr), p(i), p(status), p(scratch), nb, st),
    }
    torch.cuda.synchronize(dev)
    assert rcs == {entry: INVALID for entry in rcs}
    assert bool((f == 7).all()) and bool((i == -7).all()) and bool((d == 7).all()) and bool((b == 9).all()) and bool((status == -7).all())
    assert not bool(scratch.any())
