"""Host side of the large-cloud farthest point sampling (dispu_fps_cells*, dispu_fps_segments_auto*): size queries, the dispatch rule and
the Python argument checks.  No GPU."""
import numpy as np
import pytest


def _hp(a):
    from dispu_amd import _lib
    return _lib.C.c_void_p(a.ctypes.data)


def _offs(ns, ms):
    off, moff = np.zeros(len(ns) + 1, np.int32), np.zeros(len(ms) + 1, np.int32)
    off[1:], moff[1:] = np.cumsum(ns), np.cumsum(ms)
    return off, moff


def test_scratch_bytes_refuses_illegal_offsets():
    from dispu_amd import _lib
    L = _lib.lib()
    off, moff = _offs([300, 25000], [10, 20])
    assert L.dispu_fps_cells_scratch_bytes(2, _hp(off), _hp(moff), 0) > 0
    assert L.dispu_fps_cells_scratch_bytes(0, _hp(off), _hp(moff), 0) == 0
    assert L.dispu_fps_cells_scratch_bytes(-1, _hp(off), _hp(moff), 0) == 0
    assert L.dispu_fps_cells_scratch_bytes(2, None, _hp(moff), 0) == 0
    assert L.dispu_fps_cells_scratch_bytes(2, _hp(off), None, 0) == 0
    for bad_off, bad_moff in ((np.array([1, 300, 600], np.int32), moff),          # does not start at 0
                              (np.array([0, 300, 300], np.int32), moff),          # an empty segment
                              (np.array([0, 300, 200], np.int32), moff),          # decreasing
                              (off, np.array([0, 10, 10], np.int32)),             # a segment without samples
                              (off, np.array([2, 10, 20], np.int32))):
        assert L.dispu_fps_cells_scratch_bytes(2, _hp(bad_off), _hp(bad_moff), 0) == 0
        assert L.dispu_fps_segments_auto_scratch_bytes(2, _hp(bad_off), _hp(bad_moff)) == 0
    for cell in (1, 63, 96, 8192, -64):
        assert L.dispu_fps_cells_scratch_bytes(2, _hp(off), _hp(moff), cell) == 0
    # a segment above 2^24 points is refused; 12 * 2^20, the largest merged cloud the upsampling tool produces, is served
    big, mbig = _offs([(1 << 24) + 1], [8])
    assert L.dispu_fps_cells_scratch_bytes(1, _hp(big), _hp(mbig), 0) == 0
    ok, mok = _offs([12 << 20], [4 << 20])
    assert L.dispu_fps_cells_scratch_bytes(1, _hp(ok), _hp(mok), 0) > 0
    assert L.dispu_fps_segments_auto_scratch_bytes(1, _hp(ok), _hp(mok)) > 0


def test_scratch_bytes_grows_with_n():
    from dispu_amd import _lib
    L = _lib.lib()
    last = 0
    for n in (1, 2, 63, 64, 65, 1000, 2048, 2049, 24576, 24577, 65536, 262144, 262145, 1 << 20, 12 << 20, 1 << 24):
        off, moff = _offs([n], [7])
        for cell in (0, 64, 4096):
            need = L.dispu_fps_cells_scratch_bytes(1, _hp(off), _hp(moff), cell)
            assert need >= last and need >= 24 * n, (n, cell)
        last = L.dispu_fps_cells_scratch_bytes(1, _hp(off), _hp(moff), 0)
    # the auto entry asks for what dispu_fps_segments asks where no segment goes to the cell kernels
    off, moff = _offs([300, 5000, 24576, 30000], [10, 100, 64, 3])
    assert not L.dispu_fps_cells_wanted(30000, 3)
    assert L.dispu_fps_segments_auto_scratch_bytes(4, _hp(off), _hp(moff)) >= L.dispu_fps_segments_scratch_bytes(4, _hp(off), _hp(moff)) > 0
    off, moff = _offs([300, 64], [10, 64])
    assert L.dispu_fps_segments_auto_scratch_bytes(2, _hp(off), _hp(moff)) == 0


def test_cells_wanted_never_below_the_register_kernels():
    from dispu_amd import _lib
    L = _lib.lib()
    for n in (1, 64, 4096, 4097, 24575, 24576):
        for m in (1, 64, 1000, 8192, 1 << 20):
            assert L.dispu_fps_cells_wanted(n, m) == 0
    assert L.dispu_fps_cells_wanted(1228800, 409600) == 1          # the final stage of a 100 k-point scan
    assert L.dispu_fps_cells_wanted(30000, 1) == 0                 # one round never repays the pre-pass


def test_path_argument_is_checked():
    import torch
    from dispu_amd import upsample as U
    from dispu_amd.tf_sampling import FPS_PATHS, farthest_point_sample, fps_ragged
    assert FPS_PATHS == ("auto", "cells", "stream")
    x = torch.zeros((1, 8, 3))
    for bad in ("dense", "", None, "Cells", 0):
        with pytest.raises(ValueError, match="path must be one of"):
            farthest_point_sample(4, x, path=bad)
        with pytest.raises(ValueError, match="path must be one of"):
            fps_ragged(x[0], [0, 8], [0, 4], path=bad)
        with pytest.raises(ValueError, match="path must be one of"):
            U.fps_segments(x[0], [0, 8], [0, 4], path=bad)
    with pytest.raises(ValueError, match="ROCm device"):           # a legal path gets as far as the device check
        farthest_point_sample(4, x, path="cells")
