"""The bytes every *_scratch_bytes entry of the sorted-key and cell operators returns, pinned as literals: a caller sizes its buffer with
these entries and the operators carve the same layouts, so a refactor of the layouts must not move a single total.  The entries run on
the host alone.  The sizes sit on either side of the sorter's 2048 tile, of the 256-byte alignment and of the point where the
histogram table of n pairs (256 words per tile) overtakes n itself; each entry is also asked at the largest size it accepts and with
the arguments it refuses (0).  EXPECTED was recorded from the library before its layouts were rewritten on one carver."""
import ctypes

import numpy as np
import pytest

SIZES = (1, 63, 64, 2047, 2048, 2049, 5000, 2 ** 20 + 1, 2 ** 24)
SEG_MAX = 2 ** 24            # points per segment of a packed batch
KEYS_MAX = 2 ** 31 - 1       # keys of one sort in reconstruct.hip


def offsets(C, total):
    """C uneven segments of at least one point each that sum to total (weights 1 .. 5 in a fixed pattern, the remainder to the last)"""
    w = (np.arange(C, dtype=np.int64) * 7) % 5 + 1
    sizes = 1 + (total - C) * w // int(w.sum())
    sizes[-1] += total - int(sizes.sum())
    assert sizes.min() >= 1 and sizes.max() <= SEG_MAX and int(sizes.sum()) == total
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def moffsets(off):
    """an output table for dispu_fps_cells_scratch_bytes: min(n_c, 16) samples per segment"""
    return np.concatenate([[0], np.cumsum(np.minimum(np.diff(off.astype(np.int64)), 16))]).astype(np.int32)


# (C, total) of the packed batches: one segment up to its limit of 2^24 points, 65535 segments up to the int32 limit of the offsets
BATCHES = [(1, n) for n in SIZES] + [(3, n) for n in SIZES[1:]] + [(3, 30000000)] + \
          [(65535, 65535), (65535, 2 ** 20 + 1), (65535, 2 ** 24), (65535, 2 ** 31 - 1)]
BAD_OFFSETS = {
    "first_not_0": np.array([1, 5, 9], np.int32),
    "empty_segment": np.array([0, 5, 5], np.int32),
    "segment_above_2^24": np.array([0, SEG_MAX + 1, SEG_MAX + 2], np.int32),
}


def _cases():
    """(id, entry, arguments); an ndarray argument is passed as a pointer to its int32 data"""
    out = []
    add = lambda entry, *args: out.append(("%s(%s)" % (entry[6:-14], ", ".join(
        "off[%d]=%d" % (len(a) - 1, a[-1]) if isinstance(a, np.ndarray) else str(a) for a in args)), entry, args))
    for n in SIZES + (2 ** 31 - 1, 0, -1, 2 ** 31):
        add("dispu_radix_sort_scratch_bytes", n)
        add("dispu_grid_subsample_scratch_bytes", n, 0, 0)
    for args in ((5000, 3, 2), (10, -1, 0), (10, 0, -1)):
        add("dispu_grid_subsample_scratch_bytes", *args)
    for C, n in [(1, n) for n in SIZES + (2 ** 31 - 1,)] + [(3, n) for n in SIZES[1:]] + \
            [(65535, 65535), (65535, 2 ** 20 + 1), (65535, 2 ** 24), (65535, 2 ** 31 - 1), (0, 10), (65536, 10 ** 6), (3, 2), (1, 2 ** 31)]:
        add("dispu_poisson_cells_scratch_bytes", C, n)
    for n in SIZES + (0, SEG_MAX + 1):
        add("dispu_lattice_voxels_scratch_bytes", n)
        for band in (1, 2, 3):
            add("dispu_lattice_dilate_scratch_bytes", n, band)              # 343 * 2^24 keys are refused: band 3 ends below
    for nocc, band in ((KEYS_MAX // 343, 3), (KEYS_MAX // 343 + 1, 3), (5000, 0), (5000, 4)):
        add("dispu_lattice_dilate_scratch_bytes", nocc, band)
    for nvox in SIZES + (KEYS_MAX // 8, 0, KEYS_MAX // 8 + 1):
        add("dispu_lattice_corners_scratch_bytes", nvox)
    for nvox, nlat in [(n, n) for n in SIZES] + [(KEYS_MAX // 8, SEG_MAX), (1, SEG_MAX), (KEYS_MAX // 8, 1), (2049, 293), (0, 1), (1, 0),
                                                  (KEYS_MAX // 8 + 1, 1), (1, SEG_MAX + 1)]:
        add("dispu_contour_count_scratch_bytes", nvox, nlat)
    segmented = [(C, offsets(C, n)) for C, n in BATCHES] + [(2, o) for o in BAD_OFFSETS.values()] + \
                [(0, offsets(1, 10)), (65536, offsets(1, 10))]
    for C, off in segmented:
        add("dispu_compact_scratch_bytes", C, off)
        add("dispu_radius_count_scratch_bytes", C, off)
        add("dispu_knn_mean_dist_scratch_bytes", C, off, 8)
        add("dispu_pca_normals_scratch_bytes", C, off, 8)
        add("dispu_orient_consistent_scratch_bytes", C, off, 4)             # refused from off[C] * k = 2^31
        add("dispu_fps_cells_scratch_bytes", C, off, moffsets(off) if off[0] == 0 else off, 0)
    five = offsets(3, 5000)
    for k in (0, 1, 31, 32):
        add("dispu_knn_mean_dist_scratch_bytes", 3, five, k)
    for k in (3, 32, 33):
        add("dispu_pca_normals_scratch_bytes", 3, five, k)
        add("dispu_orient_consistent_scratch_bytes", 3, five, k)
    add("dispu_orient_consistent_scratch_bytes", 65535, offsets(65535, 2 ** 29 - 1), 4)     # the largest: off[C] * k = 2^31 - 4
    add("dispu_orient_consistent_scratch_bytes", 65535, offsets(65535, 2 ** 29), 4)
    for cell in (64, 4096, 63, 96, 8192):
        add("dispu_fps_cells_scratch_bytes", 3, five, moffsets(five), cell)
    for b, n in ((1, 1), (3, 5000), (65535, 32768), (2 ** 31 - 1, 49152), (0, 5), (5, 0), (-1, 5)):
        add("dispu_poisson_disk_scratch_bytes", b, n)
    return out


CASES = _cases()

EXPECTED = {
    "radix_sort(1)": 1792,
    "grid_subsample(1, 0, 0)": 32000,
    "radix_sort(63)": 2048,
    "grid_subsample(63, 0, 0)": 32512,
    "radix_sort(64)": 2048,
    "grid_subsample(64, 0, 0)": 32768,
    "radix_sort(2047)": 25856,
    "grid_subsample(2047, 0, 0)": 103936,
    "radix_sort(2048)": 25856,
    "grid_subsample(2048, 0, 0)": 104192,
    "radix_sort(2049)": 27392,
    "grid_subsample(2049, 0, 0)": 106752,
    "radix_sort(5000)": 63744,
    "grid_subsample(5000, 0, 0)": 213760,
    "radix_sort(1048577)": 13111040,
    "grid_subsample(1048577, 0, 0)": 38307072,
    "radix_sort(16777216)": 209747968,
    "grid_subsample(16777216, 0, 0)": 612430336,
    "radix_sort(2147483647)": 26847739904,
    "grid_subsample(2147483647, 0, 0)": 78387376384,
    "radix_sort(0)": 0,
    "grid_subsample(0, 0, 0)": 0,
    "radix_sort(-1)": 0,
    "grid_subsample(-1, 0, 0)": 0,
    "radix_sort(2147483648)": 0,
    "grid_subsample(2147483648, 0, 0)": 0,
    "grid_subsample(5000, 3, 2)": 213760,
    "grid_subsample(10, -1, 0)": 0,
    "grid_subsample(10, 0, -1)": 0,
    "poisson_cells(1, 1)": 7680,
    "poisson_cells(1, 63)": 14080,
    "poisson_cells(1, 64)": 14336,
    "poisson_cells(1, 2047)": 295424,
    "poisson_cells(1, 2048)": 295680,
    "poisson_cells(1, 2049)": 299520,
    "poisson_cells(1, 5000)": 718848,
    "poisson_cells(1, 1048577)": 149431808,
    "poisson_cells(1, 16777216)": 2390789632,
    "poisson_cells(1, 2147483647)": 306020617472,
    "poisson_cells(3, 63)": 14080,
    "poisson_cells(3, 64)": 14336,
    "poisson_cells(3, 2047)": 295424,
    "poisson_cells(3, 2048)": 295680,
    "poisson_cells(3, 2049)": 299520,
    "poisson_cells(3, 5000)": 718848,
    "poisson_cells(3, 1048577)": 149431808,
    "poisson_cells(3, 16777216)": 2390789632,
    "poisson_cells(65535, 65535)": 13797888,
    "poisson_cells(65535, 1048577)": 153887232,
    "poisson_cells(65535, 16777216)": 2395245056,
    "poisson_cells(65535, 2147483647)": 306025072896,
    "poisson_cells(0, 10)": 0,
    "poisson_cells(65536, 1000000)": 0,
    "poisson_cells(3, 2)": 0,
    "poisson_cells(1, 2147483648)": 0,
    "lattice_voxels(1)": 2816,
    "lattice_dilate(1, 1)": 2816,
    "lattice_dilate(1, 2)": 5120,
    "lattice_dilate(1, 3)": 11776,
    "lattice_voxels(63)": 3328,
    "lattice_dilate(63, 1)": 49920,
    "lattice_dilate(63, 2)": 226304,
    "lattice_dilate(63, 3)": 617472,
    "lattice_voxels(64)": 3328,
    "lattice_dilate(64, 1)": 49920,
    "lattice_dilate(64, 2)": 228608,
    "lattice_dilate(64, 3)": 626432,
    "lattice_voxels(2047)": 58880,
    "lattice_dilate(2047, 1)": 1576448,
    "lattice_dilate(2047, 2)": 7294464,
    "lattice_dilate(2047, 3)": 20013056,
    "lattice_voxels(2048)": 58880,
    "lattice_dilate(2048, 1)": 1576448,
    "lattice_dilate(2048, 2)": 7296768,
    "lattice_dilate(2048, 3)": 20022016,
    "lattice_voxels(2049)": 61184,
    "lattice_dilate(2049, 1)": 1578752,
    "lattice_dilate(2049, 2)": 7301376,
    "lattice_dilate(2049, 3)": 20033280,
    "lattice_voxels(5000)": 144640,
    "lattice_dilate(5000, 1)": 3848960,
    "lattice_dilate(5000, 2)": 17815552,
    "lattice_dilate(5000, 3)": 48882176,
    "lattice_voxels(1048577)": 29889280,
    "lattice_dilate(1048577, 1)": 806937344,
    "lattice_dilate(1048577, 2)": 3735813120,
    "lattice_dilate(1048577, 3)": 10251068928,
    "lattice_voxels(16777216)": 478183680,
    "lattice_dilate(16777216, 1)": 12910952704,
    "lattice_dilate(16777216, 2)": 59772928256,
    "lattice_dilate(16777216, 3)": 0,
    "lattice_voxels(0)": 0,
    "lattice_dilate(0, 1)": 0,
    "lattice_dilate(0, 2)": 0,
    "lattice_dilate(0, 3)": 0,
    "lattice_voxels(16777217)": 0,
    "lattice_dilate(16777217, 1)": 0,
    "lattice_dilate(16777217, 2)": 0,
    "lattice_dilate(16777217, 3)": 0,
    "lattice_dilate(6260885, 3)": 61207476736,
    "lattice_dilate(6260886, 3)": 0,
    "lattice_dilate(5000, 0)": 0,
    "lattice_dilate(5000, 4)": 0,
    "lattice_corners(1)": 2816,
    "lattice_corners(63)": 15872,
    "lattice_corners(64)": 15872,
    "lattice_corners(2047)": 467456,
    "lattice_corners(2048)": 467456,
    "lattice_corners(2049)": 469760,
    "lattice_corners(5000)": 1140992,
    "lattice_corners(1048577)": 239094528,
    "lattice_corners(16777216)": 3825467648,
    "lattice_corners(268435455)": 61207478528,
    "lattice_corners(0)": 0,
    "lattice_corners(268435456)": 0,
    "contour_count(1, 1)": 512,
    "contour_count(63, 63)": 512,
    "contour_count(64, 64)": 512,
    "contour_count(2047, 2047)": 512,
    "contour_count(2048, 2048)": 512,
    "contour_count(2049, 2049)": 512,
    "contour_count(5000, 5000)": 512,
    "contour_count(1048577, 1048577)": 14848,
    "contour_count(16777216, 16777216)": 229632,
    "contour_count(268435455, 16777216)": 524544,
    "contour_count(1, 16777216)": 229632,
    "contour_count(268435455, 1)": 524544,
    "contour_count(2049, 293)": 512,
    "contour_count(0, 1)": 0,
    "contour_count(1, 0)": 0,
    "contour_count(268435456, 1)": 0,
    "contour_count(1, 16777217)": 0,
    "compact(1, off[1]=1)": 512,
    "radius_count(1, off[1]=1)": 3328,
    "knn_mean_dist(1, off[1]=1, 8)": 3328,
    "pca_normals(1, off[1]=1, 8)": 3328,
    "orient_consistent(1, off[1]=1, 4)": 3072,
    "fps_cells(1, off[1]=1, off[1]=1, 0)": 3328,
    "compact(1, off[1]=63)": 512,
    "radius_count(1, off[1]=63)": 4096,
    "knn_mean_dist(1, off[1]=63, 8)": 4096,
    "pca_normals(1, off[1]=63, 8)": 4096,
    "orient_consistent(1, off[1]=63, 4)": 4096,
    "fps_cells(1, off[1]=63, off[1]=16, 0)": 4096,
    "compact(1, off[1]=64)": 512,
    "radius_count(1, off[1]=64)": 4096,
    "knn_mean_dist(1, off[1]=64, 8)": 4096,
    "pca_normals(1, off[1]=64, 8)": 4096,
    "orient_consistent(1, off[1]=64, 4)": 4096,
    "fps_cells(1, off[1]=64, off[1]=16, 0)": 4096,
    "compact(1, off[1]=2047)": 8448,
    "radius_count(1, off[1]=2047)": 76288,
    "knn_mean_dist(1, off[1]=2047, 8)": 76288,
    "pca_normals(1, off[1]=2047, 8)": 76288,
    "orient_consistent(1, off[1]=2047, 4)": 109056,
    "fps_cells(1, off[1]=2047, off[1]=16, 0)": 76288,
    "compact(1, off[1]=2048)": 8448,
    "radius_count(1, off[1]=2048)": 76544,
    "knn_mean_dist(1, off[1]=2048, 8)": 76544,
    "pca_normals(1, off[1]=2048, 8)": 76544,
    "orient_consistent(1, off[1]=2048, 4)": 109056,
    "fps_cells(1, off[1]=2048, off[1]=16, 0)": 76544,
    "compact(1, off[1]=2049)": 8704,
    "radius_count(1, off[1]=2049)": 79104,
    "knn_mean_dist(1, off[1]=2049, 8)": 79104,
    "pca_normals(1, off[1]=2049, 8)": 79104,
    "orient_consistent(1, off[1]=2049, 4)": 111616,
    "fps_cells(1, off[1]=2049, off[1]=16, 0)": 79104,
    "compact(1, off[1]=5000)": 20480,
    "radius_count(1, off[1]=5000)": 187392,
    "knn_mean_dist(1, off[1]=5000, 8)": 187392,
    "pca_normals(1, off[1]=5000, 8)": 187392,
    "orient_consistent(1, off[1]=5000, 4)": 267520,
    "fps_cells(1, off[1]=5000, off[1]=16, 0)": 187392,
    "compact(1, off[1]=1048577)": 4196864,
    "radius_count(1, off[1]=1048577)": 38802688,
    "knn_mean_dist(1, off[1]=1048577, 8)": 38802688,
    "pca_normals(1, off[1]=1048577, 8)": 38802688,
    "orient_consistent(1, off[1]=1048577, 4)": 55577600,
    "fps_cells(1, off[1]=1048577, off[1]=16, 0)": 38802688,
    "compact(1, off[1]=16777216)": 67141632,
    "radius_count(1, off[1]=16777216)": 620790272,
    "knn_mean_dist(1, off[1]=16777216, 8)": 620790272,
    "pca_normals(1, off[1]=16777216, 8)": 620790272,
    "orient_consistent(1, off[1]=16777216, 4)": 889192960,
    "fps_cells(1, off[1]=16777216, off[1]=16, 0)": 620790272,
    "compact(3, off[3]=63)": 512,
    "radius_count(3, off[3]=63)": 4096,
    "knn_mean_dist(3, off[3]=63, 8)": 4096,
    "pca_normals(3, off[3]=63, 8)": 4096,
    "orient_consistent(3, off[3]=63, 4)": 4096,
    "fps_cells(3, off[3]=63, off[3]=39, 0)": 4096,
    "compact(3, off[3]=64)": 512,
    "radius_count(3, off[3]=64)": 4096,
    "knn_mean_dist(3, off[3]=64, 8)": 4096,
    "pca_normals(3, off[3]=64, 8)": 4096,
    "orient_consistent(3, off[3]=64, 4)": 4096,
    "fps_cells(3, off[3]=64, off[3]=39, 0)": 4096,
    "compact(3, off[3]=2047)": 8448,
    "radius_count(3, off[3]=2047)": 76544,
    "knn_mean_dist(3, off[3]=2047, 8)": 76544,
    "pca_normals(3, off[3]=2047, 8)": 76544,
    "orient_consistent(3, off[3]=2047, 4)": 109056,
    "fps_cells(3, off[3]=2047, off[3]=48, 0)": 76544,
    "compact(3, off[3]=2048)": 8448,
    "radius_count(3, off[3]=2048)": 76544,
    "knn_mean_dist(3, off[3]=2048, 8)": 76544,
    "pca_normals(3, off[3]=2048, 8)": 76544,
    "orient_consistent(3, off[3]=2048, 4)": 109056,
    "fps_cells(3, off[3]=2048, off[3]=48, 0)": 76544,
    "compact(3, off[3]=2049)": 8704,
    "radius_count(3, off[3]=2049)": 79104,
    "knn_mean_dist(3, off[3]=2049, 8)": 79104,
    "pca_normals(3, off[3]=2049, 8)": 79104,
    "orient_consistent(3, off[3]=2049, 4)": 111616,
    "fps_cells(3, off[3]=2049, off[3]=48, 0)": 79104,
    "compact(3, off[3]=5000)": 20480,
    "radius_count(3, off[3]=5000)": 187648,
    "knn_mean_dist(3, off[3]=5000, 8)": 187648,
    "pca_normals(3, off[3]=5000, 8)": 187648,
    "orient_consistent(3, off[3]=5000, 4)": 267520,
    "fps_cells(3, off[3]=5000, off[3]=48, 0)": 187648,
    "compact(3, off[3]=1048577)": 4196864,
    "radius_count(3, off[3]=1048577)": 38802688,
    "knn_mean_dist(3, off[3]=1048577, 8)": 38802688,
    "pca_normals(3, off[3]=1048577, 8)": 38802688,
    "orient_consistent(3, off[3]=1048577, 4)": 55577600,
    "fps_cells(3, off[3]=1048577, off[3]=48, 0)": 38802688,
    "compact(3, off[3]=16777216)": 67141632,
    "radius_count(3, off[3]=16777216)": 620790272,
    "knn_mean_dist(3, off[3]=16777216, 8)": 620790272,
    "pca_normals(3, off[3]=16777216, 8)": 620790272,
    "orient_consistent(3, off[3]=16777216, 4)": 889192960,
    "fps_cells(3, off[3]=16777216, off[3]=48, 0)": 620790272,
    "compact(3, off[3]=30000000)": 120058624,
    "radius_count(3, off[3]=30000000)": 1110059776,
    "knn_mean_dist(3, off[3]=30000000, 8)": 1110059776,
    "pca_normals(3, off[3]=30000000, 8)": 1110059776,
    "orient_consistent(3, off[3]=30000000, 4)": 1590000640,
    "fps_cells(3, off[3]=30000000, off[3]=48, 0)": 1110059776,
    "compact(65535, off[65535]=65535)": 262400,
    "radius_count(65535, off[65535]=65535)": 6619392,
    "knn_mean_dist(65535, off[65535]=65535, 8)": 6619392,
    "pca_normals(65535, off[65535]=65535, 8)": 6619392,
    "orient_consistent(65535, off[65535]=65535, 4)": 3736064,
    "fps_cells(65535, off[65535]=65535, off[65535]=65535, 0)": 6619392,
    "compact(65535, off[65535]=1048577)": 4196864,
    "radius_count(65535, off[65535]=1048577)": 42996480,
    "knn_mean_dist(65535, off[65535]=1048577, 8)": 42996480,
    "pca_normals(65535, off[65535]=1048577, 8)": 42996480,
    "orient_consistent(65535, off[65535]=1048577, 4)": 55839744,
    "fps_cells(65535, off[65535]=1048577, off[65535]=851955, 0)": 42996480,
    "compact(65535, off[65535]=16777216)": 67141632,
    "radius_count(65535, off[65535]=16777216)": 624984064,
    "knn_mean_dist(65535, off[65535]=16777216, 8)": 624984064,
    "pca_normals(65535, off[65535]=16777216, 8)": 624984064,
    "orient_consistent(65535, off[65535]=16777216, 4)": 889455104,
    "fps_cells(65535, off[65535]=16777216, off[65535]=1048560, 0)": 624984064,
    "compact(65535, off[65535]=2147483647)": 8594128896,
    "radius_count(65535, off[65535]=2147483647)": 79465283584,
    "knn_mean_dist(65535, off[65535]=2147483647, 8)": 79465283584,
    "pca_normals(65535, off[65535]=2147483647, 8)": 79465283584,
    "orient_consistent(65535, off[65535]=2147483647, 4)": 0,
    "fps_cells(65535, off[65535]=2147483647, off[65535]=1048560, 0)": 79465283584,
    "compact(2, off[2]=9)": 0,
    "radius_count(2, off[2]=9)": 0,
    "knn_mean_dist(2, off[2]=9, 8)": 0,
    "pca_normals(2, off[2]=9, 8)": 0,
    "orient_consistent(2, off[2]=9, 4)": 0,
    "fps_cells(2, off[2]=9, off[2]=9, 0)": 0,
    "compact(2, off[2]=5)": 0,
    "radius_count(2, off[2]=5)": 0,
    "knn_mean_dist(2, off[2]=5, 8)": 0,
    "pca_normals(2, off[2]=5, 8)": 0,
    "orient_consistent(2, off[2]=5, 4)": 0,
    "fps_cells(2, off[2]=5, off[2]=5, 0)": 0,
    "compact(2, off[2]=16777218)": 0,
    "radius_count(2, off[2]=16777218)": 0,
    "knn_mean_dist(2, off[2]=16777218, 8)": 0,
    "pca_normals(2, off[2]=16777218, 8)": 0,
    "orient_consistent(2, off[2]=16777218, 4)": 0,
    "fps_cells(2, off[2]=16777218, off[2]=17, 0)": 0,
    "compact(0, off[1]=10)": 0,
    "radius_count(0, off[1]=10)": 0,
    "knn_mean_dist(0, off[1]=10, 8)": 0,
    "pca_normals(0, off[1]=10, 8)": 0,
    "orient_consistent(0, off[1]=10, 4)": 0,
    "fps_cells(0, off[1]=10, off[1]=10, 0)": 0,
    "compact(65536, off[1]=10)": 0,
    "radius_count(65536, off[1]=10)": 0,
    "knn_mean_dist(65536, off[1]=10, 8)": 0,
    "pca_normals(65536, off[1]=10, 8)": 0,
    "orient_consistent(65536, off[1]=10, 4)": 0,
    "fps_cells(65536, off[1]=10, off[1]=10, 0)": 0,
    "knn_mean_dist(3, off[3]=5000, 0)": 0,
    "knn_mean_dist(3, off[3]=5000, 1)": 187648,
    "knn_mean_dist(3, off[3]=5000, 31)": 187648,
    "knn_mean_dist(3, off[3]=5000, 32)": 0,
    "pca_normals(3, off[3]=5000, 3)": 0,
    "orient_consistent(3, off[3]=5000, 3)": 0,
    "pca_normals(3, off[3]=5000, 32)": 187648,
    "orient_consistent(3, off[3]=5000, 32)": 267520,
    "pca_normals(3, off[3]=5000, 33)": 0,
    "orient_consistent(3, off[3]=5000, 33)": 0,
    "orient_consistent(65535, off[65535]=536870911, 4)": 28454420992,
    "orient_consistent(65535, off[65535]=536870912, 4)": 0,
    "fps_cells(3, off[3]=5000, off[3]=48, 64)": 187648,
    "fps_cells(3, off[3]=5000, off[3]=48, 4096)": 187648,
    "fps_cells(3, off[3]=5000, off[3]=48, 63)": 0,
    "fps_cells(3, off[3]=5000, off[3]=48, 96)": 0,
    "fps_cells(3, off[3]=5000, off[3]=48, 8192)": 0,
    "poisson_disk(1, 1)": 16,
    "poisson_disk(3, 5000)": 240000,
    "poisson_disk(65535, 32768)": 34359214080,
    "poisson_disk(2147483647, 49152)": 1688849859477504,
    "poisson_disk(0, 5)": 0,
    "poisson_disk(5, 0)": 0,
    "poisson_disk(-1, 5)": 0,
}


def call(L, entry, args):
    keep = [np.ascontiguousarray(a) for a in args if isinstance(a, np.ndarray)]                 # alive during the call
    it = iter(keep)
    return getattr(L, entry)(*[ctypes.c_void_p(next(it).ctypes.data) if isinstance(a, np.ndarray) else a for a in args])


def test_the_table_names_every_case_once():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)
    assert len({c[1] for c in CASES}) == 14


@pytest.mark.parametrize("entry", sorted({c[1] for c in CASES}))
def test_scratch_bytes_are_the_recorded_ones(entry):
    from dispu_amd import _lib
    L = _lib.lib()
    got = {cid: call(L, e, args) for cid, e, args in CASES if e == entry}
    want = {cid: EXPECTED[cid] for cid in got}
    assert got == want
    assert any(v == 0 for v in got.values()) and all(v % 256 == 0 for v in got.values() if entry != "dispu_poisson_disk_scratch_bytes")
