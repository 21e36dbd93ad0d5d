"""CPU bookkeeping for the GPU cases that run the whole-cloud ops past their "second trips": a loop body that runs a second time, a
scan tier that starts splitting work, a launch that stops returning at once, a sorting pass that only exists with more key bits.

The constants those cases rest on are restated here and read back from the sources with a regular expression, so a later change of a
constant fails this file instead of silently moving a case below its threshold.  From them the file computes, for every such case of
the GPU tests, the quantity that matters (tile sums and sums per thread, workgroups, passes, segment bits, cells, cell size) and asserts
that the case crosses its threshold.  It also confirms, against the greedy oracle at about 5000 points, the construction rule that the
524289-point Poisson-disk case relies on."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

CONSTANTS = {                        # name: (file, the value the cases were built for)
    "DISPU_RADIX_TILE": ("include/dispu_hip.h", 2048),
    "kRsThreads": ("dis-pu_amd/csrc/internal.h", 256),
    "kBoundsMaxBlocks": ("dis-pu_amd/csrc/grid_subsample.hip", 1024),
    "kOrJumpIters": ("dis-pu_amd/csrc/orient_consistent.hip", 64),
    "kOrJumpLaunches": ("dis-pu_amd/csrc/orient_consistent.hip", 4),
    "kFpcMaxCells": ("dis-pu_amd/csrc/morton_cells.h", 4096),
    "kFpcMinCell": ("dis-pu_amd/csrc/morton_cells.h", 64),
    "kFpcMortonBits": ("dis-pu_amd/csrc/morton_cells.hip", 30),
}
TILE, THREADS, BOUNDS_BLOCKS = (CONSTANTS[k][1] for k in ("DISPU_RADIX_TILE", "kRsThreads", "kBoundsMaxBlocks"))
MAX_CELLS, MIN_CELL, MORTON_BITS = (CONSTANTS[k][1] for k in ("kFpcMaxCells", "kFpcMinCell", "kFpcMortonBits"))


def read_constant(name):
    path, _ = CONSTANTS[name]
    text = open(os.path.join(ROOT, path)).read()
    found = re.findall(r"(?:#define\s+%s\s+|\b%s\s*=\s*)(\d+)\b" % (name, name), text)
    assert len(found) == 1, "%s: %d definitions in %s" % (name, len(found), path)
    return int(found[0])


def test_the_constants_are_the_sources():
    for name, (_, value) in CONSTANTS.items():
        assert read_constant(name) == value, name
    import orient_oracle as OO
    assert (OO.JUMP_ITERS, OO.JUMP_LAUNCHES) == (CONSTANTS["kOrJumpIters"][1], CONSTANTS["kOrJumpLaunches"][1])
    import dispu_amd  # noqa: F401
    from dispu_amd import _lib
    assert _lib.RADIX_TILE == TILE


# ---- the quantities, as the sources compute them ----------------------------------------------------------------------------------------
def scan_sums(words):
    """(tile sums, sums per thread of scan_sums_kernel, its threads that get none) of exclusive_scan_u32 over `words` words"""
    nb = -(-words // TILE)
    per = -(-nb // THREADS)
    return nb, per, THREADS - -(-nb // per)


def sorter_table_scan(n):
    """the same for the scan inside a sorting pass: over the digit table [256][tiles]"""
    return scan_sums(256 * -(-n // TILE))


def bounds_trips(n):
    """trips of bounds_partial_kernel's stride loop for its busiest thread"""
    blocks = min(-(-n // THREADS), BOUNDS_BLOCKS)
    return -(-n // (blocks * THREADS))


def segment_passes(C):
    segbits = 0
    while (1 << segbits) < C:
        segbits += 1
    return segbits, -(-(MORTON_BITS + segbits) // 8)


def cell_size(n):
    s = MIN_CELL
    while -(-n // s) > MAX_CELLS:
        s <<= 1
    return s, -(-n // s)


# ---- every case crosses its threshold -------------------------------------------------------------------------------------------------
def test_the_scan_tier_cases():
    import test_grid_subsample_gpu as G
    import test_outliers_gpu as OUT
    import test_poisson_cells_gpu as P
    import test_radix_sort_gpu as R
    assert scan_sums(100003)[:2] == (49, 1) and scan_sums(THREADS * TILE)[:2] == (256, 1)             # where the suite stood; the last size below
    assert OUT.SCAN_TOTALS == (THREADS * TILE + 1, (2 * THREADS + 1) * TILE + 1)
    assert scan_sums(OUT.SCAN_TOTALS[0]) == (257, 2, 127) and scan_sums(OUT.SCAN_TOTALS[1]) == (514, 3, 84)   # per = 2, per = 3, idle tails
    assert R.BIG == TILE * TILE + 1 and R.TILE == TILE
    assert sorter_table_scan(R.BIG - 1)[:2] == (256, 1) and sorter_table_scan(R.BIG) == (257, 2, 127)
    sizes = [n for n, _ in G.BIG]
    assert sorted(set(sizes)) == [BOUNDS_BLOCKS * THREADS + 1, THREADS * TILE + 1] and G.STRIDE == BOUNDS_BLOCKS * THREADS
    assert bounds_trips(20000) == 1 and bounds_trips(BOUNDS_BLOCKS * THREADS) == 1 and bounds_trips(262145) == 2 and bounds_trips(524289) == 3
    assert scan_sums(524289)[1] == 2 and (524289, "one") in G.BIG and (524289, "four") in G.BIG       # run numbering, with and without keys
    assert P.BIG_LATTICE[0] ** 3 + P.BIG_LATTICE[1] == THREADS * TILE + 1


def test_the_pass_counts():
    import test_grid_subsample_gpu as G
    assert sorted(w[3] for w in G.WIDE.values()) == [2, 4, 5, 6, 7, 8]                               # beside the suite's 0, 1 and 3
    import test_fps_cells_gpu as F
    import test_normals_gpu as NRM
    import test_poisson_cells_gpu as P
    assert F.MANY == NRM.MANY and sorted(F.MANY) == [257, 65535] and P.MANY == (257, F.MANY[257])
    assert segment_passes(20) == (5, 5) and segment_passes(256) == (8, 5)                             # at most 8 segment bits so far ...
    assert segment_passes(257) == (9, 5) and segment_passes(65535) == (16, 6)                         # ... 9 bits, and the sixth pass
    assert (65534 << MORTON_BITS) > 1 << 45
    n_points = {C: int(np.array(cycle)[np.arange(C) % len(cycle)].sum()) for C, cycle in F.MANY.items()}
    assert n_points[65535] == 131070 and n_points[257] < 20000


def test_the_cell_fps_cases():
    import test_fps_cells_gpu as F
    assert cell_size(200000) == (64, 3125)                                                            # where the suite stood
    assert F.SLOT_BOUNDARY == (MAX_CELLS * MIN_CELL, MAX_CELLS * MIN_CELL + 1)
    assert cell_size(F.SLOT_BOUNDARY[0]) == (64, 4096) and cell_size(F.SLOT_BOUNDARY[1]) == (128, 2049)


def test_the_deep_chains():
    import orient_oracle as OO
    step = CONSTANTS["kOrJumpIters"][1] + 1
    sizes = [int(name.split("_")[1]) for name in OO.DEEP if name.startswith("path_")]
    assert sizes == [66, 67, 68, 4228, 274628]
    assert [OO.launches_for_depth(n - 1) for n in sizes] == [1, 2, 2, 3, 4]                           # the model itself: tests/test_orient_oracle.py
    assert step + 1 in sizes and step ** 2 < 4228 - 1 <= step ** 3 < 274628 - 1 <= step ** 4 and step ** 4 > 1 << 24
    assert "rising_4300" in OO.DEEP and OO.launches_for_depth(4300 - 2) == 3


# ---- the construction rule of the large Poisson-disk case --------------------------------------------------------------------------------
def test_lattice_with_close_pairs_follows_its_rule():
    import mesh_sample_oracle as SO
    pts, keep = SO.lattice_with_close_pairs(17, 121, seed=3)
    assert pts.shape == (17 ** 3 + 121, 3) and pts.dtype == np.float32 and int((~keep).sum()) == 121
    assert np.array_equal(SO.poisson_keep(pts, np.float32(0.4)), keep)
    d2 = SO.min_pair_d2_f32(pts[keep])
    assert d2 >= np.float32(0.48)                                                                    # the kept points: 0.7 apart at the least
    nbr, dd = SO.conflicts(pts, np.float32(0.4))
    pairs = [(i, j) for i in range(len(pts)) for j in nbr[i]]
    assert len(pairs) == 121 and len({i for i, _ in pairs} | {j for _, j in pairs}) == 242             # isolated pairs
    d = sorted(v for row in dd for v in row)
    assert d[0] == 0.0 and d[60] == 0.0 and 0.08 < d[61] and d[-1] < 0.1                             # exact duplicates, and 0.3 apart
    big, big_keep = SO.lattice_with_close_pairs(80, 12289)
    assert big.shape[0] == 524289 and int((~big_keep).sum()) == 12289
