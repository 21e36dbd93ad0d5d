"""CPU checks of tests/scratch_contract.py: the guarded scratch buffer itself, the sizes of the registered cases against the literals of
tests/test_scratch_sizes.py, the written-out map from the library's size queries to the entries they size, and that every one of
those queries and entries (and the three `temp` takers without a query) belongs to a registered case -- there is no exemption list."""
import numpy as np
import pytest

import scratch_contract as SC


def test_guards_are_detected_on_either_side():
    import torch
    s = SC.Scratch(torch.device("cpu"), 1000, "zeros")
    assert s.nbytes == 1000 and s.floats == 250 and s.buf.numel() == 2 * SC.GUARD + 1000
    assert SC.GUARD % 256 == 0 and s.offset == SC.GUARD and s.ptr().value == s.buf.data_ptr() + SC.GUARD
    assert s.guards_intact() and not s.body().any() and s.body().shape == (1000,)
    s.refill("ones")
    assert (s.body() == 0xFF).all() and s.guards_intact()
    for at in (0, SC.GUARD - 1, SC.GUARD + 1000, 2 * SC.GUARD + 999):      # the first and last byte of both guards
        old = int(s.buf[at])
        s.buf[at] = old ^ 1
        assert not s.guards_intact(), at
        s.buf[at] = old
        assert s.guards_intact()
    s.buf[SC.GUARD] = 3                                                  # the body's first and last byte are not guards
    s.buf[SC.GUARD + 999] = 3
    assert s.guards_intact() and s.body()[0] == 3 and s.body()[-1] == 3
    s.refill("zeros")
    assert not s.body().any()


def test_fills_run_in_the_stated_order():
    assert SC.ORDER == ("zeros", "stale", "ones") and SC.FILLS == {"zeros": 0x00, "ones": 0xFF} and SC.GUARD_BYTE == 0x5A


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case_is_well_formed(name):
    from dispu_amd import _lib
    case = SC.CASES[name]
    assert case.sizes() > 0 and case.sizes() == case.sizes()
    assert case.entries and (case.queries or set(case.entries) <= set(SC.TEMP_TAKERS))
    for sym in case.entries + case.queries:
        assert sym in _lib.SIGNATURES, sym
    for q in case.queries:
        assert set(case.entries) <= set(SC.QUERY_ENTRIES[q]), (q, case.entries)
    a, b = case.inputs("a"), case.inputs("b")
    assert sorted(a) == sorted(b)
    for k in a:                                                          # identical sizes, other content
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert any(a[k].tobytes() != b[k].tobytes() for k in a)
    assert case.__doc__                                                  # says what the header promises on run-to-run bytes


def test_sizes_equal_the_pinned_literals():
    import test_scratch_sizes as TS
    seen = 0
    for name, case in SC.CASES.items():
        pinned = getattr(case, "pinned", None)
        if pinned is not None:
            assert case.sizes() == TS.EXPECTED[pinned], (name, pinned)
            seen += 1
    assert seen >= 2


def test_the_map_of_size_queries_is_the_librarys():
    """every *_scratch_bytes / *_scratch_floats symbol is in the written-out map, with entries that exist"""
    from dispu_amd import _lib
    queries = {s for s in _lib.SIGNATURES if s.endswith("_scratch_bytes") or s.endswith("_scratch_floats")}
    assert queries == set(SC.QUERY_ENTRIES)
    for q, entries in SC.QUERY_ENTRIES.items():
        assert entries and all(e in _lib.SIGNATURES for e in entries), q
    assert all(e in _lib.SIGNATURES for e in SC.TEMP_TAKERS)


def test_every_scratch_taking_entry_has_a_case():
    """no exemption list: a size query, an entry it sizes, or a `temp` taker without one, that no registered case exercises fails here;
    so a new scratch-taking entry (test_the_map_of_size_queries_is_the_librarys makes it join the map) cannot come without a case"""
    assert SC.uncovered() == []
    covered = {e for c in SC.CASES.values() for e in c.entries}
    wanted = {e for entries in SC.QUERY_ENTRIES.values() for e in entries} | set(SC.TEMP_TAKERS)
    assert sorted(wanted - covered) == []
