"""Every scratch-taking entry registered in tests/scratch_contract.py on a scratch that is zero-filled, stale (as a call of the same entry
on other inputs of the same sizes left it) and all ones, with a canary on either side: the outputs must be the oracle's on zeros and
bit-identical on the other two, nothing may be written outside scratch_bytes, the inputs keep their bits, and the shape must be one
whose path writes its scratch at all.  Only the scratch's prior content varies; every input is a legal one."""
import time

import numpy as np
import pytest

import scratch_contract as SC

pytestmark = pytest.mark.gpu


def identical(got, ref, what):
    assert sorted(got) == sorted(ref)
    for name in ref:
        a, b = got[name], ref[name]
        if isinstance(b, np.ndarray):
            assert SC.same_bytes(a, b), "%s: output %s differs from the run on a zero-filled scratch" % (what, name)
        else:
            assert a == b, (what, name, a, b)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_scratch_contract(dev, name):
    case = SC.CASES[name]
    t0 = time.time()
    nbytes = case.sizes()
    assert nbytes > 0
    changed = []

    def go(s, variant):
        before = s.body()
        out = case.run(s, variant)
        assert s.guards_intact(), "%s wrote outside its scratch_bytes" % name
        assert out["rc"] == 0
        case.check_inputs(out, variant)
        changed.append(not np.array_equal(before, s.body()))
        return out

    ref = go(SC.Scratch(dev, nbytes, "zeros"), "b")             # 1. zeros: the baseline, held to the oracle
    case.check(ref, "b", dev)
    same = identical if case.bit_identical else (lambda got, _, what: case.check(got, "b", dev))
    s = SC.Scratch(dev, nbytes, "zeros")                        # 2. stale: variant a, then b on what it left
    go(s, "a")
    same(go(s, "b"), ref, "stale")
    same(go(SC.Scratch(dev, nbytes, "ones"), "b"), ref, "ones")  # 3. every byte 0xFF
    assert any(changed), "no run of %s changed its scratch: the shape takes a path that needs none" % name
    if case.refuses:                                            # 6. one byte short: refused, nothing touched
        s = SC.Scratch(dev, nbytes, "ones")
        out = case.run(s, "b", short=True)
        assert out["rc"] == SC.INVALID
        assert s.guards_intact() and bool((s.body() == 0xFF).all()), "a refused call of %s touched its scratch" % name
        case.check_inputs(out, "b")
        assert sorted(k for k in out if k != "rc" and not k.startswith("in:")) == sorted(case.sentinels)
        for k, v in case.sentinels.items():
            assert (out[k] == v).all(), "a refused call of %s wrote %s" % (name, k)
    print("%s: %d bytes of scratch, %.2f s" % (name, nbytes, time.time() - t0))
