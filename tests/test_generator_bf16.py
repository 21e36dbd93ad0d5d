"""CPU side of Generator(dtype="bf16"): the argument check that fires before any device is touched, the C ABI declaration, and the
record that the GPU test's tolerance is derived from (tests/generator_bf16_oracle.py)."""
import os
import re

import pytest

import generator_bf16_oracle as BO
from oracle import generator as OG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bad_dtype_raises_without_a_device():
    from dispu_amd.generator import Generator
    for bad in ("fp16", "float32", None, 16):
        with pytest.raises(ValueError, match="dtype"):
            Generator(dtype=bad)
    with pytest.raises(ValueError, match=r"Trainer\(dtype"):
        Generator(dtype="bf16", is_training=True)
    assert Generator(dtype="bf16", device="cpu").dtype == "bf16" and Generator(device="cpu").dtype == "f32"


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "dispu_hip.h")).read()
    m = re.search(r"int dispu_ps_local_bf16\(([^;]*)\);", text)
    assert m and "void* out" in m.group(1) and m.group(1).count(",") == 16


def test_recorded_reference_spread_holds(monkeypatch):
    """the two evaluations of the wrapped oracle (F' by the fmaf chain / in float64) on the smallest case: the recorded spread over the
    GPU test's cases bounds it, and the tolerance follows from the record"""
    from dispu_amd import synth
    P = OG.init_params(seed=1234, bias_scale=0.05, bn_random=True)
    s = BO.spread(monkeypatch, P, synth.patches(1, 256, seed=5))
    print("reference spread at (1, 256): %.3e (recorded over the GPU cases: %.3e)" % (s, BO.REF_SPREAD))
    assert 0.0 < s <= BO.REF_SPREAD
    assert BO.FINE_TOL == max(1e-5, 4 * BO.REF_SPREAD)
