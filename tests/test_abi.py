"""CPU tests of the drop-in boundary: libdispu_hip.so builds for gfx950, loads without a GPU, and exports
exactly the symbols include/dispu_hip.h declares; the ctypes table in dis-pu_amd/_lib.py covers them all, with the header's types.
No compute call is made here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dispu_build", os.path.join(ROOT, "dis-pu_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.LIB) and not os.path.exists(mod.HIPCC):
        pytest.skip("no prebuilt library and no hipcc")
    return mod.build() if os.path.exists(mod.HIPCC) else mod.LIB


def header_symbols():
    text = open(os.path.join(ROOT, "include", "dispu_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dispu_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_exports(built_lib):
    syms = header_symbols()
    assert len(syms) >= 20
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = sorted(set(re.findall(r" T (dispu_[a-z0-9_]+)", out)))
    assert exported == syms, (set(exported) ^ set(syms))


def test_library_loads_and_binding_is_complete(built_lib):
    import dispu_amd
    from dispu_amd import _lib
    assert sorted(_lib.SIGNATURES) == header_symbols()
    lib = _lib.lib()
    assert lib.dispu_version() == 5
    assert lib.dispu_fps_scratch_bytes(2, 1000, 10) == 0
    assert lib.dispu_fps_scratch_bytes(2, 30000, 10) == 2 * 30000 * 4
    assert lib.dispu_approx_match_scratch_bytes(3, 10, 20) == 3 * (20 * 30 + 2 * 10 + 20) * 4 + 4 * 4   # ratio vectors + chunk partials + stage counters
    assert lib.dispu_match_cost_scratch_bytes(2, 300, 200) == 2 * 2 * 13 * 4              # 16-partner tiles at this size
    assert lib.dispu_match_cost_grad_scratch_bytes(2, 300, 200) == 2 * 13 * 300 * 3 * 4
    assert isinstance(lib.dispu_error_string(1), bytes)


_CTYPE = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
          "float": ctypes.c_float, "double": ctypes.c_double, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
          "unsigned long": ctypes.c_ulong, "unsigned long long": ctypes.c_ulonglong}


def _kind(decl, is_return):
    """ctypes kind of one C parameter (or return) declaration: any pointer is c_void_p, except a returned const char*"""
    d = " ".join(decl.split())
    if "*" in d:
        return ctypes.c_char_p if is_return and re.fullmatch(r"const char ?\*", d) else ctypes.c_void_p
    if is_return and d == "void":
        return None
    words = [w for w in d.split(" ") if w != "const"]
    for n in (len(words), len(words) - 1):           # with and without a trailing parameter name
        if " ".join(words[:n]) in _CTYPE:
            return _CTYPE[" ".join(words[:n])]
    raise AssertionError("type not understood: %r" % decl)


def header_prototypes():
    """name -> (restype, argtypes) of every prototype of the public header, comments and preprocessor lines stripped"""
    text = open(os.path.join(ROOT, "include", "dispu_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    protos = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*\}?\s*(.*?)\b(dispu_[a-z0-9_]+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m:
            assert "dispu_" not in stmt or "(" not in stmt, "prototype not understood: %r" % stmt
            continue
        ret, name, args = m.groups()
        args = " ".join(args.split())
        argtypes = [] if args in ("", "void") else [_kind(a, False) for a in args.split(",")]
        assert name not in protos, name
        protos[name] = (_kind(ret, True), argtypes)
    return protos


def test_binding_signatures_and_constants_match_header():
    """The ctypes table and the constants of _lib.py are hand-kept copies of the public header that no compiler sees: every prototype
    has the same arity, the same kind per argument and the same return type there, and every mirrored constant the header's value."""
    from dispu_amd import _lib
    protos = header_prototypes()
    assert sorted(protos) == header_symbols() and len(protos) >= 184
    bad = {}
    for name, (ret, args) in protos.items():
        have = _lib.SIGNATURES.get(name)
        if have is None or have[0] is not ret or list(have[1]) != args:
            bad[name] = (have, (ret, args))
    assert not bad, bad

    text = open(os.path.join(ROOT, "include", "dispu_hip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define DISPU_(\w+) (\d+)\s*$", text, flags=re.M)}
    mirrored = {k for k in defines if hasattr(_lib, k)}
    assert mirrored >= {"LINEAR_PLAN_INTS", "POISSON_MAX_N", "POISSON_MAX_ROUNDS", "RADIX_TILE", "MESH_TILE", "GRID_NONFINITE", "GRID_AXIS_X",
                        "GRID_AXIS_Y", "GRID_AXIS_Z", "GRID_TOO_MANY_POINTS", "ARITH_PLAIN", "ARITH_CONTRACT", "ARITH_PINNED_EXP",
                        "MESH_BRUTE_FORCE"}
    assert {k: getattr(_lib, k) for k in mirrored} == {k: defines[k] for k in mirrored}


def test_only_gfx950_code_objects(built_lib):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", "--input=" + built_lib],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    # fall back to strings when the bundler cannot parse a shared object
    text = out.stdout.decode(errors="replace")
    if "gfx" not in text:
        text = subprocess.run(["strings", built_lib], stdout=subprocess.PIPE).stdout.decode(errors="replace")
    archs = set(re.findall(r"gfx[0-9a-f]{3,4}", text))
    assert archs == {"gfx950"}, archs


def test_shims_validate_like_the_reference():
    """Shape errors carry the reference op's InvalidArgument text and fire before any device work."""
    import torch
    import dispu_amd.tf_sampling as S
    with pytest.raises(ValueError, match="must live on a ROCm device"):
        S.farthest_point_sample(4, torch.zeros(1, 8, 3))
    with pytest.raises(TypeError):
        S.farthest_point_sample(4, [[0, 0, 0]])
