"""Generator.path(B, N): which launches a forward takes, from the switches and the shape alone.  No device and no library: a
Generator without parameters allocates nothing.  Every expected value below is written out by hand from the rules (M = 4N points per
upsampled patch, rm = B * M rows):
  stem       N <= 256 and N even
  heads      fused_heads and rm % 128 == 0;      in_chain: heads and chain_inputs
  attention  "project" / "flash" need fused_attention and M % 32 == 0 ("project" also fused_project), else "gemm"
  local      "bf16" in bf16 mode, else "fused" / "pair" by fused_local
  after      bf16: "bf16_stream" if rm % 128 == 0 else "bf16s";  "x3" if split_bf16 and rm % 128 == 0;  "plain" if in_chain else "residual"
  add3       bf16 and not in_chain
  nl_late    branches and in_chain"""
import pytest

from dispu_amd.generator import Generator, Path

SHAPES = {
    # rm = 32768 = 256 * 128, M = 1024 = 32 * 32, N = 256: every rule holds
    (32, 256): Path(stem=True, heads=True, in_chain=True, attention="project", local="fused", after="plain", add3=False, nl_late=True),
    # rm = 2000 = 15 * 128 + 80, M = 1000 = 31 * 32 + 8, N = 250 even
    (2, 250): Path(stem=True, heads=False, in_chain=False, attention="gemm", local="fused", after="residual", add3=False, nl_late=False),
    # N = 288 > 256, rm = M = 1152 = 9 * 128
    (1, 288): Path(stem=False, heads=True, in_chain=True, attention="project", local="fused", after="plain", add3=False, nl_late=True),
    # N = 264 > 256, M = 1056 = 33 * 32, rm = 1056 = 8 * 128 + 32
    (1, 264): Path(stem=False, heads=False, in_chain=False, attention="project", local="fused", after="residual", add3=False, nl_late=False),
}
TILED = [(32, 256), (1, 288)]            # rm % 128 == 0
RAGGED = [(2, 250), (1, 264)]
ALL = TILED + RAGGED

# (dtype, attribute set alone, value) -> {shape: the fields that differ from SHAPES[shape]}
CASES = [
    ("f32", None, None, {s: {} for s in ALL}),
    ("f32", "fused_local", False, {s: dict(local="pair") for s in ALL}),
    ("f32", "fused_attention", False, {s: dict(attention="gemm") for s in ALL}),
    ("f32", "fused_project", False, {(32, 256): dict(attention="flash"), (1, 288): dict(attention="flash"), (1, 264): dict(attention="flash"),
                                     (2, 250): {}}),
    ("f32", "fused_heads", False, {**{s: dict(heads=False, in_chain=False, after="residual", nl_late=False) for s in TILED},
                                   **{s: {} for s in RAGGED}}),
    ("f32", "chain_inputs", False, {**{s: dict(in_chain=False, after="residual", nl_late=False) for s in TILED}, **{s: {} for s in RAGGED}}),
    ("f32", "branches", False, {**{s: dict(nl_late=False) for s in TILED}, **{s: {} for s in RAGGED}}),
    ("f32", "split_bf16", True, {**{s: dict(after="x3") for s in TILED}, **{s: {} for s in RAGGED}}),
    ("bf16", None, None, {**{s: dict(local="bf16", after="bf16_stream") for s in TILED},
                          **{s: dict(local="bf16", after="bf16s", add3=True) for s in RAGGED}}),
    ("bf16", "chain_inputs", False, {**{s: dict(local="bf16", after="bf16_stream", in_chain=False, add3=True, nl_late=False) for s in TILED},
                                     **{s: dict(local="bf16", after="bf16s", add3=True) for s in RAGGED}}),
]


@pytest.mark.parametrize("dtype,attr,value,expect", CASES, ids=["%s-%s=%s" % c[:3] for c in CASES])
def test_path_table(dtype, attr, value, expect):
    gen = Generator(dtype=dtype)
    assert not gen._ws and not gen.P
    if attr is not None:
        assert getattr(gen, attr) is (not value)          # the default is the other side
        setattr(gen, attr, value)
    assert sorted(expect) == sorted(SHAPES)
    for (B, N), diff in expect.items():
        want = SHAPES[(B, N)]._replace(**diff)
        got = gen.path(B, N)
        assert got == want, (B, N)
        assert all(type(a) is type(b) for a, b in zip(got, want)), (B, N, got)
    assert not gen._ws                                      # deciding allocates nothing


def test_path_follows_the_switches_between_calls():
    gen = Generator()
    assert gen.path(32, 256).in_chain
    gen.chain_inputs = False
    assert not gen.path(32, 256).in_chain
    gen.chain_inputs = True
    assert gen.path(32, 256) == SHAPES[(32, 256)]


@pytest.mark.parametrize("B,N", ALL)
def test_bf16_refusals(B, N):
    gen = Generator(dtype="bf16")
    gen.split_bf16 = True
    with pytest.raises(ValueError, match="split_bf16"):
        gen.path(B, N)
    gen.split_bf16 = False
    gen.fused_local = False
    with pytest.raises(ValueError, match="fused_local"):
        gen.path(B, N)
    gen.fused_local = True
    gen.path(B, N)


def test_unset_switches_are_gone():
    gen = Generator()
    for name in ("fused_stem", "fused_residual", "split_up3"):
        assert not hasattr(gen, name), name
