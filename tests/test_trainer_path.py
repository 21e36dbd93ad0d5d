"""Trainer.path(B, N): which launches a training step takes, from the switches and the shape alone.  No device and no library: a
Trainer without parameters allocates nothing.  Every expected value below is written out by hand from the rules (M = 4N points per
upsampled patch, rm = B * M rows):
  stem         N <= 256 and N even
  after_split  0 unless rm <= 16384 and rm % 128 == 0 and after_conv's product stays fp32; then 4 if rm >= 8192 else 8.  The product
               [rm x 2048] x [2048 x 256] goes to bf16 in bf16 mode from bf16_min_macs = 1.5e9 multiply-adds on: rm >= 2862
  defer_side   rm <= 16384
  attention    "flash" / "gemm" by flash_attn
  local_bwd    "fused" needs fused_local_bwd and dtype f32 (fp32 pair tensors), else "pair"
  split_skip   overlap_dw
Refused (ValueError): N <= 16, rm % 64 != 0, M > 4096, M % 32 != 0 -- checked in that order."""
import re

import pytest

from dispu_amd.train import Path, Trainer

BASE = dict(defer_side=True, attention="flash", local_bwd="pair", split_skip=True)
SHAPES = {
    (2, 24): Path(stem=True, after_split=0, **BASE),                       # rm = 192 = 128 + 64
    (2, 40): Path(stem=True, after_split=0, **BASE),                       # rm = 320 = 2 * 128 + 64
    (4, 64): Path(stem=True, after_split=8, **BASE),                       # rm = 1024
    (1, 128): Path(stem=True, after_split=8, **BASE),                      # rm = 512
    (1, 512): Path(stem=False, after_split=8, **BASE),                     # N > 256, rm = 2048
    (1, 1024): Path(stem=False, after_split=8, **BASE),                    # rm = M = 4096, the accepted maximum
    (68, 64): Path(stem=True, after_split=0, **dict(BASE, defer_side=False)),      # rm = 17408 = 136 * 128 > 16384
    (8, 256): Path(stem=True, after_split=4, **BASE),                      # rm = 8192: the first size with 4 chunks
    (16, 256): Path(stem=True, after_split=4, **BASE),                     # rm = 16384: the last size split and deferred
    (32, 256): Path(stem=True, after_split=0, **dict(BASE, defer_side=False)),     # rm = 32768
    (17, 256): Path(stem=True, after_split=0, **dict(BASE, defer_side=False)),     # rm = 17408
}
# even, no multiple of 64 (rm = 2000 = 31 * 64 + 16); odd N (rm = 2040 = 31 * 64 + 56; 4N % 32 == 0 needs N % 8 == 0, so no odd N passes)
REFUSED = {(2, 250): "64-row tiles", (2, 255): "64-row tiles"}
BF16_PRODUCT = [(1, 1024), (8, 256), (16, 256)]       # split in f32 and rm >= 2862: after_conv runs bf16 products, unsplit
ALL = sorted(SHAPES)

# (dtype, attribute set alone, value) -> {shape: the fields that differ from SHAPES[shape]}
CASES = [
    ("f32", None, None, {}),
    ("f32", "flash_attn", False, {s: dict(attention="gemm") for s in ALL}),
    ("f32", "fused_local_bwd", True, {s: dict(local_bwd="fused") for s in ALL}),
    ("f32", "overlap_dw", False, {s: dict(split_skip=False) for s in ALL}),
    ("f32", "bf16_min_macs", 0.0, {}),                                                  # fp32 products whatever the threshold
    ("bf16", None, None, {s: dict(after_split=0) for s in BF16_PRODUCT}),
    ("bf16", "flash_attn", False, {s: dict(attention="gemm", **({"after_split": 0} if s in BF16_PRODUCT else {})) for s in ALL}),
    ("bf16", "fused_local_bwd", True, {s: dict(after_split=0) for s in BF16_PRODUCT}),  # bf16 pair tensors: the fused backward is not taken
    ("bf16", "overlap_dw", False, {s: dict(split_skip=False, **({"after_split": 0} if s in BF16_PRODUCT else {})) for s in ALL}),
    ("bf16", "bf16_min_macs", 1e12, {}),                                                # every product under the threshold: as f32
    # 1024 * 2048 * 256 = 5.4e8 multiply-adds: (4, 64) and everything above it unsplit; (1, 128) stays fp32 and split
    ("bf16", "bf16_min_macs", 5e8, {s: dict(after_split=0) for s in BF16_PRODUCT + [(4, 64), (1, 512)]}),
]


@pytest.mark.parametrize("dtype,attr,value,expect", CASES, ids=["%s-%s=%s" % c[:3] for c in CASES])
def test_path_table(dtype, attr, value, expect):
    tr = Trainer(params=None, dtype=dtype)
    assert tr.P is None and not tr._ws
    if attr is not None:
        assert getattr(tr, attr) != value                   # the default is the other side
        setattr(tr, attr, value)
    for (B, N), want in SHAPES.items():
        want = want._replace(**expect.get((B, N), {}))
        got = tr.path(B, N)
        assert got == want, (B, N)
        assert all(type(a) is type(b) for a, b in zip(got, want)), (B, N, got)
    for (B, N), text in REFUSED.items():
        with pytest.raises(ValueError, match=text):
            tr.path(B, N)
    assert not tr._ws                                       # deciding allocates nothing


def test_path_follows_the_switches_between_calls():
    tr = Trainer(params=None)
    assert tr.path(8, 256).attention == "flash"
    tr.flash_attn = False
    assert tr.path(8, 256).attention == "gemm"
    tr.flash_attn = True
    assert tr.path(8, 256) == SHAPES[(8, 256)]


# the smallest shape that breaks each rule and none of the rules checked before it
REFUSALS = [
    ((1, 16), "a patch needs more than 16 points (k-NN graph of the dense blocks), got N = 16"),
    ((1, 24), "the fused head chains work on 64-row tiles: B * 4 * N must be a multiple of 64, got B = 1, N = 24 (pad the batch)"),      # rm = 96
    ((2, 1032), "the local cell's backward inverts a cloud's k-NN graph in LDS: 4 * N <= 4096, got N = 1032"),                           # M = 4128, rm = 129 * 64
    ((4, 20), "the non-local cell's attention kernels work on 32-point tiles: 4 * N must be a multiple of 32, got N = 20"),              # M = 80, rm = 320
]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape,text", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_shape_refusals(dtype, shape, text):
    tr = Trainer(params=None, dtype=dtype)
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        tr.path(*shape)
