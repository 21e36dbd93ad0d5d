"""The device batch sampler (dispu_sample_batch, dataset.DeviceFetcher) on the GPU: exact structure against dispu_group_point /
dispu_augment fed with the kernel's own verification outputs, exact keying against the host Philox twin, and the distributions
against the reference's sampler (oracle.data.nonuniform_sampling, Common/point_operation.py:10-18) run on the host.

Statistical bounds: two-sample KS distances stay under the DKW bound sqrt(ln(2/alpha)/2) sqrt(2/n) with alpha = 1e-9 (0.1023 at
n = 2048), one-sample ones under sqrt(ln(2/alpha)/(2n)); proportions and means within six standard errors."""
import math

import numpy as np
import pytest
import torch

import sampler_oracle as SO

pytestmark = pytest.mark.gpu

ALPHA = 1e-9
SEED = 0x1234567890ABCDEF
PAD = 64                      # sentinel elements on each side of every output
F_SENT, I_SENT = 12345.0, 0x5A5A5A5A


def N(t):
    return t.detach().cpu().numpy()


class Guarded(object):
    """a device array of n elements with PAD sentinel elements on both sides"""

    def __init__(self, n, dtype, dev, off=0):
        """off: extra elements in front (PAD elements are 256 bytes; off = 1 leaves the array 4 bytes past a 16-byte boundary)"""
        self.sent = F_SENT if dtype == torch.float32 else I_SENT
        self.buf = torch.full((n + 2 * PAD + off,), self.sent, dtype=dtype, device=dev)
        self.n, self.lo = n, PAD + off

    @property
    def t(self):
        return self.buf[self.lo:self.lo + self.n]

    def intact(self):
        b = N(self.buf)
        return bool((b[:self.lo] == self.sent).all() and (b[self.lo + self.n:] == self.sent).all())


def sample(dev, gt_data, perm, start, B, P, seed=SEED, epoch=0, input_data=None, augment=True, sigma=0.01, clip=0.03, verify=True, off=0):
    """one dispu_sample_batch call with every output guarded -> dict of numpy arrays (+ 'guards', 'status'); off: see Guarded"""
    from dispu_amd import _lib
    L, G = gt_data.shape[0], gt_data.shape[1]
    f, i32 = torch.float32, torch.int32
    g = dict(input=Guarded(B * P * 3, f, dev, off), gt=Guarded(B * G * 3, f, dev, off), radius=Guarded(B, f, dev))
    if verify:
        g.update(idx=Guarded(B * P, i32, dev), rot=Guarded(B * 9, f, dev), scale=Guarded(B, f, dev), raw=Guarded(B * 4, i32, dev))
        if augment:
            g["noise"] = Guarded(B * P * 3, f, dev, off)
    status = Guarded(2, i32, dev)
    status.t.zero_()
    q = lambda k: _lib.ptr(g[k].t) if k in g else None
    rc = _lib.lib().dispu_sample_batch(L, G, P, _lib.ptr(gt_data), _lib.ptr(input_data), _lib.ptr(perm), start, B, seed, epoch, sigma, clip,
                                       int(augment), q("input"), q("gt"), q("radius"), _lib.ptr(status.t), q("idx"), q("rot"), q("scale"),
                                       q("noise"), q("raw"), _lib.stream_ptr(dev))
    _lib.check(rc, "dispu_sample_batch")
    torch.cuda.synchronize()
    out = {k: N(v.t) for k, v in g.items()}
    out["input"], out["gt"] = out["input"].reshape(B, P, 3), out["gt"].reshape(B, G, 3)
    if verify:
        out["idx"], out["rot"], out["raw"] = out["idx"].reshape(B, P), out["rot"].reshape(B, 9), out["raw"].reshape(B, 4).view(np.uint32)
        if augment:
            out["noise"] = out["noise"].reshape(B, P, 3)
    out["status"] = N(status.t)
    out["intact"] = all(v.intact() for v in g.values()) and status.intact()
    return out


def dataset(dev, L, G, seed=0, P=None):
    rng = np.random.default_rng(seed)
    gt = torch.from_numpy(rng.standard_normal((L, G, 3)).astype(np.float32)).to(dev)
    perm = torch.from_numpy(rng.permutation(L).astype(np.int32)).to(dev)
    inp = torch.from_numpy(rng.standard_normal((L, P, 3)).astype(np.float32)).to(dev) if P else None
    return gt, perm, inp


def augment_ref(dev, x, noise, rot, scale):
    """dispu_augment on numpy inputs -> numpy"""
    from dispu_amd import _lib
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    tx, tn, tr, ts = d(x), d(noise), d(rot), d(scale)
    out = torch.empty_like(tx)
    _lib.check(_lib.lib().dispu_augment(x.shape[0], x.shape[1], _lib.ptr(tx), _lib.ptr(tn), _lib.ptr(tr), _lib.ptr(ts), None, _lib.ptr(out),
                                        _lib.stream_ptr(dev)), "dispu_augment")
    torch.cuda.synchronize()
    return N(out)


def group_ref(dev, rows, idx):
    from dispu_amd import _lib
    B, G = rows.shape[0], rows.shape[1]
    P = idx.shape[1]
    tr = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(dev)
    ti = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev).view(B, P, 1)
    sub = torch.empty((B, P, 1, 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dispu_group_point(B, G, 3, P, 1, _lib.ptr(tr), _lib.ptr(ti), _lib.ptr(sub), _lib.stream_ptr(dev)), "dispu_group_point")
    torch.cuda.synchronize()
    return N(sub).reshape(B, P, 3)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------- 1. structure, exact ----
@pytest.mark.parametrize("B", [1, 8, 28])
@pytest.mark.parametrize("G,P", [(1024, 256), (4096, 1024), (64, 64)])
def test_structure_exact(dev, B, G, P):
    L, start, clip = 40, 3, 0.03
    gt_data, perm, _ = dataset(dev, L, G, seed=G + B)
    o = sample(dev, gt_data, perm, start, B, P, clip=clip)
    assert o["intact"], "a sentinel around an output was overwritten"
    assert not o["status"].any(), o["status"]
    idx = o["idx"]
    assert idx.min() >= 0 and idx.max() < G
    assert (np.diff(idx, axis=1) > 0).all(), "indices must be strictly ascending (hence distinct)"
    rows = N(gt_data)[N(perm)[start:start + B]]
    assert np.array_equal(bits(o["gt"]), bits(augment_ref(dev, rows, None, o["rot"], o["scale"])))
    sub = group_ref(dev, rows, idx)
    assert np.array_equal(bits(o["input"]), bits(augment_ref(dev, sub, o["noise"], o["rot"], o["scale"])))
    assert (np.abs(o["noise"]) <= np.float32(clip)).all() and np.abs(o["noise"]).max() > 0
    R = o["rot"].reshape(B, 3, 3).astype(np.float64)
    assert np.array_equal(o["rot"][:, [2, 5, 6, 7]], np.zeros((B, 4), np.float32)) and (o["rot"][:, 8] == 1).all()
    assert np.array_equal(R[:, 0, 0], R[:, 1, 1]) and np.array_equal(R[:, 0, 1], -R[:, 1, 0])
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    assert (o["scale"] >= np.float32(0.8)).all() and (o["scale"] <= np.float32(1.2)).all()
    assert (o["radius"] == 1).all()
    # production form (no verification outputs): the same batch
    o2 = sample(dev, gt_data, perm, start, B, P, clip=clip, verify=False)
    assert o2["intact"] and np.array_equal(bits(o2["input"]), bits(o["input"])) and np.array_equal(bits(o2["gt"]), bits(o["gt"]))


@pytest.mark.parametrize("G,P", [(1024, 256), (64, 64), (30, 7)])
def test_structure_random_false_and_no_augment(dev, G, P):
    L, start, B = 20, 5, 8
    gt_data, perm, inp = dataset(dev, L, G, seed=9, P=P)
    o = sample(dev, gt_data, perm, start, B, P, input_data=inp)
    assert o["intact"] and not o["status"].any()
    rows = N(perm)[start:start + B]
    assert np.array_equal(bits(o["input"]), bits(augment_ref(dev, N(inp)[rows], o["noise"], o["rot"], o["scale"])))
    assert np.array_equal(bits(o["gt"]), bits(augment_ref(dev, N(gt_data)[rows], None, o["rot"], o["scale"])))
    assert np.array_equal(o["idx"], np.tile(np.arange(P, dtype=np.int32), (B, 1)))
    # augment off: plain rows / plain sub-sample (G = 30, P = 7: the scalar store path, rows not 16-byte multiples)
    o = sample(dev, gt_data, perm, start, B, P, augment=False)
    assert o["intact"] and np.array_equal(o["gt"], N(gt_data)[rows])
    assert np.array_equal(o["input"], np.take_along_axis(N(gt_data)[rows], o["idx"][:, :, None].astype(np.int64), axis=1))
    assert (np.diff(o["idx"], axis=1) > 0).all() and o["idx"].min() >= 0 and o["idx"].max() < G


def test_unaligned_pointers_take_the_scalar_path(dev):
    """Rows of 4k points go out as 16-byte stores only where the pointers allow it: outputs 4 bytes past a 16-byte boundary, and a
    dataset that starts 4 bytes past one, give the same bits through the per-point path."""
    L, G, P, B, start = 12, 1024, 256, 3, 2
    gt_data, perm, inp = dataset(dev, L, G, seed=17, P=P)
    want = sample(dev, gt_data, perm, start, B, P)
    got = sample(dev, gt_data, perm, start, B, P, off=1)
    shifted = torch.empty(gt_data.numel() + 1, dtype=torch.float32, device=dev)[1:].view(L, G, 3)
    shifted.copy_(gt_data)
    assert gt_data.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    got2 = sample(dev, shifted, perm, start, B, P)
    for o in (got, got2):
        assert o["intact"] and not o["status"].any()
        for k in ("input", "gt", "noise", "idx"):
            assert np.array_equal(o[k].view(np.uint32), want[k].view(np.uint32)), k
    # random=False: the input rows are streamed from input_data, here 4 bytes past a boundary
    want = sample(dev, gt_data, perm, start, B, P, input_data=inp)
    inp1 = torch.empty(inp.numel() + 1, dtype=torch.float32, device=dev)[1:].view(L, P, 3)
    inp1.copy_(inp)
    got = sample(dev, gt_data, perm, start, B, P, input_data=inp1)
    assert got["intact"] and np.array_equal(bits(got["input"]), bits(want["input"])) and np.array_equal(bits(got["gt"]), bits(want["gt"]))


# ------------------------------------------------------------------------------------------------ 2. keying, exact ----
def test_index_and_jitter_streams_against_the_host_twin(dev):
    """The counters of the index and jitter streams, not only the patch block: the sub-sample equals the sequential process over the
    host twin's draws, the jitter equals the twin's Box-Muller values.
    The twin computes in float64, the kernel in fp32: a candidate (loc + 0.3 z) G differs by the angle's rounding (2.4e-7 of 2 pi u,
    times a radius below 5.8), a few ulp of logf / sqrtf / cosf and one ulp of the product -- under 5e-5 at G = 64 -- so a draw
    truncates alike on both sides when it keeps 1e-3 from every integer; the twin reports that margin for the draws consumed (a
    property of the seed, checked before the comparison).  Jitter: sigma times that error, under 1e-7."""
    L, G, P, B, start, epoch = 32, 64, 16, 8, 8, 0
    gt_data, perm, _ = dataset(dev, L, G, seed=5)
    o = sample(dev, gt_data, perm, start, B, P, epoch=epoch)
    assert o["intact"] and not o["status"].any()
    for i in range(B):
        want, margin = SO.subsample(SEED, epoch, start + i, G, P)
        assert margin > 1e-3, "choose another (seed, epoch): a draw of position %d is within %g of a truncation boundary" % (start + i, margin)
        assert o["idx"][i].tolist() == want, i
        twin = np.array([SO.jitter(SEED, epoch, start + i, k, 0.01, 0.03) for k in range(P)])
        assert np.abs(o["noise"][i].astype(np.float64) - twin).max() <= 1e-7, i

def test_keying_exact(dev):
    L, G, P = 64, 1024, 256
    gt_data, perm, _ = dataset(dev, L, G, seed=1)
    a = sample(dev, gt_data, perm, 8, 8, P, epoch=3)
    for i in range(8):
        assert tuple(int(w) for w in a["raw"][i]) == SO.block(SEED, 3, 8 + i), i
    # the patch scalars are the documented functions of that block
    u = np.array([[SO.u01(w) for w in r] for r in a["raw"]])
    assert np.allclose(a["scale"], 0.8 + 0.4 * u[:, 2], atol=1e-6)
    assert np.allclose(a["rot"][:, 0], np.cos(2 * np.pi * u[:, 1]), atol=1e-5) and np.allclose(a["rot"][:, 3], np.sin(2 * np.pi * u[:, 1]), atol=1e-5)
    b = sample(dev, gt_data, perm, 8, 8, P, epoch=3)
    for k in ("input", "gt", "idx", "noise", "rot", "scale", "raw"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for kw in (dict(seed=SEED + 1, epoch=3, start=8), dict(seed=SEED, epoch=4, start=8), dict(seed=SEED, epoch=3, start=9),
               dict(seed=SEED ^ (1 << 40), epoch=3, start=8)):
        c = sample(dev, gt_data, perm, kw["start"], 8, P, seed=kw["seed"], epoch=kw["epoch"])
        assert not np.array_equal(c["raw"], a["raw"]) and not np.array_equal(c["idx"], a["idx"]) and not np.array_equal(c["noise"], a["noise"]), kw
    lo, hi = sample(dev, gt_data, perm, 8, 4, P, epoch=3), sample(dev, gt_data, perm, 12, 4, P, epoch=3)
    for k in ("input", "gt", "idx", "noise", "rot", "scale", "raw", "radius"):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]).view(np.uint32), a[k].view(np.uint32)), k


# --------------------------------------------------------------------- 3. distribution against the reference's sampler ----
def ks2(a, b):
    a, b = np.sort(a), np.sort(b)
    allv = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, allv, side="right") / a.size - np.searchsorted(b, allv, side="right") / b.size).max())


def ks1_uniform(u):
    u = np.sort(u)
    n = u.size
    return float(max((np.arange(1, n + 1) / n - u).max(), (u - np.arange(n) / n).max()))


def test_distribution_against_reference_sampler(dev):
    from oracle import data as OD
    G, P, n, L = 1024, 256, 2048, 64
    gt_data, perm, _ = dataset(dev, L, G, seed=2)
    idx, noise, rot, scale = [], [], [], []
    for epoch in range(n // L):
        o = sample(dev, gt_data, perm, 0, L, P, epoch=epoch)
        assert o["intact"] and not o["status"].any()
        idx.append(o["idx"]); noise.append(o["noise"]); rot.append(o["rot"]); scale.append(o["scale"])
    idx, noise, rot, scale = np.concatenate(idx), np.concatenate(noise).ravel(), np.concatenate(rot), np.concatenate(scale)
    assert idx.shape == (n, P)
    state = np.random.get_state()
    np.random.seed(12345)
    try:
        ref = np.stack([np.sort(np.asarray(OD.nonuniform_sampling(G, P))) for _ in range(n)])
    finally:
        np.random.set_state(state)
    bound2 = math.sqrt(math.log(2 / ALPHA) / 2) * math.sqrt(2.0 / n)
    assert abs(bound2 - 0.1023) < 1e-3
    d_mean = ks2((idx / G).mean(1), (ref / G).mean(1))
    d_std = ks2((idx / G).std(1), (ref / G).std(1))
    p_dev, p_ref = float((idx[:, 0] == 0).mean()), float((ref[:, 0] == 0).mean())
    se = math.sqrt(p_dev * (1 - p_dev) / n + p_ref * (1 - p_ref) / n)
    print("KS mean %.4f std %.4f (bound %.4f); index-0 share device %.4f host %.4f (se %.4f)" % (d_mean, d_std, bound2, p_dev, p_ref, se))
    assert d_mean < bound2 and d_std < bound2
    assert abs(p_dev - p_ref) <= 6 * se
    # jitter: sigma 0.01, clip 0.03 -> clipped at 3 sigma
    nn = noise.size
    assert nn >= 100000
    clip = np.float32(0.03)
    p_clip, share = 2 * 0.5 * math.erfc(3 / math.sqrt(2)), float((np.abs(noise) == clip).mean())
    print("jitter: N %d mean %.3e (bound %.3e) share at the clip %.5f (expected %.5f)" % (nn, noise.mean(), 6 * 0.01 / math.sqrt(nn), share, p_clip))
    assert abs(float(noise.astype(np.float64).mean())) <= 6 * 0.01 / math.sqrt(nn)
    assert abs(share - p_clip) <= 6 * math.sqrt(p_clip * (1 - p_clip) / nn)
    # rotation angle and scale: uniform
    bound1 = math.sqrt(math.log(2 / ALPHA) / (2 * n))
    ang = np.mod(np.arctan2(rot[:, 3].astype(np.float64), rot[:, 0].astype(np.float64)), 2 * np.pi) / (2 * np.pi)
    d_ang, d_scale = ks1_uniform(ang), ks1_uniform((scale.astype(np.float64) - 0.8) / 0.4)
    print("KS angle %.4f scale %.4f (bound %.4f)" % (d_ang, d_scale, bound1))
    assert d_ang < bound1 and d_scale < bound1


# -------------------------------------------------------------------------------------- 4. launch count, DeviceFetcher ----
def test_device_fetcher_one_launch_and_surface(dev):
    from dispu_amd import _lib, dataset as DS
    rng = np.random.default_rng(4)
    gt = rng.standard_normal((24, 1024, 3)).astype(np.float32)
    f = DS.DeviceFetcher(gt, gt, 4, patch_num_point=256, device=dev, seed=11)
    assert len(f) == 24 and f.has_next_batch() and f.epoch == 0
    _lib.tape_begin()
    try:
        x, g, r = f.next_batch()
    finally:
        tape = _lib.tape_end()
    assert [c[2] for c in tape.calls] == ["dispu_sample_batch"]
    assert x.shape == (4, 256, 3) and g.shape == (4, 1024, 3) and r.shape == (4,) and x.is_cuda and x.is_contiguous() and g.is_contiguous()
    assert f.batch_idx == 1                                   # the reference's off-by-one: batch 0 is skipped, this one is positions 4..7
    # against a direct call at those positions with the fetcher's own permutation
    o = sample(dev, f.gt_data, f.perm, 4, 4, 256, seed=11, epoch=0)
    assert np.array_equal(bits(N(x)), bits(o["input"])) and np.array_equal(bits(N(g)), bits(o["gt"])) and (N(r) == 1).all()
    # normalisation as Fetcher's: centroid 0, furthest point at distance 1
    gd = N(f.gt_data)
    assert np.abs(gd.mean(1)).max() < 1e-5 and np.allclose(np.sqrt((gd ** 2).sum(-1)).max(1), 1.0, atol=1e-5)
    # batches do not depend on the batch size: positions 8..11 of B = 4 are the first half of positions 8..15 of B = 8
    x2 = f.next_batch()[0]
    f8 = DS.DeviceFetcher(gt, gt, 8, patch_num_point=256, device=dev, seed=11)
    assert np.array_equal(N(f8.perm), N(f.perm))
    assert np.array_equal(bits(N(f8.next_batch()[0])[:4]), bits(N(x2)))
    # epoch end: 4 more batches exist (positions 12..23), then a short batch raises
    for _ in range(3):
        f.next_batch()
    with pytest.raises(IndexError):
        f.next_batch()
    p0 = N(f.perm).copy()
    f.reset()
    assert f.epoch == 1 and f.batch_idx == 0 and sorted(N(f.perm).tolist()) == list(range(24)) and not np.array_equal(N(f.perm), p0)
    # the permutation is composed onto the previous one, from PCG64(seed)
    g2 = np.random.Generator(np.random.PCG64(11))
    want = np.arange(24)[g2.permutation(24)]
    assert np.array_equal(p0, want) and np.array_equal(N(f.perm), want[g2.permutation(24)])
    assert not N(f.status).any()


def test_refused_before_any_launch(dev):
    from dispu_amd import _lib, dataset as DS
    gt_data, perm, _ = dataset(dev, 8, 64, seed=3)
    before = (N(gt_data).copy(), N(perm).copy())
    with pytest.raises(_lib.DispuError):
        sample(dev, gt_data, perm, 0, 4, 65)                  # P > G
    with pytest.raises(_lib.DispuError):
        sample(dev, gt_data, perm, 6, 4, 32)                  # start + B > L
    with pytest.raises(ValueError):
        DS.DeviceFetcher(N(gt_data), N(gt_data), 4, patch_num_point=65, device=dev)
    _lib.tape_begin()
    try:
        with pytest.raises(_lib.DispuError):
            _lib.check(_lib.tape_lib().dispu_sample_batch(8, 64, 65, _lib.ptr(gt_data), None, _lib.ptr(perm), 0, 4, 1, 0, 0.01, 0.03, 1,
                                                          _lib.ptr(gt_data), _lib.ptr(gt_data), _lib.ptr(gt_data), _lib.ptr(perm),
                                                          None, None, None, None, None, _lib.stream_ptr(dev)), "dispu_sample_batch")
    finally:
        _lib.tape_end()
    torch.cuda.synchronize()
    assert np.array_equal(N(gt_data), before[0]) and np.array_equal(N(perm), before[1])      # nothing was written
