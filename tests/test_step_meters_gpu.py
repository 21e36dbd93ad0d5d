"""dispu_step_meters (csrc/step_meters.hip): the train loop's five per-step meters in one launch.

(a) the raw entry on synthetic distance arrays, BIT-equal to the fp32 numpy expression
        row = [loss_out[3], loss_out[0], 100 * max_b((1 * max_j d_gt_c + max_j d_pred_c) / r_b), loss_out[1], the same for _f]
    (a maximum has no rounding and numpy's float32 division is correctly rounded, so there is nothing to tolerate), over row
    lengths that exercise the scalar head / 16-byte body / scalar tail of the row reader, rows that start off a 16-byte boundary
    (odd lengths with b > 1), n_gt != n_pred, more clouds than one round of waves would need at b = 1, and maxima planted at the
    first element, the last element and inside the last partial vector; one layout lets a cloud win on its radius alone.  The rows
    of the table before and after the written one keep their sentinel.
(b) after a real Trainer.train_step / train_step_taped: the row is bit-equal to the step's own terms and to
    train._hausdorff_terms, which recomputes the distances (two nn_distance launches, four row reductions, torch glue)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 1                     # hipErrorInvalidValue
SENT = -12345.0


def p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def expected_row(dgc, dpc, dgf, dpf, radius, loss_out):
    def hd(dg, dp):
        h = (F32(1.0) * dg.max(axis=1) + dp.max(axis=1)) / radius
        assert h.dtype == F32
        return F32(100.0) * h.max()
    return np.array([loss_out[3], loss_out[0], hd(dgc, dpc), loss_out[1], hd(dgf, dpf)], F32)


def launch(dev, arrays, radius, loss_out, b, n_gt, n_pred):
    from dispu_amd import _lib
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    r, lo = torch.from_numpy(radius).to(dev), torch.from_numpy(loss_out).to(dev)
    table = torch.full((3, 5), SENT, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dispu_step_meters(b, n_gt, n_pred, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(r), p(lo), p(table, 5),
                                            _lib.stream_ptr(dev)), "dispu_step_meters")
    torch.cuda.synchronize()
    return table.cpu().numpy()


@pytest.mark.parametrize("plant", ["first", "last", "partial", "radius"])
@pytest.mark.parametrize("n_gt,n_pred", [(7, 5), (255, 1024), (1024, 1024), (4099, 1021)])
@pytest.mark.parametrize("b", [1, 5])
def test_raw_entry_bit_equal_to_numpy(dev, b, n_gt, n_pred, plant):
    rng = np.random.default_rng(1000 * b + n_gt + len(plant))
    arrays = [rng.random((b, n), dtype=F32) for n in (n_gt, n_pred, n_gt, n_pred)]              # d_gt_c, d_pred_c, d_gt_f, d_pred_f
    radius = rng.uniform(0.5, 2.0, b).astype(F32)
    assert b == 1 or len(set(radius.tolist())) > 1
    loss_out = rng.random(5, dtype=F32) * F32(50.0)
    c = b - 1                                            # the last cloud: its rows start off a 16-byte boundary when n is odd
    if plant == "radius":
        # every cloud's maxima are (3, 3) at radius 2 -> h = 3; the last cloud's are (1, 1.5) at radius 0.5 -> h = 5: it wins on its
        # radius alone (at b = 1 it is simply the only cloud)
        for a in arrays:
            a *= F32(0.5)
            a[:, a.shape[1] // 2] = F32(3.0)
            a[c] *= F32(0.25)
        radius[:] = F32(2.0)
        radius[c] = F32(0.5)
        for a, v in zip(arrays, (1.0, 1.5, 1.0, 1.5)):
            a[c, a.shape[1] // 3] = F32(v)
    else:
        for k, a in enumerate(arrays):
            n = a.shape[1]
            pos = {"first": 0, "last": n - 1, "partial": n - 2}[plant]
            a[c, pos] = F32(2.0) + rng.random(dtype=F32) + F32(k)          # above every other entry (< 1) of every cloud / radius
        radius[c] = min(radius[c], F32(0.75))                             # ... and its cloud wins: >= 2 / 0.75 > 2 * 1 / 0.5
    want = expected_row(*arrays, radius, loss_out)
    if plant != "radius":
        for k, col in ((0, 2), (2, 4)):                  # the planted entries decide the result: a reader that skips them cannot pass
            h = (arrays[k][c].max() + arrays[k + 1][c].max()) / radius[c]
            assert want[col] == F32(100.0) * h and arrays[k][c].max() >= 2.0
    got = launch(dev, arrays, radius, loss_out, b, n_gt, n_pred)
    print("b=%d n=(%d,%d) %s: row %s" % (b, n_gt, n_pred, plant, got[1]))
    assert np.array_equal(bits(got[1]), bits(want)), (got[1], want)
    assert (got[0] == F32(SENT)).all() and (got[2] == F32(SENT)).all(), "rows next to the written one were touched"


def test_bad_arguments_are_refused_before_any_launch(dev):
    from dispu_amd import _lib
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    f = torch.full((64,), SENT, dtype=torch.float32, device=dev)
    F = p(f)
    ok = [2, 8, 8, F, F, F, F, F, F, p(f, 32), st]
    for i, bad in ((0, 0), (0, -1), (1, 0), (2, 0), (2, -3)):
        args = list(ok)
        args[i] = bad
        assert lib.dispu_step_meters(*args) == INVALID, (i, bad)
    for i in range(3, 10):
        args = list(ok)
        args[i] = None
        assert lib.dispu_step_meters(*args) == INVALID, i
    torch.cuda.synchronize()
    assert (f.cpu().numpy() == F32(SENT)).all()


# ------------------------------------------------------------------------------------------- after a real step ----
@pytest.fixture(scope="module")
def trainers(dev):
    from dispu_amd import params, train
    made = {}

    def get(B):
        if B not in made:
            made[B] = train.Trainer(train.TrainOpts(), params.init_params(seed=11), device=dev)
        return made[B]
    return get


@pytest.mark.parametrize("step_fn", ["train_step", "train_step_taped"])
@pytest.mark.parametrize("B", [1, 3])
def test_row_after_a_real_step(dev, trainers, B, step_fn):
    from dispu_amd import synth, train
    tr = trainers(B)
    x, gt = synth.patch_with_gt(B, 256, 1024, seed=60 + B)
    x, gt = torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)
    radius = torch.from_numpy(np.random.default_rng(B).uniform(0.5, 2.0, B).astype(F32)).to(dev)
    table = torch.full((3, 5), SENT, dtype=torch.float32, device=dev)
    for _ in range(2):                                   # taped: the second call replays the tape the first one recorded
        terms = getattr(tr, step_fn)(x, gt, radius)
    assert train.step_meters(tr, x, radius, table[1]) is not None
    chd, fhd = train._hausdorff_terms(tr, x, gt, radius)
    torch.cuda.synchronize()
    want = np.array([float(terms["pu_loss"]), float(terms["dis_coarse_cd"]), float(chd), float(terms["dis_fine_cd"]), float(fhd)], F32)
    got = table.cpu().numpy()
    print("B=%d %s: row %s" % (B, step_fn, got[1]))
    assert np.array_equal(bits(got[1]), bits(want)), (got[1], want)
    assert np.isfinite(got[1]).all() and got[1].min() > 0
    assert (got[0] == F32(SENT)).all() and (got[2] == F32(SENT)).all()


def test_step_meters_refuses_a_bad_row_or_an_unknown_shape(dev, trainers):
    from dispu_amd import train
    tr = trainers(1)
    x = torch.zeros((2, 128, 3), device=dev)
    with pytest.raises(RuntimeError, match="no step"):
        train.step_meters(tr, x, torch.ones(2, device=dev), torch.zeros(5, device=dev))
    with pytest.raises(ValueError, match="row"):
        train.step_meters(tr, x, torch.ones(2, device=dev), torch.zeros(4, device=dev))
    with pytest.raises(ValueError, match="row"):
        train.step_meters(tr, x, torch.ones(2, device=dev), torch.zeros(5))
