"""Poisson-disk (blue-noise) selection for whole clouds: mesh_sample's poisson_disk_keep / poisson_disk_select / poisson_disk_cloud
without the size limit of the one-workgroup kernel, over a tensor or a list of clouds of any sizes in ONE launch sequence
(csrc/poisson_disk_cells.hip; dispu_poisson_cells_keep / _select in include/dispu_hip.h, which states the definition).  The result is the
sequential greedy of tests/mesh_sample_oracle.py bit for bit, and below DISPU_POISSON_MAX_N the bytes of the one-workgroup tier.

Index order is the priority order of the greedy.  A scanner writes points along lines, and a line of conflicting points in index order
is a dependency chain as long as the line: `shuffle_seed` runs the greedy in a random priority order instead (another, equally valid
blue-noise set), which settles in about ten rounds whatever the input order.

torch is used for device memory and for the index glue of `shuffle_seed` (a gather and a sort); every selection is a HIP kernel."""
import math

import numpy as np
import torch

from . import _lib
from ._util import req
from .segments import Packed, host_ptr, is_int, offsets as segment_offsets, to_device

MAX_ROUNDS = _lib.POISSON_MAX_ROUNDS
STATUS_NOT_SETTLED, STATUS_SHORT, STATUS_NONFINITE = 1, 2, _lib.POISSON_CELLS_NONFINITE


# ---- host helpers: pure functions, no device.  unshuffle_* state on the host the map that keep / select apply on the device ------------
def shuffle_permutation(shuffle_seed, c, n):
    """the priority order of cloud c under shuffle_seed: perm [n] int64, position j of the permuted cloud holds input point perm[j]"""
    return np.random.RandomState((int(shuffle_seed) + int(c)) % (2 ** 32)).permutation(int(n)).astype(np.int64)


def unshuffle_flags(flags, perm):
    """per-point values of the permuted cloud -> the input's numbering: out[perm[j]] = flags[j]"""
    flags = np.asarray(flags)
    out = np.empty_like(flags)
    out[np.asarray(perm)] = flags
    return out


def unshuffle_indices(idx, perm):
    """indices into the permuted cloud -> indices into the input, ascending there"""
    return np.sort(np.asarray(perm)[np.asarray(idx, np.int64)]).astype(np.int32)


def spacing_from_mean_nn(mean_nn, final_ratio):
    """2 d / sqrt(final_ratio): the r_hi of a cloud upsampled final_ratio times, from the mean nearest-neighbour distance d of its input.
    The hexagonal bound for 4 N points is about 1.07 d for a random input and less for an even one, and a greedy selection from
    jittered overlapping patches ends well below it (0.40 d on the CPU prototype of DESIGN section 9), so 2 d / sqrt(ratio) brackets
    the radius; a bracket twice too wide costs one bisection step."""
    req(float(final_ratio) > 0.0, "final_ratio must be positive, got %r" % (final_ratio,))
    return 2.0 * float(mean_nn) / math.sqrt(float(final_ratio))


def _check_seed(shuffle_seed):
    req(shuffle_seed is None or is_int(shuffle_seed), "shuffle_seed must be None or an integer, got %r" % (shuffle_seed,))


def _per_cloud(v, C, name, dtype):
    """a number, or one value per cloud -> a host array [C]"""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    req(a.dtype.kind in "iuf" and a.ndim <= 1, "%s must be a number or one number per cloud, got %r" % (name, v))
    if a.ndim == 0:
        a = np.full(C, a)
    req(a.shape[0] == C, "%s: one value per cloud (%d), got %d" % (name, C, a.shape[0]))
    if dtype is np.int64:
        req(a.dtype.kind in "iu" or np.all(a == np.floor(a)), "%s must be integers, got %r" % (name, v))
    return a.astype(dtype)


def _radii(r, C, name):
    with np.errstate(over="ignore"):
        a = _per_cloud(r, C, name, np.float32)
    req(bool(np.all(np.isfinite(a))), "%s must be finite as float32, got %r" % (name, r))
    return a


def _raise_on_status(status, who):
    st = status.cpu().numpy()
    if not st.any():
        return
    c = int(np.nonzero(st)[0][0])
    bits = int(st[c])
    if bits & STATUS_NONFINITE:
        raise ValueError("cloud %d holds a NaN or an infinite coordinate" % c)
    why = []
    if bits & STATUS_NOT_SETTLED:
        why.append("did not settle in DISPU_POISSON_MAX_ROUNDS = %d rounds (a conflict chain that long: points ordered along a line? "
                   "shuffle_seed=<an integer> runs the greedy in a random priority order, which settles in about ten)" % MAX_ROUNDS)
    if bits & STATUS_SHORT:
        why.append("fewer than m indices were written")
    if bits & ~7:
        why.append("unknown status bits 0x%x" % (bits & ~7))
    raise RuntimeError("%s: cloud %d %s" % (who, c, "; ".join(why)))


class _Batch(Packed):
    """the packed batch in priority order: the clouds themselves, or under shuffle_seed their permutations (perms: device int64)"""

    def __init__(self, points, who, shuffle_seed):
        Packed.__init__(self, points, who, words=3)
        _check_seed(shuffle_seed)
        self.seed = shuffle_seed
        self.perms = None

    def pack(self):
        if self.seed is not None:
            self.perms = [to_device(shuffle_permutation(self.seed, c, t.shape[0]), self.dev) for c, t in enumerate(self.clouds)]
            self.clouds = [t[p] for t, p in zip(self.clouds, self.perms)]
        Packed.pack(self)


def keep(points, radius, shuffle_seed=None, return_rounds=False):
    """Greedy dart throwing: points a float32 [n,3] tensor on a ROCm device or a list of them (any sizes from 1 to 2^24 points, one
    launch sequence), radius a number or one per cloud -> (keep u8 [n], count i32 []) (a list in gives two lists out).  keep[i] iff no
    kept point of higher priority lies strictly closer than the radius (fp32, dispu_poisson_disk_keep's definition); the priority is
    the index, or under shuffle_seed position in numpy.random.RandomState(shuffle_seed + c).permutation(n_c) -- the flags are in the
    input's numbering either way.  A radius <= 0 keeps everything.  return_rounds adds the number of rounds the evaluation took.
    ValueError for illegal arguments (before any launch) and for non-finite coordinates, RuntimeError if a cloud does not settle."""
    b = _Batch(points, "poisson_cells.keep", shuffle_seed)
    r = _radii(radius, b.C, "radius")
    b.pack()
    with torch.cuda.device(b.dev):
        L = _lib.lib()
        flags = torch.empty(b.total, dtype=torch.uint8, device=b.dev)
        count = torch.empty(b.C, dtype=torch.int32, device=b.dev)
        rounds = torch.zeros(1, dtype=torch.int32, device=b.dev)
        nbytes = L.dispu_poisson_cells_scratch_bytes(b.C, b.total)
        scratch = b.scratch(nbytes, "dispu_poisson_cells_keep")
        d_r = to_device(r, b.dev)                            # named: a temporary would be freed, and its block reused, before the call
        _lib.check(L.dispu_poisson_cells_keep(b.C, _lib.ptr(b.d_off), host_ptr(b.off), _lib.ptr(b.cloud), _lib.ptr(d_r),
                                              _lib.ptr(flags), _lib.ptr(count), _lib.ptr(rounds), _lib.ptr(scratch), nbytes,
                                              _lib.ptr(b.status), _lib.stream_ptr(b.dev)), "dispu_poisson_cells_keep")
        _raise_on_status(b.status, "poisson_cells.keep")
        if b.perms is not None:
            out = torch.empty_like(flags)
            out[torch.cat([p + int(o) for p, o in zip(b.perms, b.off[:-1])])] = flags
            flags = out
    fl = b.split(flags)
    res = (fl, count[0]) if b.single else (fl, [count[c] for c in range(b.C)])
    return res + (int(rounds.item()),) if return_rounds else res


def select(points, m, r_hi, steps=12, shuffle_seed=None, return_rounds=False):
    """Exactly m points per cloud: points as for keep, m a number or one per cloud (1 <= m_c <= n_c), r_hi a number or one per cloud
    (the start of the bisection; any finite value is legal) -> (idx i32 [m] ascending, r f32 [], count i32 []) (a list in gives three
    lists out): the first m points in priority order that the greedy keeps at the radius r the bisection ends on
    (dispu_poisson_disk_select's recurrence, bit for bit), count >= m of them in all.  Under shuffle_seed the indices are mapped back to
    the input's numbering and sorted there.  return_rounds adds the list of the rounds of the steps + 1 evaluations."""
    b = _Batch(points, "poisson_cells.select", shuffle_seed)
    ms = _per_cloud(m, b.C, "m", np.int64)
    for c in range(b.C):
        req(1 <= ms[c] <= b.clouds[c].shape[0], "poisson_cells.select: cannot select %d of %d points (cloud %d)" % (ms[c], b.clouds[c].shape[0], c))
    req(is_int(steps) and steps >= 0, "poisson_cells.select: steps must be an integer >= 0, got %r" % (steps,))
    rh = _radii(r_hi, b.C, "r_hi")
    moff = segment_offsets(ms)
    b.pack()
    with torch.cuda.device(b.dev):
        L = _lib.lib()
        idx = torch.empty(int(moff[-1]), dtype=torch.int32, device=b.dev)
        r = torch.empty(b.C, dtype=torch.float32, device=b.dev)
        count = torch.empty(b.C, dtype=torch.int32, device=b.dev)
        rounds = torch.zeros(int(steps) + 1, dtype=torch.int32, device=b.dev)
        nbytes = L.dispu_poisson_cells_scratch_bytes(b.C, b.total)
        scratch = b.scratch(nbytes, "dispu_poisson_cells_select")
        d_moff, d_rh = to_device(moff, b.dev), to_device(rh, b.dev)    # named: temporaries would be freed, and share one block, before the call
        _lib.check(L.dispu_poisson_cells_select(b.C, _lib.ptr(b.d_off), _lib.ptr(d_moff), host_ptr(b.off), host_ptr(moff),
                                                int(steps), _lib.ptr(b.cloud), _lib.ptr(d_rh), _lib.ptr(idx), _lib.ptr(r),
                                                _lib.ptr(count), _lib.ptr(rounds), _lib.ptr(scratch), nbytes, _lib.ptr(b.status),
                                                _lib.stream_ptr(b.dev)), "dispu_poisson_cells_select")
        _raise_on_status(b.status, "poisson_cells.select")
        parts = [idx[moff[c]:moff[c + 1]] for c in range(b.C)]
        if b.perms is not None:
            parts = [torch.sort(p[i.long()])[0].to(torch.int32) for p, i in zip(b.perms, parts)]
    res = (parts[0], r[0], count[0]) if b.single else (parts, [r[c] for c in range(b.C)], [count[c] for c in range(b.C)])
    return res + (rounds.cpu().tolist(),) if return_rounds else res


def mesh_cloud(mesh, m, oversample=4, seed=0, steps=12, shuffle_seed=None):
    """mesh_sample.poisson_disk_cloud without the size limit: sample_surface(mesh, oversample m) candidates, select with
    r_hi = hex_radius(mesh.total_area, m) -> (points [m,3] device f32 in sample order, r: the radius as a Python float)."""
    from .mesh_sample import hex_radius, sample_surface
    from .tf_sampling import gather_point
    m, oversample = int(m), int(oversample)
    req(m > 0 and oversample >= 1, "mesh_cloud: m must be positive and oversample >= 1")
    req(oversample * m <= 2 ** 24, "mesh_cloud: %d x %d candidates, at most 2^24" % (oversample, m))
    cand, _ = sample_surface(mesh, oversample * m, seed)
    idx, r, _ = select(cand, m, hex_radius(mesh.total_area, m), steps, shuffle_seed)
    return gather_point(cand.reshape(1, -1, 3), idx.reshape(1, -1))[0], float(r.item())


def spacing_r_hi(points, final_ratio):
    """2 d / sqrt(final_ratio) per cloud, d the mean nearest-neighbour distance of the cloud (outliers.knn_mean_distance at k = 1,
    averaged in float64 on the device): a float for a tensor, a list of floats for a list.  The r_hi of upsample_ragged's Poisson merge."""
    from .outliers import knn_mean_distance
    single = isinstance(points, torch.Tensor)
    d = knn_mean_distance(points, k=1)
    out = [spacing_from_mean_nn(float(t.double().mean().item()), final_ratio) for t in ([d] if single else d)]
    return out[0] if single else out
