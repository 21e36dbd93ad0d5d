"""Plain numpy oracles of the whole-cloud glue kernels, for tests only (csrc/cloud.hip, mode 0 of csrc/knn_general.hip,
dispu_row_mean_std of csrc/mesh_eval.hip), and the inputs the CPU and GPU tests of those kernels share.

Written from the reference operations (Common/pc_util.py:83-92 extract_knn_patch, :147-161 normalize_point_cloud, DisPU/model.py:310-311,
evaluate.py's np.nanmean / np.nanstd) and from the ORDER of float32 operations the kernels document, not from their launch code.
tests/test_cloud_ops_oracle.py holds them to oracle/upsample.py and to each other.

  normalize_replay     float32, in the kernel's own order: centroid = (((0 + x_0) + x_1) + ...) / n per axis, d = x - centroid,
                       furthest = max(0, sqrt((dx dx + dy dy) + dz dz)), out = d / furthest.  Equal to
                       oracle.upsample.normalize_point_cloud in float32 bit for bit (numpy reduces the outer axis row after row)
  normalize_f64        the same in float64, with the per-element error bound of the float32 sequence (see its docstring)
  denormalize          centroid + x * furthest in float32, the product rounded before the sum (the build pins -ffp-contract=off)
  knn                  stable argsort of ((dx dx + dy dy) + dz dz) + 0 in float32: ascending distance, ties to the lower index
  tie_facts            what a query's sorted distances say about the tie at the k-th place (the radix-select collect pass)
  nan_mean_std         np.nanmean / np.nanstd (ddof 0) in float64 with the bounds of a float64 accumulation
"""
import warnings

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24                # unit roundoff of float32
U64 = 2.0 ** -53                # and of float64
CHUNK, WAVE = 256, 64           # knn_general_kernel's collect pass: 256 points a trip, four waves of 64


# ------------------------------------------------------------------------------------------- normalisation ----
def normalize_replay(p):
    """p [b, n, 3] float32 -> (out [b, n, 3], centroid [b, 3], furthest [b]) float32, every operation rounded to float32 in the
    kernel's order.  n = 1 and clouds whose points coincide with their centroid give furthest = 0 and out = 0 / 0 = NaN."""
    p = np.ascontiguousarray(p, F32)
    b, n, _ = p.shape
    s = np.zeros((b, 3), F32)
    for i in range(n):                                           # the sequential sum of lanes 0..2
        s = s + p[:, i, :]
    c = s / F32(n)
    d = p - c[:, None, :]
    r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    f = np.maximum(F32(0), r.max(1)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = d / f[:, None, None]
    assert out.dtype == F32 and c.dtype == F32 and f.dtype == F32
    return out, c, f


def normalize_f64(p):
    """p [b, n, 3] float32 -> dict of the float64 result (out, centroid, furthest) and what the float32 sequence of normalize_replay may
    differ from it by (out_bound, centroid_bound, furthest_bound), with u = 2^-24:

      centroid   the sequential sum rounds n - 1 times, each time by at most u |partial sum| <= u (1 + n u) sum |x|; divided by n and
                 with the division's own rounding u |c| <= u mean |x|:  delta_a = n u (1 + n u) mean |x_a|  per axis a.
      furthest   d = x - c carries delta_a and its own rounding u |d|; two squares, two sums (3 u of the sum), the root (half of that
                 and its own u): |r^ - r| <= |delta|_2 + 4 u r, and a maximum moves by no more than its arguments.
      out        d^ / f^ - d / f = (d^ - d) / f^ + (d / f) (f - f^) / f^, and the division's rounding:
                 (delta_a + u |d| + |out| (|delta|_2 + 4 u f)) / f^ + u |out|  <=  (delta_a + |out| |delta|_2) / f^ + 6 u |out| f / f^,
                 with f^ the smaller of the two furthest distances, so that the bound holds to every order.
    A cloud far from the origin (mean |x| = 300, spread 1, n = 24576) has delta = 0.44: the float32 centroid is allowed to be that
    far off, and the sequence only ever uses a small part of it (the measured fractions are in tests/test_cloud_ops_gpu.py)."""
    p32 = np.ascontiguousarray(p, F32)
    x = p32.astype(np.float64)
    b, n, _ = x.shape
    c = x.mean(1)
    d = x - c[:, None, :]
    f = np.sqrt((d * d).sum(-1)).max(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = d / f[:, None, None]
    delta = n * U32 * (1.0 + n * U32) * np.abs(x).mean(1)                                   # [b, 3]
    if n == 1:
        delta = np.zeros_like(delta)                                                        # (0 + x) / 1 is exact
    dn = np.sqrt((delta * delta).sum(-1))                                                   # [b]
    fb = dn + 4 * U32 * f
    f_lo = np.maximum(f - fb, 1e-300)                                                       # no furthest the bound allows is smaller
    with np.errstate(invalid="ignore", divide="ignore"):
        ob = ((1 + 4 * U32) * delta[:, None, :] + np.abs(out) * dn[:, None, None]) / f_lo[:, None, None] \
            + 6 * U32 * np.abs(out) * (f / f_lo)[:, None, None]
    return dict(out=out, centroid=c, furthest=f, out_bound=ob, centroid_bound=delta, furthest_bound=fb)


def denormalize(x, centroid, furthest):
    """x [b, m, 3], centroid [b, 3], furthest [b] float32 -> centroid + x * furthest, float32, two roundings."""
    x, centroid, furthest = np.asarray(x, F32), np.asarray(centroid, F32), np.asarray(furthest, F32)
    prod = x * furthest[:, None, None]
    out = centroid[:, None, :] + prod
    assert out.dtype == F32
    return out


def offcentre_clouds(b, n, seed, first=0):
    """[b, n, 3] float32 clouds for the normalisation: cloud i sits at +5, at -300 or at 0.01 (i + first cycles through them) with an
    anisotropic spread (1 : 0.3 : 0.05, times 0.5 .. 2), all different."""
    rng = np.random.default_rng(seed)
    centres = (5.0, -300.0, 0.01)
    out = np.empty((b, n, 3), F32)
    for i in range(b):
        spread = np.array([1.0, 0.3, 0.05]) * rng.uniform(0.5, 2.0)
        out[i] = (rng.standard_normal((n, 3)) * spread + centres[(i + first) % 3]).astype(F32)
    return out


# --------------------------------------------------------------------------------------------------- k-NN ----
def sqdist(q, pc):
    """q [m, 3], pc [n, 3] float32 -> [m, n] float32: ((dx dx + dy dy) + dz dz) + 0 with d = q - p, every operation rounded."""
    q, pc = np.asarray(q, F32), np.asarray(pc, F32)
    d = q[:, None, :] - pc[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + F32(0)
    assert d2.dtype == F32
    return d2


def knn(q, pc, k):
    """-> (idx [m, k] int32, the sorted distances [m, n] float32).  A stable sort: equal distances keep their index order."""
    d2 = sqdist(q, pc)
    order = np.argsort(d2, axis=1, kind="stable")
    return order[:, :k].astype(np.int32), np.take_along_axis(d2, order, 1)


def knn_batch(q, pc, k):
    """q [b, m, 3], pc [b, n, 3] -> idx [b, m, k] int32."""
    return np.stack([knn(q[c], pc[c], k)[0] for c in range(len(pc))])


def tie_facts(q, pc, k):
    """One query q [3] against pc [n, 3]: from the distances alone, what the collect pass of the radix select meets.  T is the k-th
    smallest distance; `members` the indices at distance T in index order, `quota` how many of them belong to the k nearest.
      shared          len(members)
      cut             quota < shared: some of the equal points are taken and some are not
      chunks, waves   number of 256-point chunks holding members / the largest number of 64-point waves of one chunk holding members
      carry_matters   some member the quota excludes has fewer than `quota` members before it in its own wave of its own chunk: a count
                      that forgets the earlier chunks (or the earlier waves) takes it."""
    d2 = sqdist(np.asarray(q, F32)[None], pc)[0]
    T = np.sort(d2, kind="stable")[k - 1]
    members = np.nonzero(d2 == T)[0]
    quota = k - int((d2 < T).sum())
    assert 1 <= quota <= len(members)
    chunk, wave = members // CHUNK, (members % CHUNK) // WAVE
    rank = np.arange(len(members))
    in_wave = np.array([int(((chunk[:i] == chunk[i]) & (wave[:i] == wave[i])).sum()) for i in rank])
    in_chunk = np.array([int((chunk[:i] == chunk[i]).sum()) for i in rank])
    return dict(T=float(T), shared=len(members), quota=quota, cut=quota < len(members), chunks=len(set(chunk.tolist())),
                waves=max(len(set(wave[chunk == c].tolist())) for c in set(chunk.tolist())),
                carry_matters=bool(((rank >= quota) & (in_wave < quota)).any()),
                chunk_carry_matters=bool(((rank >= quota) & (in_chunk < quota)).any()))


def lattice(side, scale, permute_seed=None):
    """side^3 integer lattice points times `scale` (a power of two: every squared distance is exact, so shells of equal distance are
    exactly equal), x-major; permute_seed shuffles the index order."""
    g = np.arange(side, dtype=np.float64)
    pts = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * scale).astype(F32)
    if permute_seed is not None:
        pts = pts[np.random.default_rng(permute_seed).permutation(len(pts))]
    return np.ascontiguousarray(pts)


def lattice_case(side, scale=0.0625):
    """-> (pc [2, side^3, 3], q [2, 4, 3]): the lattice in index order and shuffled; queries at the corner (point 0), the centre point,
    the last point and the middle of the first cell (no cloud point: eight points at the same distance, then shells of 24)."""
    a, bb = lattice(side, scale), lattice(side, scale, permute_seed=side)
    mid = (side // 2) * scale
    q = np.array([[0.0, 0.0, 0.0], [mid, mid, mid], [(side - 1) * scale] * 3, [scale / 2] * 3], F32)
    return np.stack([a, bb]), np.stack([q, q])


COPIES = 600


def copies_case(n, seed):
    """-> (pc [2, n, 3], q [2, 2, 3]).  In each random cloud 600 copies of one point P sit at a fixed stride through the whole index
    range.  Query 0 is P's nearest distinct neighbour (a cloud point): the copies are the next nearest to it after a handful of
    points, so they are the tie at the k-th place for every k up to 600.  Query 1 is P itself: the tie is at distance 0."""
    rng = np.random.default_rng(seed)
    stride = (n - 8) // COPIES
    assert stride >= 2
    pcs, qs = [], []
    for c in range(2):
        pc = rng.random((n, 3)).astype(F32)
        at = 5 + c + stride * np.arange(COPIES)
        P = pc[at[0]].copy()
        pc[at] = P
        rest = np.setdiff1d(np.arange(n), at)
        near = rest[np.argmin(sqdist(P[None], pc[rest])[0])]
        pcs.append(pc)
        qs.append(np.stack([pc[near], P]))
    return np.stack(pcs), np.stack(qs)


def identical_case(n):
    """-> (pc [3, n, 3], q [3, 2, 3]).  Every point of a cloud identical.  Cloud 0: query 0 the point itself (all distances +0), query 1
    elsewhere (all distances equal and positive).  Cloud 1: another point, the same two kinds of query.  Cloud 2: every coordinate +0
    and query 0 at -0: q - p = -0 in all three axes.  (The squares of -0 are +0, so the distance is +0 with or without the kernel's
    `+ 0.0f`; the case holds the result, index order, either way.)"""
    pc = np.empty((3, n, 3), F32)
    pc[0], pc[1], pc[2] = (0.3, -1.7, 2.5), (-4.0, 0.125, 1e-3), (0.0, 0.0, 0.0)
    q = np.stack([np.stack([pc[0, 0], pc[0, 0] + F32(0.5)]), np.stack([pc[1, 0], pc[1, 0] - F32(3.0)]),
                  np.array([[-0.0, -0.0, -0.0], [1.0, 2.0, -2.0]], F32)])
    return pc, q


def random_case(b, n, m, seed):
    """-> (pc [b, n, 3], q [b, m, 3]) uniform in the unit cube; query j of cloud c is a cloud point when j + c is odd (the last point
    for j = 1, point j % n otherwise) and a point of its own otherwise."""
    rng = np.random.default_rng(seed)
    pc = rng.random((b, n, 3)).astype(F32)
    q = rng.random((b, m, 3)).astype(F32)
    for c in range(b):
        for j in range(m):
            if (j + c) % 2 == 1:
                q[c, j] = pc[c, n - 1 if j == 1 else j % n]
    return pc, q


# the tie clouds and the k each is run at: (name, builder, argument, ks, which queries (cloud, query) must show a cut tie that spans
# chunks and waves -- asserted by tests/test_cloud_ops_oracle.py from the sorted distances)
TIE_CASES = [
    ("lattice20", lattice_case, 20, (1, 256, 300, 1024, 8000), ()),                           # bitonic path: 8000 points
    ("lattice21", lattice_case, 21, (256, 300, 1024, 4096), ((0, 0), (0, 1), (0, 2), (1, 1))),   # radix path: 9261 points
    ("copies8192", lambda n: copies_case(n, 3), 8192, (1, 256, 600, 601), ()),
    ("copies24576", lambda n: copies_case(n, 4), 24576, (256, 257, 601, 4096), ((0, 0), (1, 0), (0, 1), (1, 1))),
    ("identical8192", identical_case, 8192, (1, 256, 8192), ()),
    ("identical9261", identical_case, 9261, (1, 256, 257, 4096), ((0, 0), (0, 1), (2, 0))),
]


# ------------------------------------------------------------------------------------------ row mean / std ----
def nan_mean_std(x):
    """x [b, n] float32 -> dict(mean, std [b] float64 by np.nanmean / np.nanstd with ddof 0, NaN for a row without a number, and
    mean_bound, std_bound).  With c <= n numbers in a row and u = 2^-53, a float64 accumulation of c terms in any order is off by at
    most (c - 1) u sum |x|, the division adds u |mean|; numpy's own pairwise sum is held to the same figure, so against it
      mean_bound = 2 n u mean |x| = n 2^-52 mean |x|.
    The deviations d = x - mean carry the error of the mean, e <= mean_bound, once each and a rounding of their own; sum (d + e)^2 =
    sum d^2 + c e^2 about the true mean, so the root moves by sqrt(s^2 + e^2) - s <= e^2 / (2 s); the c squares, c - 1 sums, the
    division and the root add (c + 4) / 2 roundings relative to s = the root mean square deviation, on either side:
      std_bound = max(n, 4) 2^-52 s + mean_bound^2 / (2 s)        (0 when s = 0: a row of one repeated value has mean x exactly)."""
    x = np.asarray(x, F32).astype(np.float64)
    n = x.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mean, std = np.nanmean(x, axis=1), np.nanstd(x, axis=1)
        mabs = np.nanmean(np.abs(x), axis=1)
    mb = n * 2.0 ** -52 * mabs
    with np.errstate(invalid="ignore", divide="ignore"):
        sb = np.where(std > 0, max(n, 4) * 2.0 ** -52 * std + mb * mb / (2 * std), 0.0)
    return dict(mean=mean, std=std, mean_bound=mb, std_bound=sb)


ROW_KINDS = ("scattered", "allnan", "constant", "offset")


def stat_rows(b, n, turn, seed):
    """x [b, n] float32 and the kind of each row: row i is ROW_KINDS[(i + turn) % 4] --
      scattered   normal numbers times 10^(-2..2) with a third of them NaN (at least one number kept)
      allnan      nothing but NaN: mean and std are NaN
      constant    one value repeated: the std is exactly 0
      offset      1000 + 1e-3 noise in float32: the deviations are 1e-6 of the values."""
    rng = np.random.default_rng(seed + 17 * turn)
    x = np.empty((b, n), F32)
    kinds = []
    for i in range(b):
        kind = ROW_KINDS[(i + turn) % 4]
        kinds.append(kind)
        if kind == "scattered":
            r = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(F32)
            r[rng.random(n) < 1.0 / 3.0] = np.nan
            r[n // 2] = F32(0.75)
        elif kind == "allnan":
            r = np.full(n, np.nan, F32)
        elif kind == "constant":
            r = np.full(n, F32(-3.1415927) * F32(i + 1), F32)
        else:
            r = (1000.0 + 1e-3 * rng.standard_normal(n)).astype(F32)
        x[i] = r
    return x, kinds
