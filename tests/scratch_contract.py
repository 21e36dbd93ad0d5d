"""The scratch contract of the C entries that take a caller's scratch (include/dispu_hip.h: "the library never allocates", and nothing
is promised about what the buffer holds on entry): a guarded scratch buffer, and a registry of one case per entry that the GPU test
(tests/test_scratch_contract_gpu.py) runs on a zero-filled, a stale and an all-ones scratch.  Imports without a GPU; torch, the
library and the other test modules are imported where they are used.

A case:
  sizes()                       the bytes the entry's own size query returns for the case's shape
  run(scratch, variant, short=False)   one call on the device of `scratch` -> dict of every output as numpy arrays, "rc" among them,
                                the inputs as the call left them under "in:<name>"; short: scratch_bytes = sizes() - 1
  inputs(variant)               dict name -> numpy array: what "in:<name>" must still hold
  check(out, variant, dev)      the outputs against the oracle of the entry's own test file, at that file's tolerance
  sentinels                     dict output name -> the value every element holds before the call (what a refusal must leave)
  bit_identical                 False where the header does not promise identical bytes from run to run: the stale and the all-ones
                                run are then held to check() instead
  refuses                       the header promises that a refusal leaves scratch and outputs untouched
Variants "a" and "b" have identical sizes and different content; where the entry has a status word for a non-finite segment, "a" has
one in its middle segment."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

GUARD = 4096                                                    # bytes on either side of the body; keeps the body's 256-byte alignment
GUARD_BYTE = 0x5A
FILLS = {"zeros": 0x00, "ones": 0xFF}                           # "stale" is not a fill: it is what a call on other inputs left
ORDER = ("zeros", "stale", "ones")
INVALID = 1                                                     # hipErrorInvalidValue


# every size query of the library -> the entries that take a scratch of that size
QUERY_ENTRIES = {
    "dispu_fps_scratch_bytes": ("dispu_fps_ws",),
    "dispu_fps_segments_scratch_bytes": ("dispu_fps_segments",),
    "dispu_fps_segments_auto_scratch_bytes": ("dispu_fps_segments_auto",),
    "dispu_fps_cells_scratch_bytes": ("dispu_fps_cells",),
    "dispu_pca_normals_scratch_bytes": ("dispu_pca_normals_segments",),
    "dispu_orient_consistent_scratch_bytes": ("dispu_orient_consistent_segments",),
    "dispu_knn_mean_dist_scratch_bytes": ("dispu_knn_mean_dist_segments",),
    "dispu_radius_count_scratch_bytes": ("dispu_radius_count_segments",),
    "dispu_compact_scratch_bytes": ("dispu_compact_segments",),
    "dispu_cluster_scratch_bytes": ("dispu_cluster_segments",),
    "dispu_knn_cross_scratch_bytes": ("dispu_knn_cross_segments", "dispu_transfer_attributes_segments"),
    "dispu_mls_project_scratch_bytes": ("dispu_mls_project_segments",),
    "dispu_icp_scratch_bytes": ("dispu_icp_segments",),
    "dispu_signed_distance_scratch_bytes": ("dispu_signed_distance_segments",),
    "dispu_lattice_voxels_scratch_bytes": ("dispu_lattice_voxels",),
    "dispu_lattice_dilate_scratch_bytes": ("dispu_lattice_dilate",),
    "dispu_lattice_corners_scratch_bytes": ("dispu_lattice_corners",),
    "dispu_contour_count_scratch_bytes": ("dispu_contour_count",),
    "dispu_knn_feat_scratch_bytes": ("dispu_knn_feat_strided_ws",),
    "dispu_knn_xyz_scratch_bytes": ("dispu_knn_xyz_ws",),
    "dispu_approx_match_scratch_bytes": ("dispu_approx_match_ws", "dispu_approx_match_levels_ws"),
    "dispu_emd_loss_grad_scratch_bytes": ("dispu_emd_loss_grad",),
    "dispu_match_cost_scratch_bytes": ("dispu_match_cost_ws",),
    "dispu_match_cost_grad_scratch_bytes": ("dispu_match_cost_grad_ws",),
    "dispu_linear_tn_scratch_floats": ("dispu_linear_tn", "dispu_tn_reduce_grouped"),
    "dispu_linear_tn_bf16_scratch_floats": ("dispu_linear_tn_bf16s",),
    "dispu_linear_tn_bf16_stream_scratch_floats": ("dispu_linear_tn_bf16_stream",),
    "dispu_act_bias_grad_scratch_floats": ("dispu_act_bias_grad",),
    "dispu_bn_scratch_bytes": ("dispu_bn_train", "dispu_bn_train_grad"),
    "dispu_ps_wnet_scratch_bytes": ("dispu_ps_wnet_bn_stats", "dispu_ps_wnet_grad"),
    "dispu_edge_dense_conv_grad_scratch_floats": ("dispu_edge_dense_conv_grad", "dispu_edge_dense_conv_grad_partials",
                                                  "dispu_edge_dense_conv_grad_reduce"),
    "dispu_disk_uniformity_scratch_bytes": ("dispu_disk_uniformity",),
    "dispu_geodesic_scratch_bytes": ("dispu_geodesic_distances",),
    "dispu_poisson_disk_scratch_bytes": ("dispu_poisson_disk_keep", "dispu_poisson_disk_select"),
    "dispu_poisson_cells_scratch_bytes": ("dispu_poisson_cells_keep", "dispu_poisson_cells_select"),
    "dispu_radix_sort_scratch_bytes": ("dispu_radix_sort_pairs",),
    "dispu_grid_subsample_scratch_bytes": ("dispu_grid_subsample_plan", "dispu_grid_subsample_emit"),
}
# the reference signatures: a `temp` of the reference's size and no byte count, hence no size query
TEMP_TAKERS = ("dispu_fps", "dispu_approx_match", "dispu_prob_sample")


class Scratch(object):
    """one uint8 buffer of GUARD + nbytes + GUARD bytes on `dev`: the guards hold GUARD_BYTE, the body holds `fill`"""

    def __init__(self, dev, nbytes, fill="zeros"):
        import torch
        self.dev, self.nbytes = dev, int(nbytes)
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.inputs = None                                      # a helper that is given this scratch leaves its inputs here, as numpy
        self.refill(fill)

    @property
    def offset(self):
        return GUARD

    @property
    def floats(self):                                           # for the entries sized in floats
        return self.nbytes // 4

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def refill(self, fill):
        self.buf[GUARD:GUARD + self.nbytes] = FILLS[fill] if isinstance(fill, str) else int(fill)

    def body(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().copy()

    def guards_intact(self):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.nbytes:]
        return bool((lo == GUARD_BYTE).all()) and bool((hi == GUARD_BYTE).all())


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def _N(t):
    return t.detach().cpu().numpy()


def offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return off


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class Case(object):
    entries = ()                                                # the C entries the case calls with the scratch
    queries = ()                                                # the size queries those entries are sized by
    refuses = False
    sentinels = {}
    bit_identical = True                                        # False: the header does not promise identical bytes from run to run

    def check_inputs(self, out, variant):
        want = self.inputs(variant)
        got = {k[3:]: v for k, v in out.items() if k.startswith("in:")}
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        for name, w in want.items():
            assert same_bytes(np.asarray(got[name]), np.asarray(w)), "input %s was written" % name

    @staticmethod
    def with_inputs(out, ins):
        out.update({"in:" + k: v for k, v in ins.items()})
        return out


# ---- packed-batch cell operators: three segments of 70, 200 and 64 points (a ragged last cell, more than one cell, exactly one cell), k = 8 ----
SIZES = (70, 200, 64)
K = 8
POISON = (1, 100, 1)                                            # variant "a": segment, row, axis of the non-finite coordinate
_SEED = {"a": 100, "b": 200}
_CACHE = {}


def cached(f):
    def g(*args):
        key = (f.__name__,) + args
        if key not in _CACHE:
            _CACHE[key] = f(*args)
        return _CACHE[key]
    g.__name__ = f.__name__
    return g


@cached
def clouds(variant, poison=False, salt=0):
    """three seeded samples of the unit sphere; salt: another sample of the same sizes (the second side of a pair)"""
    import normals_oracle as NO
    cs = [np.ascontiguousarray(NO.sphere(n, seed=_SEED[variant] + 10 * salt + i), np.float32).copy() for i, n in enumerate(SIZES)]
    if poison and variant == "a":
        cs[POISON[0]][POISON[1], POISON[2]] = np.nan
    for c in cs:
        c.setflags(write=False)
    return cs


OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)   # one array for the whole session: the size queries read it through a pointer


def segments(packed):
    return [packed[OFF[c]:OFF[c + 1]] for c in range(len(SIZES))]


class CellCase(Case):
    """the status word is part of the outputs: variant "a" must report [0, 1, 0] where the entry flags a non-finite segment"""
    refuses = True
    poison = True

    def off(self):
        return OFF

    def lib(self):
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        return _lib.lib()

    def check_status(self, out, variant, name="status"):
        want = [0, 1, 0] if (self.poison and variant == "a") else [0, 0, 0]
        assert out[name].tolist() == want, (out[name], want)


class Normals(CellCase):
    """dispu_pca_normals_segments: "Identical bytes from run to run." """
    entries, queries = ("dispu_pca_normals_segments",), ("dispu_pca_normals_scratch_bytes",)
    sentinels = dict(normal=7.0, variation=7.0, idx=-7, status=-7)

    def sizes(self):
        return self.lib().dispu_pca_normals_scratch_bytes(len(SIZES), _hp(self.off()), K)

    def inputs(self, variant):
        return dict(cloud=np.concatenate(clouds(variant, True)), off=self.off())

    def run(self, scratch, variant, short=False):
        import test_normals_gpu as T
        rc, nrm, var, idx, status = T.run_abi(scratch.dev, clouds(variant, True), K, scratch="short" if short else "ok", scratch_buf=scratch)
        return self.with_inputs(dict(rc=rc, normal=nrm, variation=var, idx=idx, status=status), scratch.inputs)

    def check(self, out, variant, dev=None):
        import normals_oracle as NO
        import test_normals_gpu as T
        self.check_status(out, variant)
        for c, nrm, var, idx in zip(clouds(variant, True), segments(out["normal"]), segments(out["variation"]), segments(out["idx"])):
            ref = NO.normals(c, K)
            assert np.array_equal(idx, ref["idx"])
            T.check_against_eigh(nrm, var, ref, oriented=True)


@cached
def orient_cases(variant):
    """(points, normals, neighbours) per segment: the sphere's own normals with seeded signs; variant "a" has a NaN normal"""
    import normals_oracle as NO
    out = []
    for i, p in enumerate(clouds(variant)):
        sign = np.where(np.random.RandomState(_SEED[variant] + i).random_sample(len(p)) < 0.5, -1.0, 1.0).astype(np.float32)
        nrm = np.ascontiguousarray(p * sign[:, None], np.float32)
        if variant == "a" and i == POISON[0]:
            nrm[POISON[1], POISON[2]] = np.nan
        out.append((p, nrm, NO.neighbors(p, K).astype(np.int32)))
    return out


class Orient(CellCase):
    """dispu_orient_consistent_segments: "integer
    atomics, every loop bounded, ordering by kernel boundaries only, identical bytes from run to run" """
    entries, queries = ("dispu_orient_consistent_segments",), ("dispu_orient_consistent_scratch_bytes",)
    sentinels = dict(normal=7.0, flip=9, component=-7, ncomp=-7, status=-7)
    flags = 0

    def sizes(self):
        return self.lib().dispu_orient_consistent_scratch_bytes(len(SIZES), _hp(self.off()), K)

    def inputs(self, variant):
        cs = orient_cases(variant)
        return dict(points=np.concatenate([c[0] for c in cs]), normal_in=np.concatenate([c[1] for c in cs]),
                    neighbors=np.concatenate([c[2] for c in cs]), off=self.off())

    def run(self, scratch, variant, short=False):
        import test_orient_gpu as T
        res = T.run_abi(scratch.dev, orient_cases(variant), K, flags=self.flags, scratch="short" if short else "ok", scratch_buf=scratch)
        res.pop("normal_in")
        return self.with_inputs(res, scratch.inputs)

    def check(self, out, variant, dev=None):
        import orient_oracle as OO
        import test_orient_gpu as T
        self.check_status(out, variant)
        off = self.off()
        for c, (p, nrm, nbr) in enumerate(orient_cases(variant)):
            T.assert_equals_oracle(out, off[c], off[c + 1], c, OO.orient(p, nrm, nbr, 0))


class OrientHostRounds(Orient):
    """the same entry with DISPU_ORIENT_HOST_ROUNDS: the rounds ended by reading a counter of the scratch back"""
    flags = 1


class OutliersCase(CellCase):
    def abi(self, scratch, variant):
        import test_outliers_gpu as T
        return T.Abi(scratch.dev, clouds(variant, self.poison), scratch_buf=scratch)

    def inputs(self, variant):
        return dict(cloud=np.concatenate(clouds(variant, self.poison)), off=self.off())

    def ins(self, a):
        return dict(cloud=_N(a.cloud), off=_N(a.d_off))


class MeanDist(OutliersCase):
    """dispu_knn_mean_dist_segments: "Ordinary stores, no float atomics, identical bytes from run to run." """
    entries, queries = ("dispu_knn_mean_dist_segments",), ("dispu_knn_mean_dist_scratch_bytes",)
    sentinels = dict(mean_dist=7.0, status=-7)

    def sizes(self):
        return self.lib().dispu_knn_mean_dist_scratch_bytes(len(SIZES), _hp(self.off()), K)

    def run(self, scratch, variant, short=False):
        a = self.abi(scratch, variant)
        rc, md, status = a.mean_dist(K, scratch="short" if short else "ok")
        return self.with_inputs(dict(rc=rc, mean_dist=md, status=status), self.ins(a))

    def check(self, out, variant, dev=None):
        import outliers_oracle as O
        self.check_status(out, variant)
        for c, md in zip(clouds(variant, True), segments(out["mean_dist"])):
            assert same_bytes(md, O.mean_dist(c, K).astype(np.float32))


class RadiusCount(OutliersCase):
    """dispu_radius_count_segments: "Ordinary stores, no float atomics, identical bytes from run to run." """
    entries, queries = ("dispu_radius_count_segments",), ("dispu_radius_count_scratch_bytes",)
    sentinels = dict(count=-7, status=-7)
    RADIUS, CAP = 0.5, 2 ** 31 - 1

    def sizes(self):
        return self.lib().dispu_radius_count_scratch_bytes(len(SIZES), _hp(self.off()))

    def run(self, scratch, variant, short=False):
        a = self.abi(scratch, variant)
        rc, cnt, status = a.count(self.RADIUS, self.CAP, scratch="short" if short else "ok")
        return self.with_inputs(dict(rc=rc, count=cnt, status=status), self.ins(a))

    def check(self, out, variant, dev=None):
        import outliers_oracle as O
        self.check_status(out, variant)
        for c, cnt in zip(clouds(variant, True), segments(out["count"])):
            want = O.radius_count(c, self.RADIUS, self.CAP)
            assert np.array_equal(cnt, want) and 2 < want.mean() < len(c) - 1


@cached
def keep_flags(variant):
    return (np.random.RandomState(_SEED[variant] + 7).random_sample(sum(SIZES)) < 0.6).astype(np.int32)


class Compact(OutliersCase):
    """dispu_compact_segments at rule 0: "Ordinary stores, no float atomics, identical bytes from run to run."  No status word of its
    own for non-finite input: both variants are finite"""
    entries, queries = ("dispu_compact_segments",), ("dispu_compact_scratch_bytes",)
    sentinels = dict(points=7.0, index=-7, new_off=-7)
    poison = False

    def sizes(self):
        return self.lib().dispu_compact_scratch_bytes(len(SIZES), _hp(self.off()))

    def inputs(self, variant):
        return dict(OutliersCase.inputs(self, variant), src=keep_flags(variant))

    def run(self, scratch, variant, short=False):
        import torch
        a = self.abi(scratch, variant)
        src = torch.from_numpy(keep_flags(variant)).to(scratch.dev)
        rc, pts, idx, new_off = a.compact(0, src, scratch="short" if short else "ok", status=False)
        return self.with_inputs(dict(rc=rc, points=pts, index=idx, new_off=new_off), dict(self.ins(a), src=_N(src)))

    def check(self, out, variant, dev=None):
        flags, off = keep_flags(variant) != 0, self.off()
        packed = np.concatenate(clouds(variant))
        kept = int(flags.sum())
        want_off = np.concatenate([[0], np.cumsum([flags[off[c]:off[c + 1]].sum() for c in range(len(SIZES))])]).astype(np.int32)
        assert np.array_equal(out["new_off"], want_off)
        assert same_bytes(out["points"][:kept], packed[flags]) and (out["points"][kept:] == 7.0).all()
        local = np.concatenate([np.nonzero(flags[off[c]:off[c + 1]])[0] for c in range(len(SIZES))]).astype(np.int32)
        assert np.array_equal(out["index"][:kept], local) and (out["index"][kept:] == -7).all()


class Cluster(CellCase):
    """dispu_cluster_segments: "The labels are a pure function of the input, so the bytes are identical from run to run although the
    components are found with integer atomics".  The head ints the header documents ([0, 4) link launches short of a cap, [4, 8) the
    same for the flatten launches, [8] the clusters of the batch) are outputs"""
    entries, queries = ("dispu_cluster_segments",), ("dispu_cluster_scratch_bytes",)
    sentinels = dict(labels=-7, core=9, sizes=-7, nclusters=-7, status=-7)
    EPS, MIN_POINTS = 0.3, 3

    def sizes(self):
        return self.lib().dispu_cluster_scratch_bytes(len(SIZES), _hp(self.off()))

    def inputs(self, variant):
        return dict(cloud=np.concatenate(clouds(variant, True)), off=self.off())

    def run(self, scratch, variant, short=False):
        import test_cluster_gpu as T
        res = T.run_abi(scratch.dev, clouds(variant, True), self.EPS, self.MIN_POINTS, scratch="short" if short else "ok", scratch_buf=scratch)
        if not short:
            res["head"] = scratch.body()[:9 * 4].view(np.int32).copy()
        return self.with_inputs(res, scratch.inputs)

    def check(self, out, variant, dev=None):
        import cluster_oracle as O
        self.check_status(out, variant)
        off, total = self.off(), 0
        for c, p in enumerate(clouds(variant, True)):
            labels, core, sizes = O.dbscan(p, self.EPS, self.MIN_POINTS)
            lo, hi = off[c], off[c + 1]
            assert np.array_equal(out["labels"][lo:hi], labels) and np.array_equal(out["core"][lo:hi].astype(bool), core)
            assert out["nclusters"][c] == len(sizes) and np.array_equal(out["sizes"][lo:lo + len(sizes)], sizes)
            assert not out["sizes"][lo + len(sizes):hi].any()
            assert len(sizes) >= 1 and (labels == -1).any()      # the shape has clusters, borders or noise to find
            total += len(sizes)
        assert not out["head"][:8].any() and out["head"][8] == total


class CrossCase(CellCase):
    """queries: another sample of the same sizes as the references"""

    def qs(self, variant):
        return clouds(variant, self.poison, 1)

    def rs(self, variant):
        return clouds(variant, False, 0)

    def inputs(self, variant):
        return dict(queries=np.concatenate(self.qs(variant)), refs=np.concatenate(self.rs(variant)), qoff=self.off(), roff=self.off())


@cached
def cross_knn(variant):
    import attributes_oracle as A
    c = CrossCase()
    return [A.knn_cross(q, r, K) for q, r in zip(c.qs(variant), c.rs(variant))]


@cached
def ref_attrs(variant):
    r = np.random.RandomState(_SEED[variant] + 3)
    return (r.random_sample((sum(SIZES), 3)) * 4 - 1).astype(np.float32), r.randint(-3, 40, sum(SIZES)).astype(np.int32)


class AttrCase(CrossCase):
    def abi(self, scratch, variant):
        import test_attributes_gpu as T
        return T.Abi(scratch.dev, self.qs(variant), self.rs(variant), scratch_buf=scratch)

    def sizes(self):
        return self.lib().dispu_knn_cross_scratch_bytes(len(SIZES), _hp(self.off()), _hp(self.off()))

    def ins(self, a):
        return dict(queries=_N(a.q), refs=_N(a.r), qoff=_N(a.d_qoff), roff=_N(a.d_roff))


class KnnCross(AttrCase):
    """dispu_knn_cross_segments: "identical bytes from run to run" """
    entries, queries = ("dispu_knn_cross_segments",), ("dispu_knn_cross_scratch_bytes",)
    sentinels = dict(idx=-7, d2=7.0, status=-7)

    def run(self, scratch, variant, short=False):
        a = self.abi(scratch, variant)
        rc, idx, d2, status = a.knn(K, scratch="short" if short else "ok")
        return self.with_inputs(dict(rc=rc, idx=idx, d2=d2, status=status), self.ins(a))

    def check(self, out, variant, dev=None):
        self.check_status(out, variant)
        for (widx, wd2), idx, d2 in zip(cross_knn(variant), segments(out["idx"]), segments(out["d2"])):
            assert np.array_equal(idx, widx) and same_bytes(d2, wd2.astype(np.float32))


class Transfer(AttrCase):
    """dispu_transfer_attributes_segments, inverse-distance features and nearest labels in one call: "identical bytes from run to run" """
    entries, queries = ("dispu_transfer_attributes_segments",), ("dispu_knn_cross_scratch_bytes",)
    sentinels = dict(out_feat=7.0, out_labels=-7, status=-7)

    def inputs(self, variant):
        feat, labels = ref_attrs(variant)
        return dict(AttrCase.inputs(self, variant), feat=feat, labels=labels)

    def run(self, scratch, variant, short=False):
        a = self.abi(scratch, variant)
        feat, labels = ref_attrs(variant)
        rc, of, ol, status = a.transfer(K, 0, 3, feat, labels, scratch="short" if short else "ok")
        return self.with_inputs(dict(rc=rc, out_feat=of, out_labels=ol, status=status), dict(self.ins(a), feat=feat, labels=labels))

    def check(self, out, variant, dev=None):
        import attributes_oracle as A
        self.check_status(out, variant)
        feat, labels = ref_attrs(variant)
        for (widx, wd2), of, ol, f, l in zip(cross_knn(variant), segments(out["out_feat"]), segments(out["out_labels"]), segments(feat),
                                             segments(labels)):
            assert same_bytes(of, A.transfer_from_knn(widx, wd2, f, "idw").astype(np.float32))
            assert np.array_equal(ol, l[widx[:, 0]])


class Mls(CrossCase):
    """dispu_mls_project_segments at iterations = 2 (both sides of the position ping-pong): "Ordinary stores, no atomics, identical bytes
    from run to run."  The oracle as tests/test_mls_gpu.py holds it: the first step to one fp32 ulp, two iterations as two chained calls
    of the library itself on a scratch of its own (so the second step's reference is not independent of the library)"""
    entries, queries = ("dispu_mls_project_segments",), ("dispu_mls_project_scratch_bytes",)
    sentinels = dict(out=7.0, idx=-7, status=-7)
    SUPPORT = 1.5

    def qs(self, variant):                                      # noisy samples of the sphere the references lie on
        base = clouds(variant, False, 1)
        out = []
        for i, q in enumerate(base):
            noise = np.random.RandomState(_SEED[variant] + 50 + i).standard_normal(q.shape) * 0.01
            out.append((q.astype(np.float64) + noise).astype(np.float32))
        if variant == "a":
            out[POISON[0]][POISON[1], POISON[2]] = np.nan
        return out

    def sizes(self):
        return self.lib().dispu_mls_project_scratch_bytes(len(SIZES), _hp(self.off()), _hp(self.off()))

    def run(self, scratch, variant, short=False):
        import test_mls_gpu as T
        qs, rs = self.qs(variant), self.rs(variant)
        rc, out, idx, status = T.run_abi(scratch.dev, qs, rs, K, self.SUPPORT, iterations=2, scratch="short" if short else "ok", scratch_buf=scratch)
        return self.with_inputs(dict(rc=rc, out=out, idx=idx, status=status), scratch.inputs)

    def check(self, out, variant, dev=None):
        import mls_oracle as O
        import test_mls_gpu as T
        self.check_status(out, variant)
        qs, rs = self.qs(variant), self.rs(variant)
        rc, one, idx1, _ = T.run_abi(dev, qs, rs, K, self.SUPPORT)
        assert rc == 0
        for q, r, o, i in zip(qs, rs, segments(one), segments(idx1)):
            T.check_step(q, o, i, O.step(q, r, K, self.SUPPORT), cap=False)
        rc, two, idx2, _ = T.run_abi(dev, segments(one), rs, K, self.SUPPORT)
        assert rc == 0 and T.same_bits(out["out"], two) and np.array_equal(out["idx"], idx2)


class SignedDistance(CrossCase):
    """dispu_signed_distance_segments: "Ordinary stores, no atomics, identical bytes from run to run." """
    entries, queries = ("dispu_signed_distance_segments",), ("dispu_signed_distance_scratch_bytes",)
    sentinels = dict(out=7.0, status=-7)
    SUPPORT = 1.5

    def qs(self, variant):                                      # a shell of radii 0.7 .. 1.3 around the sphere
        out = []
        for i, q in enumerate(clouds(variant, False, 1)):
            rad = np.random.RandomState(_SEED[variant] + 60 + i).uniform(0.7, 1.3, (len(q), 1))
            out.append((q.astype(np.float64) * rad).astype(np.float32))
        if variant == "a":
            out[POISON[0]][POISON[1], POISON[2]] = np.nan
        return out

    def inputs(self, variant):
        return dict(CrossCase.inputs(self, variant), normals=np.concatenate(self.rs(variant)))

    def sizes(self):
        return self.lib().dispu_signed_distance_scratch_bytes(len(SIZES), _hp(self.off()), _hp(self.off()))

    def run(self, scratch, variant, short=False):
        import test_reconstruct_gpu as T
        rs = self.rs(variant)
        rc, out, status = T.run_sd(scratch.dev, self.qs(variant), rs, rs, K, self.SUPPORT, scratch="short" if short else "ok", scratch_buf=scratch)
        return self.with_inputs(dict(rc=rc, out=out, status=status), scratch.inputs)

    def check(self, out, variant, dev=None):
        import reconstruct_oracle as R
        self.check_status(out, variant)
        for q, r, got in zip(self.qs(variant), self.rs(variant), segments(out["out"])):
            assert same_bytes(got, R.signed_distance(q, r, r, K, self.SUPPORT).astype(np.float32))


class Icp(CrossCase):
    """dispu_icp_segments, point to point, iterations = 2, tolerance 0: "Ordinary stores only, identical bytes from run to run."  The
    oracle as tests/test_icp_gpu.py holds it: one step within its bound of the float64 oracle, k iterations as k chained calls of the
    library itself on a scratch of its own (so the second step's reference is not independent of the library)"""
    entries, queries = ("dispu_icp_segments",), ("dispu_icp_scratch_bytes",)
    sentinels = dict(T=7.0, aligned=7.0, corr=-7, inliers=-7, rmse=7.0, iters=-7, flag=-7, status=-7)

    def qs(self, variant):                                      # every reference segment under a small motion, rounded to fp32
        import icp_oracle as O
        out = [O.apply64(O.motion(r), r).astype(np.float32) for r in self.rs(variant)]
        if variant == "a":
            out[POISON[0]][POISON[1], POISON[2]] = np.nan
        return out

    def sizes(self):
        return self.lib().dispu_icp_scratch_bytes(len(SIZES), _hp(self.off()), _hp(self.off()))

    def run(self, scratch, variant, short=False):
        import test_icp_gpu as T
        res = T.run_abi(scratch.dev, self.qs(variant), self.rs(variant), iterations=2, scratch="short" if short else "ok", scratch_buf=scratch)
        return self.with_inputs(res, scratch.inputs)

    def check(self, out, variant, dev=None):
        import icp_oracle as O
        import test_icp_gpu as T
        self.check_status(out, variant)
        qs, rs = self.qs(variant), self.rs(variant)
        one = T.run_abi(dev, qs, rs, iterations=1)
        assert one["rc"] == 0 and not one["status"].any() and (one["iters"] == 1).all() and not one["flag"].any()
        for c, (src, p) in enumerate(zip(qs, rs)):
            ref = O.step(O.identity(), src, p)
            bound = 64 * len(src) * 2.0 ** -53 * ref["cond"] * max(1.0, float(np.abs(np.concatenate([p, src])).max()))
            assert np.abs(one["T"][c] - ref["T"]).max() <= bound
        two = T.run_abi(dev, qs, rs, init=list(one["T"]), iterations=1)
        assert two["rc"] == 0 and (out["iters"] == 2).all()
        assert T.same_bytes(out, two, [n for n in T.OUTS if n != "iters"])


# ---- dispu_fps_cells, dispu_poisson_cells_* ------------------------------------------------------------------------------------------------
MS = (16, 50, 64)                                               # samples per segment


class FpsCells(CellCase):
    """dispu_fps_cells at cell = 0: "The indices are those of dispu_fps_ws and dispu_fps_segments bit for bit" """
    entries, queries = ("dispu_fps_cells",), ("dispu_fps_cells_scratch_bytes",)
    sentinels = dict(idx=-1, status=9)

    MOFF = np.concatenate([[0], np.cumsum(MS)]).astype(np.int32)

    def moff(self):
        return self.MOFF

    def sizes(self):
        return self.lib().dispu_fps_cells_scratch_bytes(len(SIZES), _hp(self.off()), _hp(self.moff()), 0)

    def inputs(self, variant):
        return dict(cloud=np.concatenate(clouds(variant, True)), off=self.off(), moff=self.moff())

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        L, dev = self.lib(), scratch.dev
        off, moff = self.off(), self.moff()
        x = torch.from_numpy(np.concatenate(clouds(variant, True))).to(dev)
        d_off, d_moff = torch.from_numpy(off).to(dev), torch.from_numpy(moff).to(dev)
        out = torch.full((int(moff[-1]),), -1, dtype=torch.int32, device=dev)
        status = torch.full((len(SIZES),), 9, dtype=torch.int32, device=dev)
        rc = L.dispu_fps_cells(len(SIZES), _lib.ptr(d_off), _lib.ptr(d_moff), _hp(off), _hp(moff), _lib.ptr(x), scratch.ptr(),
                               scratch.nbytes - (1 if short else 0), _lib.ptr(out), _lib.ptr(status), 0, 0, _lib.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        return self.with_inputs(dict(rc=rc, idx=_N(out), status=_N(status)), dict(cloud=_N(x), off=_N(d_off), moff=_N(d_moff)))

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        self.check_status(out, variant)
        moff = self.moff()
        for c, (p, m) in enumerate(zip(clouds(variant, True), MS)):
            assert np.array_equal(out["idx"][moff[c]:moff[c + 1]], O.farthest_point_sample(m, p[None], contract=0)[0])


class PoissonCase(CellCase):
    """finite input only: a non-finite segment is "not evaluated", which the keep case's variant "a" has"""
    refuses = False                                             # the header promises a refusal, not an untouched scratch
    R = (0.3, 0.2, 0.35)

    def sizes(self):
        return self.lib().dispu_poisson_cells_scratch_bytes(len(SIZES), sum(SIZES))


class PoissonKeep(PoissonCase):
    """dispu_poisson_cells_keep: "the result is the sequential one bit for bit, whatever the timing, the launch shape or the packing, and
    identical from run to run (no float atomics)" """
    entries, queries = ("dispu_poisson_cells_keep",), ("dispu_poisson_cells_scratch_bytes",)

    def inputs(self, variant):
        return dict(points=np.concatenate(clouds(variant, True)), off=self.off(), radius=np.float32(self.R))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        L, dev = self.lib(), scratch.dev
        off = self.off()
        pts = torch.from_numpy(np.concatenate(clouds(variant, True))).to(dev)
        d_off, d_r = torch.from_numpy(off).to(dev), torch.from_numpy(np.float32(self.R)).to(dev)
        keep = torch.full((sum(SIZES),), 9, dtype=torch.uint8, device=dev)
        count = torch.full((len(SIZES),), -7, dtype=torch.int32, device=dev)
        status = torch.full((len(SIZES),), -7, dtype=torch.int32, device=dev)
        rounds = torch.full((1,), -7, dtype=torch.int32, device=dev)
        rc = L.dispu_poisson_cells_keep(len(SIZES), _lib.ptr(d_off), _hp(off), _lib.ptr(pts), _lib.ptr(d_r), _lib.ptr(keep), _lib.ptr(count),
                                        _lib.ptr(rounds), scratch.ptr(), scratch.nbytes, _lib.ptr(status), _lib.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        return self.with_inputs(dict(rc=rc, keep=_N(keep), count=_N(count), rounds=_N(rounds), status=_N(status)),
                                dict(points=_N(pts), off=_N(d_off), radius=_N(d_r)))

    def check(self, out, variant, dev=None):
        import mesh_sample_oracle as SO
        assert out["status"].tolist() == ([0, 4, 0] if variant == "a" else [0, 0, 0])
        off = self.off()
        for c, (p, r) in enumerate(zip(clouds(variant, True), self.R)):
            if out["status"][c]:
                continue
            want = SO.poisson_keep(p, np.float32(r))
            assert np.array_equal(out["keep"][off[c]:off[c + 1]].astype(bool), want) and out["count"][c] == int(want.sum())
            assert 0.1 * len(p) < want.sum() < 0.9 * len(p)


class PoissonSelect(PoissonCase):
    """dispu_poisson_cells_select, 12 bisection steps: "dispu_poisson_disk_select's bisection bit for bit" """
    entries, queries = ("dispu_poisson_cells_select",), ("dispu_poisson_cells_scratch_bytes",)
    M, STEPS = (16, 50, 20), 12
    poison = False

    MOFF = np.concatenate([[0], np.cumsum(M)]).astype(np.int32)

    def moff(self):
        return self.MOFF

    def r_hi(self):
        return np.float32([4.0 * np.sqrt(1.0 / m) for m in self.M])

    def inputs(self, variant):
        return dict(points=np.concatenate(clouds(variant)), off=self.off(), moff=self.moff(), r_hi=self.r_hi())

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        L, dev = self.lib(), scratch.dev
        off, moff = self.off(), self.moff()
        pts = torch.from_numpy(np.concatenate(clouds(variant))).to(dev)
        d_off, d_moff, d_r = torch.from_numpy(off).to(dev), torch.from_numpy(moff).to(dev), torch.from_numpy(self.r_hi()).to(dev)
        idx = torch.full((int(moff[-1]),), -7, dtype=torch.int32, device=dev)
        r_out = torch.full((len(SIZES),), 7.0, dtype=torch.float32, device=dev)
        count = torch.full((len(SIZES),), -7, dtype=torch.int32, device=dev)
        status = torch.full((len(SIZES),), -7, dtype=torch.int32, device=dev)
        rounds = torch.full((self.STEPS + 1,), -7, dtype=torch.int32, device=dev)
        rc = L.dispu_poisson_cells_select(len(SIZES), _lib.ptr(d_off), _lib.ptr(d_moff), _hp(off), _hp(moff), self.STEPS, _lib.ptr(pts),
                                          _lib.ptr(d_r), _lib.ptr(idx), _lib.ptr(r_out), _lib.ptr(count), _lib.ptr(rounds), scratch.ptr(),
                                          scratch.nbytes, _lib.ptr(status), _lib.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        return self.with_inputs(dict(rc=rc, idx=_N(idx), r_out=_N(r_out), count=_N(count), rounds=_N(rounds), status=_N(status)),
                                dict(points=_N(pts), off=_N(d_off), moff=_N(d_moff), r_hi=_N(d_r)))

    def check(self, out, variant, dev=None):
        import mesh_sample_oracle as SO
        assert not out["status"].any()
        moff = self.moff()
        for c, (p, m, r) in enumerate(zip(clouds(variant), self.M, self.r_hi())):
            widx, wr, wcount = SO.poisson_select(p, m, r, self.STEPS)
            assert np.array_equal(out["idx"][moff[c]:moff[c + 1]], widx)
            assert np.float32(out["r_out"][c]).tobytes() == np.float32(wr).tobytes() and out["count"][c] == wcount


# ---- the sorter ----------------------------------------------------------------------------------------------------------------------------
class RadixSort(Case):
    """dispu_radix_sort_pairs, n = 2049 (two tiles): "No float atomics anywhere: two runs give identical bytes" (csrc/radix_sort.hip;
    the header: "identical bytes from run to run").  Variant "a" has few distinct keys in long runs, "b" random ones"""
    entries, queries = ("dispu_radix_sort_pairs",), ("dispu_radix_sort_scratch_bytes",)
    n = 2049
    pinned = "radix_sort(2049)"                                 # the id of these arguments in tests/test_scratch_sizes.py

    def __init__(self, bits):
        self.bits = bits                                        # 9: two passes, the result on one ping-pong side; 17: three, on the other

    def lib(self):
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        return _lib.lib()

    def sizes(self):
        return self.lib().dispu_radix_sort_scratch_bytes(self.n)

    def inputs(self, variant):
        rng = np.random.default_rng(self.bits + (0 if variant == "a" else 1000))
        mask = np.uint64((1 << self.bits) - 1)
        if variant == "a":
            keys = np.sort(rng.integers(0, 4, self.n, dtype=np.uint64))[::-1].copy() & mask
        else:
            keys = rng.integers(0, 1 << 62, self.n, dtype=np.uint64) & mask
        vals = (np.arange(self.n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5BD1E995 + (variant == "a"))
        return dict(keys=keys, vals=vals)

    def run(self, scratch, variant, short=False):
        import test_radix_sort_gpu as T
        i = self.inputs(variant)
        ko, vo = T._sort(scratch.dev, i["keys"], i["vals"], self.bits, scratch_buf=scratch)     # raises on rc != 0, asserts the inputs' bits
        return self.with_inputs(dict(rc=0, keys=ko, vals=vo), scratch.inputs)

    def check(self, out, variant, dev=None):
        i = self.inputs(variant)
        order = np.argsort(i["keys"], kind="stable")
        assert np.array_equal(out["keys"], i["keys"][order]) and np.array_equal(out["vals"], i["vals"][order])


# ---- entries over dense [b, n, 3] batches -------------------------------------------------------------------------------------------------
class DenseCase(Case):
    """helpers of the cases below: the library, device copies, one dict of inputs per variant"""

    def lib(self):
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        return _lib.lib()

    def dev_inputs(self, scratch, variant):
        import torch
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(scratch.dev) for k, v in self.inputs(variant).items()}

    def finish(self, scratch, rc, outs, ins):
        import torch
        torch.cuda.synchronize(scratch.dev)
        out = dict(rc=rc)
        out.update({k: _N(v) for k, v in outs.items()})
        return self.with_inputs(out, {k: _N(v) for k, v in ins.items()})

    def stream(self, scratch):
        from dispu_amd import _lib
        return _lib.stream_ptr(scratch.dev)


@cached
def dense_cloud(variant, b, n, salt=0):
    return np.random.default_rng(_SEED[variant] + 1000 * salt + n).random((b, n, 3)).astype(np.float32)


class Fps(DenseCase):
    """dispu_fps_ws at n = 4100, m = 64: the wave path that keeps the sorted permutation in the scratch.  "The indices are those of
    dispu_fps_ws and dispu_fps_segments bit for bit" -- indices are integers: identical bytes or wrong ones"""
    entries, queries = ("dispu_fps_ws",), ("dispu_fps_scratch_bytes",)
    B, N, M = 2, 4100, 64

    def sizes(self):
        return self.lib().dispu_fps_scratch_bytes(self.B, self.N, self.M)

    def inputs(self, variant):
        return dict(xyz=dense_cloud(variant, self.B, self.N))

    def call(self, L, d, out, scratch):
        from dispu_amd import _lib
        return L.dispu_fps_ws(self.B, self.N, self.M, _lib.ptr(d["xyz"]), scratch.ptr(), scratch.nbytes, _lib.ptr(out), 1, self.stream(scratch))

    def run(self, scratch, variant, short=False):
        import torch
        d = self.dev_inputs(scratch, variant)
        out = torch.full((self.B, self.M), -1, dtype=torch.int32, device=scratch.dev)
        return self.finish(scratch, self.call(self.lib(), d, out, scratch), dict(idx=out), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        assert np.array_equal(out["idx"], O.farthest_point_sample(self.M, self.inputs(variant)["xyz"], contract=1))


class FpsReference(Fps):
    """dispu_fps, the reference signature: temp is the reference's {32, n} floats and no byte count.  Indices: identical bytes or
    wrong ones ("bit for bit")"""
    entries, queries = ("dispu_fps",), ()

    def sizes(self):
        return 32 * self.N * 4

    def call(self, L, d, out, scratch):
        from dispu_amd import _lib
        return L.dispu_fps(self.B, self.N, self.M, _lib.ptr(d["xyz"]), scratch.ptr(), _lib.ptr(out), 1, self.stream(scratch))


class KnnFeat(DenseCase):
    """dispu_knn_feat_strided_ws at n = 1025, c = 24, k = 17: the chunked path ("searched in chunks of <= 256 candidates by the
    wave-per-query kernel and merged ... Same results": indices, identical bytes or wrong ones)"""
    entries, queries = ("dispu_knn_feat_strided_ws",), ("dispu_knn_feat_scratch_bytes",)
    B, N, C_, K_ = 1, 1025, 24, 17

    def sizes(self):
        return self.lib().dispu_knn_feat_scratch_bytes(self.B, self.N, self.N, self.C_, self.K_)

    def inputs(self, variant):
        return dict(points=np.random.default_rng(_SEED[variant] + 5).standard_normal((self.B, self.N, self.C_)).astype(np.float32))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        idx = torch.full((self.B, self.N, self.K_), -7, dtype=torch.int32, device=scratch.dev)
        dist = torch.full((self.B, self.N, self.K_), 7.0, dtype=torch.float32, device=scratch.dev)
        rc = self.lib().dispu_knn_feat_strided_ws(self.B, self.N, self.N, self.C_, self.K_, _lib.ptr(d["points"]), self.C_, _lib.ptr(d["points"]),
                                                  self.C_, _lib.ptr(dist), _lib.ptr(idx), scratch.ptr(), scratch.nbytes, self.stream(scratch))
        return self.finish(scratch, rc, dict(idx=idx, dist=dist), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        p = self.inputs(variant)["points"]
        od, oi = O.knn_point_2(self.K_, p, p)
        assert np.array_equal(out["idx"], oi[..., 1]) and np.array_equal(out["dist"], od)


class MatchCase(DenseCase):
    """b = 2, n = 300, m = 200: more than one 128-partner chunk"""
    B, N, M = 2, 300, 200

    def inputs(self, variant):
        from dispu_amd import synth
        s = 0 if variant == "b" else 50
        return dict(xyz1=synth.patches(self.B, self.N, seed=self.N + s), xyz2=synth.patches(self.B, self.M, seed=self.M + 1 + s))


class ApproxMatchWs(MatchCase):
    """dispu_approx_match_ws in pinned-exp mode: tests/test_ops_gpu.py holds it to the oracle's chunked order bit for bit, and two
    calls to the same bits ("combine their partial sums in a fixed order (no atomics)")"""
    entries, queries = ("dispu_approx_match_ws",), ("dispu_approx_match_scratch_bytes",)
    refuses = True
    sentinels = dict(match=-3.0)
    ARITH = 1 | 2                                               # DISPU_ARITH_CONTRACT | DISPU_ARITH_PINNED_EXP

    def sizes(self):
        return self.lib().dispu_approx_match_scratch_bytes(self.B, self.N, self.M)

    def call(self, L, d, match, scratch, nbytes):
        from dispu_amd import _lib
        return L.dispu_approx_match_ws(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), _lib.ptr(match), scratch.ptr(), nbytes,
                                       self.ARITH, self.stream(scratch))

    def run(self, scratch, variant, short=False):
        import torch
        d = self.dev_inputs(scratch, variant)
        match = torch.full((self.B, self.M, self.N), -3.0, dtype=torch.float32, device=scratch.dev)
        return self.finish(scratch, self.call(self.lib(), d, match, scratch, scratch.nbytes - (1 if short else 0)), dict(match=match), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        i = self.inputs(variant)
        assert np.array_equal(out["match"], O.approx_match(i["xyz1"], i["xyz2"], contract=1, pinned_exp=True, chunk=O.AM_CHUNK))


class ApproxMatchReference(ApproxMatchWs):
    """dispu_approx_match, the reference signature: temp is the reference's [b, 2 (n + m)] floats and no byte count.  Pinned-exp mode:
    "bit-exact to the oracle's chunk = 0 order" (tests/test_ops_gpu.py)"""
    entries, queries = ("dispu_approx_match",), ()
    refuses = False

    def sizes(self):
        return self.B * 2 * (self.N + self.M) * 4

    def call(self, L, d, match, scratch, nbytes):
        from dispu_amd import _lib
        return L.dispu_approx_match(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), _lib.ptr(match), scratch.ptr(), self.ARITH,
                                    self.stream(scratch))

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        i = self.inputs(variant)
        assert np.array_equal(out["match"], O.approx_match(i["xyz1"], i["xyz2"], contract=1, pinned_exp=True, chunk=0))


@cached
def oracle_match(variant):
    from oracle import oracle as O
    i = MatchCase().inputs(variant)
    return O.approx_match(i["xyz1"], i["xyz2"])


class MatchCostWs(MatchCase):
    """dispu_match_cost_ws on the oracle's match: a fixed-order reduction over per-tile partials in the scratch (no atomics); its test
    (tests/test_ops_gpu.py) holds the cost to the oracle at rtol 1e-5"""
    entries, queries = ("dispu_match_cost_ws",), ("dispu_match_cost_scratch_bytes",)
    bit_identical = False                                       # the header is silent on run-to-run bytes: the test's tolerance on every fill

    def sizes(self):
        return self.lib().dispu_match_cost_scratch_bytes(self.B, self.N, self.M)

    def inputs(self, variant):
        return dict(MatchCase.inputs(self, variant), match=oracle_match(variant))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        cost = torch.full((self.B,), 7.0, dtype=torch.float32, device=scratch.dev)
        rc = self.lib().dispu_match_cost_ws(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), _lib.ptr(d["match"]), _lib.ptr(cost),
                                            scratch.ptr(), 1, self.stream(scratch))
        return self.finish(scratch, rc, dict(cost=cost), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        i = self.inputs(variant)
        assert np.allclose(out["cost"], O.match_cost(i["xyz1"], i["xyz2"], i["match"]), rtol=1e-5)


class MatchCostGradWs(MatchCostWs):
    """dispu_match_cost_grad_ws on the oracle's match: per-tile partial rows in the scratch, summed in a fixed order (no atomics); its
    test (tests/test_ops_gpu.py) holds both gradients to the oracle at atol 3e-5"""
    entries, queries = ("dispu_match_cost_grad_ws",), ("dispu_match_cost_grad_scratch_bytes",)

    def sizes(self):
        return self.lib().dispu_match_cost_grad_scratch_bytes(self.B, self.N, self.M)

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        g1 = torch.full((self.B, self.N, 3), 7.0, dtype=torch.float32, device=scratch.dev)
        g2 = torch.full((self.B, self.M, 3), 7.0, dtype=torch.float32, device=scratch.dev)
        rc = self.lib().dispu_match_cost_grad_ws(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), _lib.ptr(d["match"]), _lib.ptr(g1),
                                                 _lib.ptr(g2), scratch.ptr(), 1, self.stream(scratch))
        return self.finish(scratch, rc, dict(grad1=g1, grad2=g2), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        i = self.inputs(variant)
        o1, o2 = O.match_cost_grad(i["xyz1"], i["xyz2"], i["match"])
        assert np.allclose(out["grad1"], o1, atol=3e-5) and np.allclose(out["grad2"], o2, atol=3e-5)


class PoissonDiskKeep(DenseCase):
    """dispu_poisson_disk_keep, b = 2, n = 300: "identical from run to run (no float atomics)" """
    entries, queries = ("dispu_poisson_disk_keep",), ("dispu_poisson_disk_scratch_bytes",)
    B, N, R = 2, 300, (0.08, 0.12)

    def sizes(self):
        return self.lib().dispu_poisson_disk_scratch_bytes(self.B, self.N)

    def inputs(self, variant):
        return dict(points=dense_cloud(variant, self.B, self.N, 3), radius=np.float32(self.R))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        keep = torch.full((self.B, self.N), 9, dtype=torch.uint8, device=scratch.dev)
        count = torch.full((self.B,), -7, dtype=torch.int32, device=scratch.dev)
        status = torch.full((self.B,), 77, dtype=torch.int32, device=scratch.dev)
        rc = self.lib().dispu_poisson_disk_keep(self.B, self.N, _lib.ptr(d["points"]), _lib.ptr(d["radius"]), _lib.ptr(keep), _lib.ptr(count),
                                                scratch.ptr(), scratch.nbytes, _lib.ptr(status), self.stream(scratch))
        return self.finish(scratch, rc, dict(keep=keep, count=count, status=status), d)

    def check(self, out, variant, dev=None):
        import mesh_sample_oracle as SO
        pts = self.inputs(variant)["points"]
        want = np.stack([SO.poisson_keep(pts[c], np.float32(self.R[c])) for c in range(self.B)])
        assert not out["status"].any() and np.array_equal(out["keep"].astype(bool), want)
        assert np.array_equal(out["count"], want.sum(axis=1).astype(np.int32)) and 0.1 < want.mean() < 0.9


class GridSubsample(DenseCase):
    """dispu_grid_subsample_plan, then dispu_grid_subsample_emit over the same scratch, n = 3000 with two feature and two label columns:
    "reproduced bit for bit" against tests/grid_subsample_oracle.py; variant "a" has a coarser grid (fewer, longer runs)"""
    entries, queries = ("dispu_grid_subsample_plan", "dispu_grid_subsample_emit"), ("dispu_grid_subsample_scratch_bytes",)
    N, FD, LD = 3000, 2, 2

    def sizes(self):
        return self.lib().dispu_grid_subsample_scratch_bytes(self.N, self.FD, self.LD)

    def dl(self, variant):
        return 0.25 if variant == "a" else 0.07

    def inputs(self, variant):
        r = np.random.default_rng(_SEED[variant] + 9)
        return dict(points=r.random((self.N, 3)).astype(np.float32), features=r.standard_normal((self.N, self.FD)).astype(np.float32),
                    classes=r.integers(-2, 5, (self.N, self.LD)).astype(np.int32))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        L, dev = self.lib(), scratch.dev
        d = self.dev_inputs(scratch, variant)
        m, status = C.c_int(0), C.c_int(0)
        rc = L.dispu_grid_subsample_plan(self.N, _lib.ptr(d["points"]), self.dl(variant), scratch.ptr(), scratch.nbytes, C.byref(m), C.byref(status),
                                         None, self.stream(scratch))
        assert rc == 0 and status.value == 0 and 0 < m.value <= self.N
        op = torch.full((m.value, 3), 7.0, dtype=torch.float32, device=dev)
        of = torch.full((m.value, self.FD), 7.0, dtype=torch.float32, device=dev)
        oc = torch.full((m.value, self.LD), -7, dtype=torch.int32, device=dev)
        rc = L.dispu_grid_subsample_emit(self.N, m.value, self.FD, self.LD, _lib.ptr(d["points"]), _lib.ptr(d["features"]), _lib.ptr(d["classes"]),
                                         scratch.ptr(), scratch.nbytes, _lib.ptr(op), _lib.ptr(of), _lib.ptr(oc), self.stream(scratch))
        return self.finish(scratch, rc, dict(points=op, features=of, classes=oc), d)

    def check(self, out, variant, dev=None):
        import grid_subsample_oracle as O
        i = self.inputs(variant)
        op, of, oc = O.compute(i["points"], i["features"], i["classes"], self.dl(variant))
        assert same_bytes(out["points"], op) and same_bytes(out["features"], of) and same_bytes(out["classes"], oc)
        assert 100 < len(op) < self.N


class KnnXyz(DenseCase):
    """dispu_knn_xyz_ws at b = 2, n = 4097, m = 64, k = 16: the chunked path ("cut into chunks of <= 1024 candidates, searched by the
    wave-per-query kernel and merged ... Same results": indices and fp32 distances, identical bytes or wrong ones)"""
    entries, queries = ("dispu_knn_xyz_ws",), ("dispu_knn_xyz_scratch_bytes",)
    B, N, M, K_ = 2, 4097, 64, 16

    def sizes(self):
        return self.lib().dispu_knn_xyz_scratch_bytes(self.B, self.N, self.M, self.K_)

    def inputs(self, variant):
        return dict(support=dense_cloud(variant, self.B, self.N, 5), query=dense_cloud(variant, self.B, self.M, 6))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        idx = torch.full((self.B, self.M, self.K_), -7, dtype=torch.int32, device=scratch.dev)
        dist = torch.full((self.B, self.M, self.K_), 7.0, dtype=torch.float32, device=scratch.dev)
        rc = self.lib().dispu_knn_xyz_ws(self.B, self.N, self.M, self.K_, _lib.ptr(d["support"]), _lib.ptr(d["query"]), _lib.ptr(idx),
                                         _lib.ptr(dist), scratch.ptr(), scratch.nbytes, 0, self.stream(scratch))
        return self.finish(scratch, rc, dict(idx=idx, dist=dist), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        i = self.inputs(variant)
        widx, wdist = O.knn_batch(i["support"], i["query"], self.K_, return_dist=True)
        assert np.array_equal(out["idx"], widx) and np.array_equal(out["dist"], wdist)


class PoissonDiskSelect(PoissonDiskKeep):
    """dispu_poisson_disk_select, b = 2, n = 300, m = 60, 12 bisection steps: as dispu_poisson_disk_keep, "identical from run to run
    (no float atomics)" """
    entries, queries = ("dispu_poisson_disk_select",), ("dispu_poisson_disk_scratch_bytes",)
    M, STEPS = 60, 12

    def r_hi(self):
        return np.float32([4.0 * np.sqrt(1.0 / self.M)] * self.B)

    def inputs(self, variant):
        return dict(points=dense_cloud(variant, self.B, self.N, 3), r_hi=self.r_hi())

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        idx = torch.full((self.B, self.M), -7, dtype=torch.int32, device=scratch.dev)
        r_out = torch.full((self.B,), 7.0, dtype=torch.float32, device=scratch.dev)
        count = torch.full((self.B,), -7, dtype=torch.int32, device=scratch.dev)
        status = torch.full((self.B,), 77, dtype=torch.int32, device=scratch.dev)
        rc = self.lib().dispu_poisson_disk_select(self.B, self.N, self.M, self.STEPS, _lib.ptr(d["points"]), _lib.ptr(d["r_hi"]), _lib.ptr(idx),
                                                  _lib.ptr(r_out), _lib.ptr(count), scratch.ptr(), scratch.nbytes, _lib.ptr(status),
                                                  self.stream(scratch))
        return self.finish(scratch, rc, dict(idx=idx, r_out=r_out, count=count, status=status), d)

    def check(self, out, variant, dev=None):
        import mesh_sample_oracle as SO
        pts = self.inputs(variant)["points"]
        assert not out["status"].any()
        for c in range(self.B):
            widx, wr, wcount = SO.poisson_select(pts[c], self.M, self.r_hi()[c], self.STEPS)
            assert np.array_equal(out["idx"][c], widx) and out["count"][c] == wcount
            assert np.float32(out["r_out"][c]).tobytes() == np.float32(wr).tobytes()


class ApproxMatchLevelsWs(ApproxMatchWs):
    """dispu_approx_match_levels_ws: what it documents in `temp` is its only output ("the ten (ratioL, ratioR) vector pairs and pass 2's
    partial sums of the last level, byte for byte what dispu_approx_match_ws leaves there"; tests/test_emd_loss_gpu.py holds it to that,
    and so does check(), whose reference is therefore the library's other entry, held to the oracle in turn).  The ratioR row of the LAST level is not among the outputs: no launch stores it, every reader finishes it from
    pass 2's partials (csrc/approxmatch.hip: am_finish_col), so those m words per cloud keep whatever the caller's buffer held.  Nor are
    the b + 1 counter words at the end, which nothing writes or reads"""
    entries, queries = ("dispu_approx_match_levels_ws",), ("dispu_approx_match_scratch_bytes",)
    sentinels = {}
    LEVELS, CHUNK = 10, 128                                     # AM_LEVELS, AM_CH of csrc/approxmatch.hip

    def documented(self, body):
        """per cloud: remL[10][n] ratL[10][n] remR[10][m] ratR[10][m] p1 p3 p2 -> all of it but ratR[9]"""
        n, m = self.N, self.M
        per = 2 * self.LEVELS * (n + m) + 2 * ((m + self.CHUNK - 1) // self.CHUNK) * n + ((n + self.CHUNK - 1) // self.CHUNK) * m
        words = body[:4 * self.B * per].view(np.uint32).reshape(self.B, per)
        last = 2 * self.LEVELS * n + self.LEVELS * m + (self.LEVELS - 1) * m
        return np.ascontiguousarray(np.concatenate([words[:, :last], words[:, last + m:]], axis=1))

    def run(self, scratch, variant, short=False):
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        rc = self.lib().dispu_approx_match_levels_ws(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), scratch.ptr(),
                                                     scratch.nbytes - (1 if short else 0), self.ARITH, self.stream(scratch))
        out = self.finish(scratch, rc, {}, d)
        if not short:
            out["temp"] = self.documented(scratch.body())
        return out

    def check(self, out, variant, dev=None):
        full = Scratch(dev, self.sizes(), "zeros")
        ref = ApproxMatchWs().run(full, variant)
        assert ref["rc"] == 0 and same_bytes(out["temp"], self.documented(full.body()))
        ApproxMatchWs().check(ref, variant)


class EmdLossGrad(MatchCase):
    """dispu_emd_loss_grad (per-chunk partial gradients and costs in the scratch, combined in a fixed order; its test,
    tests/test_emd_loss_gpu.py, asserts "two runs bit-identical").  `temp` is what dispu_approx_match_levels_ws left on a zero-filled
    buffer of its own; dpred starts at zero.  The reference, as in that test and not independent of the library: tests/emd_oracle.py's
    float64 sums over the `match` dispu_approx_match_ws wrote for the same clouds; cost 1e-5 relative, dpred 1e-5 of max |reference|"""
    entries, queries = ("dispu_emd_loss_grad",), ("dispu_emd_loss_grad_scratch_bytes",)
    refuses = True
    sentinels = dict(cost=7.0, dpred=0.0)
    ARITH, COEF = 1 | 2, 10.0 * 0.5 / (2 * 200)

    def sizes(self):
        return self.lib().dispu_emd_loss_grad_scratch_bytes(self.B, self.N, self.M)

    def inputs(self, variant):
        return dict(MatchCase.inputs(self, variant), radius=np.linspace(0.5, 2.0, self.B).astype(np.float32))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        L, dev = self.lib(), scratch.dev
        d = self.dev_inputs(scratch, variant)
        nt = L.dispu_approx_match_scratch_bytes(self.B, self.N, self.M)
        temp = torch.zeros((nt,), dtype=torch.uint8, device=dev)
        rc = L.dispu_approx_match_levels_ws(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), _lib.ptr(temp), nt, self.ARITH,
                                            self.stream(scratch))
        assert rc == 0
        cost = torch.full((self.B,), 7.0, dtype=torch.float32, device=dev)
        dpred = torch.zeros((self.B, self.N, 3), dtype=torch.float32, device=dev)
        rc = L.dispu_emd_loss_grad(self.B, self.N, self.M, _lib.ptr(d["xyz1"]), _lib.ptr(d["xyz2"]), _lib.ptr(temp), _lib.ptr(d["radius"]), self.COEF,
                                   _lib.ptr(cost), _lib.ptr(dpred), scratch.ptr(), scratch.nbytes - (1 if short else 0), self.ARITH,
                                   self.stream(scratch))
        return self.finish(scratch, rc, dict(cost=cost, dpred=dpred), d)

    def check(self, out, variant, dev=None):
        import emd_oracle as EO
        import test_emd_loss_gpu as T
        i = self.inputs(variant)
        ref = ApproxMatchWs().run(Scratch(dev, ApproxMatchWs().sizes(), "zeros"), variant)
        assert ref["rc"] == 0
        want = EO.emd_value_grad(i["xyz1"], i["xyz2"], ref["match"], None)
        T.each_close(out["cost"], want["cost"], 1e-5, "emd cost")
        T.close(out["dpred"], (self.COEF / i["radius"].astype(np.float64))[:, None, None] * want["grad1"], 1e-5, "emd dpred")


class DiskUniformity(DenseCase):
    """dispu_disk_uniformity on the smallest fixture of tests/test_mesh_eval_ops_gpu.py with more than one wave of disks (S = 63,
    R = 2): that test asserts "run to run: bit-identical, scratch included".  The S R double terms and S R kept flags the entry leaves
    in the scratch are outputs (it fills all of it).  Variant "a": the same disks scored for another cloud size N, so other terms"""
    entries, queries = ("dispu_disk_uniformity",), ("dispu_disk_uniformity_scratch_bytes",)
    refuses = True
    sentinels = dict(out=7.0)
    S, R = 63, 2

    def N(self, variant):
        return 8192 if variant == "a" else 1100

    def sizes(self):
        return self.lib().dispu_disk_uniformity_scratch_bytes(self.S, self.R)

    def inputs(self, variant):
        import mesh_oracle as MO
        pts = MO.uniformity_points()
        rows = MO.uniformity_rows(self.S, pts.shape[0])
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        return dict(points=np.ascontiguousarray(pts, np.float32), offsets=off, members=np.concatenate(rows).astype(np.int32),
                    radii=np.ascontiguousarray(MO.UNI_RADII), pct=np.ascontiguousarray(MO.UNI_PCT), N=np.int64([self.N(variant)]))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        out = torch.full((self.R,), 7.0, dtype=torch.float64, device=scratch.dev)
        rc = self.lib().dispu_disk_uniformity(self.S, self.R, d["points"].shape[0], _lib.ptr(d["points"]), _lib.ptr(d["offsets"]),
                                              _lib.ptr(d["members"]), _lib.ptr(d["radii"]), _lib.ptr(d["pct"]), self.N(variant), scratch.ptr(),
                                              scratch.nbytes - (1 if short else 0), _lib.ptr(out), self.stream(scratch))
        res = self.finish(scratch, rc, dict(out=out), d)
        if not short:
            M = self.S * self.R
            body = scratch.body()
            res.update(term=body[:8 * M].view(np.float64).copy(), kept=body[8 * M:12 * M].view(np.int32).copy())
        return res

    def check(self, out, variant, dev=None):
        import mesh_oracle as MO
        import test_mesh_eval_ops_gpu as T
        i = self.inputs(variant)
        rows = MO.uniformity_rows(self.S, i["points"].shape[0])
        kept, term, mean = MO.uniform_terms(rows, MO.UNI_RADII, i["points"], MO.UNI_PCT, self.N(variant))
        assert np.array_equal(out["kept"], kept) and (out["term"][kept == 0] == 0.0).all()
        c = np.array([len(r) for r in rows], np.float64)
        tb = (c + 8.0) * T.U52 * np.abs(term)
        T.near(out["term"][kept != 0], term[kept != 0], tb[kept != 0], "uniformity terms")
        for j in range(self.R):
            sel = np.nonzero(kept[j::self.R])[0] * self.R + j
            assert sel.size
            T.near(out["out"][j:j + 1], mean[j:j + 1], (self.S + 8.0) * T.U52 * abs(mean[j]) + tb[sel].sum() / sel.size, "uniformity out[%d]" % j)


class GeodesicDistances(DenseCase):
    """dispu_geodesic_distances on the cube fixture of tests/geodesic_fixtures.py (one seed, 30 targets across an edge), window_cap
    4096 on every run: "Bit-identical run to run"; the status word is an output, so the stale and the all-ones run must agree on it.
    The scratch is the per-seed window arena (counter and vertex hash live in LDS).  Held to tests/geodesic_oracle.py at 1e-9
    relative, as tests/test_geodesic_gpu.py does"""
    entries, queries = ("dispu_geodesic_distances",), ("dispu_geodesic_scratch_bytes",)
    refuses = True
    sentinels = dict(dist=7.0, status=-7)
    CAP, MAXD = 4096, 4.0

    def fixture(self, variant):
        import geodesic_fixtures as GF
        return GF.cube_case(30, 0 if variant == "b" else 7)

    def sizes(self):
        return self.lib().dispu_geodesic_scratch_bytes(1, self.CAP)

    def inputs(self, variant):
        v, f, (sf, sb), t, tf, exp = self.fixture(variant)
        return dict(points=t.astype(np.float32), point_face=tf.astype(np.int32))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        from dispu_amd import mesh as M
        dev = scratch.dev
        v, f, (sf, sb), t, tf, exp = self.fixture(variant)
        mesh = M.Mesh(v, f, dev)
        T = mesh.geodesic_tables()
        d = self.dev_inputs(scratch, variant)
        fid, bary = M._seed_arrays(mesh, [sf], [sb])
        seed_pts = torch.from_numpy(mesh.surface_points(fid, bary).astype(np.float32)).to(dev)
        cand_off, cand = M.disk_members(seed_pts, d["points"], np.array([np.float32(self.MAXD * (1.0 + 2.0 ** -12))], np.float32))
        total = int(cand_off[1].item())
        assert total == 30
        dsf, dsb = torch.from_numpy(fid).to(dev), torch.from_numpy(np.ascontiguousarray(bary)).to(dev)
        dist = torch.full((total,), 7.0, dtype=torch.float64, device=dev)
        status = torch.full((1,), -7, dtype=torch.int32, device=dev)
        rc = self.lib().dispu_geodesic_distances(
            1, _lib.ptr(dsf), _lib.ptr(dsb), _lib.ptr(T["dev_verts64"]), _lib.ptr(T["dev_faces"]), _lib.ptr(T["dev_twin"]), _lib.ptr(T["dev_edge_geo"]),
            _lib.ptr(T["dev_pseudo"]), _lib.ptr(T["dev_fan_off"]), _lib.ptr(T["dev_fan"]), 30, _lib.ptr(d["points"]), _lib.ptr(d["point_face"]),
            _lib.ptr(cand_off), _lib.ptr(cand), self.MAXD, self.CAP, scratch.ptr(), scratch.nbytes - (1 if short else 0), _lib.ptr(dist),
            _lib.ptr(status), self.stream(scratch))
        out = self.finish(scratch, rc, dict(dist=dist, status=status), d)
        if not short:
            out["cand"] = _N(cand)                              # the candidate list the distances are aligned with
        return out

    def check(self, out, variant, dev=None):
        import geodesic_oracle as GO
        from dispu_amd import mesh as M
        v, f, (sf, sb), t, tf, exp = self.fixture(variant)
        mesh = M.Mesh(v, f, dev)
        assert out["status"].tolist() == [0] and np.array_equal(out["cand"], np.arange(30))
        ref = GO.geodesic(mesh.verts, mesh.faces, sf, sb, t.astype(np.float32), tf, self.MAXD)
        np.testing.assert_allclose(out["dist"], ref, rtol=1e-9, atol=0)
        np.testing.assert_allclose(out["dist"], exp, rtol=1e-5, atol=0)


class ProbSample(DenseCase):
    """dispu_prob_sample, the reference signature: temp is the reference's [b, n] floats (the cumulative sums, every one written) and
    no byte count; b = 2, n = 8193 (two scan chunks), m = 300: "cumulative sums bit-identical to the oracle's restatement"
    (tests/test_ops_gpu.py), and the sums left in temp are outputs"""
    entries, queries = ("dispu_prob_sample",), ()
    B, N, M = 2, 8193, 300

    def sizes(self):
        return self.B * self.N * 4

    def inputs(self, variant):
        rng = np.random.default_rng(_SEED[variant] + 77)
        w, r = rng.random((self.B, self.N)).astype(np.float32), rng.random((self.B, self.M)).astype(np.float32)
        r[:, 0], r[:, -1] = 0.0, 1.0
        return dict(weights=w, draws=r)

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        out = torch.full((self.B, self.M), -7, dtype=torch.int32, device=scratch.dev)
        rc = self.lib().dispu_prob_sample(self.B, self.N, self.M, _lib.ptr(d["weights"]), _lib.ptr(d["draws"]), scratch.ptr(), _lib.ptr(out),
                                          self.stream(scratch))
        res = self.finish(scratch, rc, dict(idx=out), d)
        res["temp"] = scratch.body().view(np.float32).reshape(self.B, self.N).copy()
        return res

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        i = self.inputs(variant)
        ro, rt = O.prob_sample(i["weights"], i["draws"], return_temp=True)
        assert np.array_equal(out["idx"], ro) and np.array_equal(out["temp"], rt)


# ---- the lattice and contour entries (csrc/reconstruct.hip): the small sphere of tests/test_reconstruct_gpu.py, 200 points at voxel 0.25 ----
RECON_N, RECON_H = 200, 0.25


@cached
def recon_stage(variant):
    """the oracle's stages on a 200-point sphere: points, occ, act (band 1), lat, corner"""
    import normals_oracle as NO
    import reconstruct_oracle as R
    p = np.ascontiguousarray(NO.sphere(RECON_N, seed=0 if variant == "b" else 31), np.float32)
    occ = R.occupied_voxels(p, RECON_H, 1)
    act = R.dilate(occ, 1)
    lat, corner = R.lattice(act)
    return dict(points=p, occ=occ, act=act, lat=lat, corner=corner)


class LatticeCase(DenseCase):
    refuses = True

    def i64(self, dev, m):
        import torch
        return torch.full((m,), -7, dtype=torch.int64, device=dev)


class LatticeVoxels(LatticeCase):
    """dispu_lattice_voxels: "Ordinary stores, no atomics, identical bytes from run to run" (the lattice entries' common line); the
    sorted unique voxel keys against reconstruct_oracle.occupied_voxels, exactly"""
    entries, queries = ("dispu_lattice_voxels",), ("dispu_lattice_voxels_scratch_bytes",)
    sentinels = dict(occ=-7, count=-7, status=-7)

    def sizes(self):
        return self.lib().dispu_lattice_voxels_scratch_bytes(RECON_N)

    def inputs(self, variant):
        return dict(points=recon_stage(variant)["points"])

    def run(self, scratch, variant, short=False):
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        occ, cnt, status = self.i64(scratch.dev, RECON_N), C.c_int(-7), C.c_int(-7)
        rc = self.lib().dispu_lattice_voxels(RECON_N, _lib.ptr(d["points"]), RECON_H, 1, _lib.ptr(occ), C.byref(cnt), C.byref(status), scratch.ptr(),
                                             scratch.nbytes - (1 if short else 0), self.stream(scratch))
        out = self.finish(scratch, rc, dict(occ=occ), d)
        out.update(count=np.int64(cnt.value), status=np.int64(status.value))
        return out

    def check(self, out, variant, dev=None):
        want = recon_stage(variant)["occ"]
        assert out["status"] == 0 and out["count"] == len(want) and np.array_equal(out["occ"][:len(want)], want)
        assert (out["occ"][len(want):] == -7).all()


class LatticeDilate(LatticeCase):
    """dispu_lattice_dilate on the first 40 occupied voxels of the sphere: identical bytes from run to run (as dispu_lattice_voxels);
    against reconstruct_oracle.dilate, exactly"""
    entries, queries = ("dispu_lattice_dilate",), ("dispu_lattice_dilate_scratch_bytes",)
    sentinels = dict(act=-7, count=-7)
    NOCC = 40

    def __init__(self, band):
        self.band = band                                        # 1: 27 keys per voxel; 3: 343, other pass and tile counts

    def nk(self):
        return self.NOCC * (2 * self.band + 1) ** 3

    def sizes(self):
        return self.lib().dispu_lattice_dilate_scratch_bytes(self.NOCC, self.band)

    def inputs(self, variant):
        return dict(occ=np.ascontiguousarray(recon_stage(variant)["occ"][:self.NOCC]))

    def run(self, scratch, variant, short=False):
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        act, cnt = self.i64(scratch.dev, self.nk()), C.c_longlong(-7)
        rc = self.lib().dispu_lattice_dilate(self.NOCC, _lib.ptr(d["occ"]), self.band, _lib.ptr(act), C.byref(cnt), scratch.ptr(),
                                             scratch.nbytes - (1 if short else 0), self.stream(scratch))
        out = self.finish(scratch, rc, dict(act=act), d)
        out.update(count=np.int64(cnt.value))
        return out

    def check(self, out, variant, dev=None):
        import reconstruct_oracle as R
        want = R.dilate(self.inputs(variant)["occ"], self.band)
        assert out["count"] == len(want) and np.array_equal(out["act"][:len(want)], want) and (out["act"][len(want):] == -7).all()


class LatticeCorners(LatticeCase):
    """dispu_lattice_corners on the first 300 active voxels of the sphere: identical bytes from run to run (as dispu_lattice_voxels);
    against reconstruct_oracle.lattice, exactly"""
    entries, queries = ("dispu_lattice_corners",), ("dispu_lattice_corners_scratch_bytes",)
    sentinels = dict(lat=-7, corner=-7, count=-7)
    NVOX = 300

    def sizes(self):
        return self.lib().dispu_lattice_corners_scratch_bytes(self.NVOX)

    def inputs(self, variant):
        return dict(act=np.ascontiguousarray(recon_stage(variant)["act"][:self.NVOX]))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        d = self.dev_inputs(scratch, variant)
        lat, cnt = self.i64(scratch.dev, 8 * self.NVOX), C.c_longlong(-7)
        corner = torch.full((self.NVOX, 8), -7, dtype=torch.int32, device=scratch.dev)
        rc = self.lib().dispu_lattice_corners(self.NVOX, _lib.ptr(d["act"]), _lib.ptr(lat), _lib.ptr(corner), C.byref(cnt), scratch.ptr(),
                                              scratch.nbytes - (1 if short else 0), self.stream(scratch))
        out = self.finish(scratch, rc, dict(lat=lat, corner=corner), d)
        out.update(count=np.int64(cnt.value))
        return out

    def check(self, out, variant, dev=None):
        import reconstruct_oracle as R
        lat, corner = R.lattice(self.inputs(variant)["act"])
        assert out["count"] == len(lat) and np.array_equal(out["lat"][:len(lat)], lat) and (out["lat"][len(lat):] == -7).all()
        assert np.array_equal(out["corner"], corner)


class ContourCount(LatticeCase):
    """dispu_contour_count on the sphere's whole lattice: identical bytes from run to run (as dispu_lattice_voxels).  Its outputs are
    held to the oracle the way tests/test_reconstruct_gpu.py does: dispu_contour_emit (which takes no scratch) on them gives
    reconstruct_oracle.reconstruct's vertices bit for bit and its faces exactly.  Variant "a": the same lattice, the values of another
    surface (a sphere of radius 0.7 about the origin), so other counts in the same places"""
    entries, queries = ("dispu_contour_count",), ("dispu_contour_count_scratch_bytes",)
    sentinels = dict(slot_number=-7, tri_start=-7, nverts=-7, nfaces=-7)

    def shape(self):
        st = recon_stage("b")
        return len(st["act"]), len(st["lat"])

    def sizes(self):
        return self.lib().dispu_contour_count_scratch_bytes(*self.shape())

    @staticmethod
    @cached
    def want():
        import reconstruct_oracle as R
        p = recon_stage("b")["points"]
        return R.reconstruct(p, p, RECON_H)

    def inputs(self, variant):
        import reconstruct_oracle as R
        st = recon_stage("b")
        if variant == "b":
            values = self.want()["f"]
        else:
            pos = R.lattice_positions(st["lat"], RECON_H).astype(np.float64)
            values = (np.linalg.norm(pos, axis=1) - 0.7).astype(np.float32)
        return dict(corner=st["corner"].astype(np.int32), values=np.ascontiguousarray(values, np.float32))

    def run(self, scratch, variant, short=False):
        import torch
        from dispu_amd import _lib
        nvox, nlat = self.shape()
        d = self.dev_inputs(scratch, variant)
        num = torch.full((7 * nlat,), -7, dtype=torch.int32, device=scratch.dev)
        start = torch.full((nvox,), -7, dtype=torch.int32, device=scratch.dev)
        nv, nf = C.c_longlong(-7), C.c_longlong(-7)
        rc = self.lib().dispu_contour_count(nvox, nlat, _lib.ptr(d["corner"]), _lib.ptr(d["values"]), _lib.ptr(num), _lib.ptr(start), C.byref(nv),
                                            C.byref(nf), scratch.ptr(), scratch.nbytes - (1 if short else 0), self.stream(scratch))
        out = self.finish(scratch, rc, dict(slot_number=num, tri_start=start), d)
        out.update(nverts=np.int64(nv.value), nfaces=np.int64(nf.value))
        return out

    def check(self, out, variant, dev=None):
        import torch
        from dispu_amd import _lib
        want, st = self.want(), recon_stage("b")
        nvox, nlat = self.shape()
        assert out["nverts"] == len(want["verts"]) and out["nfaces"] == len(want["faces"])
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        i = self.inputs(variant)
        lat, corner, f, num, start = T(st["lat"]), T(i["corner"]), T(i["values"]), T(out["slot_number"]), T(out["tri_start"])
        verts = torch.full((int(out["nverts"]), 3), -7.0, dtype=torch.float32, device=dev)
        faces = torch.full((int(out["nfaces"]), 3), -7, dtype=torch.int32, device=dev)
        rc = self.lib().dispu_contour_emit(nvox, nlat, RECON_H, _lib.ptr(lat), _lib.ptr(corner), _lib.ptr(f), _lib.ptr(num), _lib.ptr(start),
                                           int(out["nverts"]), int(out["nfaces"]), _lib.ptr(verts), _lib.ptr(faces), _lib.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        assert rc == 0 and same_bytes(_N(verts), want["verts"]) and np.array_equal(_N(faces), want["faces"])


class FpsSegments(DenseCase):
    """dispu_fps_segments on two segments either side of 4096 points (the wave path keeps its sorted permutation in the scratch), 64
    samples each: "The indices are those of dispu_fps_ws and dispu_fps_segments bit for bit" -- indices, identical bytes or wrong ones"""
    entries, queries = ("dispu_fps_segments",), ("dispu_fps_segments_scratch_bytes",)
    NS, MS_ = (4000, 4200), (64, 64)
    OFFS = None

    def offs(self):
        if type(self).OFFS is None:                             # kept alive: the entries read them through pointers
            type(self).OFFS = (np.concatenate([[0], np.cumsum(self.NS)]).astype(np.int32), np.concatenate([[0], np.cumsum(self.MS_)]).astype(np.int32))
        return type(self).OFFS

    def query(self, L):
        return L.dispu_fps_segments_scratch_bytes

    def sizes(self):
        off, moff = self.offs()
        return self.query(self.lib())(len(self.NS), _hp(off), _hp(moff))

    def inputs(self, variant):
        off, moff = self.offs()
        rng = np.random.default_rng(_SEED[variant] + sum(self.NS))
        return dict(xyz=rng.random((sum(self.NS), 3)).astype(np.float32), off=off, moff=moff)

    def call(self, L, d, out, status, scratch):
        from dispu_amd import _lib
        off, moff = self.offs()
        return L.dispu_fps_segments(len(self.NS), _lib.ptr(d["off"]), _lib.ptr(d["moff"]), _hp(off), _hp(moff), _lib.ptr(d["xyz"]), scratch.ptr(),
                                    scratch.nbytes, _lib.ptr(out), 1, self.stream(scratch))

    def run(self, scratch, variant, short=False):
        import torch
        d = self.dev_inputs(scratch, variant)
        out = torch.full((sum(self.MS_),), -1, dtype=torch.int32, device=scratch.dev)
        status = torch.full((len(self.NS),), 9, dtype=torch.int32, device=scratch.dev)
        rc = self.call(self.lib(), d, out, status, scratch)
        return self.finish(scratch, rc, dict(idx=out, status=status), d)

    def check(self, out, variant, dev=None):
        from oracle import oracle as O
        off, moff = self.offs()
        x = self.inputs(variant)["xyz"]
        for c, m in enumerate(self.MS_):
            want = O.farthest_point_sample(m, x[off[c]:off[c + 1]][None], contract=1)[0]
            assert np.array_equal(out["idx"][moff[c]:moff[c + 1]], want), c


class FpsSegmentsAuto(FpsSegments):
    """dispu_fps_segments_auto on one segment of 24577 points (the cell kernels) and one of 300, 64 samples each: indices, "bit for
    bit" those of dispu_fps_segments; the status words are outputs"""
    entries, queries = ("dispu_fps_segments_auto",), ("dispu_fps_segments_auto_scratch_bytes",)
    NS = (24577, 300)
    OFFS = None

    def query(self, L):
        return L.dispu_fps_segments_auto_scratch_bytes

    def call(self, L, d, out, status, scratch):
        from dispu_amd import _lib
        off, moff = self.offs()
        return L.dispu_fps_segments_auto(len(self.NS), _lib.ptr(d["off"]), _lib.ptr(d["moff"]), _hp(off), _hp(moff), _lib.ptr(d["xyz"]),
                                         scratch.ptr(), scratch.nbytes, _lib.ptr(out), _lib.ptr(status), 1, self.stream(scratch))

    def check(self, out, variant, dev=None):
        FpsSegments.check(self, out, variant, dev)
        assert not out["status"][0]                             # the served segment; the small one's word is the entry's to leave or write


# ---- training reductions: per-workgroup partials in the scratch, then a finalize kernel -----------------------------------------------------
class TrainCase(Case):
    """The entry's own test helper IS the case: it is given the scratch, runs the entry and holds every output to the float64 oracle
    (tests/train_ops_oracle.py or float64 autograd) at its file's tolerances, and asserts that its inputs keep their bits.  The header
    promises no identical bytes for these entries (several accumulate with float atomics), so every fill is held to those tolerances:
    run() raises where one is missed, and check() has nothing left to compare"""
    bit_identical = False
    seeds = {"a": 1000, "b": 0}                                 # "b": the helper's own inputs

    def lib(self):
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        return _lib.lib()

    def inputs(self, variant):                                  # the helper draws its arrays from this seed
        return dict(seed=np.int64([self.seeds[variant]]))

    def check_inputs(self, out, variant):                       # the helper asserted it (untouched())
        pass

    def check(self, out, variant, dev=None):
        assert out["rc"] == 0

    def run(self, scratch, variant, short=False):
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        self.helper(scratch.dev, _lib, scratch, self.seeds[variant])
        return dict(rc=0)


class BnTrain(TrainCase):
    """dispu_bn_train, then dispu_bn_train_grad over the same scratch, 1025 rows x 8 channels: one row into a second block of partials"""
    entries, queries = ("dispu_bn_train", "dispu_bn_train_grad"), ("dispu_bn_scratch_bytes",)

    def sizes(self):
        return self.lib().dispu_bn_scratch_bytes(1025, 8)

    def helper(self, dev, L, scratch, seed):
        import test_train_ops_gpu as T
        import train_ops_oracle as TO
        try:
            T.bn_both(dev, L, 1025, 8, 10, 10, 9, 11, 0, 1, 1, 0, scratch_buf=scratch, seed=seed)
        finally:
            TO.release()


class ActBiasGrad(TrainCase):
    """dispu_act_bias_grad with dbias, 1000 rows x 65 columns (a second trip of the column loop), ReLU mask, a separate dZ"""
    entries, queries = ("dispu_act_bias_grad",), ("dispu_act_bias_grad_scratch_floats",)

    def sizes(self):
        return 4 * self.lib().dispu_act_bias_grad_scratch_floats(1000, 65)

    def helper(self, dev, L, scratch, seed):
        import test_train_ops_gpu as T
        import train_ops_oracle as TO
        try:
            T.abg(dev, L, 1000, 65, 1, "sep", True, 0, (68, 65, 70), seed=5 + seed, scratch_buf=scratch)
        finally:
            TO.release()


class PsWnet(TrainCase):
    """dispu_ps_wnet_bn_stats, then dispu_ps_wnet_grad over the same scratch, 3 clouds of 100 points (300 rows x 16 pairs)"""
    entries, queries = ("dispu_ps_wnet_bn_stats", "dispu_ps_wnet_grad"), ("dispu_ps_wnet_scratch_bytes",)

    def sizes(self):
        return self.lib().dispu_ps_wnet_scratch_bytes(300)

    def helper(self, dev, L, scratch, seed):
        import test_train_fused_gpu as T
        try:
            T.test_wnet_bn_stats_and_grad(dev, L, 3, 100, scratch_buf=scratch, seed=seed)
        finally:
            del T._KEEP[:]


class EdgeDenseConvGrad(TrainCase):
    """dispu_edge_dense_conv_grad, then dispu_edge_dense_conv_grad_partials followed by dispu_edge_dense_conv_grad_reduce, all over one
    scratch: C = 24, 2 clouds of 256 points (64 tiles of partials); the two-halves form must give the one-launch weight gradients bit for
    bit, as tests/test_train_fused_gpu.py asserts"""
    entries = ("dispu_edge_dense_conv_grad", "dispu_edge_dense_conv_grad_partials", "dispu_edge_dense_conv_grad_reduce")
    queries = ("dispu_edge_dense_conv_grad_scratch_floats",)

    def sizes(self):
        return 4 * self.lib().dispu_edge_dense_conv_grad_scratch_floats(512, 24)

    def helper(self, dev, L, scratch, seed):
        import test_train_fused_gpu as T
        try:
            T.test_edge_dense_conv_grad(dev, L, 24, 2, 256, scratch_buf=scratch, seed=seed)
        finally:
            del T._KEEP[:]


# ---- the weight-gradient (TN) products: split partials in the scratch, then a reduction ------------------------------------------------------
class TnProduct(Case):
    """One case of tests/tn_paths.py whose plan has splits >= 2, through launch() of tests/test_tn_paths_gpu.py: "Deterministic:
    M-splits are summed in a fixed order from `scratch`".  Variant "b" is the table's small-integer data, held exactly to the integer
    reference (out and dbias); "a" its standard-normal data.  deferred: dispu_tn_defer arms the product, which then leaves its
    reduction to one dispu_tn_reduce_grouped call that reads the partials from the same scratch"""

    def __init__(self, fam, group, deferred=False):
        self.fam, self.group, self.deferred = fam, group, deferred
        entry = {"f32": "dispu_linear_tn", "bf16": "dispu_linear_tn_bf16s", "stream": "dispu_linear_tn_bf16_stream"}[fam]
        self.entries = (entry, "dispu_tn_reduce_grouped") if deferred else (entry,)
        self.queries = ({"f32": "dispu_linear_tn_scratch_floats", "bf16": "dispu_linear_tn_bf16_scratch_floats",
                         "stream": "dispu_linear_tn_bf16_stream_scratch_floats"}[fam],)

    def case(self):
        import tn_paths as TP
        c = next(c for c in TP.CASES if c.group == self.group and c.fam == self.fam and c.scratch == "exact" and c.bias and
                 c.lay == "al" and c.olay == "al" and TP.case_plan(c).splits >= 2)
        assert TP.case_plan(c).splits >= 2
        return c

    def sizes(self):
        import tn_paths as TP
        return 4 * TP.scratch_floats(self.case())

    def kind(self, variant):
        return "int" if variant == "b" else "flt"

    def inputs(self, variant):
        import tn_paths as TP
        X, Z, o0, b0 = TP.operands(self.case(), self.kind(variant))
        return dict(x=X, z=Z)

    def run(self, scratch, variant, short=False):
        import torch
        import dispu_amd  # noqa: F401
        from dispu_amd import _lib
        import test_tn_paths_gpu as T
        import tn_paths as TP
        c, dev = self.case(), scratch.dev
        ops = TP.operands(c, self.kind(variant))
        host, t, base = T.upload(dev, c, ops)
        if self.deferred:
            descs = (_lib.TnReduceDesc * 1)()
            p = T.launch(dev, _lib, c, t, base, desc=C.c_void_p(C.addressof(descs)), scratch_buf=scratch)
            assert descs[0].splits == p.splits and descs[0].part == scratch.ptr().value
            table = torch.frombuffer(bytearray(C.string_at(C.addressof(descs), C.sizeof(descs))), dtype=torch.uint8).to(dev)
            rc = _lib.lib().dispu_tn_reduce_grouped(1, C.c_void_p(C.addressof(descs)), C.c_void_p(table.data_ptr()), _lib.stream_ptr(dev))
        else:
            p, rc = T.launch(dev, _lib, c, t, base, scratch_buf=scratch), 0      # launch raises on a return code
        torch.cuda.synchronize(dev)
        assert p.splits >= 2
        win, db = T.collect(c, host, t)                          # also: nothing written round out and dbias
        lo = TP.layout(c)
        keep = lambda a, off, ld, stride, rows, cols: np.stack([np.lib.stride_tricks.as_strided(a[off + z * stride:], shape=(rows, cols), strides=(4 * ld, 4)).copy()
                                                                 for z in range(c.batch)])
        ins = {}
        if not (c.storage & 1):
            ins["x"] = keep(t["x"].cpu().numpy(), lo.xoff, lo.ldx, lo.sx, c.M, c.K)
        if not (c.storage & 2):
            ins["z"] = keep(t["z"].cpu().numpy(), lo.xoff * 0 + lo.zoff, lo.ldz, lo.sz, c.M, c.N)
        return self.with_inputs(dict(rc=rc, out=win, dbias=db), ins)

    def check_inputs(self, out, variant):
        want = self.inputs(variant)
        for k in ("x", "z"):
            if "in:" + k in out:
                assert same_bytes(out["in:" + k], want[k]), "input %s was written" % k

    def check(self, out, variant, dev=None):
        import tn_paths as TP
        c = self.case()
        want, wdb = TP.expected_int(c, TP.operands(c, "int"))
        assert np.array_equal(out["out"].astype(np.float64), want) and np.array_equal(out["dbias"].astype(np.float64), wdb)


CASES = {
    "pca_normals": Normals(),
    "orient_consistent": Orient(),
    "orient_consistent_host_rounds": OrientHostRounds(),
    "knn_mean_dist": MeanDist(),
    "radius_count": RadiusCount(),
    "compact": Compact(),
    "cluster": Cluster(),
    "knn_cross": KnnCross(),
    "transfer_attributes": Transfer(),
    "mls_project": Mls(),
    "icp": Icp(),
    "signed_distance": SignedDistance(),
    "fps_cells": FpsCells(),
    "poisson_cells_keep": PoissonKeep(),
    "poisson_cells_select": PoissonSelect(),
    "fps_ws": Fps(),
    "fps": FpsReference(),
    "knn_feat_strided_ws": KnnFeat(),
    "approx_match_ws": ApproxMatchWs(),
    "approx_match": ApproxMatchReference(),
    "match_cost_ws": MatchCostWs(),
    "match_cost_grad_ws": MatchCostGradWs(),
    "poisson_disk_keep": PoissonDiskKeep(),
    "poisson_disk_select": PoissonDiskSelect(),
    "knn_xyz_ws": KnnXyz(),
    "approx_match_levels_ws": ApproxMatchLevelsWs(),
    "prob_sample": ProbSample(),
    "emd_loss_grad": EmdLossGrad(),
    "disk_uniformity": DiskUniformity(),
    "geodesic_distances": GeodesicDistances(),
    "grid_subsample": GridSubsample(),
    "fps_segments": FpsSegments(),
    "fps_segments_auto": FpsSegmentsAuto(),
    "lattice_voxels": LatticeVoxels(),
    "lattice_dilate_band1": LatticeDilate(1),
    "lattice_dilate_band3": LatticeDilate(3),
    "lattice_corners": LatticeCorners(),
    "contour_count": ContourCount(),
    "bn_train": BnTrain(),
    "act_bias_grad": ActBiasGrad(),
    "ps_wnet": PsWnet(),
    "edge_dense_conv_grad": EdgeDenseConvGrad(),
    "linear_tn": TnProduct("f32", "f32/T11/int"),
    "linear_tn_bf16s": TnProduct("bf16", "bf16/128032/split"),
    "linear_tn_bf16_stream": TnProduct("stream", "stream/256/0"),
    "tn_defer_reduce_grouped": TnProduct("f32", "f32/T11/int", deferred=True),
    "radix_sort_bits9": RadixSort(9),
    "radix_sort_bits17": RadixSort(17),
}


def uncovered():
    """the size queries, and the `temp` takers without one, that no registered case exercises yet"""
    covered_q = {q for c in CASES.values() for q in c.queries}
    covered_e = {e for c in CASES.values() for e in c.entries}
    return sorted(set(QUERY_ENTRIES) - covered_q) + sorted(set(TEMP_TAKERS) - covered_e)
