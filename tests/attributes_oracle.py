"""numpy restatement of the cross-cloud k-NN and the attribute transfer (include/dispu_hip.h: dispu_knn_cross_segments,
dispu_transfer_attributes_segments; csrc/attributes.hip) for one segment: the yardstick of the attribute tests.
d2 = ((dx*dx + dy*dy) + dz*dz) with every operation rounded to fp32, the neighbour order is the order of the keys
(d2 bits << 32 | reference index), and the weights are float64 operations added in an explicit loop in ascending rank."""
import numpy as np


def sqdist_cross(q, r):
    """[len(q), len(r)] fp32: d2 in the kernel's order, one rounding per operation"""
    q, r = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(r, np.float32)
    with np.errstate(over="ignore"):
        dx = q[:, None, 0] - r[None, :, 0]
        dy = q[:, None, 1] - r[None, :, 1]
        dz = q[:, None, 2] - r[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def knn_cross(q, r, k, chunk=512):
    """-> (idx [len(q), k] int32, d2 [len(q), k] fp32): the k' = min(k, len(r)) smallest keys (d2 bits << 32 | index) of every query in
    ascending order, -1 / +inf beyond k'"""
    q, r = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(r, np.float32)
    nq, m = q.shape[0], r.shape[0]
    kp = min(k, m)
    idx = np.full((nq, k), -1, np.int32)
    d2o = np.full((nq, k), np.inf, np.float32)
    ar = np.arange(m, dtype=np.uint64)[None, :]
    for lo in range(0, nq, chunk):
        hi = min(nq, lo + chunk)
        d2 = sqdist_cross(q[lo:hi], r)
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ar
        keys = np.sort(keys, axis=1)[:, :kp]
        idx[lo:hi, :kp] = (keys & np.uint64(0xFFFFFFFF)).astype(np.int32)
        d2o[lo:hi, :kp] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2o


def transfer_from_knn(idx, d2, feat, mode="idw"):
    """[nq, F] fp32 from knn_cross's output: idw -- w_j = 1.0 / max((double)d2_j, 1e-10), den = sum w_j, num_f = sum w_j * (double)feat,
    both in ascending rank, out = (float)(num_f / den); nearest -- the row of rank 0"""
    feat = np.ascontiguousarray(feat, np.float32)
    if mode == "nearest":
        return feat[idx[:, 0]].copy()
    assert mode == "idw"
    nq, k = idx.shape
    den = np.zeros(nq, np.float64)
    num = np.zeros((nq, feat.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        for j in range(k):                                      # ascending rank, one double operation each
            live = idx[:, j] >= 0
            if not live.any():
                break
            w = np.float64(1.0) / np.maximum(d2[:, j].astype(np.float64), np.float64(1e-10))
            row = feat[np.where(live, idx[:, j], 0)].astype(np.float64)
            den = np.where(live, den + w, den)
            num = np.where(live[:, None], num + w[:, None] * row, num)
        return (num / den[:, None]).astype(np.float32)


def transfer(q, r, feat, k=3, mode="idw"):
    idx, d2 = knn_cross(q, r, k)
    return transfer_from_knn(idx, d2, feat, mode)


def nearest_label(q, r, labels):
    idx, _ = knn_cross(q, r, 1)
    return np.ascontiguousarray(labels, np.int32)[idx[:, 0]]
