"""Training data path: counterpart of DisPU/dataset.py (Fetcher :81-143, load_h5_data :52-78, normalize_point_cloud
:26-40) and of the augmentations of Common/point_operation.py it calls.

Same class / method names and the same numpy global-RNG call sequence as the reference (a run seeded with
np.random.seed reproduces the reference's batch order, sub-sampling, jitter, angles and scales -- including
next_batch's off-by-one, which skips the first batch of every epoch).  What differs: the patch arrays live in HBM
and every batch is produced by two device launches (row gather of the 256-of-1024 sub-sample through
dispu_group_point, then dispu_augment), returning device tensors ready for Trainer.train_step; the reference does
this in numpy on a background thread and feeds the result through a TF placeholder.

DeviceFetcher has the same surface but makes every per-batch draw on the device (one dispu_sample_batch launch per batch, Philox
draws keyed by seed / epoch / position): the reference's distributions, not numpy's sequence.  It is what the training loop uses.
"""
import numpy as np
import torch

from . import _lib


def nonuniform_sampling(num=4096, sample_num=1024):
    """Common/point_operation.py:10-18 (host RNG logic; index list only)."""
    sample = set()
    loc = np.random.rand() * 0.8 + 0.1
    while len(sample) < sample_num:
        a = int(np.random.normal(loc=loc, scale=0.3) * num)
        if a < 0 or a >= num:
            continue
        sample.add(a)
    return list(sample)


def load_patches(path, in_num=256, out_num=1024, random=True):
    """load_h5_data (dataset.py:52-78): returns (input, gt) arrays [n, P, 3].  HDF5 files are read through the HDF5 C
    library (dispu_amd.h5: ctypes binding, same library h5py wraps); .npz / .npy files with the same dataset names
    ('poisson_<num>') are read directly."""
    if path.endswith((".h5", ".hdf5")):
        from . import h5
        with h5.File(path) as f:
            gt = f["poisson_%d" % out_num]
            inp = gt if random else f["poisson_%d" % in_num]
    elif path.endswith(".npz"):
        z = np.load(path)
        gt = z["poisson_%d" % out_num]
        inp = gt if random else z["poisson_%d" % in_num]
    else:
        gt = np.load(path)
        inp = gt
    assert len(inp) == len(gt)
    return np.asarray(inp, np.float32), np.asarray(gt, np.float32)


class Fetcher(object):
    """Fetcher(opts-like values, arrays) with reset() / has_next_batch() / next_batch() -> (input[B,256,3],
    gt[B,1024,3], radius[B]) device tensors."""

    def __init__(self, input_patches, gt_patches, batch_size, patch_num_point=256, augment=True, shuffle=True, random=True,
                 jitter_sigma=0.01, jitter_max=0.03, device=None):
        self.device = torch.device(device if device is not None else "cuda:0")
        gt = np.asarray(gt_patches)
        inp = np.asarray(input_patches)
        # load_h5_data (dataset.py:70-74): one-time host preprocessing in the arrays' own dtype, same expression order
        # as the reference; both sets are normalised by the GROUND TRUTH's centroid / furthest distance
        centroid = np.mean(gt, axis=1, keepdims=True)
        pc = gt - centroid
        furthest = np.amax(np.sqrt(np.sum(pc ** 2, axis=-1, keepdims=True)), axis=1, keepdims=True)
        inp = inp - centroid
        self._input_host = np.ascontiguousarray(inp / furthest, np.float32)
        self._gt_host = np.ascontiguousarray(pc / furthest, np.float32)
        self.batch_size, self.patch_num_point = int(batch_size), int(patch_num_point)
        self.length = self._input_host.shape[0]
        self.augment, self.shuffle, self.random = augment, shuffle, random
        self.jitter_sigma, self.jitter_max = jitter_sigma, jitter_max
        self.reset()

    def __len__(self):
        return self.length

    def reset(self):
        self.idxs = np.arange(0, self.length)
        if self.shuffle:
            np.random.shuffle(self.idxs)
            self._input_host = self._input_host[self.idxs]
            self._gt_host = self._gt_host[self.idxs]
        self.input_data = torch.from_numpy(self._input_host).to(self.device)     # resident in HBM for the epoch
        self.gt_data = torch.from_numpy(self._gt_host).to(self.device)
        self.num_batches = (self.length + self.batch_size - 1) // self.batch_size
        self.batch_idx = 0

    def has_next_batch(self):
        return self.batch_idx < self.num_batches

    def next_batch(self):
        """dataset.py:118-143, same RNG draws in the same order."""
        L = _lib.lib()
        dev = self.device
        st = _lib.stream_ptr(dev)
        self.batch_idx += 1
        start = self.batch_idx * self.batch_size
        end = min((self.batch_idx + 1) * self.batch_size, self.length)
        bsize = max(end - start, 0)
        x = self.input_data[start:end].contiguous()
        gt = self.gt_data[start:end].contiguous()
        radius = torch.ones(bsize, dtype=torch.float32, device=dev)
        if self.random:
            if bsize != self.batch_size:
                raise IndexError("short batch (%d of %d): the reference fails here too (dataset.py:131-134 indexes "
                                 "batch_input_data[i] for i < batch_size)" % (bsize, self.batch_size))
            idx = np.stack([np.asarray(nonuniform_sampling(self.input_data.shape[1], sample_num=self.patch_num_point), np.int32)
                            for _ in range(self.batch_size)])
            didx = torch.from_numpy(idx).to(dev).view(bsize, self.patch_num_point, 1)
            sub = torch.empty((bsize, self.patch_num_point, 1, 3), dtype=torch.float32, device=dev)
            _lib.check(L.dispu_group_point(bsize, x.shape[1], 3, self.patch_num_point, 1, _lib.ptr(x), _lib.ptr(didx), _lib.ptr(sub), st),
                       "dispu_group_point")
            x = sub.view(bsize, self.patch_num_point, 3)
        if self.augment and bsize:
            n_in = x.shape[1]
            noise = np.clip(self.jitter_sigma * np.random.randn(bsize, n_in, 3), -1 * self.jitter_max, self.jitter_max)
            rot = np.empty((bsize, 3, 3))
            for k in range(bsize):
                angles = np.random.uniform(size=(3)) * 2 * np.pi           # three angles drawn, z rotation used (z_rotated=True)
                c, s = np.cos(angles[2]), np.sin(angles[2])
                rot[k] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
            scales = np.random.uniform(0.8, 1.2, bsize)
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
            dn, dr, ds = d(noise), d(rot.reshape(bsize, 9)), d(scales)
            xo, go = torch.empty_like(x), torch.empty_like(gt)
            _lib.check(L.dispu_augment(bsize, n_in, _lib.ptr(x), _lib.ptr(dn), _lib.ptr(dr), _lib.ptr(ds), None, _lib.ptr(xo), st), "dispu_augment")
            _lib.check(L.dispu_augment(bsize, gt.shape[1], _lib.ptr(gt), None, _lib.ptr(dr), _lib.ptr(ds), None, _lib.ptr(go), st), "dispu_augment")
            x, gt = xo, go
        return x, gt, radius


class DeviceFetcher(object):
    """Fetcher's surface (len / reset / has_next_batch / next_batch -> device (input, gt, radius)) with every per-batch draw made on
    the device: next_batch() is ONE launch of dispu_sample_batch (csrc/batch_sampler.hip) -- no host draw, no upload, no device-to-host
    copy.  The normalised dataset is uploaded once; reset() draws the epoch's row permutation on the host from
    np.random.Generator(PCG64(seed)), composes it onto the previous epoch's (the reference reshuffles its arrays in place,
    dataset.py:98-103) and uploads L int32 values.  A patch's sub-sample, jitter, rotation and scale are Philox draws keyed by
    (seed, epoch, position in the permutation): the batches of a (seed, epoch) do not depend on the batch size.  The distributions are
    the reference's, the draw sequence is not (Fetcher keeps numpy's for reference-reproducible runs).

    Kept from the reference: next_batch() pre-increments batch_idx, so the first batch of every epoch is skipped; a short batch
    raises.  The sampler's status word (candidate loop exhausted / bad permutation entry) is read once per epoch, in reset().

    shard=(rank, world): this process is one of `world` data-parallel ranks.  batch_size stays the GLOBAL batch B (it must divide by
    world); next_batch() draws the B / world patches at positions [batch_idx * B + rank * B / world, ...) of the epoch, i.e. rows
    [rank * B / world, (rank + 1) * B / world) of the unsharded fetcher's batch, bit for bit.  Everything else (len, the permutation
    stream, the skipped first batch, the short-batch error, the epoch counting) is that of the unsharded fetcher: ranks built with
    the same seed need no communication."""

    def __init__(self, input_patches, gt_patches, batch_size, patch_num_point=256, augment=True, shuffle=True, random=True,
                 jitter_sigma=0.01, jitter_max=0.03, device=None, seed=0, shard=None):
        self.shard = None
        if shard is not None:
            rank, world = int(shard[0]), int(shard[1])
            if world <= 0 or not 0 <= rank < world:
                raise ValueError("shard=(rank, world) needs 0 <= rank < world, got %r" % (tuple(shard),))
            if int(batch_size) % world:
                raise ValueError("the global batch of %d patches does not divide over %d ranks" % (int(batch_size), world))
            self.shard = (rank, world)
        self.device = torch.device(device if device is not None else "cuda:0")
        gt = np.asarray(gt_patches)
        inp = np.asarray(input_patches)
        # load_h5_data (dataset.py:70-74), exactly as Fetcher does it
        centroid = np.mean(gt, axis=1, keepdims=True)
        pc = gt - centroid
        furthest = np.amax(np.sqrt(np.sum(pc ** 2, axis=-1, keepdims=True)), axis=1, keepdims=True)
        self.batch_size, self.patch_num_point = int(batch_size), int(patch_num_point)
        self.length, self.gt_num_point = int(gt.shape[0]), int(gt.shape[1])
        self.augment, self.shuffle, self.random = bool(augment), bool(shuffle), bool(random)
        self.jitter_sigma, self.jitter_max = float(jitter_sigma), float(jitter_max)
        if self.patch_num_point > (self.gt_num_point if self.random else inp.shape[1]):
            raise ValueError("cannot draw %d distinct points from a patch of %d" % (self.patch_num_point,
                                                                                   self.gt_num_point if self.random else inp.shape[1]))
        if not self.random and inp.shape[1] != self.patch_num_point:
            raise ValueError("random=False needs input patches of patch_num_point = %d points, got %d" % (self.patch_num_point, inp.shape[1]))
        self.gt_data = torch.from_numpy(np.ascontiguousarray(pc / furthest, np.float32)).to(self.device)      # resident for the whole run
        self.input_data = None if self.random else torch.from_numpy(np.ascontiguousarray((inp - centroid) / furthest, np.float32)).to(self.device)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._rng = np.random.Generator(np.random.PCG64(self.seed))
        self._perm = np.arange(self.length, dtype=np.int64)
        self.perm = torch.zeros(self.length, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.epoch = -1
        self.reset()

    def __len__(self):
        return self.length

    def check_status(self):
        """the sampler's status word (one device-to-host copy; reset() calls this once per epoch)."""
        s = self.status.cpu().numpy()
        if s[0]:
            raise RuntimeError("dispu_sample_batch ran out of candidate rounds during epoch %d (the set was filled with the lowest "
                               "unused indices): %d of %d points is too dense for the rejection sampler" %
                               (self.epoch, self.patch_num_point, self.gt_num_point))
        if s[1]:
            raise RuntimeError("dispu_sample_batch met a permutation entry outside [0, %d)" % self.length)

    def status_flags(self):
        """the sampler's two status words as they are on the device (int32 [2], no copy, nothing raised): a data-parallel loop
        gathers every rank's and decides for all of them (train.fit_parallel)."""
        return self.status

    def reset(self):
        if self.epoch >= 0:
            self.check_status()
        if self.shuffle:
            self._perm = self._perm[self._rng.permutation(self.length)]
        self.perm.copy_(torch.from_numpy(self._perm.astype(np.int32)))
        self.epoch += 1
        self.num_batches = (self.length + self.batch_size - 1) // self.batch_size
        self.batch_idx = 0

    def has_next_batch(self):
        return self.batch_idx < self.num_batches

    def next_batch(self, verify=False):
        """-> (input [B, P, 3], gt [B, G, 3], radius [B]); verify=True adds a dict of the kernel's verification outputs (tests)."""
        B, P, G = self.batch_size, self.patch_num_point, self.gt_num_point
        self.batch_idx += 1
        start = self.batch_idx * B
        bsize = max(min((self.batch_idx + 1) * B, self.length) - start, 0)
        if bsize != B:
            raise IndexError("short batch (%d of %d): the reference fails here too (dataset.py:131-134 indexes "
                             "batch_input_data[i] for i < batch_size)" % (bsize, B))
        if self.shard is not None:                       # this rank's rows of the global batch
            B //= self.shard[1]
            start += self.shard[0] * B
        dev = self.device
        buf = torch.empty(B * (P + G) * 3 + B, dtype=torch.float32, device=dev)       # one allocation, three views
        x, gt, radius = buf[:B * P * 3].view(B, P, 3), buf[B * P * 3:B * (P + G) * 3].view(B, G, 3), buf[B * (P + G) * 3:]
        v = None
        if verify:
            v = dict(idx=torch.empty((B, P), dtype=torch.int32, device=dev), rot=torch.empty((B, 9), device=dev),
                     scale=torch.empty(B, device=dev), noise=torch.empty((B, P, 3), device=dev) if self.augment else None,
                     raw=torch.empty((B, 4), dtype=torch.int32, device=dev))
        q = (lambda k: _lib.ptr(v[k])) if verify else (lambda k: None)
        _lib.check(_lib.tape_lib().dispu_sample_batch(
            self.length, G, P, _lib.ptr(self.gt_data), _lib.ptr(self.input_data), _lib.ptr(self.perm), start, B, self.seed, self.epoch,
            self.jitter_sigma, self.jitter_max, int(self.augment), _lib.ptr(x), _lib.ptr(gt), _lib.ptr(radius), _lib.ptr(self.status),
            q("idx"), q("rot"), q("scale"), q("noise"), q("raw"), _lib.stream_ptr(dev)), "dispu_sample_batch")
        return (x, gt, radius, v) if verify else (x, gt, radius)
