"""Dis-PU training step on MI355X: generator forward in training mode, the reference's loss, hand-written backward,
gradient all-reduce and Adam.

Counterpart of DisPU/model.py: `Model.build_model` (:68-87: coarse/fine = G(input); pu_loss = 1000 CD(coarse) +
weight_fine(epoch) * 1000 CD(fine) + repulsion_w * repulsion(fine)), `setup_optimizer` (:158-178: staircase LR decay
over epochs, Adam beta1 = opts.beta on every generator variable) and the per-batch body of `train` (:215-232).
The reference obtains gradients from TF1 autodiff; here every backward op is an explicit C-ABI launch
(include/dispu_hip.h, "training step").  torch supplies device memory, the stream and torch.distributed only.
The Trainer names the layers and their order; which GEMM entry a dense product goes to is decided in products.py (Products),
where and when a launch is submitted in schedule.py (StepSchedule).

Execution differences from the reference (not results):
  * parameters, gradients and both Adam moments live in four flat fp32 buffers (1.05 M floats each): ONE RCCL
    all-reduce and ONE Adam launch per step;
  * concat / tile tensors are column slices of wide buffers (the dense blocks' edge tensor is one
    [B*N*16, 72+2C] matrix whose slices are the inputs and outputs of l0/l1/l2), their gradients likewise;
  * duplicate_up's 482-wide conv is evaluated per source point (as in inference) and differentiated in that form.
Training-mode forward values equal the inference path's except for BatchNorm (batch statistics here).
"""
import collections
import contextlib
import ctypes
import math
import os
import weakref
from collections import OrderedDict
from functools import partial

import numpy as np
import torch

from . import _lib
from ._util import f32, req
from .generator import BN_EPS, DENSE_BLOCKS, GROWTH, K_NEIGH, _Opts, gen_grid
from .products import Products, _p
from .schedule import StepSchedule

BN_DECAY = 0.95      # DisPU/generator.py:39 bn_decay
BN = "refine/PointShuffle/weight_net/wconv0/bn/"
BN_CH = 16            # its channels (the weight net's 3 -> 16 conv, Common/ops.py:181-191)
FE, UP, CS = "generator/feature_extraction_coarse/", "generator/upshuffle_0/", "generator/coarse_coordinate_regressor/"      # scopes
PS, FS = "refine/PointShuffle/", "refine/fine_coordinate_regressor/"

Path = collections.namedtuple("Path", "stem after_split defer_side attention local_bwd split_skip")      # see Trainer.path


def _dense_blocks():
    """(d, C, col, in_col, width) of every dense block: C input channels, its 3 * GROWTH + C output columns feat[:, col:in_col] --
    the features accumulate right-to-left inside feat[:, 0:480], so block d reads feat[:, in_col:480] (through its prep conv)"""
    rows, col = [], 456
    for d, C in enumerate([24] + [48] * (DENSE_BLOCKS - 1), 1):
        rows.append((d, C, col - 3 * GROWTH - C, col, 3 * GROWTH + C))
        col = rows[-1][2]
    assert col == 0
    return tuple(rows)


BLOCKS = _dense_blocks()


class TrainOpts(_Opts):
    """the training-side defaults of DisPU/configs.py"""
    base_lr_g = 0.001
    beta = 0.9
    lr_decay = True
    decay_step = 30
    lr_decay_rate = 0.7
    lr_clip = 1e-6
    use_repulse = True
    repulsion_w = 1.0
    use_uniform = False   # model.py:86 (the get_uniform_loss line ships commented out)
    uniform_w = 10.0      # DisPU/configs.py:42
    use_emd = False       # model.py:77 (the dis_fine_emd line ships commented out)
    emd_w = 10.0          # model.py:77, the literal in front of earth_mover (configs.py has no flag for it)


def weight_fine(epoch):
    """model.py:52-54 piecewise_constant(epoch, [10, 20, 30], [0.01, 0.1, 0.5, 1.0])."""
    return 0.01 if epoch <= 10 else 0.1 if epoch <= 20 else 0.5 if epoch <= 30 else 1.0


def learning_rate(opts, epoch):
    """model.py:160-170."""
    lr = opts.base_lr_g
    if opts.lr_decay:
        lr = max(opts.base_lr_g * opts.lr_decay_rate ** math.floor(epoch / opts.decay_step), opts.lr_clip)
    return lr


class _Step(object):
    """What forward() leaves for loss_backward(), _recompute_pair_tensors() and backward(): the shape, the input, the workspace, the path
    (Trainer.path) and the two flags of the current forward."""
    __slots__ = ("B", "N", "M", "rn", "rm", "x", "ws", "path", "coarse", "dcoarse", "dfine", "fresh", "stash_ready")

    def __init__(self, B, N, up, x, ws, path):
        self.B, self.N, self.M, self.rn, self.rm = B, N, N * up, B * N, B * N * up
        self.x, self.ws, self.path = x, ws, path
        self.coarse, self.dcoarse, self.dfine = (ws[k].view(self.rm, 3) for k in ("coarse", "dcoarse", "dfine"))    # as row matrices
        self.fresh = True                 # until the first backward(): the atomics accumulators (dprep, dup128s) are zero-filled for exactly ONE
        self.stash_ready = False          # the pair tensors of the local cell's backward are in place (_recompute_pair_tensors)


def _attr_of(owner, name):                               # a Trainer switch that lives on its StepSchedule / its Products
    return property(lambda self: getattr(getattr(self, owner), name), lambda self, v: setattr(getattr(self, owner), name, v))


class Trainer(object):
    """Trainer(opts, params).train_step(input[B,N,3], gt[B,4N,3], radius[B]) -> dict of loss terms.

    `params`: the same name -> array mapping Generator.load_params takes (oracle/generator.py:layer_shapes names)."""

    def __init__(self, opts=None, params=None, device=None, process_group=None, dtype="f32", comm_thread=None, collectives_at_world_1=False):
        """dtype "f32": the reference's arithmetic (every product on the fp32 matrix pipe, bit-equal to an fmaf chain).
        dtype "bf16" (BASELINE configs[4]): mixed precision -- master weights, activations and gradients stay fp32 in HBM,
        the dense products (forward, dX, dW) round their operands to bf16 and run on v_mfma_f32_32x32x16_bf16 with fp32
        accumulation (csrc/linear_bf16.hip); the 3-wide coordinate heads, the loss, BatchNorm, softmax and Adam stay fp32."""
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        self.dtype = dtype
        self.bf16 = dtype == "bf16"
        self.opts = opts if opts is not None else TrainOpts()
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type == "cuda" and self.device.index is None:       # torch.device("cuda") != torch.device("cuda:0")
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.up_ratio = int(self.opts.up_ratio)
        if self.up_ratio != 4:
            raise NotImplementedError("the shipped generator graph is built for up_ratio 4")
        self.pg = process_group
        self.epoch = 0
        self.global_step = 0
        self._ws = {}
        self._bn_scratch = None
        self._step = None                     # the current forward's record (_Step)
        self._tapes = {}
        self._ar = None                       # parallel.BucketedAllReduce over flat_g (data parallel only, see _reducer)
        self._ar_armed = False                # True inside train_step(): backward() may start a bucket's all-reduce as soon as it is complete
        # a ONE-rank process group normally means "no collectives".  True keeps them (a 1-rank RCCL communicator executes the real
        # stream / event ordering of the data-parallel step: the dry run of tests/test_distributed_gpu.py on the one GPU a test box has)
        self.collectives_at_world_1 = bool(collectives_at_world_1)
        # None: the transport's default (RCCL: the launching thread enqueues the collectives).  True: a background thread does -- the step
        # is launch-bound at 8 patches per GPU and a collective call costs ~30 us of host time (parallel._Lane)
        self.comm_thread = comm_thread

        # ---- switches: each default is the measured best; the other value is the reference side of a test (profiles/EXPERIMENTS.md
        # lists the switches that were removed once measurements had settled them)
        # (overlap_dw, dw_streams, group_reduce and defer_side live on the step's schedule, schedule.StepSchedule: the properties below)
        # overlap_dw: weight-gradient products (dW = X^T dZ) are off the backward chain: only Adam reads them.  They run on a second
        # HIP stream next to the dX products that ARE the chain (both read dZ; at 8 patches neither fills 256 CUs alone).
        # dw_streams: side streams the weight-gradient products are spread over (round-robin)
        # group_reduce: the split reductions of the weight-gradient products are not launched one by one: every product describes the
        # reduction it left undone (dispu_tn_defer) and a stream's descriptors run as ONE launch when that stream is joined (join,
        # _bucket_point): ~20 launches of 4 - 25 us per step become 3.  False: every product reduces itself (bit-identical)
        # defer_side: side work is submitted behind the chain's kernels (set by forward() from the batch size, see StepSchedule)
        self.sched = StepSchedule(self.device, overlap_dw=True, dw_streams=2, defer_side=True, group_reduce=True)
        # non-local cell: flash-style attention forward (+ per-row log-sum-exp) and a recomputing backward (csrc/attention_train.hip);
        # False = round 3's path through a materialised [B, M, M] probability tensor (the parity twin)
        self.flash_attn = True
        # the local cell's backward (feature x weight gradient, conv1's dX, conv0's gather) as ONE recomputing launch (csrc/ps_local_bwd.hip,
        # fp32 storage only): h1 / dz0 / wv / the inverted neighbour graph never exist in HBM.  Correct and tested, but 40 us slower per 8-patch
        # step than the five-launch path (1.595 vs 1.555 ms): OFF by default
        self.fused_local_bwd = False
        # the dense products: their GEMM entries, bf16 weight images and per-stream scratch (bf16_stream, bf16_min_macs: the properties below)
        inv = weakref.WeakMethod(self._invalidate_recordings)     # weak: no cycle keeps a dropped Trainer's device memory until the collector runs
        self.prod = Products(self.device, self.sched, self.bf16, lambda: inv()())
        self.P = None
        if params is not None:
            self.load_params(params)

    overlap_dw, dw_streams, group_reduce, defer_side = (_attr_of("sched", n) for n in ("overlap_dw", "dw_streams", "group_reduce", "defer_side"))
    bf16_stream, bf16_min_macs, _scratch = (_attr_of("prod", n) for n in ("bf16_stream", "bf16_min_macs", "scratch"))
    st = property(lambda self: self.sched.st)            # the stream pointer the launches go to

    # --------------------------------------------------------------------------------------------- parameters ----
    def _invalidate_recordings(self):
        """Launch tapes hold RAW device pointers (flat parameter / gradient / moment buffers, W^T copies,
        scratch, workspaces).  Whenever one of those buffers is re-allocated every recording is dropped, so the next
        train_step_taped records afresh instead of replaying launches onto freed memory.  The bf16 images of the weights
        (Products.packs) are keyed by the weight's address: dropped with the tapes that point at them."""
        self._tapes.clear()
        # the schedule's device copies of reduction tables: only tapes (dropped above) and the step being recorded point at them; a moved
        # scratch buffer makes new table contents anyway
        if self.prod.packs or self.sched.tables:
            torch.cuda.synchronize(self.device)
        self.prod.packs.clear()
        self.sched.drop_tables()

    def load_params(self, params):
        dev = self.device
        self._invalidate_recordings()
        self._ws.clear()
        if self._ar is not None:              # the reducer holds views of the old gradient buffer
            self._ar.close()
            self._ar = None
        names = [k for k in params if k.endswith(("/weights", "/biases", "/gamma", "/beta"))]
        sizes = [int(np.asarray(params[k]).size) for k in names]
        # every tensor starts on a 16-byte boundary inside the flat buffers
        offs, total = [], 0
        for s in sizes:
            offs.append(total)
            total += (s + 3) & ~3
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        # gradients and, behind them, the 2 x 16 BatchNorm moving statistics in ONE buffer: data parallel, both are reduced over the
        # replicas by the same two bucket collectives (a collective call costs ~30 us of host time whatever its size -- two more for
        # 128 bytes of statistics were 4 % of the 8-patch step, tests/test_distributed_gpu.py:test_rccl_branch_on_one_rank)
        self._red = torch.zeros(total + 2 * BN_CH, dtype=torch.float32, device=dev)
        self.flat_g = self._red[:total]
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        self.P, self.G, self.names = OrderedDict(), OrderedDict(), names
        for k, o, s in zip(names, offs, sizes):
            shp = np.asarray(params[k]).shape
            self.P[k] = self.flat_p[o:o + s].view(shp)
            self.G[k] = self.flat_g[o:o + s].view(shp)
            self.P[k].copy_(torch.from_numpy(np.ascontiguousarray(params[k], np.float32)))
        # W^T copies for the dX products (refreshed once per step by ONE launch, csrc/train_fused.hip:transpose_batched_kernel):
        # every 2-D weight whose transposed rows stay 16-byte aligned (K % 4 == 0)
        self.flat_pT = torch.zeros_like(self.flat_p)
        self.PT, desc = OrderedDict(), []
        for k, o, s in zip(names, offs, sizes):
            shp = np.asarray(params[k]).shape
            if k.endswith("/weights") and len(shp) == 2 and shp[0] % 4 == 0 and shp[1] % 4 == 0 and shp[0] >= 16:
                self.PT[k] = self.flat_pT[o:o + s].view(shp[1], shp[0])
                desc += [o, shp[0], shp[1]]
        self._t_desc = torch.tensor(desc, dtype=torch.int32, device=dev)
        self._stats = self._red[total:]
        self.moving_mean, self.moving_var = self._stats[:BN_CH], self._stats[BN_CH:]
        self.moving_mean.copy_(torch.from_numpy(np.ascontiguousarray(params[BN + "moving_mean"], np.float32)))
        self.moving_var.copy_(torch.from_numpy(np.ascontiguousarray(params[BN + "moving_variance"], np.float32)))
        self.grid = torch.from_numpy(gen_grid(self.up_ratio)).to(dev)
        self.adam_t = 0
        # data parallel: the reducer (and, under gloo, its lane's process group -- dist.new_group is a collective) is built HERE, where
        # every rank passes in the same order, not lazily inside whichever of train_step / all_reduce_grads a rank reaches first
        self._reducer()

    def params(self):
        """current parameters as the name -> numpy mapping Generator.load_params / the oracle take."""
        out = OrderedDict((k, v.detach().cpu().numpy().copy()) for k, v in self.P.items())
        out[BN + "moving_mean"] = self.moving_mean.cpu().numpy().copy()
        out[BN + "moving_variance"] = self.moving_var.cpu().numpy().copy()
        return out

    def grads(self):
        return OrderedDict((k, v.detach().cpu().numpy().copy()) for k, v in self.G.items())

    # ---------------------------------------------------------------------------------------------- workspace ----
    def _workspace(self, B, N):
        key = (B, N)
        if key in self._ws:
            return self._ws[key]
        dev, f32, i32 = self.device, torch.float32, torch.int32
        M = N * self.up_ratio
        rn, rm, k = B * N, B * M, K_NEIGH
        E = lambda *shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
        Z = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
        pt = torch.bfloat16 if self.bf16 else f32      # storage type of the pair tensors / dF'
        ws = dict(
            feat=E(rn, 480), dfeat=E(rn, 480),
            prep=[None, None] + [E(rn, 48) for _ in range(2, DENSE_BLOCKS + 1)],
            # zero-filled once per step, off the chain (atomics accumulate into them): the dense blocks' input gradients (one per block:
            # the dW products on the side streams read them) and the skip branch's share of d(up128)
            zeroed=E((DENSE_BLOCKS - 1) * rn * 48 + rm * 128),
            kidx=[None] + [E(rn, k + 1, dtype=i32) for _ in range(DENSE_BLOCKS)],
            h256=E(rn, 256), dh256=E(rn, 256), gcode=E(rm, 2),
            up256=E(rm, 256), dup256=E(rm, 256), up128=E(rm, 128), dup128=E(rm, 128),
            c256=E(rm, 256), dc256=E(rm, 256), c64=E(rm, 64), dc64=E(rm, 64), coarse=E(B, M, 3), dcoarse=E(B, M, 3),
            psidx=E(rm, k, dtype=i32), inv_off=E(B, M + 1, dtype=i32), inv=E(B, M * k, dtype=i32),
            gmax=Z(rm, 144), dgmax=E(rm, 136), skip=E(rm, 256), dskip=E(rm, 256),
            # local cell: conv0 per source point (G, A), the pair tensors h0 / h1 / wv are RECOMPUTED for the backward pass
            gm=E(rm, 128), am=E(rm, 128), dG=E(rm, 128), dAneg=E(rm, 128),
            # (dtype "bf16": stored as bf16 -- the GEMMs that read them round their operands to bf16 anyway)
            h0=E(rm * k, 128, dtype=pt), h1=E(rm * k, 128, dtype=pt), dz1=E(rm * k, 128, dtype=pt), dz0=E(rm * k, 128, dtype=pt),
            wv=E(rm * k, 16), dwv=E(rm * k, 16),
            bn_stats=E(48), bn_scale=E(16), bn_shift=E(16), bn_sums=E(32),
            hp=E(rm, 2048), dhp=E(rm, 2048, dtype=pt), aft=E(rm, 256), daft=E(rm, 256),
            kv=E(rm, 128), dkv=E(rm, 128), q=E(rm, 64), dq=E(rm, 64), att=E(rm, 64), datt=E(rm, 64), lse=E(rm), dvec=E(rm),
            S=None if self.flash_attn else E(B, M, M), dS=None if self.flash_attn else E(B, M, M),
            nl=E(rm, 256), dnl=E(rm, 256), sum=E(rm, 256), agg=E(rm, 256), dagg=E(rm, 256),
            f256=E(rm, 256), df256=E(rm, 256), f64=E(rm, 64), df64=E(rm, 64), z=E(rm, 3), dz=E(rm, 3), fine=E(B, M, 3), dfine=E(B, M, 3),
            # loss
            cd=[dict(d_gt=E(B, M), i_gt=E(B, M, dtype=i32), d_pred=E(B, M), i_pred=E(B, M, dtype=i32), g_gt=E(B, M), g_pred=E(B, M),
                     dgt_unused=E(B, M, 3), rowmean=E(B), rowmax=E(B)) for _ in range(2)],      # one set per Chamfer term
            ball=E(B, M, 20, dtype=i32), ball_cnt=E(B, M, dtype=i32), rep=E(B, M), rowmean=E(B), rowmax=E(B),
            loss_vals=Z(9), r07=torch.full((B,), 0.07, dtype=f32, device=dev), zeros=Z(1))
        ws["dprep"] = [None, None] + [ws["zeroed"][i * rn * 48:(i + 1) * rn * 48].view(rn, 48) for i in range(DENSE_BLOCKS - 1)]
        ws["dup128s"] = ws["zeroed"][(DENSE_BLOCKS - 1) * rn * 48:].view(rm, 128)
        # grid code of duplicate_up: row (cloud*up + r)*N + i carries grid[r]
        ws["gcode"].view(B, self.up_ratio, N, 2).copy_(self.grid.view(1, self.up_ratio, 1, 2).expand(B, self.up_ratio, N, 2))
        self._ws[key] = ws
        return ws

    def _zero(self, t):
        """t.zero_() on the stream launches currently go to, as a memset through the library (a plain C call: tape-able, and cheaper
        than the torch op)."""
        L = _lib.tape_lib()
        st = self.st if self.st is not None else _lib.stream_ptr(self.device)
        _lib.check(L.dispu_memset_async(_lib.C.c_void_p(t.data_ptr()), 0, t.numel() * t.element_size(), st), "memset")

    # ----------------------------------------------------------------------------------------------- helpers ----
    def _lin(self, X, xoff, K, wname, act, Y, yoff, N, M=None, bias=True, W=None, woff=0):
        """Y[:, yoff:yoff+N] = act(X[:, xoff:xoff+K] . W + b)"""
        W = self.P[wname + "/weights"] if W is None else W
        self.prod.linear(X.shape[0] if M is None else M, K, N, X, xoff, W, woff, 0, self.P[wname + "/biases"] if bias else None, act, Y, yoff)

    def _lin_bwd(self, X, xoff, K, wname, N, dY, dyoff, dX=None, dxoff=0, acc_dx=False, M=None, bias=True, W=None, dW=None, woff=0,
                 db=None, side=True, after=None):
        """backward of _lin given dZ = dY[:, dyoff:dyoff+N] ALREADY multiplied by the layer's own relu' (its producer did that):
        db += colsum dZ and dW += X^T dZ on the second stream (ordered after `after`, see Products.tn), dX[:, dxoff:dxoff+K] (+)= dZ . W^T
        (Products.linear; through the step's W^T copy where there is one)."""
        M = X.shape[0] if M is None else M
        W = self.P[wname + "/weights"] if W is None else W
        dW = self.G[wname + "/weights"] if dW is None else dW
        if db is None and bias:
            db = self.G[wname + "/biases"]
        # the dX product IS the backward chain: it is queued first; the dW product (read by Adam only) follows on the second stream,
        # ordered after dZ by an event recorded BEFORE the dX launch (dX never writes what the dW product reads)
        ev = self.sched.fork_point() if (self.overlap_dw and dX is not None) else after
        if dX is not None:
            WT = self.PT.get(wname + "/weights") if (wname is not None and woff == 0 and K == W.shape[0]) else None
            self.prod.linear(M, N, K, dY, dyoff, W, woff, 1, None, 0, dX, dxoff, acc_dx, WT)
        self.prod.tn(1, M, K, N, X, xoff, X.stride(0), 0, dY, dyoff, dY.stride(0), 0, dW, woff, dW.stride(0), 0, 1, dbias=db, side=side, after=ev,
                     wgrad=True)

    # ------------------------------------------------------------------------------------------------- path ----
    def path(self, B, N):
        """What a step over B patches of N points launches, decided once from the switches and the shape (M = 4N points per upsampled
        patch, rm = B * M rows).  No device access, and nothing is kept here: forward() keeps its result for the other passes.
          stem          one launch per dense block (dispu_stem_block's shape rule: even clouds of at most 256 points), else layer0,
                        then k-NN + edge_dense_conv + a prep product per block
          after_split   K-chunks of after_conv's split contraction (4 or 8, see _fwd_after_conv); 0: one product through _lin
          defer_side    side work is submitted behind the chain's kernels (up to 16 patches of 256, see StepSchedule)
          attention     "flash" (csrc/attention_train.hip) | "gemm" (through a materialised [B, M, M] probability tensor)
          local_bwd     "pair" (five launches through the pair tensors) | "fused" (one recomputing launch, fp32 pair-tensor storage only)
          split_skip    the skip branch's d(up128) in a buffer of its own, summed in the coarse chain (next to overlap_dw's branches)
        Shape limits of the fused training kernels are refused here instead of as a bare hipErrorInvalidValue mid-step:
        dispu_mlp_chain_stash / dispu_mlp_chain_grad tile 64 rows; dispu_knn_invert sorts one cloud's graph in LDS."""
        M = N * self.up_ratio
        rm = B * M
        req(N > K_NEIGH, "a patch needs more than %d points (k-NN graph of the dense blocks), got N = %d" % (K_NEIGH, N))
        req(rm % 64 == 0, "the fused head chains work on 64-row tiles: B * %d * N must be a multiple of 64, got B = %d, N = %d "
                          "(pad the batch)" % (self.up_ratio, B, N))
        req(M <= 4096, "the local cell's backward inverts a cloud's k-NN graph in LDS: %d * N <= 4096, got N = %d" % (self.up_ratio, N))
        req(M % 32 == 0, "the non-local cell's attention kernels work on 32-point tiles: %d * N must be a multiple of 32, got N = %d"
                         % (self.up_ratio, N))
        # after_conv's split: fp32 products only (its input hp is stored as fp32 in both dtypes; bf16 products have their own tiles)
        split = rm <= 16384 and rm % 128 == 0 and not self.prod.use_bf16(1, rm, 2048, 256)
        # the fused local backward needs fp32 pair tensors (dtype "f32"); its other two conditions always hold here: whole 8-point groups
        # (rm * 16 % 64 == 0 follows from rm % 64 == 0) and conv1's W^T copy (128 x 128 passes load_params' rule)
        return Path(stem=N <= 256 and N % 2 == 0, after_split=(4 if rm >= 8192 else 8) if split else 0, defer_side=rm <= 16 * 1024,
                    attention="flash" if self.flash_attn else "gemm", local_bwd="fused" if self.fused_local_bwd and not self.bf16 else "pair",
                    split_skip=bool(self.overlap_dw))

    def _w(self, scope, D=None):
        """weights and biases of a scope as pointers: the parameters', or those of D = self.G / self.PT"""
        D = self.P if D is None else D
        return _p(D[scope + "/weights"]), _p(D[scope + "/biases"])

    def _dense_w(self, d, D=None):
        """the six weight / bias pointers of dense block d (l0, l1, l2)"""
        sc = FE + "layer%d/l" % d
        return self._w(sc + "0", D) + self._w(sc + "1", D) + self._w(sc + "2", D)

    def _chain(self, first, head):
        """the eight weight / bias pointers of a head chain: the conv `first`, then fc_layer0 .. fc_layer2 of the regressor `head`"""
        return self._w(first) + self._w(head + "fc_layer0") + self._w(head + "fc_layer1") + self._w(head + "fc_layer2")

    def _chain_T(self, first, head):
        """what a head chain's backward multiplies by, last layer first: fc_layer2's weights, then the W^T copies of fc_layer1, fc_layer0, `first`"""
        P, PT = self.P, self.PT
        return _p(P[head + "fc_layer2/weights"]), _p(PT[head + "fc_layer1/weights"]), _p(PT[head + "fc_layer0/weights"]), _p(PT[first + "/weights"])

    # ----------------------------------------------------------------------------------------------- forward ----
    def forward(self, inputs):
        """training-mode forward (BatchNorm batch statistics, moving averages updated); keeps every activation."""
        if not (isinstance(inputs, torch.Tensor) and inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() == 3
                and inputs.shape[2] == 3):
            raise ValueError("Trainer expects a float32 [B,N,3] tensor on a ROCm device")
        x = inputs.contiguous()
        B, N, _ = x.shape
        path = self.path(B, N)
        sched = self.sched
        sched.st = _lib.stream_ptr(x.device)
        self.defer_side = path.defer_side                # see __init__
        s = self._step = _Step(B, N, self.up_ratio, x, self._workspace(B, N), path)
        self._fwd_features(s)
        self._fwd_coarse(s)
        # The k-NN graph of the coarse cloud heads the step's critical path (knn -> BatchNorm statistics -> fused local cell ->
        # after_conv -> fine head): its two launches are queued BEFORE the ~8 launches of the non-local branch, which has slack
        # (round 4: queued after them, the graph waited ~70 us for the host to get there -- tools/trace_timeline.py)
        nb = _lib.tape_lib().dispu_ps_wnet_scratch_bytes(s.rm)
        if self._bn_scratch is None or self._bn_scratch.numel() * 8 < nb:
            self._bn_scratch = torch.empty((nb + 7) // 8, dtype=torch.float64, device=self.device)
        with sched.branch(2):
            self._fwd_graph(s)
        # PointShuffle2 (ops.py:1012-1087) in the inference path's form: no [B, M, 16, 134] grouped tensor.  The k-NN graph and the
        # weight net's BatchNorm statistics (from the neighbour offsets) on a branch, next to the per-point halves of conv0
        # (G = up128.Wf + xyz.(Wc + Wr) + b0, A = xyz.Wc; h0 = relu(G[j] - A[i])) that need neither
        self._fwd_conv0(s)
        # non-local cell (its attention kept for the backward as O + one log-sum-exp per query).  It reads up128 only: a branch next to
        # the grouping, the skip and the local cell; merged before add3.  Its ~8 launches are SUBMITTED after the local cell and
        # after_conv below (the chain), but ordered after this point of the stream.
        sched.defer_branch(0, partial(self._fwd_nonlocal, s))
        sched.merge(2)
        # skip (a second branch next to the local cell): gather-max straight from xyz / up128, then 134 -> 256
        sched.defer_branch(1, partial(self._fwd_skip, s))
        self._fwd_local(s)
        self._fwd_after_conv(s)
        sched.merge(0)
        sched.merge(1)
        self._fwd_fine(s)
        return s.ws["coarse"], s.ws["fine"]

    def _fwd_features(self, s):
        # feature extraction: layer0 and the four dense blocks, accumulating right-to-left inside feat[:, 0:480]
        L, ws, x, stem = _lib.tape_lib(), s.ws, s.x, s.path.stem
        B, N, rn, k1 = s.B, s.N, s.rn, K_NEIGH + 1
        feat = ws["feat"]
        l0 = self._w(FE + "layer0")
        if not stem:       # (fused stem: the first block's launch evaluates layer0 while it stages its cloud)
            _lib.check(L.dispu_linear_small_k(rn, 3, 24, _p(x), 3, *l0, 0, _p(feat, 456), 480, self.st), "layer0")
        for d, C, col, in_col, width in BLOCKS:
            if d == 1:
                F, foff = feat, 456
            else:
                if not stem:                   # (fused stem: the previous block's launch already ran this block's bottleneck conv)
                    self._lin(feat, in_col, 480 - in_col, FE + "layer%d_prep" % d, 1, ws["prep"][d], 0, 48)
                F, foff = ws["prep"][d], 0
            ldf, kidx = F.stride(0), ws["kidx"][d]
            if stem:
                # search + edge features + dense_conv in one launch (csrc/edge.hip, KNN variant); the neighbour table stays for the backward pass
                last, first = d == DENSE_BLOCKS, d == 1
                prep = (None, None) if last else self._w(FE + "layer%d_prep" % (d + 1))
                _lib.check(L.dispu_stem_block(rn, N, C, _p(F, foff), ldf, k1, 1, *self._dense_w(d), _p(feat, col), 480, _p(kidx), *prep,
                                              480 - in_col, None if last else _p(ws["prep"][d + 1]), 48, _p(x) if first else None,
                                              *(l0 if first else (None, None)), _p(feat, 456) if first else None, 480, self.st), "stem_block")
            else:
                _lib.check(L.dispu_knn_feat_strided(B, N, N, C, k1, _p(F, foff), ldf, _p(F, foff), ldf, None, _p(kidx), self.st), "knn_feat")
                # the inference kernel (csrc/edge.hip): edge features, three chained convs and the max in one launch; nothing is kept
                # for the backward pass, which recomputes the block on chip (csrc/edge_bwd.hip)
                _lib.check(L.dispu_edge_dense_conv(rn, N, C, _p(F, foff), ldf, _p(kidx), k1, 1, *self._dense_w(d), _p(feat, col), 480, self.st),
                           "edge_dense_conv")

    def _fwd_coarse(self, s):
        # duplicate_up (per source point) + coarse regressor
        L, ws = _lib.tape_lib(), s.ws
        w1 = self.P[UP + "conv1/weights"]
        self._lin(ws["feat"], 0, 480, None, 0, ws["h256"], 0, 256, bias=False, W=w1)
        _lib.check(L.dispu_dup_grid(s.B, s.N, 256, self.up_ratio, _p(ws["h256"]), 256, _p(w1, 480 * 256), _p(self.P[UP + "conv1/biases"]),
                                    _p(self.grid), _p(ws["up256"]), 256, self.st), "dup_grid")
        # conv2 -> fc_layer0 -> fc_layer1 -> fc_layer2 in ONE launch (csrc/mlp_chain.hip), every intermediate stashed for the backward
        _lib.check(L.dispu_mlp_chain_stash(s.rm, 256, 128, 256, 64, _p(ws["up256"]), 256, *self._chain(UP + "conv2", CS),
                                           _p(ws["up128"]), 128, _p(ws["c256"]), 256, _p(ws["c64"]), 64, None, 0, 0, None, 0,
                                           _p(s.coarse), 3, self.st), "mlp_chain[coarse]")

    def _fwd_graph(self, s):
        # the k-NN graph of the coarse cloud and the weight net's BatchNorm statistics (from the neighbour offsets)
        L, ws, P, M, k = _lib.tape_lib(), s.ws, self.P, s.M, K_NEIGH
        _lib.check(L.dispu_knn_xyz(s.B, M, M, k, _p(s.coarse), _p(s.coarse), _p(ws["psidx"]), None, _lib.ARITH_PLAIN, self.st), "knn_xyz")
        _lib.check(L.dispu_ps_wnet_bn_stats(s.rm, M, k, 16, _p(ws["psidx"]), _p(s.coarse), *self._w(PS + "weight_net/wconv0"),
                                            _p(P[BN + "gamma"]), _p(P[BN + "beta"]), BN_EPS, BN_DECAY, _p(ws["bn_stats"]), _p(ws["bn_scale"]),
                                            _p(ws["bn_shift"]), _p(self.moving_mean), _p(self.moving_var), _p(self._bn_scratch),
                                            self._bn_scratch.numel() * 8, self.st), "ps_wnet_bn_stats")

    def _fwd_conv0(self, s):
        # the per-point halves of the local cell's conv0: G = up128.Wf + xyz.(Wc + Wr) + b0, A = xyz.Wc
        ws, w0 = s.ws, self.P[PS + "conv0/weights"]
        self._lin(ws["up128"], 0, 128, None, 0, ws["gm"], 0, 128, bias=False, W=w0, woff=6 * 128)
        _lib.check(_lib.tape_lib().dispu_ps_prep(s.rm, 128, _p(s.coarse), _p(w0), _p(self.P[PS + "conv0/biases"]), _p(ws["gm"]), 128,
                                                 _p(ws["am"]), 128, self.st), "ps_prep")

    def _fwd_nonlocal(self, s):
        L, ws, B, M = _lib.tape_lib(), s.ws, s.B, s.M
        up128, kv, q, att = ws["up128"], ws["kv"], ws["q"], ws["att"]
        self._lin(up128, 0, 128, PS + "PointShuffle/conv_kv", 0, kv, 0, 128)
        self._lin(up128, 0, 128, PS + "PointShuffle/conv_query", 0, q, 0, 64)
        if s.path.attention == "flash":
            # softmax(Q.K^T / 8).V on chip; what the backward needs is att and ONE float per query (csrc/attention_train.hip)
            _lib.check(L.dispu_attention_fwd_lse(B, M, M, 64, _p(q), 64, _p(kv), 128, _p(kv, 64), 128, 0.125, _p(att), 64, _p(ws["lse"]),
                                                 self.st), "attention_fwd_lse")
        else:
            S = ws["S"]
            _lib.check(self.prod.batched(B, M, 64, M, _p(q), 64, M * 64, _p(kv), 128, M * 128, 1, None, 0, _p(S), M, M * M,
                                             None, 0, 0, None, 0, 0, self.st), "scores")
            _lib.check(L.dispu_softmax_rows(s.rm, M, 0.125, _p(S), M, self.st), "softmax")
            _lib.check(self.prod.batched(B, M, M, 64, _p(S), M, M * M, _p(kv, 64), 128, M * 128, 0, None, 0, _p(att), 64,
                                             M * 64, None, 0, 0, None, 0, 0, self.st), "att.V")
        self._lin(att, 0, 64, PS + "PointShuffle/conv_back_project", 1, ws["nl"], 0, 256)
        # what the backward needs and nothing in the forward touches (zeroed accumulators, the W^T copies: ~45 us of kernels),
        # behind the branch's own kernels
        self._backward_prep(ws)

    def _fwd_skip(self, s):
        ws = s.ws
        _lib.check(_lib.tape_lib().dispu_ps_skip_max(s.rm, s.M, K_NEIGH, 128, _p(ws["psidx"]), _p(s.coarse), _p(ws["up128"]), 128,
                                                     _p(ws["gmax"]), 144, self.st), "skip_max")
        self._lin(ws["gmax"], 0, 134, PS + "skip", 1, ws["skip"], 0, 256)

    def _fwd_local(self, s):
        # the fused cell (conv1, weight_net with the folded BatchNorm, feature x weight)
        ws = s.ws
        _lib.check(_lib.tape_lib().dispu_ps_local(s.rm, s.M, K_NEIGH, 128, _p(ws["psidx"]), _p(s.coarse), _p(ws["gm"]), 128, _p(ws["am"]),
                                                  *self._w(PS + "conv1"), *self._w(PS + "weight_net/wconv0"), _p(ws["bn_scale"]),
                                                  _p(ws["bn_shift"]), _p(ws["hp"]), self.st), "ps_local")

    def _fwd_after_conv(self, s):
        # after_conv, [rows x 2048] x [2048 x 256].  At <= 16 patches the rows give 32 - 128 tiles of 128 x 256 -- a fraction of the chip --
        # and the tile rule falls back to 512 L2-bound 64 x 64 tiles (139 us in the 8-patch step for a 55 us product): the contraction is
        # split into K-chunks run as one batched launch that fills the chip with 128 x 256 tiles, a second launch adds the chunks in
        # order, then bias and ReLU (reassociated; `fine` is tolerance-checked).  fp32 products only (bf16 products have their own tiles)
        L, ws, rm, nsp = _lib.tape_lib(), s.ws, s.rm, s.path.after_split
        if not nsp:
            self._lin(ws["hp"], 0, 2048, PS + "after_conv", 1, ws["aft"], 0, 256)
            return
        if ws.get("aft_parts") is None or ws["aft_parts"].numel() < nsp * rm * 256:
            ws["aft_parts"] = torch.empty((nsp * rm, 256), dtype=torch.float32, device=self.device)
        wa, ba = self._w(PS + "after_conv")
        kc = 2048 // nsp
        _lib.check(L.dispu_linear(nsp, rm, kc, 256, _p(ws["hp"]), 2048, kc, wa, 256, kc * 256, 0, None, 0, _p(ws["aft_parts"]), 256, rm * 256,
                                  None, 0, 0, None, 0, 0, self.st), "dispu_linear[split-K]")
        _lib.check(L.dispu_linear_splitk_finish(rm, 256, nsp, _p(ws["aft_parts"]), rm * 256, ba, 1, _p(ws["aft"]), 256, self.st),
                   "dispu_linear_splitk_finish")

    def _fwd_fine(self, s):
        L, ws, rm = _lib.tape_lib(), s.ws, s.rm
        _lib.check(L.dispu_add3(rm * 256, _p(ws["aft"]), _p(ws["skip"]), _p(ws["nl"]), _p(ws["sum"]), self.st), "add3")
        # aggregation -> fine regressor (fc_layer0, fc_layer1, fc_layer2) -> coarse + sigmoid(.) - 0.5 in one launch
        _lib.check(L.dispu_mlp_chain_stash(rm, 256, 256, 256, 64, _p(ws["sum"]), 256, *self._chain(PS + "aggregation", FS),
                                           _p(ws["agg"]), 256, _p(ws["f256"]), 256, _p(ws["f64"]), 64, _p(ws["z"]), 3, 1, _p(s.coarse), 3,
                                           _p(ws["fine"]), 3, self.st), "mlp_chain[fine]")

    def _recompute_pair_tensors(self, s):
        """h0 = relu(G[j] - A[i]), h1 = relu(h0.W1 + b1), wv = relu(BN(offsets.Ww + bw)) [B*M*16, .] and the inverted k-NN graph: what
        the local cell's backward reads.  The forward kernel (csrc/ps_local.hip) keeps them on chip; they are rebuilt here, on an
        auxiliary stream next to the loss and the fine head's backward.  dtype "f32": the same fmaf chains as the forward kernel,
        hence the same values and the same ReLU decisions.  dtype "bf16": conv1 is rebuilt with bf16 PRODUCTS (and h0 / h1 are stored as
        bf16) while the forward's fused cell ran fp32 products -- the masks (h1 > 0) and the h1 values entering dwv are those of the
        bf16 rebuild, i.e. they can differ from the forward's at pre-activations within bf16 rounding of zero; that is part of the
        mixed-precision approximation and sits inside the tolerances of tests/test_train_bf16_gpu.py (loss terms 2 %, gradient cosine
        >= 0.97), not a separate error source."""
        if s.stash_ready:
            return
        L, ws, rm, M, k = _lib.tape_lib(), s.ws, s.rm, s.M, K_NEIGH
        fused = s.path.local_bwd == "fused"
        if not fused:
            _lib.check(L.dispu_knn_invert(s.B, M, k, _p(ws["psidx"]), _p(ws["inv_off"]), _p(ws["inv"]), self.st), "knn_invert")
        if ws["h0"].dtype == torch.bfloat16:
            _lib.check(L.dispu_ps_gather_sub_relu_bf16(rm, M, k, 128, _p(ws["psidx"]), _p(ws["gm"]), 128, _p(ws["am"]), 128, _p(ws["h0"]), 128,
                                                       self.st), "gather_sub_relu_bf16")
        else:
            _lib.check(L.dispu_ps_gather_sub_relu(rm, M, k, 128, _p(ws["psidx"]), _p(ws["gm"]), 128, _p(ws["am"]), 128, _p(ws["h0"]), 128, self.st),
                       "gather_sub_relu")
        if not fused:                                    # (fused backward: only h0 is needed in HBM -- the dW1 = h0^T . dz1 product reads it)
            self._lin(ws["h0"], 0, 128, PS + "conv1", 1, ws["h1"], 0, 128)
            _lib.check(L.dispu_ps_weight_net(rm, M, k, 16, _p(ws["psidx"]), _p(s.coarse), *self._w(PS + "weight_net/wconv0"),
                                             _p(ws["bn_scale"]), _p(ws["bn_shift"]), _p(ws["wv"]), self.st), "weight_net")
        s.stash_ready = True

    # -------------------------------------------------------------------------------------------------- loss ----
    def _chamfer(self, pred, gt, radius, coef, dpred, slot):
        """one Chamfer term (loss_utils.py:45-64 with nn_distance(gt, pred)): its un-scaled value into loss_vals[slot] and
        d(coef * CD)/d pred into dpred -- three launches (nn_distance, value, gradient) + one memset."""
        L = _lib.tape_lib()
        full = self._step.ws
        ws = full["cd"][slot]
        B, n_gt, n_pred = gt.shape[0], gt.shape[1], pred.shape[1]
        _lib.check(L.dispu_nn_distance(B, n_gt, _p(gt), n_pred, _p(pred), _p(ws["d_gt"]), _p(ws["i_gt"]), _p(ws["d_pred"]),
                                       _p(ws["i_pred"]), _lib.ARITH_CONTRACT, self.st), "nn_distance")
        _lib.check(L.dispu_chamfer_loss_grad(B, n_gt, _p(gt), n_pred, _p(pred), _p(ws["d_gt"]), _p(ws["i_gt"]), _p(ws["d_pred"]),
                                             _p(ws["i_pred"]), _p(radius), coef, _p(full["loss_vals"], slot), _p(dpred), self.st),
                   "chamfer_loss_grad")

    def _uniform_tables(self, B, N):
        """the level tables of the uniform term for B patches of N points (loss_utils.UniformTables; the gradient carries uniform_w);
        ValueError for a patch size whose fine cloud leaves a ball with fewer than two slots."""
        from . import loss_utils
        M = N * self.up_ratio
        need = loss_utils.uniform_min_points()
        if M < need:
            raise ValueError("use_uniform needs at least %d fine points (int(M * 0.004) >= 2 slots in the smallest ball): a patch size of "
                             "at least %d at up_ratio %d, got %d (%d fine points)" % (need, -(-need // self.up_ratio), self.up_ratio, N, M))
        return loss_utils.UniformTables(B, M, scale=float(self.opts.uniform_w))

    def _uniform_workspace(self, ws, B, N):
        """the uniform term's buffers (csrc/uniform_loss.hip), added to the workspace the first time the term runs at this shape: seeds of
        the fine cloud, per-ball value partials, and the HOST level tables the launch reads, one per uniform_w -- a launch tape records
        their addresses, so they live as long as the workspace."""
        w = float(self.opts.uniform_w)
        if "utabs" not in ws:
            tab = self._uniform_tables(B, N)
            dev, M = self.device, N * self.up_ratio
            nb = _lib.lib().dispu_fps_scratch_bytes(B, M, tab.npoint)
            ws.update(utabs={w: tab}, useeds=torch.empty((B, tab.npoint), dtype=torch.int32, device=dev),
                      upart=torch.empty((tab.nlevels, B * tab.npoint), dtype=torch.float32, device=dev),
                      ufps_tmp=torch.empty((nb // 4,), dtype=torch.float32, device=dev) if nb else None, ufps_bytes=nb)
        if w not in ws["utabs"]:
            ws["utabs"][w] = self._uniform_tables(B, N)
        return ws["utabs"][w]

    def _emd_workspace(self, ws, B, N):
        """the EMD term's buffers (csrc/approxmatch.hip), added to the workspace the first time the term runs at this shape: the auction's
        scratch (ratio vectors and chunk partials; no [B, M, M] match), the fused launch's partial sums, one raw cost per cloud."""
        if "emd_cost" not in ws:
            L, M, dev = _lib.lib(), N * self.up_ratio, self.device
            nt, ns = L.dispu_approx_match_scratch_bytes(B, M, M), L.dispu_emd_loss_grad_scratch_bytes(B, M, M)
            ws.update(emd_temp=torch.empty(((nt + 3) // 4,), dtype=torch.float32, device=dev), emd_temp_bytes=nt,
                      emd_scratch=torch.empty(((ns + 3) // 4,), dtype=torch.float32, device=dev), emd_scratch_bytes=ns,
                      emd_cost=torch.zeros((B,), dtype=torch.float32, device=dev))

    def _check_targets(self, gt, radius, B, M):
        """gt [B, 4N, 3] / radius [B] float32 on the device: the loss workspace (d_gt, i_gt, g_gt, ...) is sized [B, 4N]
        and the kernels take raw pointers, so anything else must be refused here (DisPU/model.py:47-49 placeholders)."""
        gt, radius = f32(gt, "gt"), f32(radius, "radius")
        req(gt.dim() == 3 and tuple(gt.shape) == (B, M, 3),
            "gt must have shape (%d, %d, 3) for this batch, got %s" % (B, M, tuple(gt.shape)))
        req(radius.dim() == 1 and radius.shape[0] == B, "radius must have shape (%d,), got %s" % (B, tuple(radius.shape)))
        req(gt.device == self.device and radius.device == self.device, "gt / radius must live on %s" % self.device)
        return gt, radius

    def loss_backward(self, gt, radius):
        """pu_loss of model.py:75-87 at the current epoch; fills dcoarse / dfine with its gradient."""
        s, sched = self._step, self.sched
        B, N, ws = s.B, s.N, s.ws
        gt, radius = self._check_targets(gt, radius, B, s.M)
        wf = weight_fine(self.epoch)
        repulse, uniform, emd = bool(self.opts.use_repulse), bool(getattr(self.opts, "use_uniform", False)), bool(getattr(self.opts, "use_emd", False))
        tab = self._uniform_workspace(ws, B, N) if uniform else None     # refuses a patch size the term cannot take, before any launch
        if emd:
            self._emd_workspace(ws, B, N)
        # side work is submitted behind the fine term's launches (the chain): the pair tensors of the local cell's backward (needed much
        # later) and the coarse term
        sched.defer_branch(2, partial(self._recompute_pair_tensors, s))    # off the chain: needed by the local cell's backward only
        with sched.branch(0):                                        # the coarse term next to the fine term and the repulsion term
            self._chamfer(ws["coarse"], gt, radius, 1000.0, ws["dcoarse"], 0)
        # fine term: nn_distance, then value + gradient (which zero-fills dfine); the repulsion term's ball query runs next to it and
        # adds its gradient once the Chamfer gradient is in place
        # the uniform term's seeds (farthest point sampling of the fine cloud) run on the same branch; its fused value + gradient launch
        # follows the Chamfer gradient like the repulsion gradient does
        if repulse or uniform:
            with sched.branch(1):
                self._loss_queries(s, repulse, tab)
        # the EMD term's auction (21 launches, reads fine and gt only) runs on a branch of its own next to the Chamfer launches: ordered
        # after THIS point of the stream, submitted behind the fine term's launches (the chain); its fused cost + gradient launch follows
        # the Chamfer gradient on the chain (which zero-fills dfine), like the two terms above
        ev_emd = sched.fork_point() if (emd and self.overlap_dw) else None
        self._chamfer(ws["fine"], gt, radius, 1000.0 * wf, ws["dfine"], 1)
        if emd:
            with sched.branch(3, ev_emd):
                _lib.check(_lib.tape_lib().dispu_approx_match_levels_ws(B, s.M, s.M, _p(ws["fine"]), _p(gt), _p(ws["emd_temp"]), ws["emd_temp_bytes"],
                                                                        _lib.ARITH_CONTRACT, self.st), "approx_match_levels_ws")   # as loss_utils.earth_mover
        if repulse or uniform:
            sched.merge(1)
        self._loss_ball_terms(s, repulse, tab)
        if emd:
            sched.merge(3)
            _lib.check(_lib.tape_lib().dispu_emd_loss_grad(B, s.M, s.M, _p(ws["fine"]), _p(gt), _p(ws["emd_temp"]), _p(radius),
                                                           float(self.opts.emd_w) * wf / s.rm, _p(ws["emd_cost"]), _p(ws["dfine"]), _p(ws["emd_scratch"]),
                                                           ws["emd_scratch_bytes"], _lib.ARITH_CONTRACT, self.st), "emd_loss_grad")
        sched.merge(0)
        self._loss_finalize(s, wf, repulse, tab, emd, radius)
        terms = self._terms(ws["loss_vals"], wf, uniform, emd)
        sched.flush(prio=0)                                          # the recompute branch: submitted behind the loss's own launches
        return terms

    def _loss_queries(self, s, repulse, tab):
        """what the repulsion and uniform terms need of the fine cloud before their gradients: the ball query, the seeds"""
        L, ws, B, M, fine = _lib.tape_lib(), s.ws, s.B, s.M, s.ws["fine"]
        if repulse:
            _lib.check(L.dispu_query_ball(B, M, M, _p(ws["r07"]), 20, _p(fine), _p(fine), _p(ws["ball"]), _p(ws["ball_cnt"]),
                                          _lib.ARITH_CONTRACT, self.st), "query_ball")   # as loss_utils.get_repulsion_loss
        if tab is not None:
            _lib.check(L.dispu_fps_ws(B, M, tab.npoint, _p(fine), _p(ws["ufps_tmp"]), ws["ufps_bytes"], _p(ws["useeds"]),
                                      _lib.ARITH_CONTRACT, self.st), "fps")              # as loss_utils.get_uniform_loss

    def _loss_ball_terms(self, s, repulse, tab):
        """value and gradient of the repulsion and uniform terms, added to dfine behind the fine Chamfer gradient"""
        L, ws, B, M, fine = _lib.tape_lib(), s.ws, s.B, s.M, s.ws["fine"]
        if repulse:
            _lib.check(L.dispu_repulsion_loss_grad(B * M, M, 20, 0.001, self.opts.repulsion_w / (B * M * 4.0), _p(fine), _p(ws["ball"]),
                                                   _p(ws["rep"]), _p(ws["dfine"]), self.st), "repulsion_loss_grad")
        if tab is not None:
            _lib.check(L.dispu_uniform_loss_grad(B, M, tab.npoint, tab.nlevels, ctypes.addressof(tab.ns), ctypes.addressof(tab.levels), _p(fine),
                                                 _p(ws["useeds"]), _p(ws["upart"]), _p(ws["dfine"]), None, None, _lib.ARITH_CONTRACT, self.st),
                       "uniform_loss_grad")

    def _loss_finalize(self, s, wf, repulse, tab, emd, radius):
        """the terms' partial values -> loss_vals[2:] (pu_loss and its weighted terms) in one launch"""
        L, ws, B, M, uniform = _lib.tape_lib(), s.ws, s.B, s.M, tab is not None
        out, rep = ws["loss_vals"], _p(ws["rep"]) if repulse else None
        if emd:
            _lib.check(L.dispu_pu_loss_finalize_e(_p(out), rep, B * M, wf, float(self.opts.repulsion_w),
                                                  _p(ws["upart"]) if uniform else None, tab.nlevels if uniform else 0,
                                                  B * tab.npoint if uniform else 0, float(self.opts.uniform_w) if uniform else 0.0,
                                                  _p(ws["emd_cost"]), _p(radius), B, M, float(self.opts.emd_w), _p(out, 2), self.st), "pu_loss_finalize_e")
        elif uniform:
            _lib.check(L.dispu_pu_loss_finalize_u(_p(out), rep, B * M, wf, float(self.opts.repulsion_w),
                                                  _p(ws["upart"]), tab.nlevels, B * tab.npoint, float(self.opts.uniform_w), _p(out, 2), self.st),
                       "pu_loss_finalize_u")
        else:
            _lib.check(L.dispu_pu_loss_finalize(_p(out), rep, B * M, wf, float(self.opts.repulsion_w), _p(out, 2), self.st), "pu_loss_finalize")

    @staticmethod
    def _terms(out, wf, uniform=False, emd=False):
        vals = out[2:9 if emd else 8 if uniform else 6].clone()  # device scalars that survive the next step
        terms = {"dis_coarse_cd": vals[0], "dis_fine_cd": vals[1], "repulsion_loss": vals[2], "pu_loss": vals[3], "weight_fine": wf}
        if uniform:
            terms["uniform_loss"] = vals[5]                     # uniform_w * get_uniform_loss(fine)
        if emd:
            terms["dis_fine_emd"] = vals[6]                     # emd_w * earth_mover(fine, gt, radius)
        return terms

    # ---------------------------------------------------------------------------------------------- backward ----
    def backward(self):
        """gradients of pu_loss w.r.t. every trainable variable, accumulated into the flat gradient buffer.
        ReLU gradients never run as separate passes: the kernel that produces a layer's dY applies that layer's mask (the fused head
        chains, the gathers, Products.act_bias_grad), so every dY arriving at _lin_bwd is already the pre-activation gradient dZ."""
        s = self._step
        if not s.fresh:
            # a second backward() on the same forward (new targets / loss weights): the atomics accumulators still hold the previous,
            # already masked gradients -- clear them again, on this stream, before anything accumulates
            self._zero(s.ws["zeroed"])
        s.fresh = False
        if not s.stash_ready:                           # backward() without loss_backward(): rebuild the pair tensors here
            with self.sched.branch(2):
                self._recompute_pair_tensors(s)
        self._backward_refine(s)
        self._bucket_point(0)                            # data parallel: every refine/* gradient is queued -> its all-reduce starts
        self._backward_generator(s)
        self.sched.join()                     # every dW is in the flat gradient buffer from here on (all-reduce, Adam)

    def _backward_refine(self, s):
        """fine head, then the local cell on the chain with the non-local cell, the skip and the weight net as branches next to it"""
        ws, sched = s.ws, self.sched
        self._bwd_fine(s)
        # local cell first: the host needs ~0.1 ms to queue the two branches below, the chain must not sit idle meanwhile; the
        # branches themselves only need the head chain's dskip / dnl, so they are ordered after THIS point of the stream, not after the
        # product
        ev_br = sched.fork_point() if self.overlap_dw else None
        self._lin_bwd(ws["hp"], 0, 2048, PS + "after_conv", 256, ws["daft"], 0, ws["dhp"])
        # non-local cell: reads dnl, writes datt / dS / dkv / dq / dup128 -- nothing the local cell or the skip branch touches, so
        # it runs as a branch next to them; merged before anything else accumulates into dup128
        sched.defer_branch(0, partial(self._bwd_nonlocal, s), ev_br)
        # skip branch (a second branch): 134 -> 256 backward; its max gradient is scattered after the merges below
        sched.defer_branch(1, partial(self._bwd_skip, s), ev_br)
        # after_conv's dX (0.1 - 0.15 ms on the GPU) is queued: submit the two branches the chain will wait for behind it; the weight
        # gradients stay deferred until the chain's next three kernels are queued too
        sched.flush(prio=0)
        sched.merge(2)                                        # h0 / h1 / wv / the inverted graph are in place
        self._bwd_local_product(s)
        # the weight net's backward (dwv -> BatchNorm -> 3 -> 16 conv -> atomics into dcoarse) next to the conv1 / conv0 gradients
        sched.defer_branch(2, partial(self._bwd_weight_net, s))
        self._bwd_local_convs(s)
        # the main queue now holds after_conv's dX, the feature x weight gradient, conv1's dX and the gather (~0.35 ms of kernels at 8
        # patches): time to submit the side work that piled up behind them (five weight gradients, the non-local and skip branches)
        sched.flush()
        sched.merge(0)                                        # dup128 holds the non-local cell's part from here on
        self._bwd_conv0(s)
        sched.merge(1)
        if not s.path.split_skip:
            self._skip_max_grad(s, ws["dup128"])
        sched.merge(2)                                        # the weight net's share of dcoarse
        # the refine branch's weight-gradient products submitted so far (after_conv's 2048 x 256 with its ~100 MB of partials among them)
        # get their grouped reduction HERE, in the shadow of the coarse chain's backward; whatever is left at join() is small.  (All of
        # them at join(): 35 us of reductions between the last product and Adam.)
        sched.flush_reductions()

    def _backward_generator(self, s):
        # coarse head and duplicate_up, then the dense blocks, last to first (every block has its own dE / dprep: the dW products on
        # the second stream read them while the chain moves on, no join inside the loop)
        sched = self.sched
        self._bwd_coarse(s)
        for blk in reversed(BLOCKS):
            scr = self._bwd_block_partials(s, blk)
            # the block's recomputing backward kernel (40 - 80 us) is queued: submit some of the side work deferred so far behind it
            # (the coarse head's weight gradients, the previous blocks' reductions and prep gradients) -- a few launches per block,
            # as many as the kernel's duration hides
            tail = blk[0] == 1 and self.overlap_dw
            sched.flush(n=None if tail else 5)
            reduce_partials = partial(self._bwd_block_reduce, s, blk, scr, sched.fork_point() if (self.overlap_dw and not tail) else None)
            if tail:
                # the last block of the backward: everything deferred so far is on the side streams by now; this block's own
                # reduction (and layer0's weight gradient below) follow their producer on the chain's stream -- Adam waits for
                # them either way, and a hop to a side stream and back costs more than the two launches take
                reduce_partials()
            else:
                sched.defer(reduce_partials)
            self._bwd_block_prep(s, blk)
        # layer0 (no activation, input has no gradient)
        self._lin_bwd(s.x.view(s.rn, 3), 0, 3, FE + "layer0", 24, s.ws["dfeat"], 456, None, side=False)

    def _bwd_fine(self, s):
        L, ws, rm = _lib.tape_lib(), s.ws, s.rm
        # fine = coarse + sigmoid(z) - 0.5
        _lib.check(L.dispu_sigmoid_offset_grad(rm * 3, _p(ws["z"]), _p(s.dfine), _p(ws["dz"]), _p(s.dcoarse), self.st), "sigmoid_grad")
        ag = PS + "aggregation"
        # fc_layer2 -> fc_layer1 -> fc_layer0 -> aggregation backward and the three branch masks of
        # sum = relu(after) + relu(skip) + relu(nl) in ONE launch (csrc/mlp_chain_bwd.hip); the four dW products follow on the side streams
        _lib.check(L.dispu_mlp_chain_grad(rm, 256, 256, 256, _p(ws["dz"]), 3, *self._chain_T(ag, FS),
                                          _p(ws["f64"]), 64, _p(ws["f256"]), 256, _p(ws["agg"]), 256, None, 0, None, 0,
                                          _p(ws["df64"]), 64, _p(ws["df256"]), 256, _p(ws["dagg"]), 256,
                                          _p(ws["aft"]), _p(ws["skip"]), _p(ws["nl"]), 256, _p(ws["daft"]), _p(ws["dskip"]), _p(ws["dnl"]), 256,
                                          self.st), "mlp_chain_grad[fine]")
        grp = self.sched.fork_group()
        self._lin_bwd(ws["f64"], 0, 64, FS + "fc_layer2", 3, ws["dz"], 0, after=grp)
        self._lin_bwd(ws["f256"], 0, 256, FS + "fc_layer1", 64, ws["df64"], 0, after=grp)
        self._lin_bwd(ws["agg"], 0, 256, FS + "fc_layer0", 256, ws["df256"], 0, after=grp)
        self._lin_bwd(ws["sum"], 0, 256, ag, 256, ws["dagg"], 0, after=grp)

    def _bwd_nonlocal(self, s):
        L, ws, B, M = _lib.tape_lib(), s.ws, s.B, s.M
        dup128 = ws["dup128"]
        self._lin_bwd(ws["att"], 0, 64, PS + "PointShuffle/conv_back_project", 256, ws["dnl"], 0, ws["datt"])
        S, dS, kv, dkv, q = ws["S"], ws["dS"], ws["kv"], ws["dkv"], ws["q"]
        if s.path.attention == "flash":
            # dQ, dK, dV with the probabilities recomputed tile by tile from Q, K and the forward's log-sum-exp: two launches
            _lib.check(L.dispu_attention_bwd(B, M, M, 64, _p(q), 64, _p(kv), 128, _p(kv, 64), 128, 0.125, _p(ws["att"]), 64,
                                             _p(ws["lse"]), _p(ws["datt"]), 64, _p(ws["dq"]), 64, _p(dkv), 128, _p(dkv, 64), 128,
                                             _p(ws["dvec"]), self.st), "attention_bwd")
        else:
            # dP = dO . V^T
            _lib.check(self.prod.batched(B, M, 64, M, _p(ws["datt"]), 64, M * 64, _p(kv, 64), 128, M * 128, 1, None, 0, _p(dS), M, M * M,
                                             None, 0, 0, None, 0, 0, self.st), "dP")
            # dV = P^T . dO  -> dkv[:, 64:128]
            self.prod.tn(B, M, M, 64, S, 0, M, M * M, ws["datt"], 0, 64, M * 64, dkv, 64, 128, M * 128, 0)
            _lib.check(L.dispu_softmax_rows_grad(s.rm, M, 0.125, _p(S), M, _p(dS), M, self.st), "softmax_grad")
            # dQ = dS . K
            _lib.check(self.prod.batched(B, M, M, 64, _p(dS), M, M * M, _p(kv), 128, M * 128, 0, None, 0, _p(ws["dq"]), 64, M * 64,
                                             None, 0, 0, None, 0, 0, self.st), "dQ")
            # dK = dS^T . Q -> dkv[:, 0:64]
            self.prod.tn(B, M, M, 64, dS, 0, M, M * M, q, 0, 64, M * 64, dkv, 0, 128, M * 128, 0)
        self._lin_bwd(ws["up128"], 0, 128, PS + "PointShuffle/conv_kv", 128, dkv, 0, dup128)
        self._lin_bwd(ws["up128"], 0, 128, PS + "PointShuffle/conv_query", 64, ws["dq"], 0, dup128, 0, acc_dx=True)

    def _bwd_skip(self, s):
        ws = s.ws
        self._lin_bwd(ws["gmax"], 0, 134, PS + "skip", 256, ws["dskip"], 0, ws["dgmax"])
        if s.path.split_skip:                            # the skip branch's d(up128) in its own buffer, summed in the coarse chain
            self._skip_max_grad(s, ws["dup128s"])

    def _skip_max_grad(self, s, dup128):
        ws = s.ws
        _lib.check(_lib.tape_lib().dispu_ps_skip_max_grad(s.rm, s.M, K_NEIGH, 128, _p(ws["psidx"]), _p(s.coarse), _p(ws["up128"]), 128,
                                                          _p(ws["gmax"]), 144, _p(ws["dgmax"]), 136, _p(s.dcoarse), _p(dup128), 128, 1, self.st),
                   "ps_skip_max_grad")

    def _bwd_local_product(self, s):
        """the feature x weight product's gradient: dwv and dz1 -- with conv1's dX and conv0's gather in the same launch on the fused path"""
        L, ws, rm = _lib.tape_lib(), s.ws, s.rm
        if s.path.local_bwd == "fused":
            # one launch: dwv, dz1 (for the side-stream dW1), dG (atomics into the zeroed buffer) and -dA; h1 / dz0 / wv stay on chip
            self._zero(ws["dG"])
            _lib.check(L.dispu_ps_local_grad(rm, s.M, _p(ws["psidx"]), _p(s.coarse), _p(ws["gm"]), 128, _p(ws["am"]), *self._w(PS + "conv1"),
                                             _p(self.PT[PS + "conv1/weights"]), *self._w(PS + "weight_net/wconv0"), _p(ws["bn_scale"]),
                                             _p(ws["bn_shift"]), _p(ws["dhp"]), _p(ws["dz1"]), _p(ws["dwv"]), _p(ws["dG"]), _p(ws["dAneg"]), self.st),
                       "ps_local_grad")
        else:
            _lib.check(L.dispu_ps_point_matmul_grad_relu_s(rm, K_NEIGH, 128, 16, _p(ws["h1"]), 128, _p(ws["wv"]), _p(ws["dhp"]), 2048, _p(ws["dz1"]),
                                                           128, _p(ws["dwv"]), 1 if ws["h1"].dtype == torch.bfloat16 else 0, self.st),
                       "point_matmul_grad")

    def _bwd_weight_net(self, s):
        ws, P, G = s.ws, self.P, self.G
        wn = PS + "weight_net/wconv0"
        _lib.check(_lib.tape_lib().dispu_ps_wnet_grad(s.rm, s.M, K_NEIGH, 16, _p(ws["psidx"]), _p(s.coarse), *self._w(wn), _p(ws["bn_stats"]),
                                                      _p(ws["bn_scale"]), _p(ws["bn_shift"]), _p(P[BN + "gamma"]), _p(ws["dwv"]), *self._w(wn, G),
                                                      _p(G[BN + "gamma"]), _p(G[BN + "beta"]), _p(s.dcoarse), _p(ws["bn_sums"]),
                                                      _p(self._bn_scratch), self._bn_scratch.numel() * 8, self.st), "ps_wnet_grad")

    def _bwd_local_convs(self, s):
        ws = s.ws
        if s.path.local_bwd == "fused":
            self._lin_bwd(ws["h0"], 0, 128, PS + "conv1", 128, ws["dz1"], 0, None)            # dW1, db1 only: the dX product ran inside the fused launch
            return
        self._lin_bwd(ws["h0"], 0, 128, PS + "conv1", 128, ws["dz1"], 0, ws["dz0"])      # dz0 holds dh0: conv0's relu' rides in the gather
        # conv0 in its per-source-point form: dh0 * (G[j] - A[i] > 0) -> dG (gather through the inverted graph), -dA; then [B*M, 128] products
        _lib.check(_lib.tape_lib().dispu_ps_conv0_gather_grad_s(s.rm, s.M, K_NEIGH, 128, _p(ws["psidx"]), _p(ws["inv_off"]), _p(ws["inv"]),
                                                                _p(ws["dz0"]), 128, 1 if ws["dz0"].dtype == torch.bfloat16 else 0, _p(ws["gm"]), 128,
                                                                _p(ws["am"]), 128, _p(ws["dG"]), 128, _p(ws["dAneg"]), 128, self.st),
                   "conv0_gather_grad")

    def _bwd_conv0(self, s):
        ws, G = s.ws, self.G
        w0, dw0 = self.P[PS + "conv0/weights"], G[PS + "conv0/weights"]
        self._lin_bwd(ws["up128"], 0, 128, None, 128, ws["dG"], 0, ws["dup128"], 0, acc_dx=True, W=w0, dW=dw0, woff=6 * 128, bias=False,
                      db=G[PS + "conv0/biases"])
        _lib.check(_lib.tape_lib().dispu_ps_prep_grad(s.rm, 128, _p(s.coarse), _p(w0), _p(ws["dG"]), 128, _p(ws["dAneg"]), 128, _p(s.dcoarse),
                                                      _p(dw0), self.st), "ps_prep_grad")

    def _bwd_coarse(self, s):
        # coarse regressor and duplicate_up
        L, ws, G, rm = _lib.tape_lib(), s.ws, self.G, s.rm
        c2, dup128, dcoarse = UP + "conv2", ws["dup128"], s.dcoarse
        # fc_layer2 -> fc_layer1 -> fc_layer0 (+ everything already accumulated in dup128, then conv2's relu') -> conv2 (duplicate_up's
        # relu') in one launch
        _lib.check(L.dispu_mlp_chain_grad(rm, 256, 128, 256, _p(dcoarse), 3, *self._chain_T(c2, CS),
                                          _p(ws["c64"]), 64, _p(ws["c256"]), 256, _p(ws["up128"]), 128, _p(dup128), 128,
                                          _p(ws["dup128s"]) if s.path.split_skip else None, 128, _p(ws["dc64"]), 64, _p(ws["dc256"]), 256, _p(dup128), 128,
                                          _p(ws["up256"]), None, None, 256, _p(ws["dup256"]), None, None, 256, self.st),
                   "mlp_chain_grad[coarse]")
        # the chain goes on first (d(up256) summed over the four copies -> the 480-wide product below); the head's four weight
        # gradients are queued on the side streams after it
        _lib.check(L.dispu_dup_sum_grad(s.B, s.N, 256, self.up_ratio, _p(ws["dup256"]), 256, _p(ws["dh256"]), 256, self.st), "dup_sum_grad")
        w1, dw1 = self.P[UP + "conv1/weights"], G[UP + "conv1/weights"]
        grp = self.sched.fork_group()
        self._lin_bwd(ws["c64"], 0, 64, CS + "fc_layer2", 3, dcoarse, 0, after=grp)
        self._lin_bwd(ws["c256"], 0, 256, CS + "fc_layer1", 64, ws["dc64"], 0, after=grp)
        self._lin_bwd(ws["up128"], 0, 128, CS + "fc_layer0", 256, ws["dc256"], 0, after=grp)
        self._lin_bwd(ws["up256"], 0, 256, c2, 128, dup128, 0, after=grp)
        self.prod.tn(1, rm, 2, 256, ws["gcode"], 0, 2, 0, ws["dup256"], 0, 256, 0, dw1, 480 * 256, 256, 0, 1,
                     dbias=G[UP + "conv1/biases"], side=True, after=grp, wgrad=True)   # read by Adam only: off the chain like every other dW
        self._lin_bwd(ws["feat"], 0, 480, None, 256, ws["dh256"], 0, ws["dfeat"], 0, bias=False, W=w1, dW=dw1)

    def _bwd_block_partials(self, s, blk):
        # the block's backward on the chain; its weight-gradient partials (a scratch buffer per block) are summed on a side stream
        d, C, col, _, _ = blk
        L, ws, rn = _lib.tape_lib(), s.ws, s.rn
        F, dF, off = (ws["feat"], ws["dfeat"], 456) if d == 1 else (ws["prep"][d], ws["dprep"][d], 0)      # (dprep: zero-filled in forward(), off the chain)
        scr = self.prod.scratch_floats(L.dispu_edge_dense_conv_grad_scratch_floats(rn, C), "edge%d" % d)
        _lib.check(L.dispu_edge_dense_conv_grad_partials(rn, s.N, C, _p(F, off), F.stride(0), _p(ws["kidx"][d]), K_NEIGH + 1, 1, *self._dense_w(d),
                                                         _p(ws["dfeat"], col), 480, _p(dF, off), dF.stride(0), _p(scr), scr.numel(), self.st),
                   "edge_dense_conv_grad_partials")
        return scr

    def _bwd_block_reduce(self, s, blk, scr, ev):
        st_r = self.sched.side_stream(ev)[0] if ev is not None else self.st
        _lib.check(_lib.tape_lib().dispu_edge_dense_conv_grad_reduce(s.rn, blk[1], _p(scr), scr.numel(), *self._dense_w(blk[0], self.G), st_r),
                   "edge_dense_conv_grad_reduce")

    def _bwd_block_prep(self, s, blk):
        d, _, _, in_col, _ = blk
        if d > 1:
            F, dF = s.ws["prep"][d], s.ws["dprep"][d]
            self.prod.act_bias_grad(s.rn, 48, dF, 0, F, 0, 1, dF, 0, None)        # prep = relu(.): its mask (dF came from atomics)
            self._lin_bwd(s.ws["feat"], in_col, 480 - in_col, FE + "layer%d_prep" % d, 48, dF, 0, s.ws["dfeat"], in_col, acc_dx=True)

    # -------------------------------------------------------------------------------------------------- step ----
    def _backward_prep(self, ws):
        L = _lib.tape_lib()
        self._zero(ws["zeroed"])          # the dense blocks' input gradients, the skip branch's d(up128): accumulated with atomics
        if self._t_desc.numel():          # W^T copies for the dX products and the fused head chains
            _lib.check(L.dispu_transpose_batched(self._t_desc.numel() // 3, _p(self._t_desc), _p(self.flat_p), _p(self.flat_pT), self.st),
                       "transpose_batched")

    def zero_grad(self):
        self.sched.st = _lib.stream_ptr(self.device)
        self._zero(self.flat_g)

    def _reducer(self):
        """data parallel (process group of > 1 rank): the flat gradient buffer as TWO all-reduce buckets in the order the backward
        pass completes them -- [refine/*] (3.1 MB: final once the local / non-local / skip cells are through, half a backward
        before the rest) and [generator/*] (1.0 MB: feature extractor, duplicate_up, coarse regressor) -- on a comm lane next to
        the compute streams (parallel.BucketedAllReduce).  None without a process group."""
        if self._ar is None:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(self.pg) == 1 and not self.collectives_at_world_1):
                return None
            from . import parallel
            first = next(k for k in self.names if k.startswith("refine/"))
            split = (self.P[first].data_ptr() - self.flat_p.data_ptr()) // 4
            assert all(k.startswith("refine/") == ((self.P[k].data_ptr() - self.flat_p.data_ptr()) // 4 >= split) for k in self.names)
            self._ar = parallel.BucketedAllReduce(self._red, [(split, self._red.numel()), (0, split)], self.pg, threaded=self.comm_thread)
        return self._ar

    def _bucket_point(self, i):
        """every gradient of bucket i has been QUEUED (main stream, or a weight-gradient stream): start its all-reduce behind them,
        while the backward pass goes on.  Eager steps only: a launch tape replays kernels, not collectives -- there every
        bucket is launched by all_reduce_grads() after the replay."""
        if not self._ar_armed:                           # backward() on its own never communicates: only train_step() arms the early launch
            return
        ar = self._reducer()
        if ar is None or _lib.taping() is not None or ar.launched(i):
            return
        self.sched.flush_all()                           # deferred weight gradients of the bucket go to their streams first, then their pending split reductions
        evs = []
        for s in [torch.cuda.current_stream(self.device)] + self.sched.side_streams:
            ev = torch.cuda.Event()
            ev.record(s)
            evs.append(ev)
        ar.launch(i, after=evs)

    def all_reduce_grads(self):
        """gradient all-reduce (RCCL over xGMI) of the 4.2 MB buffer, in the buckets of _reducer(): whatever backward() has not
        launched yet is launched here, then the current stream waits for all of it.  The 1/world average is folded into the Adam
        launch.  BN moving statistics (per-rank batch statistics) ride at the tail of the refine bucket and are averaged here."""
        ar = self._reducer()
        if ar is None:
            return 1
        world = ar.finish()
        if world > 1:
            self._stats.mul_(1.0 / world)                # summed with the refine bucket; the gradients' 1/world rides in the Adam launch
        return world

    def adam(self, world=1):
        """tf.train.AdamOptimizer(lr, beta1=opts.beta) (model.py:178)."""
        self.adam_t += 1
        b1, b2 = float(self.opts.beta), 0.999
        lr = learning_rate(self.opts, self.epoch)
        lr_t = lr * math.sqrt(1.0 - b2 ** self.adam_t) / (1.0 - b1 ** self.adam_t)
        _lib.check(_lib.tape_lib().dispu_adam(self.flat_p.numel(), _p(self.flat_p), _p(self.flat_g), _p(self.flat_m), _p(self.flat_v),
                                         lr_t, b1, b2, 1e-8, 1.0 / world, _lib.stream_ptr(self.device)), "dispu_adam")

    def train_step_taped(self, inputs, gt, radius):
        """train_step with forward + loss + backward re-issued from a LAUNCH TAPE (dis-pu_amd/_lib.py:Tape): the same launches on the
        same streams in the same order as the eager step, recorded once per (B, N, loss weights) with their ctypes arguments already
        converted, then replayed as a flat loop of foreign calls.  The eager step spends ~10 us of Python per launch (1.4 ms for ~130
        launches at 8 patches -- as long as the GPU's critical chain, so the main queue idles wherever a chain kernel is submitted
        behind side work); the replay spends ~1.5 us and the GPU-side schedule is the eager one (a hipGraph replay of the same step ran
        its branches nearly one after the other on this runtime, 11 - 15 % slower than eager: removed in round 5).  Inputs are
        copied into static buffers (the tape holds raw pointers); the all-reduce and Adam stay eager."""
        B, N = inputs.shape[0], inputs.shape[1]
        gt, radius = self._check_targets(gt, radius, B, N * self.up_ratio)
        wf = weight_fine(self.epoch)
        uniform = bool(getattr(self.opts, "use_uniform", False))
        if uniform:
            self._uniform_tables(B, N)                       # refuses a patch size the term cannot take, before any launch
        emd = bool(getattr(self.opts, "use_emd", False))
        key = (B, N, wf, self.opts.use_repulse, uniform, float(getattr(self.opts, "uniform_w", 0.0)) if uniform else None,
               emd, float(self.opts.emd_w) if emd else None, torch.cuda.current_stream(self.device).cuda_stream)
        t = self._tapes.get(key)
        if t is None:
            st = dict(x=inputs.clone(), gt=gt.clone(), radius=radius.clone())
            mm, mv = self.moving_mean.clone(), self.moving_var.clone()
            for _ in range(2):                               # every workspace / scratch buffer exists and has its final size
                self.zero_grad()
                self.forward(st["x"])
                self.loss_backward(st["gt"], st["radius"])
                self.backward()
            self.moving_mean.copy_(mm)                       # the warm-up passes are not training steps
            self.moving_var.copy_(mv)
            torch.cuda.synchronize(self.device)
            _lib.tape_begin()
            try:
                self.zero_grad()
                self.forward(st["x"])
                self.loss_backward(st["gt"], st["radius"])
                self.backward()
            finally:
                st["tape"] = _lib.tape_end()
            self.moving_mean.copy_(mm)                       # ... and neither is the recording pass
            self.moving_var.copy_(mv)
            st["loss_vals"] = self._workspace(B, N)["loss_vals"]
            t = self._tapes[key] = st
        t["x"].copy_(inputs)
        t["gt"].copy_(gt)
        t["radius"].copy_(radius)
        t["tape"].replay()
        terms = self._terms(t["loss_vals"], wf, uniform, emd)
        world = self.all_reduce_grads()
        self.adam(world)
        self.global_step += 1
        return terms

    def train_step(self, inputs, gt, radius):
        """one iteration of the loop body of Model.train (model.py:215-232) -> loss terms (device scalars)."""
        if isinstance(inputs, torch.Tensor) and inputs.dim() == 3:       # refuse bad targets before any launch
            self._check_targets(gt, radius, inputs.shape[0], inputs.shape[1] * self.up_ratio)
            if getattr(self.opts, "use_uniform", False):
                self._uniform_tables(inputs.shape[0], inputs.shape[1])
        self.zero_grad()
        self.forward(inputs)
        terms = self.loss_backward(gt, radius)
        self._ar_armed = True                            # data parallel: the refine bucket's all-reduce starts inside backward()
        try:
            self.backward()
        finally:
            self._ar_armed = False
        world = self.all_reduce_grads()
        self.adam(world)
        self.global_step += 1
        return terms


# ------------------------------------------------------------------------------------------------------ train phase ----
# Counterpart of Model.train / Model.train_one_epoch (DisPU/model.py:181-303): the epoch loop around Trainer.train_step.
LOG_FORMAT = "epoch %04d g_loss=%.9f  coarse_cd=%.9f  coarse_hd=%.9f  fine_cd=%.9f fine_hd=%.9f  time=%.4f"


def format_log_line(epoch, g_loss, coarse_cd, coarse_hd, fine_cd, fine_hd, seconds, dis_fine_emd=None):
    """the per-epoch line of log_train.txt (model.py:220-222; the last field is the epoch's duration in MINUTES).  With the EMD term
    on (TrainOpts.use_emd) the line gains a `dis_fine_emd=` column at its end; without it the line is the reference's."""
    line = LOG_FORMAT % (epoch, g_loss, coarse_cd, coarse_hd, fine_cd, fine_hd, seconds / 60.0)
    return line if dis_fine_emd is None else line + "  dis_fine_emd=%.9f" % dis_fine_emd


def format_args(opts):
    """args.txt (model.py:198-200): one `name: value` line per option, sorted by name."""
    d = opts if isinstance(opts, dict) else {k: getattr(opts, k) for k in dir(opts) if not k.startswith("_") and not callable(getattr(opts, k))}
    return "".join("%s: %s\n" % (k, d[k]) for k in sorted(d))


def steps_per_epoch(n_examples, batch_size):
    """model.py:239: int(n / B) - 1 (one batch fewer than fit: Fetcher.next_batch skips the first batch of every epoch)."""
    return int(int(n_examples) / int(batch_size)) - 1


def _hausdorff_terms(trainer, inputs, gt, radius):
    """100 * hausdorff_loss of the step's coarse and fine clouds (model.py:76,79: logged, never differentiated)."""
    from . import loss_utils
    ws = trainer._workspace(inputs.shape[0], inputs.shape[1])
    with torch.no_grad():
        return 100.0 * loss_utils.hausdorff_loss(ws["coarse"], gt, radius=radius), 100.0 * loss_utils.hausdorff_loss(ws["fine"], gt, radius=radius)


def train_one_epoch(trainer, fetcher, batch_size, train_step_fn="eager", hd_fn=_hausdorff_terms):
    """model.py:229-303 -> (g_loss, coarse_cd, coarse_hd, fine_cd, fine_hd, seconds, steps): the epoch's means and its duration.
    The five sums are accumulated in a device tensor and read ONCE, after the last step: no per-step host synchronisation.
    A step whose terms hold "dis_fine_emd" (TrainOpts.use_emd) adds that mean as a sixth value in front of `seconds`."""
    import time
    if train_step_fn not in ("eager", "taped"):
        raise ValueError("train_step_fn must be 'eager' or 'taped'")
    step = trainer.train_step if train_step_fn == "eager" else trainer.train_step_taped
    n = steps_per_epoch(len(fetcher), batch_size)
    acc = None
    t0 = time.time()
    for _ in range(n):
        x, gt, radius = fetcher.next_batch()
        terms = step(x, gt, radius)
        chd, fhd = hd_fn(trainer, x, gt, radius)
        cols = (terms["pu_loss"], terms["dis_coarse_cd"], chd, terms["dis_fine_cd"], fhd)
        if "dis_fine_emd" in terms:
            cols += (terms["dis_fine_emd"],)
        row = torch.stack([torch.as_tensor(v, dtype=torch.float32).reshape(()) for v in cols])
        acc = row if acc is None else acc.to(row.device) + row
    if acc is None:
        vals = [0.0] * 5                                 # AverageMeter.avg of an empty epoch
    else:
        vals = (acc / n).tolist()                        # the epoch's one read-back (also waits for its last step)
    return tuple(vals) + (time.time() - t0, n)


def _step_and_batch(trainer, fetcher, opts, train_step_fn):
    """-> (the step function train_step_fn names, the batch size B): what both epoch loops refuse before they touch anything."""
    if train_step_fn not in ("eager", "taped"):
        raise ValueError("train_step_fn must be 'eager' or 'taped'")
    B = int(getattr(opts, "batch_size", getattr(fetcher, "batch_size", 0)))
    if B <= 0:
        raise ValueError("opts.batch_size (or fetcher.batch_size) must be positive")
    return (trainer.train_step if train_step_fn == "eager" else trainer.train_step_taped), B


@contextlib.contextmanager
def _run_files(trainer, fetcher, opts, log_dir, restore, save_fn, restore_fn, log, rank=0):
    """The set-up of fit and fit_parallel -> (restore epoch, save_fn, emit): the checkpoint module's functions where none are given;
    the restore (on EVERY rank) and the fetcher's catch-up; then, on rank 0 alone, <log_dir>/log_train.txt ('w', or 'a' when
    restoring: open until the block ends) and args.txt.  emit(line) writes a line to the log and hands it to `log` (rank 0; a
    no-op elsewhere)."""
    from . import checkpoint
    save_fn = checkpoint.save_train_state if save_fn is None else save_fn
    restore_fn = checkpoint.restore_train_state if restore_fn is None else restore_fn
    if rank == 0:
        os.makedirs(log_dir, exist_ok=True)
    restore_epoch = 0
    if restore:
        restore_epoch = int(restore_fn(log_dir, trainer))
        # a fetcher that counts its epochs (DeviceFetcher: permutation stream and draws keyed by the epoch) is brought to the restored
        # one, so a resumed run sees the batches the uninterrupted run would have seen
        while getattr(fetcher, "epoch", restore_epoch) < restore_epoch:
            fetcher.reset()
    fout = open(os.path.join(log_dir, "log_train.txt"), "a" if restore else "w") if rank == 0 else None
    try:
        if rank == 0:
            with open(os.path.join(log_dir, "args.txt"), "w") as f:
                f.write(format_args(opts))

        def emit(line):
            if rank == 0:
                fout.write(line + "\n")
                fout.flush()
                if log is not None:
                    log(line)

        yield restore_epoch, save_fn, emit
    finally:
        if fout is not None:
            fout.close()


def _end_epoch(trainer, fetcher, opts, emit, save, records, best, vals, seconds, steps):
    """The epoch tail of fit and fit_parallel, given the epoch's five logged values: fetcher.reset(), trainer.epoch += 1, the log
    line, save(epoch) when epoch % opts.epoch_per_save == 0 and fine_cd is strictly below `best`, the record.  -> the new best."""
    g, ccd, chd, fcd, fhd = vals[:5]
    emd = vals[5] if len(vals) > 5 else None         # the EMD term's column (TrainOpts.use_emd)
    fetcher.reset()
    trainer.epoch += 1
    epoch = int(trainer.epoch)
    emit(format_log_line(epoch, g, ccd, chd, fcd, fhd, seconds, emd))
    saved = None
    if epoch % int(opts.epoch_per_save) == 0 and fcd < best:
        best = fcd
        saved = save(epoch)
    records.append(dict(epoch=epoch, g_loss=g, coarse_cd=ccd, coarse_hd=chd, fine_cd=fcd, fine_hd=fhd, seconds=seconds,
                        steps=steps, saved=saved))
    if emd is not None:
        records[-1]["dis_fine_emd"] = emd
    return best


def fit(trainer, fetcher, opts, log_dir, restore=False, train_step_fn="eager", save_fn=None, restore_fn=None, hd_fn=_hausdorff_terms,
        log=None):
    """Model.train (model.py:181-227): epochs restore_epoch .. opts.training_epoch - 1 of int(len / B) - 1 steps each; after every epoch
    fetcher.reset(), trainer.epoch += 1 (weight_fine and the learning rate follow it), one line in <log_dir>/log_train.txt ('w', or
    'a' when restoring), and checkpoint.save_train_state when epoch % opts.epoch_per_save == 0 and the epoch's mean fine_cd is
    strictly below the best one saved so far.  args.txt lists the options.  Returns the per-epoch records.  On restore a fetcher
    with an `epoch` counter is reset() up to the restored epoch (the host Fetcher has none: it goes on from numpy's global state).

    Single process only: it raises when a process group of more than one rank is active (fit_parallel is the data-parallel loop).
    save_fn(log_dir, trainer, epoch) / restore_fn(log_dir, trainer) -> restore epoch / hd_fn default to the checkpoint module and
    loss_utils.hausdorff_loss; `log` is called with every line written."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("fit() is single-process: data-parallel training loops are out of scope")
    _, B = _step_and_batch(trainer, fetcher, opts, train_step_fn)
    records, best = [], math.inf
    with _run_files(trainer, fetcher, opts, log_dir, restore, save_fn, restore_fn, log) as (restore_epoch, save_fn, emit):
        emit("train_dataset: %d" % len(fetcher))
        for _ in range(restore_epoch, int(opts.training_epoch)):
            *vals, seconds, steps = train_one_epoch(trainer, fetcher, B, train_step_fn, hd_fn)
            best = _end_epoch(trainer, fetcher, opts, emit, lambda epoch: save_fn(log_dir, trainer, epoch), records, best,
                              vals, seconds, steps)
    return records


# -------------------------------------------------------------------------------------- data-parallel train phase ----
_HD_COLUMNS = (2, 4)       # of a step-meter row [g_loss, coarse_cd, coarse_hd, fine_cd, fine_hd]: max over ranks; the others: mean


def step_meters(trainer, inputs, radius, row):
    """row[0:5] = [pu_loss, 1000 CD_coarse, 100 HD_coarse, 1000 CD_fine, 100 HD_fine] of the step `trainer` has just run on
    `inputs` / `radius` (train_step or train_step_taped), in ONE launch on the current stream (dispu_step_meters,
    csrc/step_meters.hip): the loss values are copied from the step's loss_vals, the Hausdorff terms are reduced from the
    nearest-neighbour distances the step's Chamfer terms left in the workspace -- bit-equal to what _hausdorff_terms recomputes
    with two more nn_distance launches.  `row`: 5 contiguous float32 on the trainer's device (a row of the epoch's table).
    Never part of a launch tape: the row pointer changes with every step."""
    B, N = int(inputs.shape[0]), int(inputs.shape[1])
    M = N * trainer.up_ratio
    req(isinstance(row, torch.Tensor) and row.dtype == torch.float32 and row.numel() == 5 and row.is_contiguous()
        and row.device == trainer.device, "row must be 5 contiguous float32 on %s" % trainer.device)
    radius = f32(radius, "radius")
    req(radius.dim() == 1 and radius.shape[0] == B and radius.device == trainer.device and radius.is_contiguous(),
        "radius must be a contiguous (%d,) tensor on %s" % (B, trainer.device))
    if (B, N) not in trainer._ws:
        raise RuntimeError("step_meters: no step has run on a (%d, %d) batch" % (B, N))
    ws = trainer._ws[(B, N)]
    c, f = ws["cd"]
    _lib.check(_lib.lib().dispu_step_meters(B, M, M, _p(c["d_gt"]), _p(c["d_pred"]), _p(f["d_gt"]), _p(f["d_pred"]), _p(radius),
                                            _p(ws["loss_vals"], 2), _p(row), _lib.stream_ptr(trainer.device)), "dispu_step_meters")
    return row


def _step_meters_fn(trainer, x, gt, radius, row):
    step_meters(trainer, x, radius, row)


def reduce_meter_tables(tables, steps, width=5):
    """tables [world, steps * width] (every rank's step-meter table) -> the epoch's logged values, in float64: per step the mean
    over ranks of the loss / CD columns and the MAX over ranks of the two Hausdorff columns (hausdorff_loss is a max over the
    batch, and the global batch is the union of the ranks' shards), then the mean over steps.  width 6: the EMD term's column
    (TrainOpts.use_emd) behind the five, a mean over ranks like the other loss columns."""
    if steps <= 0:
        return [0.0] * width                             # AverageMeter.avg of an empty epoch
    t = np.asarray(tables, np.float64).reshape(-1, steps, width)
    per_step = t.mean(axis=0)
    per_step[:, _HD_COLUMNS] = t[:, :, _HD_COLUMNS].max(axis=0)
    return [float(v) for v in per_step.mean(axis=0)]


def fill_meter_table(trainer, fetcher, table, steps, step, meter_fn=_step_meters_fn, width=5):
    """the steps of one epoch as fit_parallel runs them: next_batch, the step function, meter_fn into row s of `table`
    ([steps * width + 2] float32 on the trainer's device); the fetcher's two status flags go behind the rows (zeros for a fetcher
    without status_flags()).  width 6 (TrainOpts.use_emd): the step's dis_fine_emd, a device scalar, is copied behind the five
    meters.  Launches only: nothing here waits for the device."""
    for s in range(steps):
        x, gt, radius = fetcher.next_batch()
        terms = step(x, gt, radius)
        meter_fn(trainer, x, gt, radius, table[s * width:s * width + 5])
        if width > 5:
            table[s * width + 5:s * width + 6].copy_(torch.as_tensor(terms["dis_fine_emd"], dtype=torch.float32).reshape(1))
    flags_of = getattr(fetcher, "status_flags", None)
    table[steps * width:].copy_(torch.as_tensor(flags_of() if flags_of is not None else (0, 0)))


def fit_parallel(trainer, fetcher, opts, log_dir, restore=False, train_step_fn="eager", group=None, save_fn=None, restore_fn=None,
                 meter_fn=None, log=None):
    """Model.train (model.py:181-227) for world >= 1 ranks of `group` (None: the default process group; no group initialised: one
    rank, a complete single-process loop).  Every rank calls it with its own replica and its own shard of the fetcher.

    Sharding.  opts.batch_size is the GLOBAL batch B (the reference's --batch_size); rank r draws positions
    [batch * B + r * B / world, + B / world) of the epoch (dataset.DeviceFetcher(shard=(r, world)): same seed and permutation on
    every rank, no communication).  Every rank runs steps_per_epoch(len(fetcher), B) steps per epoch.
    Per step: fetcher.next_batch(), the step function (its gradient all-reduce keeps the replicas bit-identical), and
    meter_fn(trainer, x, gt, radius, row) -- default step_meters, one launch -- into row `step` of a device table.  Nothing in the
    epoch waits for the device.
    Epoch end: ONE collective, an all-gather of the rank's [steps * 5 + 2] floats (the table and the fetcher's two status flags).
    Every rank reduces on the host in float64 (reduce_meter_tables: mean over ranks, max over ranks for the Hausdorff columns, per
    step; then the mean over steps), so all ranks hold identical values and take the same save decision.  A status flag set on ANY
    rank raises the same RuntimeError on EVERY rank in that epoch.
    Artefacts: rank 0 alone writes log_train.txt, args.txt and checkpoints (fit's formats and save rule: epoch % epoch_per_save
    == 0 and fine_cd < best); a barrier follows each save.  trainer.epoch += 1 and fetcher.reset() happen on every rank; every
    rank returns the same records (`saved` is rank 0's; `seconds` alone is each rank's own clock).
    Restore: EVERY rank calls restore_fn(log_dir, trainer).  It only reads, and the calls must be symmetric: Trainer.load_params
    builds the gradient reducer eagerly, which under gloo creates a process group -- a collective every rank has to reach.  The
    fetcher is then reset() up to the restored epoch, as in fit.

    ValueError on every rank before the first step: B % world != 0; world > 1 with a fetcher whose `shard` is not (rank, world)
    (the host Fetcher has none); a trainer whose process group is not `group`."""
    import time
    import torch.distributed as dist
    step, B = _step_and_batch(trainer, fetcher, opts, train_step_fn)
    active = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if active else 1
    rank = dist.get_rank(group) if active else 0
    if B % world:
        raise ValueError("the global batch of %d patches does not divide over %d ranks" % (B, world))
    if world > 1:
        shard = getattr(fetcher, "shard", None)
        if shard is None or tuple(shard) != (rank, world):
            raise ValueError("rank %d of %d needs a fetcher with shard=(%d, %d), got %r" % (rank, world, rank, world, shard))
        norm = lambda g: None if g is dist.group.WORLD else g          # None names the default group
        if norm(getattr(trainer, "pg", None)) is not norm(group):
            raise ValueError("the trainer all-reduces over another process group than the loop's")
    meter_fn = _step_meters_fn if meter_fn is None else meter_fn
    records, best = [], math.inf
    with _run_files(trainer, fetcher, opts, log_dir, restore, save_fn, restore_fn, log, rank) as (restore_epoch, save_fn, emit):
        n = max(steps_per_epoch(len(fetcher), B), 0)
        W = 6 if getattr(getattr(trainer, "opts", None), "use_emd", False) else 5      # the EMD term's column behind the five meters
        table = torch.zeros(n * W + 2, dtype=torch.float32, device=getattr(trainer, "device", "cpu"))

        def save(epoch):
            saved = save_fn(log_dir, trainer, epoch) if rank == 0 else None
            if world > 1:
                box = [saved]
                dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                saved = box[0]
                dist.barrier(group=group)              # no rank runs ahead of a checkpoint another process may read
            return saved

        emit("train_dataset: %d" % len(fetcher))
        for _ in range(restore_epoch, int(opts.training_epoch)):
            t0 = time.time()
            fill_meter_table(trainer, fetcher, table, n, step, meter_fn, W)
            if world > 1:
                from . import parallel
                every = parallel._all_gather_rows(table.view(1, -1), world, group).cpu().numpy()      # the epoch's one collective
            else:
                every = table.view(1, -1).cpu().numpy()                                               # ... and its one read-back
            bad = [(r, int(every[r, n * W] != 0), int(every[r, n * W + 1] != 0)) for r in range(world) if every[r, n * W:].any()]
            if bad:
                raise RuntimeError("epoch %d: the batch sampler reported a failure on rank(s) %s (rank, candidate rounds exhausted, "
                                   "permutation entry out of range)" % (int(trainer.epoch), bad))
            vals = reduce_meter_tables(every[:, :n * W], n, W)
            best = _end_epoch(trainer, fetcher, opts, emit, save, records, best, vals, time.time() - t0, n)
    return records
