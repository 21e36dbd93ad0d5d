"""Dis-PU generator forward pass (inference) on MI355X.

Counterpart of DisPU/generator.py:21-88 (`Generator(opts, is_training)(inputs) -> (coarse, fine)`), issuing the
same op sequence as the reference graph (Common/ops.py: feature_extraction_GCN :1437, dense_conv :1897,
duplicate_up :1152, coordinate_regressor :1089, PointShuffle2 :1012, PointNonLocalCell :302) through the C ABI
of libdispu_hip.so.  torch is used for device memory and the launch stream only.

What is different from the reference's execution (not its results):
  * no tf.concat / tf.tile / gather_nd tensors: dense-block outputs are written straight into one
    [rows, 480] feature buffer, prep convs read column slices of it;
  * the xyz k-NN of PointShuffle2 runs on the device (reference: tf.py_func -> nanoflann on the host);
  * duplicate_up's 482-wide conv is evaluated once per SOURCE point (same fmaf chain, 4x fewer FLOPs);
  * PointShuffle2's conv0 over [B,N,16,134] is evaluated per source point (linear in its input groups,
    16x fewer FLOPs; reassociated -> tolerance-checked).
Everything up to and including `coarse` is bit-identical to oracle/generator.py (fp32 MFMA == fmaf chain).
"""
import collections
import contextlib
import math

import numpy as np
import torch

from . import _lib

K_NEIGH = 16
GROWTH = 24
DENSE_BLOCKS = 4
BN_EPS = 1e-3


def gen_grid(up_ratio):
    """Common/ops.py:60-76."""
    sq = int(math.sqrt(up_ratio)) + 1
    for i in range(sq, 0, -1):
        if up_ratio % i == 0:
            num_x, num_y = i, up_ratio // i
            break
    gx = np.linspace(-0.2, 0.2, num_x, dtype=np.float32)
    gy = np.linspace(-0.2, 0.2, num_y, dtype=np.float32)
    x, y = np.meshgrid(gx, gy)
    return np.stack([x, y], -1).reshape(-1, 2).astype(np.float32)


def _off(t, o):
    """the address of t's element o (t is float32 or int32: 4-byte elements)"""
    return _lib.C.c_void_p(t.data_ptr() + 4 * o)


Path = collections.namedtuple("Path", "stem heads in_chain attention local after add3 nl_late")


class _Opts(object):
    patch_num_point = 256
    up_ratio = 4


def linear_profile_name(plan, batch, M, K, N):
    """The profile row of a dispu_linear call from its plan (_lib.linear_plan): the instantiation rocprofv3 reports,
    "linear<BM, BN, 2, 2, BK, transb, edge, epi>[MxKxN]" or "linear_skinny<NG, transb>[MxKxN]".  A call split into a tiled head and a
    skinny tail is named after its head."""
    tf = lambda v: "true" if v else "false"
    tiled = [l for l in plan if l[0] == "tiled"]
    if tiled:
        _, _, _, bm, bn, bk, tb, edge, epi = tiled[0]
        return "linear<%d, %d, 2, 2, %d, %s, %s, %d>[%dx%dx%d]" % (bm, bn, bk, tf(tb), tf(edge), epi, M * batch, K, N)
    if plan:
        return "linear_skinny<%d, %s>[%dx%dx%d]" % (plan[-1][3], tf(plan[-1][4]), M, K, N)
    return "linear"


class Generator(object):
    """Generator(opts, is_training=False)(inputs[B,N,3]) -> (coarse[B,4N,3], fine[B,4N,3]).

    `params` maps the TF variable names of the reference graph ('generator/feature_extraction_coarse/layer0/weights',
    ..., see oracle/generator.py:layer_shapes) to arrays: weights [C_in_total, C_out], biases [C_out], plus the
    four BatchNorm vectors of 'refine/PointShuffle/weight_net/wconv0/bn/'.

    Threading / streams: one Generator serves ONE caller at a time on the stream current at the call (like a session's run()).  The
    forward forks its non-local branch onto a private auxiliary stream and joins it before it returns; workspace buffers are reused
    by the next call with the same (B, N), and the results (return_views = False) are fresh tensors ordered on the caller's stream.
    Use one Generator per concurrent caller (two in flight: bench.py's alt_two_in_flight holds two)."""

    MAX_POINTS = 2048 * 256   # input points (B*N) per launch sequence: keeps every row*stride product below 2^31 and the workspace
                              # (~17 MB per 256 input points, dominated by F' [B*4N, 2048]) at ~35 GB; larger batches run in chunks
                              # of max(1, MAX_POINTS // N) patches

    def __init__(self, opts=None, is_training=False, name="Generator", params=None, device=None, dtype="f32"):
        # dtype = "bf16" (inference only): ONE rounded product -- F' is stored as bf16 by the local cell (dispu_ps_local_bf16) and
        # after_conv multiplies it with the bf16 image of its weight, fp32 accumulation; everything else is the fp32 path, so the
        # numerics do not depend on the batch size.  Checked before the device is touched.
        if dtype not in ("f32", "bf16"):
            raise ValueError("Generator dtype must be 'f32' or 'bf16', got %r" % (dtype,))
        if dtype == "bf16" and is_training:
            raise ValueError("Generator(dtype='bf16') is the inference mode; mixed-precision training is Trainer(dtype='bf16')")
        self.dtype = dtype
        self.opts = opts if opts is not None else _Opts()
        self.is_training = is_training
        self.name = name
        self.num_point = int(self.opts.patch_num_point)
        self.up_ratio = int(self.opts.up_ratio)
        if self.up_ratio != 4:
            raise NotImplementedError("the shipped generator graph is built for up_ratio 4 (DisPU/configs.py)")
        self.out_num_point = self.num_point * self.up_ratio
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.P = {}
        self._ws = {}
        self.profile = None          # set to [] to collect (name, start_event, end_event) per launch
        self.fused_local = True      # PointShuffle2 local cell in one kernel (False: the 4-kernel chain, for A/B tests)
        self.fused_attention = True  # non-local cell attention on chip (False: GEMM -> softmax -> GEMM through HBM)
        self.fused_project = True    # conv_back_project as the attention kernel's epilogue (False: separate GEMM)
        # EXPLORATORY: after_conv's products as 3-way split-bf16 MFMAs (fp32-accurate, not the fmaf chain; the branch is
        # tolerance-checked).  Off by default; bench.py --split-bf16 reports it beside the strict-fp32 line.
        self.split_bf16 = False
        self._planes = {}
        self._aft_bt = None          # dtype = "bf16": after_conv's weight as bf16 [256][2048] (dispu_bf16_pack), made by load_params
        # non-local cell on a second stream next to the grouping / skip / local cell (round 4: on by default, -1 % since the head chains
        # form their own inputs -- the branch now joins right before the fine chain; rounds 1 - 3 measured it +1 %)
        self.branches = True           # False: everything on the launch stream (profiling passes: every kernel alone on the device)
        self._aux = None
        self.fused_heads = True      # one launch per head chain
        self.keep_intermediates = False   # fused heads: also write the aggregation output (tests compare it)
        # round 4: the head chains form their own input tiles (csrc/mlp_chain.hip XMODE): duplicate_up's rows from the per-source-point
        # product (no dup_grid launch, no [B*4N, 256] tensor) and relu(after_conv) + skip + non-local in the fine chain's loader (the
        # residual reads leave the after_conv GEMM's epilogue).  False = the producer kernels of rounds 1 - 3 (bit-identical results; A/B tests)
        self.chain_inputs = True
        # forward() computes into a reusable per-(B, N) workspace.  By default the two results are returned as fresh
        # tensors (like sess.run in the reference); return_views = True hands out the workspace buffers themselves
        # (no copies -- bench.py / hipGraph capture), which the NEXT call with the same (B, N) overwrites.
        self.return_views = False
        # optional caller-owned [B, 4N, 3] float32 buffer the fine head writes its clouds into instead of the workspace's (the
        # sharded serving loop alternates two of them so that the all-gather of one step overlaps the next step: parallel.GatherPipeline)
        self.fine_out = None
        self._trainer = None
        if params is not None:
            self.load_params(params)

    # ------------------------------------------------------------------------------------------ weights ----
    def load_params(self, params):
        dev = self.device
        if self.is_training:
            # training graph (DisPU/generator.py:22-31 with is_training=True; DisPU/model.py:68): BatchNorm on batch
            # statistics with moving averages updated (decay 0.95), every activation kept for the backward pass.  The
            # forward is Trainer.forward (train.py); `trainer` exposes loss / backward / Adam on the same variables.
            from .train import Trainer, TrainOpts
            topts = TrainOpts()
            for k in dir(self.opts):
                if not k.startswith("_"):
                    setattr(topts, k, getattr(self.opts, k))
            self._trainer = Trainer(opts=topts, params=params, device=dev)
            self.P = self._trainer.P
            return
        self.P = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev) for k, v in params.items()}
        self._planes = {}
        bn = "refine/PointShuffle/weight_net/wconv0/bn/"
        g, b = params[bn + "gamma"].astype(np.float64), params[bn + "beta"].astype(np.float64)
        mu, var = params[bn + "moving_mean"].astype(np.float64), params[bn + "moving_variance"].astype(np.float64)
        scale = g / np.sqrt(var + BN_EPS)
        self.bn_scale = torch.from_numpy(scale.astype(np.float32)).to(dev)
        self.bn_shift = torch.from_numpy((b - mu * scale).astype(np.float32)).to(dev)
        self.grid = torch.from_numpy(gen_grid(self.up_ratio)).to(dev)
        w1 = self.P["generator/upshuffle_0/conv1/weights"]
        self.w_up_feat = w1[:480].contiguous()
        self.w_up_grid = w1[480:482].contiguous()
        w0 = self.P["refine/PointShuffle/conv0/weights"]
        self.w_c0_feat = w0[6:134].contiguous()
        # the three 1x1 convs that read up128 (conv_kv, conv_query, the feature part of PointShuffle2's conv0) as ONE
        # [128, 320] GEMM: columns 0:128 K|V, 128:192 Q, 192:320 conv0 features (its bias is added in ps_prep)
        nlp = "refine/PointShuffle/PointShuffle/"
        self.w_up3 = torch.cat([self.P[nlp + "conv_kv/weights"], self.P[nlp + "conv_query/weights"], self.w_c0_feat], dim=1).contiguous()
        self.b_up3 = torch.cat([self.P[nlp + "conv_kv/biases"], self.P[nlp + "conv_query/biases"],
                                torch.zeros(128, dtype=torch.float32, device=dev)]).contiguous()
        wsk = self.P["refine/PointShuffle/skip/weights"]
        self.w_skip_pad = torch.cat([wsk, torch.zeros((10, wsk.shape[1]), dtype=torch.float32, device=dev)], dim=0).contiguous()
        if self.dtype == "bf16":
            # packed once per parameter set, on the stream current here: forward (and a captured graph) holds no pack launch
            w = self.P["refine/PointShuffle/after_conv/weights"]
            bt = torch.empty((256, 2048), dtype=torch.bfloat16, device=dev)
            _lib.check(_lib.lib().dispu_bf16_pack(2048, 256, _lib.ptr(w), 256, 1, _lib.ptr(bt), _lib.stream_ptr(dev)), "dispu_bf16_pack")
            self._aft_bt = bt

    def _w(self, scope):
        return self.P[scope + "/weights"], self.P[scope + "/biases"]

    # ---------------------------------------------------------------------------------------- workspace ----
    def _workspace(self, B, N):
        key = (B, N)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev, f32, i32 = self.device, torch.float32, torch.int32
        M = N * self.up_ratio
        rn, rm, k = B * N, B * M, K_NEIGH

        def E(*shape, dtype=f32):
            return torch.empty(shape, dtype=dtype, device=dev)

        ws = dict(
            feat=E(rn, 480), prep=E(rn, 48), prep_b=E(rn, 48), kidx=E(rn, k + 1, dtype=i32), h256=E(rn, 256),
            up256=E(rm, 256), up128=E(rm, 128), c256=E(rm, 256), c64=E(rm, 64), coarse=E(B, M, 3),
            psidx=E(rm, k, dtype=i32), up3=E(rm, 320), att=E(rm, 64), nl=E(rm, 256),
            skipin=torch.zeros((rm, 144), dtype=f32, device=dev), skip=E(rm, 256), am=E(rm, 128),
            fp=E(rm, 2048, dtype=torch.bfloat16 if self.dtype == "bf16" else f32), aft=E(rm, 256), agg=E(rm, 256),
            f256=E(rm, 256), f64=E(rm, 64), fine=E(B, M, 3))
        ws["kv"], ws["q"], ws["gm"] = ws["up3"][:, 0:128], ws["up3"][:, 128:192], ws["up3"][:, 192:320]   # views, row stride 320
        self._ws[key] = ws
        return ws

    def _extra(self, store, key, shape, dtype=torch.float32):
        """store[key], a buffer that only some paths need: allocated when such a path first runs (again if a launch needs a larger one)"""
        t = store.get(key)
        if t is None or t.numel() < math.prod(shape):
            t = store[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return t

    # ------------------------------------------------------------------------------------------- launch ----
    def _call(self, name, fn, *args):
        """One C-ABI launch; when self.profile is a list, bracket it with HIP events on the launch stream."""
        if self.profile is None:
            _lib.check(fn(*args), name)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(fn(*args), name)
        e1.record()
        self.profile.append((name, e0, e1))

    def _linear(self, st, X, K, W, bias, act, Y, N, M=None, ldx=None, ldw=None, ldy=None, batch=1, sx=0, sw=0, sy=0,
                transb=0, R1=None, R2=None, xoff=0, woff=0, yoff=0):
        """Y[:, yoff:yoff+N] = R2 + R1 + act(X[:, xoff:xoff+K] . W + bias) via dispu_linear (element offsets in floats)."""
        M = X.shape[0] if M is None else M
        ldx = X.stride(0) if ldx is None else ldx
        ldw = W.stride(0) if ldw is None else ldw
        ldy = Y.stride(0) if ldy is None else ldy
        x, w, b, y, r1, r2 = _off(X, xoff), _off(W, woff), _lib.ptr(bias), _off(Y, yoff), _lib.ptr(R1), _lib.ptr(R2)
        ldr1 = R1.stride(0) if R1 is not None else 0
        ldr2 = R2.stride(0) if R2 is not None else 0
        name = "linear"
        if self.profile is not None:     # "linear<BM, BN, 2, 2, BK, transb, edge, epi>[MxKxN]": the instantiation rocprofv3 reports
            plan = _lib.linear_plan(batch, M, K, N, x, ldx, sx, w, ldw, sw, transb, b, None, None, act, y, ldy, sy, r1, ldr1, 0, r2, ldr2, 0,
                                    None, 0, 0)
            name = linear_profile_name(plan, batch, M, K, N)
        self._call(name, _lib.lib().dispu_linear, batch, M, K, N, x, ldx, sx, w, ldw, sw, transb, b, act, y, ldy, sy, r1, ldr1, 0, r2, ldr2, 0, st)

    def __call__(self, inputs):
        return self.forward(inputs)

    @property
    def trainer(self):
        """the Trainer behind a Generator(is_training=True): loss_backward / backward / adam / train_step (train.py)."""
        return self._trainer

    def path(self, B, N):
        """What a forward over B patches of N points launches, decided once from the switches and the shape (M = 4N points per upsampled
        patch, rm = B * M rows).  No device access, and nothing is kept: the switches may change between two calls.
          stem       one launch per dense block (search + edge features + dense_conv, csrc/edge.hip KNN variant: even clouds of at most
                     256 points), else the dispu_knn_feat_strided_ws -> dispu_edge_dense_conv pair
          heads      one launch per head chain (whole 128-row tiles);  in_chain: the chains also form their own input tiles
          attention  "project" | "flash" (on chip: M % 32 == 0) | "gemm" (GEMM -> softmax -> GEMM through a score buffer)
          local      "bf16" | "fused" | "pair" (the four-kernel chain through [rm * 16, .] pair tensors)
          after      after_conv: "bf16_stream" | "bf16s" | "x3" (split_bf16) | "plain" | "residual" (+ skip + nl in the GEMM's epilogue)
          add3       (aft + skip) + nl by dispu_add3 into ws["sum"], which the fine head then reads instead of ws["aft"]
          nl_late    the non-local branch joins in front of the fine chain (its loader is nl's first reader), not of after_conv"""
        bf16 = self.dtype == "bf16"
        if bf16 and (self.split_bf16 or not self.fused_local):
            raise ValueError("Generator(dtype='bf16') stores F' as bf16 in the fused local cell: it excludes split_bf16 and fused_local = False")
        M = N * self.up_ratio
        tiles = B * M % 128 == 0
        heads = bool(self.fused_heads and tiles)
        in_chain = bool(heads and self.chain_inputs)
        on_chip = self.fused_attention and M % 32 == 0
        if bf16:
            after = "bf16_stream" if tiles else "bf16s"
        elif self.split_bf16 and tiles:
            after = "x3"
        else:
            after = "plain" if in_chain else "residual"
        return Path(stem=N <= 256 and N % 2 == 0, heads=heads, in_chain=in_chain,
                    attention="project" if on_chip and self.fused_project else "flash" if on_chip else "gemm",
                    local="bf16" if bf16 else "fused" if self.fused_local else "pair", after=after,
                    add3=bf16 and not in_chain, nl_late=bool(self.branches and in_chain))

    def forward(self, inputs):
        if not self.P:
            raise RuntimeError("Generator has no parameters: call load_params() first")
        if self.is_training:
            coarse, fine = self._trainer.forward(inputs)
            return (coarse, fine) if self.return_views else (coarse.clone(), fine.clone())
        if not (isinstance(inputs, torch.Tensor) and inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() == 3
                and inputs.shape[2] == 3):
            raise ValueError("Generator expects a float32 [B,N,3] tensor on a ROCm device")
        inputs = inputs.contiguous()
        B, N, _ = inputs.shape
        if N <= K_NEIGH:
            raise ValueError("Generator needs patches of at least %d points (the dense blocks take the k + 1 = %d nearest "
                             "neighbours of every point), got N = %d" % (K_NEIGH + 1, K_NEIGH + 1, N))
        chunk = max(1, self.MAX_POINTS // N)                    # patches per launch sequence
        if B > chunk:                                           # patches are independent: run the batch in chunks
            if self.return_views:
                raise ValueError("return_views needs B <= %d at N = %d (one workspace)" % (chunk, N))
            outs = [self.forward(inputs[lo:lo + chunk]) for lo in range(0, B, chunk)]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        path = self.path(B, N)
        M = N * self.up_ratio
        fine = self.fine_out
        if fine is not None and not (isinstance(fine, torch.Tensor) and fine.device == inputs.device and fine.dtype == torch.float32
                                     and tuple(fine.shape) == (B, M, 3) and fine.is_contiguous()):
            raise ValueError("fine_out must be a contiguous float32 [%d, %d, 3] tensor on %s" % (B, M, inputs.device))
        ws = self._workspace(B, N)
        coarse, fine = ws["coarse"], ws["fine"] if fine is None else fine
        st = _lib.stream_ptr(inputs.device)
        self._features(ws, path, inputs, st)
        self._coarse_head(ws, path, B, N, st)
        ev_up3, ev_nl = self._non_local(ws, path, B, N, st)     # what its stream records once up3 / nl are written (None: it ran on st)
        self._knn_skip(ws, B, M, st)
        self._join(ev_up3)
        self._local(ws, path, B, N, st)
        self._join(None if path.nl_late else ev_nl)
        self._after_conv(ws, path, B * M, st)
        self._join(ev_nl if path.nl_late else None)             # nl is first read by the fine chain's loader
        self._fine_head(ws, path, B * M, fine, st)
        return (coarse, fine) if self.return_views else (coarse.clone(), fine.clone())

    def _join(self, event):
        if event is not None:
            torch.cuda.current_stream(self.device).wait_event(event)

    def _chain(self, first, head):
        """the eight weight / bias pointers of a head chain: the conv `first`, then fc_layer0 .. fc_layer2 of the regressor `head`"""
        return [_lib.ptr(t) for scope in (first, head + "fc_layer0", head + "fc_layer1", head + "fc_layer2") for t in self._w(scope)]

    def _features(self, ws, path, inputs, st):
        """feature_extraction_GCN (ops.py:1437-1486): features accumulate right-to-left inside feat[:, 0:480]"""
        L, ptr = _lib.lib(), _lib.ptr
        B, N, _ = inputs.shape
        rn, k1, feat = B * N, K_NEIGH + 1, ws["feat"]
        fe = "generator/feature_extraction_coarse/"
        wl0, bl0 = self._w(fe + "layer0")
        if not path.stem:  # (stem: the first block's launch evaluates layer0 while it stages its cloud)
            self._call("layer0", L.dispu_linear_small_k, rn, 3, 24, ptr(inputs), 3, ptr(wl0), ptr(bl0), 0, _off(feat, 456), 480, st)
        col = 456          # left edge of the features produced so far
        for d in range(1, DENSE_BLOCKS + 1):
            pbuf, nxt = (ws["prep"], ws["prep_b"]) if d % 2 == 0 else (ws["prep_b"], ws["prep"])   # block d reads pbuf while its launch writes nxt
            if d == 1:
                F, ldf, foff, C = feat, 480, 456, 24
            else:
                if not path.stem:                                    # (stem: the previous block's launch already ran this bottleneck conv)
                    w, b = self._w(fe + "layer%d_prep" % d)
                    self._linear(st, feat, 480 - col, w, b, 1, pbuf, 48, xoff=col)
                F, ldf, foff, C = pbuf, 48, 0, 48
            convs = [ptr(t) for l in range(3) for t in self._w(fe + "layer%d/l%d" % (d, l))]
            width = 3 * GROWTH + C
            col -= width
            if path.stem:
                # + the next block's bottleneck conv over [this block's outputs | the 480 - (col + width) older columns] for d < 4
                last = d == DENSE_BLOCKS
                wp, bp = (None, None) if last else self._w(fe + "layer%d_prep" % (d + 1))
                layer0 = (ptr(inputs), ptr(wl0), ptr(bl0), _off(feat, 456)) if d == 1 else (None, None, None, None)
                self._call("stem_block", L.dispu_stem_block, rn, N, C, _off(F, foff), ldf, k1, 1, *convs, _off(feat, col), 480,
                           ptr(ws["kidx"]) if self.keep_intermediates else None, ptr(wp), ptr(bp), 480 - col - width,
                           None if last else ptr(nxt), 48, *layer0, 480, st)
                continue
            nbf = L.dispu_knn_feat_scratch_bytes(B, N, N, C, k1)      # > 0 for 512 < N <= 4096 (second pass of 16x): chunked search
            scratch = ptr(self._extra(ws, "knnf_scratch", (nbf,), torch.uint8)) if nbf else None
            self._call("knn_feat", L.dispu_knn_feat_strided_ws, B, N, N, C, k1, _off(F, foff), ldf, _off(F, foff), ldf, None, ptr(ws["kidx"]),
                       scratch, nbf, st)
            self._call("edge_dense_conv", L.dispu_edge_dense_conv, rn, N, C, _off(F, foff), ldf, ptr(ws["kidx"]), k1, 1, *convs,
                       _off(feat, col), 480, st)
        assert col == 0

    def _coarse_head(self, ws, path, B, N, st):
        """duplicate_up (ops.py:1152-1199) + coarse coordinate_regressor (:1089-1110); up128 (PointShuffle2's input) is written on the way"""
        L, ptr = _lib.lib(), _lib.ptr
        rm = B * N * self.up_ratio
        _, b1 = self._w("generator/upshuffle_0/conv1")
        conv2, cs = "generator/upshuffle_0/conv2", "generator/coarse_coordinate_regressor/"
        self._linear(st, ws["feat"], 480, self.w_up_feat, None, 0, ws["h256"], 256)
        if path.in_chain:          # duplicate_up's rows formed from the per-source-point product in the chain's loader
            self._call("mlp_chain[coarse]", L.dispu_mlp_chain_dup, B, N, self.up_ratio, 256, 128, 256, 64, ptr(ws["h256"]), 256, ptr(self.w_up_grid),
                       ptr(b1), ptr(self.grid), *self._chain(conv2, cs), ptr(ws["up128"]), 128, 0, None, 0, ptr(ws["coarse"]), 3, st)
            return
        self._call("dup_grid", L.dispu_dup_grid, B, N, 256, self.up_ratio, ptr(ws["h256"]), 256, ptr(self.w_up_grid), ptr(b1), ptr(self.grid),
                   ptr(ws["up256"]), 256, st)
        if path.heads:             # conv2 -> fc_layer0 -> fc_layer1 -> fc_layer2 in one launch
            self._call("mlp_chain[coarse]", L.dispu_mlp_chain, rm, 256, 128, 256, 64, ptr(ws["up256"]), 256, *self._chain(conv2, cs),
                       ptr(ws["up128"]), 128, 0, None, 0, ptr(ws["coarse"]), 3, st)
        else:
            w, b = self._w(conv2)
            self._linear(st, ws["up256"], 256, w, b, 1, ws["up128"], 128)
            w, b = self._w(cs + "fc_layer0")
            self._linear(st, ws["up128"], 128, w, b, 1, ws["c256"], 256)
            w, b = self._w(cs + "fc_layer1")
            self._linear(st, ws["c256"], 256, w, b, 1, ws["c64"], 64)
            w, b = self._w(cs + "fc_layer2")
            self._call("coarse", L.dispu_linear_small_n, rm, 64, 3, ptr(ws["c64"]), 64, ptr(w), ptr(b), 0, None, 0, ptr(ws["coarse"]), 3, st)

    def _non_local(self, ws, path, B, N, st):
        """PointNonLocalCell (ops.py:302-346) and conv0's feature part.  Both read up128 only: with self.branches they run on a second
        stream next to the grouping / skip / local cell (the small launches of one side fill the CUs the other leaves idle; captured into
        the same hipGraph as two parallel branches).  Returns the events recorded there once up3 and nl are written, else (None, None)."""
        L, ptr = _lib.lib(), _lib.ptr
        M, q, kv, sb = N * self.up_ratio, ws["q"], ws["kv"], st
        br, aux, ev_up3, ev_nl = self.branches, None, None, None
        if br:
            if self._aux is None:
                self._aux = (torch.cuda.Stream(device=self.device), torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event())
            aux, ev_fork, ev_up3, ev_nl = self._aux
            ev_fork.record(torch.cuda.current_stream(self.device))
            aux.wait_event(ev_fork)
            sb = _lib.C.c_void_p(aux.cuda_stream)
        with (torch.cuda.stream(aux) if br else contextlib.nullcontext()):
            # K|V, Q and conv0's feature part, N = 320 as 256 + 64 columns: each launch reads up128 once (128 x 256 / 128 x 64 tiles)
            self._linear(sb, ws["up128"], 128, self.w_up3, self.b_up3, 0, ws["up3"], 256)
            self._linear(sb, ws["up128"], 128, self.w_up3, self.b_up3[256:], 0, ws["up3"], 64, woff=256, yoff=256)
            if br:
                ev_up3.record(aux)
            w_bp, b_bp = self._w("refine/PointShuffle/PointShuffle/conv_back_project")
            if path.attention == "project":
                # softmax(Q.K^T / 8).V.W_bp on chip: neither the [B, M, M] logits nor the [B*M, 64] attention output reach HBM
                self._call("attention_project", L.dispu_attention_project, B, M, M, 64, ptr(q), 320, ptr(kv), 320, _off(kv, 64), 320, 0.125,
                           ptr(w_bp), ptr(b_bp), 256, ptr(ws["nl"]), 256, sb)
            elif path.attention == "flash":
                # softmax(Q.K^T / 8).V on chip (flash style): the [B, M, M] logits never exist in HBM
                self._call("attention", L.dispu_attention, B, M, M, 64, ptr(q), 320, ptr(kv), 320, _off(kv, 64), 320, 0.125, ptr(ws["att"]), 64, sb)
            else:
                s = self._extra(self._ws, ("scores", B, N), (B, M, M))
                self._linear(sb, q, 64, kv, None, 0, s, M, M=M, ldx=320, ldw=320, ldy=M, batch=B, sx=M * 320, sw=M * 320, sy=M * M, transb=1)
                self._call("softmax", L.dispu_softmax_rows, B * M, M, 0.125, ptr(s), M, sb)
                self._linear(sb, s, M, kv, None, 0, ws["att"], 64, M=M, ldx=M, ldw=320, ldy=64, batch=B, sx=M * M, sw=M * 320, sy=M * 64, woff=64)
            if path.attention != "project":
                self._linear(sb, ws["att"], 64, w_bp, b_bp, 1, ws["nl"], 256)
            if br:
                ev_nl.record(aux)
        return ev_up3, ev_nl

    def _knn_skip(self, ws, B, M, st):
        """PointShuffle2 (ops.py:1012-1087): the k nearest coarse points of every coarse point, and the skip connection"""
        L, ptr = _lib.lib(), _lib.ptr
        rm, k, coarse = B * M, K_NEIGH, ws["coarse"]
        nb = L.dispu_knn_xyz_scratch_bytes(B, M, M, k)             # > 0 for M > 1024 (second pass of 16x upsampling): chunked search
        scratch = ptr(self._extra(ws, "knn_scratch", (nb,), torch.uint8)) if nb else None
        self._call("knn_xyz", L.dispu_knn_xyz_ws, B, M, M, k, ptr(coarse), ptr(coarse), ptr(ws["psidx"]), None, scratch, nb, _lib.ARITH_PLAIN, st)
        self._call("skip_max", L.dispu_ps_skip_max, rm, M, k, 128, ptr(ws["psidx"]), ptr(coarse), ptr(ws["up128"]), 128, ptr(ws["skipin"]), 144, st)
        _, b = self._w("refine/PointShuffle/skip")
        # K padded 134 -> 144 with zero columns / zero weight rows (exact) so the GEMM takes its predicate-free path
        self._linear(st, ws["skipin"], 144, self.w_skip_pad, b, 1, ws["skip"], 256)

    def _local(self, ws, path, B, N, st):
        """PointShuffle2's local cell: conv0 per source point, conv1 per pair -> F' [rm, 2048]"""
        L, ptr = _lib.lib(), _lib.ptr
        M, k, ps = N * self.up_ratio, K_NEIGH, "refine/PointShuffle/"
        rm, coarse, psidx, gm, am = B * M, ws["coarse"], ws["psidx"], ws["gm"], ws["am"]
        w0, b0 = self._w(ps + "conv0")
        self._call("ps_prep", L.dispu_ps_prep, rm, 128, ptr(coarse), ptr(w0), ptr(b0), ptr(gm), 320, ptr(am), 128, st)
        w1, b1 = self._w(ps + "conv1")
        wnet = [ptr(t) for t in self._w(ps + "weight_net/wconv0") + (self.bn_scale, self.bn_shift)]
        if path.local != "pair":
            # gather_sub_relu + conv1 + weight_net + feature x weight in one kernel: only F' touches HBM ("bf16": as bf16, RNE at the store)
            name, fn = ("ps_local_bf16", L.dispu_ps_local_bf16) if path.local == "bf16" else ("ps_local", L.dispu_ps_local)
            self._call(name, fn, rm, M, k, 128, ptr(psidx), ptr(coarse), ptr(gm), 320, ptr(am), ptr(w1), ptr(b1), *wnet, ptr(ws["fp"]), st)
            return
        rows = rm * k              # the [rm * 16, .] pair tensors (A/B tests only: the default path never allocates them)
        flat = self._extra(self._ws, ("pair", B, N), (rows * 272,))
        x1, x2, wv = (t.view(rows, -1) for t in flat.split([rows * 128, rows * 128, rows * 16]))
        self._call("gather_sub_relu", L.dispu_ps_gather_sub_relu, rm, M, k, 128, ptr(psidx), ptr(gm), 320, ptr(am), 128, ptr(x1), 128, st)
        self._linear(st, x1, 128, w1, b1, 1, x2, 128)
        self._call("weight_net", L.dispu_ps_weight_net, rm, M, k, 16, ptr(psidx), ptr(coarse), *wnet, ptr(wv), st)
        self._call("point_matmul", L.dispu_ps_point_matmul, rm, k, 128, 16, ptr(x2), 128, ptr(wv), ptr(ws["fp"]), 2048, st)

    def _after_conv(self, ws, path, rm, st):
        """aft = relu(F' . W + b), and where the fine chain does not form its own input, (aft + skip) + nl in that association"""
        L, ptr = _lib.lib(), _lib.ptr
        w, b = self._w("refine/PointShuffle/after_conv")
        fp, aft = ws["fp"], ws["aft"]
        if path.after == "bf16_stream":
            # bf16(F') . bf16(W), fp32 accumulation: the streaming kernel on the pre-packed weight where its shape rules hold ...
            self._call("linear_bf16_stream[%dx2048x256]" % rm, L.dispu_linear_bf16_stream, rm, 2048, 256, ptr(fp), 2048, 1,
                       ptr(self._aft_bt), 2048, ptr(b), 1, ptr(aft), 256, 0, 1, 0, st)
        elif path.after == "bf16s":
            # ... else the generic bf16 kernel on the fp32 weight (rounded on load: the same products in the same order, bit-identical)
            self._call("linear_bf16s[%dx2048x256]" % rm, L.dispu_linear_bf16s, 1, rm, 2048, 256, ptr(fp), 2048, 0, ptr(w), 256, 0, 0,
                       ptr(b), 1, ptr(aft), 256, 0, None, 0, 0, 1, st)
        elif path.after == "x3":
            pl = self._planes.get("after_conv")
            if pl is None:
                pl = torch.empty((3 * 2048 * 256,), dtype=torch.bfloat16, device=self.device)
                _lib.check(L.dispu_bf16x3_split_weights(2048, 256, ptr(w), 256, ptr(pl), st), "dispu_bf16x3_split_weights")
                self._planes["after_conv"] = pl
            skip, nl = (None, None) if path.in_chain else (ptr(ws["skip"]), ptr(ws["nl"]))
            self._call("linear_bf16x3[%dx2048x256]" % rm, L.dispu_linear_bf16x3, rm, 2048, 256, ptr(fp), 2048, ptr(pl), ptr(b), 1,
                       ptr(aft), 256, skip, 256, nl, 256, st)
        else:                      # + skip + nl in the GEMM's epilogue ("residual") or in the fine chain's loader ("plain")
            r1, r2 = (None, None) if path.after == "plain" else (ws["skip"], ws["nl"])
            self._linear(st, fp, 2048, w, b, 1, aft, 256, R1=r1, R2=r2)
        if path.add3:              # into a buffer of its own: aft stays the product
            total = self._extra(ws, "sum", (rm, 256))
            self._call("add3", L.dispu_add3, rm * 256, ptr(aft), ptr(ws["skip"]), ptr(ws["nl"]), ptr(total), st)

    def _fine_head(self, ws, path, rm, fine, st):
        """aggregation + fine coordinate_regressor (is_off) + residual on coarse (generator.py:76-81)"""
        L, ptr = _lib.lib(), _lib.ptr
        agg, fs = "refine/PointShuffle/aggregation", "refine/fine_coordinate_regressor/"
        x, coarse = ws["sum"] if path.add3 else ws["aft"], ws["coarse"]
        if path.heads:
            tail = (ptr(ws["agg"]) if self.keep_intermediates else None, 256, 1, ptr(coarse), 3, ptr(fine), 3, st)
            if path.in_chain:      # relu(after_conv) + skip + nl in the chain's loader
                self._call("mlp_chain[fine]", L.dispu_mlp_chain_sum3, rm, 256, 256, 256, 64, ptr(x), ptr(ws["skip"]), ptr(ws["nl"]), 256,
                           *self._chain(agg, fs), *tail)
            else:
                self._call("mlp_chain[fine]", L.dispu_mlp_chain, rm, 256, 256, 256, 64, ptr(x), 256, *self._chain(agg, fs), *tail)
            return
        w, b = self._w(agg)
        self._linear(st, x, 256, w, b, 1, ws["agg"], 256)
        w, b = self._w(fs + "fc_layer0")
        self._linear(st, ws["agg"], 256, w, b, 1, ws["f256"], 256)
        w, b = self._w(fs + "fc_layer1")
        self._linear(st, ws["f256"], 256, w, b, 1, ws["f64"], 64)
        w, b = self._w(fs + "fc_layer2")
        self._call("fine", L.dispu_linear_small_n, rm, 64, 3, ptr(ws["f64"]), 64, ptr(w), ptr(b), 1, ptr(coarse), 3, ptr(fine), 3, st)
