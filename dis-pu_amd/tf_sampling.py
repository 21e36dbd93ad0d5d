"""Farthest point sampling / point gather -- same names, argument order and return values as the
reference wrapper tf_ops/sampling/tf_sampling.py:29-56 (torch tensors instead of TF tensors)."""
import torch

from . import _lib
from ._util import f32, i32, req
from .segments import host_ptr, to_device


FPS_PATHS = ("auto", "cells", "stream")


def _check_path(path):
    req(path in FPS_PATHS, "path must be one of %s, got %r" % (", ".join(repr(p) for p in FPS_PATHS), path))
    return path


def fps_ragged(inp, off, moff, arith=_lib.ARITH_CONTRACT, path="auto", cell=0):
    """farthest_point_sample per segment of a packed batch: inp [sum n_c, 3] (device), off / moff host offsets of the points and of the
    samples -> idx [sum m_c] int32, local to each segment; every path returns the same indices.  path: "stream" = dispu_fps_segments
    (above 24576 points the streaming kernel), "cells" = the cell-skipping kernels of csrc/fps_cells.hip for EVERY segment (cell: forced
    cell size, 0 = automatic), "auto" = dispu_fps_segments_auto.  A segment the cell kernels refuse for a non-finite coordinate
    (status != 0) is sampled again through dispu_fps_segments, so such input behaves as on the "stream" path."""
    import numpy as np
    _check_path(path)
    off, moff = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(moff, np.int32)
    req(off.ndim == 1 and off.shape == moff.shape and len(off) >= 1, "off and moff must be [C + 1] offsets")
    C = len(off) - 1
    inp = inp.contiguous()
    dev = inp.device
    out = torch.empty((int(moff[-1]),), dtype=torch.int32, device=dev)
    if C == 0:
        return out
    L = _lib.lib()
    d_off, d_moff = to_device(off, dev), to_device(moff, dev)
    st = _lib.stream_ptr(dev)

    def stream_call(o, mo, d_o, d_mo, x, res):
        nbytes = L.dispu_fps_segments_scratch_bytes(len(o) - 1, host_ptr(o), host_ptr(mo))
        temp = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev) if nbytes else None
        _lib.check(L.dispu_fps_segments(len(o) - 1, _lib.ptr(d_o), _lib.ptr(d_mo), host_ptr(o), host_ptr(mo), _lib.ptr(x), _lib.ptr(temp),
                                        nbytes, _lib.ptr(res), int(arith), st), "dispu_fps_segments")

    if path == "stream":
        stream_call(off, moff, d_off, d_moff, inp, out)
        return out
    n_c, m_c = np.diff(off), np.diff(moff)
    if path == "cells":
        nbytes = L.dispu_fps_cells_scratch_bytes(C, host_ptr(off), host_ptr(moff), int(cell))
        req(nbytes > 0, "dispu_fps_cells refuses these segments (illegal offsets or cell size, or a segment above 2^24 points)")
        uses_cells = True
    else:
        req(int(cell) == 0, "a forced cell size needs path='cells'")
        uses_cells = any(L.dispu_fps_cells_wanted(int(n), int(m)) for n, m in zip(n_c, m_c) if n > 24576)
        nbytes = L.dispu_fps_segments_auto_scratch_bytes(C, host_ptr(off), host_ptr(moff))
        if uses_cells and nbytes == 0:           # a segment above 2^24 points: only the streaming kernel takes it
            stream_call(off, moff, d_off, d_moff, inp, out)
            return out
    temp = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
    status = torch.zeros((C,), dtype=torch.int32, device=dev) if uses_cells else None
    if path == "cells":
        _lib.check(L.dispu_fps_cells(C, _lib.ptr(d_off), _lib.ptr(d_moff), host_ptr(off), host_ptr(moff), _lib.ptr(inp), _lib.ptr(temp),
                                     nbytes, _lib.ptr(out), _lib.ptr(status), int(arith), int(cell), st), "dispu_fps_cells")
    else:
        _lib.check(L.dispu_fps_segments_auto(C, _lib.ptr(d_off), _lib.ptr(d_moff), host_ptr(off), host_ptr(moff), _lib.ptr(inp),
                                             _lib.ptr(temp), nbytes, _lib.ptr(out), _lib.ptr(status), int(arith), st),
                   "dispu_fps_segments_auto")
    if uses_cells:
        for c in np.nonzero(status.cpu().numpy())[0]:          # non-finite segments: the existing entry, one segment at a time
            o1, m1 = np.array([0, n_c[c]], np.int32), np.array([0, m_c[c]], np.int32)
            stream_call(o1, m1, to_device(o1, dev), to_device(m1, dev), inp[int(off[c]):int(off[c + 1])],
                        out[int(moff[c]):int(moff[c + 1])])
    return out


def farthest_point_sample(npoint, inp, arith=_lib.ARITH_CONTRACT, path="auto"):
    """(npoint:int, inp[b,n,3] f32) -> idx[b,npoint] i32.   tf_sampling.py:48-56; no gradient (:57).
    idx[:,0] == 0; ties follow the reference kernel's rule (tf_sampling_g.cu:146,158).
    path: "stream" = dispu_fps_ws; "cells" = the cell-skipping kernels for large clouds (csrc/fps_cells.hip) whatever the shape;
    "auto" = the batch as a ragged batch with trivial offsets through dispu_fps_segments_auto where dispu_fps_cells_wanted(n, npoint)
    says the cell kernels are faster, dispu_fps_ws (which that entry would pick itself) otherwise.  All paths return the same indices."""
    _check_path(path)
    inp = f32(inp, "inp")
    req(int(npoint) > 0, "FarthestPointSample expects positive npoint")
    req(inp.dim() == 3 and inp.shape[2] == 3, "FarthestPointSample expects (batch_size,num_points,3) inp shape")
    b, n, _ = inp.shape
    req(n > 0, "FarthestPointSample expects (batch_size,num_points,3) inp shape")
    L = _lib.lib()
    if b > 0 and (path == "cells" or (path == "auto" and n > 24576 and L.dispu_fps_cells_wanted(n, int(npoint)))):
        req(b * n < 2 ** 31 and b * int(npoint) < 2 ** 31, "the batch does not fit int32 offsets")
        import numpy as np
        off, moff = np.arange(b + 1, dtype=np.int64) * n, np.arange(b + 1, dtype=np.int64) * int(npoint)
        return fps_ragged(inp.reshape(-1, 3), off, moff, arith, path).reshape(b, int(npoint))
    out = torch.empty((b, int(npoint)), dtype=torch.int32, device=inp.device)
    nbytes = L.dispu_fps_scratch_bytes(b, n, int(npoint))
    temp = torch.empty((nbytes // 4,), dtype=torch.float32, device=inp.device) if nbytes else None
    _lib.check(L.dispu_fps_ws(b, n, int(npoint), _lib.ptr(inp), _lib.ptr(temp), nbytes, _lib.ptr(out), int(arith),
                              _lib.stream_ptr(inp.device)), "dispu_fps_ws")
    return out


def prob_sample(inp, inpr):
    """(inp[b,ncategory] f32 weights, inpr[b,npoints] f32 uniform randoms) -> [b,npoints] i32   tf_sampling.py:12-20
    (optional op, unused by the shipped graph; no gradient :21): the index of the first cumulative weight >= r * total."""
    inp, inpr = f32(inp, "inp"), f32(inpr, "inpr")
    req(inp.dim() == 2, "ProbSample expects (batch_size,num_choices) inp shape")
    req(inpr.dim() == 2 and inpr.shape[0] == inp.shape[0], "ProbSample expects (batch_size,num_points) inpr shape")
    b, n = inp.shape
    m = inpr.shape[1]
    req(n > 0, "ProbSample expects (batch_size,num_choices) inp shape")
    out = torch.empty((b, m), dtype=torch.int32, device=inp.device)
    temp = torch.empty((b, n), dtype=torch.float32, device=inp.device)      # the op's allocate_temp {b, n}: cumulative sums
    _lib.check(_lib.lib().dispu_prob_sample(b, n, m, _lib.ptr(inp), _lib.ptr(inpr), _lib.ptr(temp), _lib.ptr(out),
                                            _lib.stream_ptr(inp.device)), "dispu_prob_sample")
    return out


class _GatherPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, idx):
        b, n, _ = inp.shape
        m = idx.shape[1]
        out = torch.empty((b, m, 3), dtype=torch.float32, device=inp.device)
        _lib.check(_lib.lib().dispu_gather_point(b, n, m, _lib.ptr(inp), _lib.ptr(idx), _lib.ptr(out),
                                                 _lib.stream_ptr(inp.device)), "dispu_gather_point")
        ctx.save_for_backward(idx)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, out_g):
        (idx,) = ctx.saved_tensors
        return gather_point_grad_raw(ctx.n, idx, out_g.contiguous()), None


def gather_point_grad_raw(n, idx, out_g):
    b, m = idx.shape
    inp_g = torch.empty((b, n, 3), dtype=torch.float32, device=out_g.device)
    _lib.check(_lib.lib().dispu_gather_point_grad(b, n, m, _lib.ptr(out_g), _lib.ptr(idx), _lib.ptr(inp_g),
                                                  _lib.stream_ptr(out_g.device)), "dispu_gather_point_grad")
    return inp_g


def gather_point(inp, idx):
    """(inp[b,n,3] f32, idx[b,m] i32) -> [b,m,3].   tf_sampling.py:29-37; gradient :43-47."""
    inp, idx = f32(inp, "inp"), i32(idx, "idx")
    req(inp.dim() == 3 and inp.shape[2] == 3, "GatherPoint expects (batch_size,num_points,3) inp shape")
    req(idx.dim() == 2 and idx.shape[0] == inp.shape[0], "GatherPoint expects (batch_size,num_result) idx shape")
    return _GatherPoint.apply(inp, idx)


def gather_point_grad(inp, idx, out_g):
    """sampling_module.gather_point_grad(inp, idx, out_g) -> [b,n,3]   (tf_sampling.py:43-47)."""
    inp, idx, out_g = f32(inp, "inp"), i32(idx, "idx"), f32(out_g, "out_g")
    req(inp.dim() == 3 and inp.shape[2] == 3, "GatherPointGradGpuOp expects (batch_size,num_points,3) inp")
    req(idx.dim() == 2 and idx.shape[0] == inp.shape[0], "GatherPointGradGpuOp expects (batch_size,num_result) idx shape")
    req(out_g.dim() == 3 and out_g.shape[0] == inp.shape[0] and out_g.shape[1] == idx.shape[1] and out_g.shape[2] == 3,
        "GatherPointGradGpuOp expects (batch_size,num_result,3) out_g shape")
    return gather_point_grad_raw(inp.shape[1], idx, out_g)
