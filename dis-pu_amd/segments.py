"""The packed ragged batch of the whole-cloud operations, once: clouds of different sizes concatenated into one [sum n_c, 3] array,
segment c = rows [off[c], off[c + 1]), with the offsets on the host (the entries of include/dispu_hip.h plan from them) and on the
device, and one status word per cloud.  normals.py, outliers.py, upsample.py and tf_sampling.fps_ragged build theirs here (Packed);
attributes.py, mls.py and reconstruct.py, whose operators search one batch from another, build the two of theirs here (Pair).  The
argument checks they share live here too, so a refusal reads the same whichever operation raises it."""
import math

import numpy as np
import torch

from . import _lib
from ._util import req

MAX_CLOUDS = 65535
MAX_POINTS = 1 << 24
SUPPORT_MIN, SUPPORT_MAX = 1.0, 4.0                          # of the Wendland weights (mls_project, signed_distance), in k-th distances


def host_ptr(a):
    """a numpy array as the const pointer of a host-side argument"""
    return _lib.C.c_void_p(a.ctypes.data)


def to_device(a, device):
    return torch.from_numpy(a).to(device)


def is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_int_range(v, lo, hi, name):
    req(is_int(v) and lo <= v <= hi, "%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    return int(v)


def check_support(v):
    ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and SUPPORT_MIN <= float(v) <= SUPPORT_MAX
    req(ok and math.isfinite(float(v)), "support must be a number in %g .. %g, got %r" % (SUPPORT_MIN, SUPPORT_MAX, v))
    return float(v)


def scratch_buffer(nbytes, what, dev, noun="clouds"):
    """what: the entry that sized the scratch; 0 bytes is its refusal"""
    req(nbytes > 0, "%s refuses these %s" % (what, noun))
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def check_cloud(t, what):
    req(isinstance(t, torch.Tensor), "%s: expected a float32 [n, 3] tensor on a ROCm device, got %s" % (what, type(t).__name__))
    req(t.is_cuda, "%s must live on a ROCm device (dis-pu_amd has no CPU path)" % what)
    req(t.dtype == torch.float32, "%s must be float32, got %s" % (what, t.dtype))
    req(t.dim() == 2 and t.shape[1] == 3, "%s: expected an [n, 3] tensor, got shape %s" % (what, tuple(t.shape)))


def offsets(counts):
    """counts [C] -> int32 offsets [C + 1] (host), refused (ValueError) when the total does not fit an int32 offset."""
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("a packed batch holds at most 2^31 - 1 rows, got %d" % off[-1])
    return off.astype(np.int32)


def split(t, off, single):
    """the rows of a packed tensor per segment of off: a list, or for a single cloud its rows alone"""
    return t[off[0]:off[1]] if single else [t[off[c]:off[c + 1]] for c in range(len(off) - 1)]


def as_list(v):
    """a tensor -> [v], a list or a tuple -> a list, anything else -> None"""
    return [v] if isinstance(v, torch.Tensor) else list(v) if isinstance(v, (list, tuple)) else None


class Packed(object):
    """a tensor or a list of tensors, checked, packed once.  who: the caller's name;  label: how a message names cloud i;  home: how it
    names the device every cloud must share (dev, or that of cloud 0);  words: output words per point, for the bound of limit()."""

    def __init__(self, points, who, words=None, label="cloud %d", dev=None, home="cloud 0"):
        self.single = isinstance(points, torch.Tensor)
        clouds = as_list(points)
        req(clouds is not None, "points must be a float32 [n, 3] tensor on a ROCm device or a list of them, got %s" % type(points).__name__)
        req(len(clouds) >= 1, "%s needs at least one cloud" % who)
        req(len(clouds) <= MAX_CLOUDS, "at most %d clouds per call, got %d" % (MAX_CLOUDS, len(clouds)))
        for i, c in enumerate(clouds):
            check_cloud(c, label % i)
            req(1 <= c.shape[0] <= MAX_POINTS, "%s has %d points, expected 1 .. 2^24" % (label % i, c.shape[0]))
            req(c.device == (clouds[0].device if dev is None else dev), "%s lives on another device than %s" % (label % i, home))
        self.clouds, self.C, self.dev = clouds, len(clouds), clouds[0].device
        off = np.zeros(self.C + 1, np.int64)
        np.cumsum([int(c.shape[0]) for c in clouds], out=off[1:])
        self.total = int(off[-1])
        self.off = off.astype(np.int32)                      # exact once a limit() has passed
        if words is not None:
            self.limit(words)

    def limit(self, words, unit="output words", tail=""):
        """the int32 bound of what the caller indexes: `words` per point"""
        req(self.total * words < 2 ** 31, "a packed batch holds at most 2^31 - 1 %s, got %d points%s" % (unit, self.total, tail))

    def pack(self, status=True):
        """after every check that needs no launch"""
        self.cloud = self.pack_like(self.clouds)
        self.d_off = to_device(self.off, self.dev)
        self.status = torch.zeros((self.C,), dtype=torch.int32, device=self.dev) if status else None

    def pack_like(self, ts):
        """per-point companions of the clouds (normals, neighbours, features, labels), one tensor per cloud -> packed as the cloud is"""
        return (ts[0] if self.C == 1 else torch.cat(list(ts))).contiguous()

    def split(self, t, off=None):
        """off: another offset table than the batch's own, after a compaction"""
        return split(t, self.off if off is None else off, self.single)

    def scratch(self, nbytes, what):
        return scratch_buffer(nbytes, what, self.dev)

    def refuse_non_finite(self, status=None):
        bad = np.nonzero((self.status if status is None else status).cpu().numpy())[0]
        req(len(bad) == 0, "cloud %d holds a NaN or an infinite coordinate" % (int(bad[0]) if len(bad) else -1))


class Pair(object):
    """queries and the clouds they are searched in, a tensor pair or two lists of equal length: two packed batches of one device, and
    what joins them.  who: the caller's name;  name: what the caller calls its second argument ("refs", "points");  refs None: every
    cloud against itself, one batch packed once."""

    def __init__(self, queries, refs, who, name="refs"):
        if refs is not None:                                 # the shapes of the two arguments first
            if isinstance(queries, torch.Tensor):
                req(isinstance(refs, torch.Tensor), "%s: queries is a tensor, so %s must be one too, got %s" % (who, name, type(refs).__name__))
            else:
                req(isinstance(queries, (list, tuple)) and isinstance(refs, (list, tuple)),
                    "queries and %s must be float32 [n, 3] tensors on a ROCm device or two lists of them, got %s and %s"
                    % (name, type(queries).__name__, type(refs).__name__))
                req(len(queries) >= 1, "%s needs at least one cloud" % who)
                req(len(queries) == len(refs), "%d query clouds but %d reference clouds" % (len(queries), len(refs)))
        q = self.queries = Packed(queries, who, label="queries of cloud %d", home="the queries of cloud 0")
        self.refs = q if refs is None else Packed(refs, who, label=name + " of cloud %d", dev=q.dev, home="the queries of cloud 0")
        self.single, self.C, self.dev, self.nq = q.single, q.C, q.dev, q.total
        for b, what in ((q, "query"), (self.refs, "reference")):         # the int32 offsets of either side
            req(b.total < 2 ** 31, "a packed batch holds at most 2^31 - 1 %s points, got %d" % (what, b.total))

    def width(self, w):
        req(self.nq * w < 2 ** 31, "a packed batch holds at most 2^31 - 1 output words, got %d queries x %d" % (self.nq, w))

    def pack(self, sizer):
        """after every check that needs no launch.  sizer: the name of the entry that sizes the operator's scratch"""
        self.queries.pack()
        if self.refs is not self.queries:
            self.refs.pack(status=False)
        self.nbytes = getattr(_lib.lib(), sizer)(self.C, host_ptr(self.queries.off), host_ptr(self.refs.off))
        self.scratch = self.queries.scratch(self.nbytes, sizer)

    def head(self):
        """the arguments every entry starts with"""
        q, r = self.queries, self.refs
        return (self.C, _lib.ptr(q.d_off), host_ptr(q.off), _lib.ptr(r.d_off), host_ptr(r.off))

    def tail(self):
        """and ends with"""
        return (_lib.ptr(self.queries.status), _lib.ptr(self.scratch), self.nbytes, _lib.stream_ptr(self.dev))
