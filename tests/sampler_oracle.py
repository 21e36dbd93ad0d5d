"""Host twins for the device batch sampler (dis-pu_amd/csrc/batch_sampler.hip), written from the published Philox4x32-10 definition
(Salmon et al., SC'11; Random123's constants) and the counter layout of DESIGN.md "Train phase" -- independent of the kernel source.
Pure Python integers: slow, exact."""
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

STREAM_PATCH, STREAM_INDEX, STREAM_JITTER = 0, 1, 2


def philox4x32_10(counter, key):
    """(c0, c1, c2, c3), (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = [int(c) & MASK for c in counter]
    k0, k1 = [int(k) & MASK for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (c0, c1, c2, c3)


def block(seed, epoch, position, stream=STREAM_PATCH, number=0):
    """the sampler's Philox block: key = (seed low, seed high), counter = (block number, stream id, position, epoch)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((number, stream, position, epoch), (seed & MASK, seed >> 32))


def u01(w):
    """(w >> 8) * 2^-24"""
    return (int(w) >> 8) / float(1 << 24)


def normal_cos(w_radius, w_angle):
    """Box-Muller, cosine branch: sqrt(-2 ln(1 - u(w_radius))) cos(2 pi u(w_angle)), in float64."""
    import math
    return math.sqrt(-2.0 * math.log(1.0 - u01(w_radius))) * math.cos(2.0 * math.pi * u01(w_angle))


def jitter(seed, epoch, position, k, sigma, clip):
    """the three jitter values of input point k (block number k of the jitter stream): (w0, w1) -> cosine and sine, (w2, w3) -> cosine."""
    import math
    w = block(seed, epoch, position, STREAM_JITTER, k)
    r = math.sqrt(-2.0 * math.log(1.0 - u01(w[0])))
    n = (r * math.cos(2.0 * math.pi * u01(w[1])), r * math.sin(2.0 * math.pi * u01(w[1])), normal_cos(w[2], w[3]))
    return tuple(min(max(sigma * v, -clip), clip) for v in n)


def subsample(seed, epoch, position, G, P, max_draws=1 << 16):
    """The sequential rejection process over the index stream (block number = draw number): loc from the patch block's w0,
    a = int((loc + 0.3 z) G) truncated toward zero, accepted while 0 <= a < G and new, until P distinct indices are held.
    -> (sorted indices, margin): margin is the smallest distance of a consumed draw to a value where truncation or the range test
    changes its outcome (every integer but 0, which lies inside the interval (-1, 1) that truncates to index 0)."""
    loc = u01(block(seed, epoch, position)[0]) * 0.8 + 0.1
    held, margin = set(), float("inf")
    for d in range(max_draws):
        w = block(seed, epoch, position, STREAM_INDEX, d)
        x = (loc + 0.3 * normal_cos(w[0], w[1])) * G
        n = round(x)
        margin = min(margin, min(abs(x + 1), abs(x - 1)) if n == 0 else abs(x - n))
        if -1.0 < x < G:
            held.add(int(x))
            if len(held) == P:
                return sorted(held), margin
    raise RuntimeError("no %d distinct indices in %d draws" % (P, max_draws))
