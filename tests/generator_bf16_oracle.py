"""The CPU reference of Generator(dtype="bf16") and the record of how sharply it is defined.

The mode is the fp32 generator with ONE rounded product: after_conv (Common/ops.py:1078) multiplies F' and its weight both rounded to
bf16 (nearest even), accumulating in fp32.  The reference is oracle.generator.generator_forward with oracle.generator.linear wrapped
(`patch`, through the test's monkeypatch): the one call whose W.shape == (2048, 256) rounds x and W first.  Nothing under oracle/ changes.

That reference is DISCONTINUOUS in F': an element the GPU computes one fp32 ulp away from the oracle's may fall to the other bf16
neighbour, a step of 2^-8 relative in that factor.  (The GPU's F' is the oracle's chain on a reassociated conv0, DESIGN: "reassociated
-> tolerance-checked".)  So the tolerance on `fine` is not the fp32 test's 1e-5 by decree; it is measured on the CPU: the wrapped oracle
is evaluated twice on the GPU test's own inputs, once with F' from the oracle's fmaf chain and once with F' formed in float64 and cast to
fp32 (oracle.generator.matmul_nn wrapped the same way: the 4-D call), and the largest |fine_a - fine_b| over the cases is REF_SPREAD.
FINE_TOL = max(1e-5, 4 x REF_SPREAD): 1e-5 is the fp32 test's own figure, the factor 4 is there because a handful of cases samples the
maximum over ~10^4 coordinates poorly.  tests/test_generator_bf16.py recomputes the spread on the smallest case and holds it to the
record."""
import numpy as np
import torch

from oracle import generator as OG

# largest |fine_a - fine_b| of the two reference evaluations over CASES (measured on the CPU, float32 outputs)
REF_SPREAD = 1.1324882507324219e-06      # (3, 256): 1.0728836059570312e-06, (2, 250): 1.1324882507324219e-06
FINE_TOL = max(1e-5, 4 * REF_SPREAD)


def bf16_round(a):
    """float32 array rounded to bf16 (nearest even), returned as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def patch(monkeypatch, f64_fp=False):
    """Wrap oracle.generator.linear (the after_conv call rounds both operands to bf16) and, with f64_fp, oracle.generator.matmul_nn
    (the local cell's feature x weight product, the 4-D call, in float64 cast to fp32)."""
    lin, mnn = OG.linear, OG.matmul_nn

    def linear(x, W, b=None, relu=False):
        if W.shape == (2048, 256):
            return lin(bf16_round(x), bf16_round(W), b, relu)
        return lin(x, W, b, relu)

    def matmul_nn(a, bm):
        if a.ndim == 4:
            return np.matmul(a.astype(np.float64), bm.astype(np.float64)).astype(np.float32)
        return mnn(a, bm)

    monkeypatch.setattr(OG, "linear", linear)
    if f64_fp:
        monkeypatch.setattr(OG, "matmul_nn", matmul_nn)


def cases():
    """(name, params, inputs) of the GPU test's end-to-end cases: (3, 256) on tests/test_generator_gpu.py's `setup` inputs, and (2, 250)."""
    from dispu_amd import synth
    P = OG.init_params(seed=1234, bias_scale=0.05, bn_random=True)
    return [("3x256", P, synth.patches(3, 256, seed=5)), ("2x250", P, synth.patches(2, 250, seed=11))]


def spread(monkeypatch, P, x):
    """max |fine_a - fine_b| of the two evaluations of the wrapped oracle on (P, x)."""
    with monkeypatch.context() as m:
        patch(m)
        _, fa = OG.generator_forward(P, x)
    with monkeypatch.context() as m:
        patch(m, f64_fp=True)
        _, fb = OG.generator_forward(P, x)
    return float(np.abs(fa - fb).max())
