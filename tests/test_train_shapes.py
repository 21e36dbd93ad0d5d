"""Which inputs the shape cases of tests/test_train_shapes_gpu.py run on, decided by the reference alone (no GPU).

The row-wise activation-gradient check allows 1 % of a tensor's rows to be off by more than 1e-3, because an fp32 forward takes
another ReLU / max / arg-min branch than the float64 oracle at near-ties.  How many near-ties there are is a property of the
INPUT: on synth.patch_with_gt(2, 24, 96, seed=1) rounding alone flags half the rows, on (4, 64) seed 2 it flags 14.8 %.  An input
like that would leave the allowance no room to tell a kernel bug from rounding, and one with no near-ties at all would need no
allowance.  So every committed (B, N, seed) has to pass this proxy: the oracle evaluated in float32 (oracle.train_oracle.DT
monkeypatched, nothing else changed) against itself in float64, under the measures the device is held to
(tests/train_step_checks.py), with HALF the row allowance and a TENTH of the parameter-gradient bound:

    share of rows above 1e-3, worst of the seven watched activation gradients   <= 0.5 %   (the device check allows 1 %)
    relative L2 of a parameter gradient, worst                                  <= 3e-4    (the device check allows 3e-3)

For a tensor of fewer than 200 rows 0.5 % means no row at all.  The proxy is not the device -- its fma chains flip other near-ties
-- it only keeps inputs out whose near-ties would drown the check.  (1, 1024): seeds 1 - 6 flag 1.27, 0.59, 1.46, 4.98, 1.56 and
2.64 % of a tensor's rows; 7 is the first that passes, so that case runs the full set of checks like every other.
Run with -s for the table."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_checks as K  # noqa: E402

from oracle import train_oracle as T  # noqa: E402

SHARE, GRAD_L2 = 0.5 * K.ROW_SHARE, 0.1 * K.GRAD_L2


@pytest.mark.parametrize("B,N,seed", K.SHAPE_CASES)
def test_float32_oracle_stays_inside_half_the_allowance(B, N, seed, monkeypatch):
    flagged, share, l2 = K.float32_proxy(B, N, seed, lambda dt: monkeypatch.setattr(T, "DT", dt))
    print("[measured] proxy (%d, %d, seed %d): %d rows flagged in the worst tensor (%.2f %%, bound %.1f %%), worst gradient rel L2 %.1e "
          "(bound %.0e)" % (B, N, seed, flagged, 100 * share, 100 * SHARE, l2, GRAD_L2))
    assert share <= SHARE, (flagged, share)
    assert l2 <= GRAD_L2, l2
