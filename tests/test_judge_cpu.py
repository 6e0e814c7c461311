"""CPU: the shared definitions of oracle/judge.py on hand-made cases, independently of any one operation.  Every figure below
is exact in float64 (powers of two and small multiples of them).  Each operation's CPU suite tests its own bound judge --
with its allowance and its NaN rule -- on planted errors."""
import numpy as np

from oracle import judge as J

U, T = 2.0 ** -23, 2.0 ** -126


def test_the_shared_judge_on_hand_made_cases():
    assert (J.U, J.TINY, J.MARGIN) == (U, T, 4.0)
    # units without an allowance: 3 units of scale 1, 1 unit of scale 2, none
    assert J.units([1 + 3 * U, 2 - 2 * U, 4.0], [1.0, 2.0, 4.0], [1.0, 2.0, 4.0]) == 3.0
    # ... the three allowances on one case: errors T, 3 T at scale T, and 2 units at scale 1
    got, ref, scale = [T, 3 * T, 1 + 2 * U], [0.0, 0.0, 1.0], [T, T, 1.0]
    assert J.units(got, ref, scale) == 3 * 2.0 ** 23
    assert J.units(got, ref, scale, tiny=T) == 2 * 2.0 ** 23            # T is forgiven, 3 T counts as 2 T
    assert J.units(got, ref, scale, allow=[0.0, 2 * T, U], tiny=T) == 1.0   # allow takes the rest of 3 T and one of the 2 units
    assert J.units(got, ref, scale, allow=U, tiny=T) == 1.0             # a scalar allowance: every element
    # ... what counts as infinite, and what as nothing
    inf = float("inf")
    assert J.units([1.0, np.nan], [1.0, 1.0], 1.0) == inf and J.units([np.inf], [1.0], 1.0) == inf
    assert J.units([1.0], [1.0, 1.0], 1.0) == inf and J.units([1.0, 2.0], [1.0, 2 + U], [1.0, 0.0]) == inf
    assert J.units([1.0, 2.0], [1.0, 2.0], [1.0, 0.0]) == 0.0 and J.units([], [], []) == 0.0
    # the bound
    assert J.band(0.5) == 4 * U and J.band(3.0) == 12 * U
    assert J.within(4.0, 0.0) and not J.within(4.5, 1.0) and J.within(8.0, 2.0) and not J.within(inf, 100.0)
    # both NaN rules: -0.0 is 0.0; NaN matches nothing, or NaN
    got, want = [0.0, np.nan, 1.0, np.nan], [-0.0, np.nan, 2.0, 1.0]
    assert J.mismatches(got, want) == 3 and J.mismatches(got, want, nan_equal=True) == 2
    assert J.mismatches([1.0], [1.0, 1.0]) == 2 and J.mismatches([1.0], [1.0, 1.0], nan_equal=True) == 2
    # round16: ties to even at 1 (steps 2^-10 and 2^-7) ...
    for kind, h in (("f16", 2.0 ** -11), ("bf16", 2.0 ** -8)):          # h: half a step
        x = np.array([1 + h, 1 + 3 * h, 1 + 5 * h, 1 + 2.5 * h, -(1 + 3 * h)])
        assert J.round16(x, kind).tolist() == [1.0, 1 + 4 * h, 1 + 4 * h, 1 + 2 * h, -(1 + 4 * h)], kind
    # ... and gradual underflow: below 2^-14 / 2^-126 the step stays 2^-24 / 2^-133
    for kind, s in (("f16", 2.0 ** -24), ("bf16", 2.0 ** -133)):
        x = np.array([0.5 * s, 1.5 * s, 2.5 * s, 5.25 * s, -0.75 * s, 0.0])
        assert J.round16(x, kind).tolist() == [0.0, 2 * s, 2 * s, 5 * s, -s, 0.0], kind
    assert J.round16(2.0 ** -14 + 2.0 ** -25, "f16") == 2.0 ** -14      # the first normal binade has the same step
    assert J.round_common16(1 + 2.0 ** -9) == 1.0 and J.round_common16(1.5) == 1.5
    assert J.stored(1 + 2.0 ** -12, "f32") == 1 + 2.0 ** -12 and J.stored(1 + 2.0 ** -12, "f16") == 1.0
    # a 16-bit store: the closed interval of the rounded band ends (band(0) x scale = 4 x 2^-23 x 2^14 = 2^-7: one bf16 step above 1)
    lo, hi = J.interval16([1.0], [2.0 ** 14], 0.0, "bf16")
    assert (lo[0], hi[0]) == (1 - 2.0 ** -7, 1 + 2.0 ** -7)
    assert J.outside16([1 + 2.0 ** -7, 1 + 2.0 ** -6, np.nan], [1.0] * 3, 2.0 ** 14, 0.0, "bf16") == 2
    assert J.outside16_abs([1 + 2.0 ** -7], [1.0], 2.0 ** -8, "bf16") == 1        # half a step: the band end rounds back to 1
    assert J.outside16([1.0], [1.0, 1.0], 1.0, 0.0, "f16") == 2                   # a wrong shape: every element
