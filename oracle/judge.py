"""The judge of the op-by-op suites, defined once (TEST INFRASTRUCTURE, see oracle/__init__.py).  Needs numpy only.

The rule: a kernel's error, in units of 2^-23 x a per-element scale, is at most MARGIN * max(e32, 1), e32 being the figure of
the numpy float32 restatement on the same inputs; a stored 16-bit element lies in [round16(ref - band), round16(ref + band)]
of the same band (rounding is monotone, so the interval is exact).

Each oracle/*_ref.py binds these functions under the names its tests use, with ITS absolute allowance (`tiny`, `allow`) and
ITS NaN rule (`nan_equal`); tests/test_judge_cpu.py pins the definitions here on hand-made cases, the CPU suite of each
operation tests its bound judge on planted errors.
"""
import numpy as np

U = 2.0 ** -23
TINY = 2.0 ** -126                      # the absolute allowance of the modules that take one: below it float32 is subnormal
MARGIN = 4.0                            # the project's margin over plain fp32 arithmetic
FMT = {"f16": (11, -14), "bf16": (8, -126)}          # significant bits, exponent of the smallest normal number


# ------------------------------------------------------------------------------------------------------- 16-bit rounding
def round16(x, kind):
    """float64 -> the nearest value of the 16-bit type (ties to even, gradual underflow), as float64; monotone.  No
    overflow handling: the tests stay far below 65504."""
    p, emin = FMT[kind]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                                 # |x| in [2^(e-1), 2^e)
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
    return np.rint(x / q) * q


def round_common16(x):
    """values every storage type holds exactly: rounded to fp16, then to bf16 (an fp16 number's bf16 rounding is an fp16
    number again: fewer significant bits on the same exponent, subnormals included)"""
    return round16(round16(x, "f16"), "bf16")


def stored(val, dt):
    """the exact value as the storage type holds it"""
    return np.asarray(val, np.float64) if dt == "f32" else round16(val, dt)


# ------------------------------------------------------------------------------------------------------- units of 2^-23 x scale
def units(got, ref, scale, allow=0.0, tiny=0.0):
    """worst |got - ref| in units of 2^-23 x scale over EVERY element, after the absolute allowances `allow` (per element)
    and `tiny`; a non-finite value, a wrong shape, or an error where the scale is 0 counts as infinite"""
    got, ref, scale = (np.asarray(v, np.float64) for v in (got, ref, scale))
    if got.shape != ref.shape:
        return float("inf")
    scale = np.broadcast_to(scale, ref.shape)
    err = np.maximum(np.abs(got - ref) - np.broadcast_to(np.asarray(allow, np.float64), ref.shape) - tiny, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0.0, 0.0, err / (U * scale))
    u = np.where(np.isfinite(got), u, np.inf)
    return float(np.nan_to_num(u, nan=np.inf, posinf=np.inf).max()) if u.size else 0.0


def band(e32):
    """the allowed error per unit of scale: MARGIN * max(e32, 1) * 2^-23"""
    return MARGIN * max(float(e32), 1.0) * U


def within(kernel_units, e32):
    return kernel_units <= MARGIN * max(float(e32), 1.0)


# ------------------------------------------------------------------------------------------------------- 16-bit stores
def outside_interval(got, lo, hi):
    """the number of elements outside their closed interval (non-finite ones and a wrong shape included)"""
    got, lo, hi = (np.asarray(v, np.float64) for v in (got, lo, hi))
    if got.shape != lo.shape:
        return int(lo.size)
    return int((~((got >= lo) & (got <= hi))).sum())


def outside16_abs(got, ref, d, kind):
    """16-bit stores: the number of elements outside [round16(ref - d), round16(ref + d)], d an absolute band"""
    ref, d = np.asarray(ref, np.float64), np.asarray(d, np.float64)
    return outside_interval(got, round16(ref - d, kind), round16(ref + d, kind))


def interval16(ref, scale, e32, kind):
    """the closed interval of 16-bit values a kernel that computes in fp32 within the band and rounds once may store"""
    ref, scale = np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    b = band(e32) * scale
    return round16(ref - b, kind), round16(ref + b, kind)


def outside16(got, ref, scale, e32, kind):
    """the number of stored elements outside their interval (non-finite ones included); a wrong shape: every element"""
    ref = np.asarray(ref, np.float64)
    return outside16_abs(got, ref, band(e32) * np.broadcast_to(np.asarray(scale, np.float64), ref.shape), kind)


def excess16(got, ref, scale, kind):
    """for the record: the worst error beyond the ideal rounding of the float64 value, in units of 2^-23 x scale (no
    absolute allowance in any module)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    extra = np.maximum(np.abs(got - ref) - np.abs(round16(ref, kind) - ref), 0.0)
    return units(ref + extra, ref, scale)


# ------------------------------------------------------------------------------------------------------- exact quantities
def mismatches(got, want, nan_equal=False):
    """the number of elements that are not the exact value, as values (-0.0 equals 0.0); a NaN matches nothing, or, with
    nan_equal, a NaN; a wrong shape: every element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return int(want.size)
    same = got == want
    if nan_equal:
        same = same | (np.isnan(got) & np.isnan(want))
    return int((~same).sum())
