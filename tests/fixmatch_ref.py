"""numpy oracle of FixMatch's distribution alignment (count and align, csrc/selftrain.hip) and readers for
tests/golden/g18_fixmatch.npz.  Values of a 16-bit tensor travel as float32 arrays that hold them exactly."""
import json

import numpy as np

DTYPES = ("f32", "f16", "bf16")


def round_to(a, dtype: str) -> np.ndarray:
    """float32 array (or scalar) rounded to nearest even in `dtype`, back as float32; NaN stays NaN"""
    a = np.asarray(a, dtype=np.float32)
    if dtype == "f32":
        return a
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    assert dtype == "bf16"
    bits = np.atleast_1d(a).view(np.uint32).astype(np.uint64)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)   # round to nearest, ties to even
    out = np.where(np.isnan(np.atleast_1d(a)), np.float32(np.nan), rounded.view(np.float32))
    return out.reshape(a.shape).astype(np.float32)


def threshold_in(threshold: float, dtype: str) -> np.float32:
    """the double `threshold` rounded to `dtype`, as a compare against a tensor of that dtype rounds its scalar operand"""
    if dtype == "f32":
        return np.float32(threshold)
    if dtype == "f16":
        return np.float32(np.float16(threshold))
    # double -> bf16 directly; through float32 first is the same unless the double sits within 2^-29 of a bf16 tie
    return np.float32(round_to(np.float32(threshold), "bf16"))


def count(x: np.ndarray, threshold: float, dtype: str) -> int:
    """how many stored labels are >= the rounded threshold; NaN counts as below"""
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.asarray(x, dtype=np.float32) >= threshold_in(threshold, dtype)))


def ratios(c1: int, n: int, source):
    """(r0, r1) in float32 in the reference's order: source / (counts / counts.sum()); 0 for an empty class"""
    s0, s1 = np.float32(source[0]), np.float32(source[1])
    c0, fn = n - c1, np.float32(n)
    r0 = s0 / (np.float32(c0) / fn) if c0 else np.float32(0)
    r1 = s1 / (np.float32(c1) / fn) if c1 else np.float32(0)
    return np.float32(r0), np.float32(r1)


def align(x: np.ndarray, source, threshold: float, dtype: str) -> np.ndarray:
    """clip(x * (x < t ? r0 : r1), 0, 1): the product in float32, rounded once to `dtype`; NaN passes the clip"""
    x = np.asarray(x, dtype=np.float32)
    t = threshold_in(threshold, dtype)
    r0, r1 = ratios(count(x, threshold, dtype), x.size, source)
    with np.errstate(invalid="ignore"):
        prod = round_to(x * np.where(x < t, r0, r1).astype(np.float32), dtype)
        return np.where(prod < 0, np.float32(0), np.where(prod > 1, np.float32(1), prod)).astype(np.float32)


# ---- the fixture ----------------------------------------------------------------------------------------------------
def da_array(fixture, key: str, dtype: str) -> np.ndarray:
    """a stored `da_*` tensor as float32: fp32 as it is, 16-bit types from their bit patterns"""
    a = fixture[key]
    if dtype == "f32":
        return a.astype(np.float32)
    if dtype == "f16":
        return a.view(np.float16).astype(np.float32)
    return (a.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def da_cases(fixture):
    return json.loads(str(fixture["da_index"]))


def fm_states(fixture, tag: str):
    """[state before iteration 0, ..., before iteration 5, final state] of run `tag`, each {name: float32 array}"""
    keys, shapes = json.loads(str(fixture["fm_state_keys"])), json.loads(str(fixture["fm_state_shapes"]))
    bits = fixture["fm_pre0"].view(np.int32).copy()
    flats = [bits.copy()]
    for row in fixture[f"fm_{tag}_chain"]:
        bits = bits + row   # int32 arrays wrap, as the generator's difference did
        flats.append(bits.copy())
    out = []
    for flat in flats:
        state, o = {}, 0
        for k, shape in zip(keys, shapes):
            n = int(np.prod(shape)) if shape else 1
            state[k] = flat[o:o + n].view(np.float32).reshape(shape).copy()
            o += n
        assert o == flat.size
        out.append(state)
    return out
