"""float64 / numpy oracle of the pseudo-labelling step (torch_em_amd.ops.pseudo_label, csrc/selftrain.hip).

Values travel as float64 arrays that hold numbers exactly representable in the storage type ("f32", "f16", "bf16").
Semantics (checked against the reference's DefaultPseudoLabeler on the CPU by tests/test_selftrain_cpu.py):
  labels = x, or sigmoid(x) evaluated in float64 and rounded ONCE to the storage type;
  mask   = (labels >= round(t)) | (labels <= round(1 - t))  as float32 0 / 1 (both sides), or labels >= round(t) as bool
           (one side): the compare runs on the stored label against the threshold rounded to the storage type, 1 - t formed
           in double first;
  mask_sample = k: every sample gets sample k's mask.
"""
import numpy as np

MANTISSA_BITS = {"f32": 23, "f16": 10, "bf16": 7}
MIN_NORMAL_EXP = {"f32": -126, "f16": -14, "bf16": -126}


def round_dtype(v, dt: str) -> np.ndarray:
    """float64 -> nearest value of the storage type (ties to even), returned as float64.  16-bit types go through float32
    first, as torch converts a double scalar or tensor."""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    if dt == "f32":
        return f.astype(np.float64)
    if dt == "f16":
        return f.astype(np.float16).astype(np.float64)
    bits = np.atleast_1d(f).view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64).reshape(np.shape(f))


def ulp(v, dt: str) -> np.ndarray:
    """spacing of the storage type at |v| (v != 0; denormals get the spacing of the smallest normal binade)"""
    e = np.floor(np.log2(np.abs(np.asarray(v, dtype=np.float64))))
    return 2.0 ** (np.maximum(e, MIN_NORMAL_EXP[dt]) - MANTISSA_BITS[dt])


def sigmoid64(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def labels_ref(x, sigmoid: bool, dt: str) -> np.ndarray:
    return round_dtype(sigmoid64(x), dt) if sigmoid else np.asarray(x, dtype=np.float64)


def mask_ref(labels, t, both_sides: bool, dt: str, mask_sample=None):
    """the reference compare applied to stored labels; None without a threshold"""
    if t is None:
        return None
    labels = np.asarray(labels, dtype=np.float64)
    t_hi, t_lo = float(round_dtype(float(t), dt)), float(round_dtype(1.0 - float(t), dt))
    src = labels if mask_sample is None else labels[mask_sample:mask_sample + 1]
    mask = ((src >= t_hi) | (src <= t_lo)).astype(np.float32) if both_sides else src >= t_hi
    return np.ascontiguousarray(np.broadcast_to(mask, labels.shape))


def threshold_distance(labels, t, both_sides: bool, dt: str) -> np.ndarray:
    """distance of every label from the nearest threshold of its compare, in ulps of the storage type at the label"""
    labels = np.asarray(labels, dtype=np.float64)
    d = np.abs(labels - float(round_dtype(float(t), dt)))
    if both_sides:
        d = np.minimum(d, np.abs(labels - float(round_dtype(1.0 - float(t), dt))))
    return d / ulp(np.maximum(np.abs(labels), 1e-300), dt)
