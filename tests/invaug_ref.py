"""numpy oracle of the per-sample dihedral transform (`ops.dihedral`, csrc/invaug.hip): the index map of include/tem_hip.h
written out element by element, on raw bit patterns so NaN payloads and -0.0 compare exactly."""
import json

import numpy as np
import torch

INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)
# (h, v) -> codes for k = -1, 0, 1, 2: x.flip(-1) if h, .flip(-2) if v, then torch.rot90(., k, (-2, -1))
CODE_TABLE = {(0, 0): (3, 0, 5, 6), (0, 1): (1, 2, 7, 4), (1, 0): (7, 4, 1, 2), (1, 1): (5, 6, 3, 0)}
_VIEW = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def index_map(code: int, H: int, W: int):
    """(r, s): integer arrays of the output's shape with out[i, j] = src[r[i, j], s[i, j]]"""
    Ho, Wo = (W, H) if code & 1 else (H, W)
    i, j = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    r, s = (j, i) if code & 1 else (i, j)
    if code & 2:
        r = H - 1 - r
    if code & 4:
        s = W - 1 - s
    return r, s


def dihedral_np(x: np.ndarray, codes) -> np.ndarray:
    """x [N, ..., H, W] (any dtype) -> the transformed array; all codes transpose or none does unless H == W"""
    N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    assert len(codes) == N
    odd = any(c & 1 for c in codes)
    out = np.empty(x.shape[:-2] + ((W, H) if odd else (H, W)), dtype=x.dtype)
    for n, c in enumerate(codes):
        r, s = index_map(int(c), H, W)
        out[n] = x[n][..., r, s]
    return out


# ---- readers of tests/golden/g19_invertible.npz ---------------------------------------------------------------------
def _unflatten(fixture, flat):
    keys, shapes = json.loads(str(fixture["ia_state_keys"])), json.loads(str(fixture["ia_state_shapes"]))
    state, o = {}, 0
    for k, shape in zip(keys, shapes):
        n = int(np.prod(shape)) if shape else 1
        state[k] = flat[o:o + n].view(np.float32).reshape(shape).copy()
        o += n
    assert o == flat.size
    return state


def ia_states(fixture, tag: str):
    """the student of run `tag` before the first optimizer step and after every one, each {name: float32 array}"""
    flat = fixture["ia_pre0"].view(np.int32).copy()
    out = [_unflatten(fixture, flat)]
    for row in fixture[f"ia_{tag}_chain"]:
        flat = flat + row   # int32 arrays wrap, as the generator's difference did
        out.append(_unflatten(fixture, flat))
    return out


def ia_teachers(fixture, tag: str, students_after, momentum: float, reinit: bool):
    """the teacher before iteration 0, 1, ... and after the last: the reference's update from `ia_<tag>_teacher0` and the
    student after each iteration, in float32 on the CPU (gen_golden_invertible.py asserts that this gives the reference's
    teachers bit for bit)"""
    teachers = [{k: torch.from_numpy(v) for k, v in _unflatten(fixture, fixture[f"ia_{tag}_teacher0"].view(np.int32)).items()}]
    for i, student in enumerate(students_after):
        m = min(1 - 1 / (i + 1), momentum) if reinit else momentum
        teachers.append({k: teachers[-1][k] * m + torch.from_numpy(student[k]) * (1.0 - m) for k in teachers[0]})
    return teachers


def bits(t: torch.Tensor) -> np.ndarray:
    """the raw bit patterns of a tensor of 1-, 2- or 4-byte elements as an unsigned numpy array"""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).numpy().view(_VIEW[t.element_size()])


def patterned(shape, dtype: torch.dtype, seed: int = 0) -> torch.Tensor:
    """every element distinct where the width allows, with NaN payloads, infinities and -0.0 among the floats"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    size = torch.empty((), dtype=dtype).element_size()
    if dtype == torch.bool:
        return torch.from_numpy(rng.integers(0, 2, n).astype(np.bool_)).reshape(shape)
    if size == 1:
        raw = rng.integers(0, 256, n).astype(np.uint8)
        return torch.from_numpy(raw).view(dtype).reshape(shape)
    if size == 2:
        raw = (rng.permutation(max(n, 1 << 16))[:n] & 0xFFFF).astype(np.uint16)
        special = np.array([0x8000, 0x7FC1, 0xFFFF, 0x7C01, 0x7F80, 0xFF81, 0x0001], dtype=np.uint16)   # -0.0, NaN payloads, ...
    else:
        raw = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        special = np.array([0x80000000, 0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0x7F800000, 0xFFC12345, 0x00000001], dtype=np.uint32)
    k = min(len(special), n)
    raw[rng.permutation(n)[:k]] = special[:k]
    signed = raw.view({2: np.int16, 4: np.int32}[size])
    return torch.from_numpy(signed.copy()).view(dtype).reshape(shape)
