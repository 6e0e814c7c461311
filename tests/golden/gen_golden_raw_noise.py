"""Golden vectors of the noise transforms' numpy branch by IMPORTING THE REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_raw_noise.py <torch-em checkout>

Same loader as gen_golden_raw.py (the reference's transform/raw.py by path, an empty stub for `torchvision`).  For each of
AdditiveGaussianNoise, AdditivePoissonNoise and PoissonNoise: np.random.seed(seed), then the reference class on a small
float32 array -- shapes (5, 7) and (2, 3, 4, 5), default arguments and one other range, clip_kwargs=None once.  Writes
g16_raw_noise.npz, data only.  Keys: `numpy_version`, `cases`, `input.<shape>`; per case `<case>.cls` (index into CLASSES),
`.input`, `.range` (the two bounds handed to the class), `.clip` (0: clip_kwargs=None, 1: the default), `.seed`, `.out`.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_raw import load_reference  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(OUT, "g16_raw_noise.npz")
CLASSES = ["AdditiveGaussianNoise", "AdditivePoissonNoise", "PoissonNoise"]
RANGE_KEY = {"AdditiveGaussianNoise": "scale", "AdditivePoissonNoise": "lam", "PoissonNoise": "multiplier"}
A, B = (5, 7), (2, 3, 4, 5)
# name: (class, shape, range or None for the default, clip?, seed)
CASES = {
    "gauss_default": ("AdditiveGaussianNoise", A, None, 1, 21),
    "gauss_range": ("AdditiveGaussianNoise", B, (0.1, 0.5), 1, 22),
    "gauss_noclip": ("AdditiveGaussianNoise", B, None, 0, 23),
    "padd_default": ("AdditivePoissonNoise", B, None, 1, 24),
    "padd_range": ("AdditivePoissonNoise", A, (2.0, 30.0), 1, 25),
    "padd_noclip": ("AdditivePoissonNoise", A, (0.5, 4.0), 0, 26),
    "pois_default": ("PoissonNoise", A, None, 1, 27),
    "pois_range": ("PoissonNoise", B, (20.0, 200.0), 1, 28),
    "pois_noclip": ("PoissonNoise", B, None, 0, 29),
}
DEFAULT_RANGE = {"AdditiveGaussianNoise": (0.0, 0.3), "AdditivePoissonNoise": (0.0, 0.1), "PoissonNoise": (5.0, 10.0)}


def data(shape):
    return np.random.RandomState(1600 + len(shape)).rand(*shape).astype("float32")


def build(module, cls, rng, clip):
    kwargs = {} if rng is None else {RANGE_KEY[cls]: tuple(rng)}
    if not clip:
        kwargs["clip_kwargs"] = None
    return getattr(module, cls)(**kwargs)


def main(checkout):
    raw = load_reference(os.path.join(os.path.abspath(checkout), "torch_em"))
    res = {"numpy_version": np.array(np.__version__), "cases": np.array(sorted(CASES))}
    for name, (cls, shape, rng, clip, seed) in CASES.items():
        key = "x".join(str(v) for v in shape)
        x = data(shape)
        res["input." + key] = x
        np.random.seed(seed)
        out = build(raw, cls, rng, clip)(x)
        res.update({f"{name}.cls": np.int32(CLASSES.index(cls)), f"{name}.input": np.array(key),
                    f"{name}.range": np.asarray(DEFAULT_RANGE[cls] if rng is None else rng, dtype=np.float64),
                    f"{name}.clip": np.int32(clip), f"{name}.seed": np.int32(seed), f"{name}.out": out})
        print(name, cls, shape, out.dtype, "out range", float(out.min()), float(out.max()))
    np.savez_compressed(FIXTURE, **res)
    print(os.path.getsize(FIXTURE), "bytes, numpy", np.__version__)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(f"usage: {sys.argv[0]} <torch-em checkout>")
    main(sys.argv[1])
