"""Golden vectors of the raw transforms by IMPORTING THE REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_raw.py <torch-em checkout>

Loads the reference's transform/raw.py by path (an empty stub stands in for `torchvision` / `torchvision.transforms`, which
the reference touches only when a blur or the mean-teacher default is CALLED) and writes g15_raw_transforms.npz, data only.
Keys: `numpy_version`, `cases` (the case names), `input.<name>` (the inputs; cases of one data kind and shape share one);
per case `<case>.input` (the name of its input), `.kind` (which transform, see KINDS), `.args` (float64 vector, meaning per
kind below) and `.out` (the reference's output).  Additionally
  * percentile cases: `.v_lower`, `.v_upper` (np.percentile(x, q, axis, keepdims=True) as the reference forms them);
  * integer inputs (`u8`, `i16`): `.out` is the reference on x.astype("float32") -- what the device path computes --, and
    `.out_int` its output on the integer array itself (percentiles interpolated in float64);
  * RandomPercentileNormalization: `.draws` = the first 4 pairs of sample_percentiles() of a fresh, equally seeded object;
    `.out` is the call of another fresh object (its first draw); `.out_per_sample`: each entry of the first axis
    transformed one after another by ONE object (draws 0, 1, ...), stacked -- what per_sample=True computes for a batch;
  * RandomContrast: np.random.seed(args[4]) precedes the call; `.out_per_sample` as above.
args: normalize (axis mode); percentile (lower, upper, axis mode); rpn (seed, normal?, mean, std, lower bounds, upper
bounds); contrast (alpha lo, alpha hi, mean, clip?, seed); chain (lower, upper, alpha lo, alpha hi, mean, seed).
axis mode: 0 axis=None, 1 all axes but the first (per sample), 2 all axes but the first two (per channel).
"""
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(OUT, "g15_raw_transforms.npz")
KINDS = {"normalize": 0, "percentile": 1, "rpn": 2, "contrast": 3, "chain": 4}


def load_reference(ref):
    for name in ("torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    spec = importlib.util.spec_from_file_location("reference_raw", os.path.join(ref, "transform", "raw.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def axis_of(mode, ndim):
    return None if mode == 0 else tuple(range(mode, ndim))


def data(kind, shape, seed):
    rng = np.random.RandomState(seed)
    if kind == "uniform":
        return rng.rand(*shape).astype("float32")
    if kind == "normal":
        return (rng.randn(*shape) * 3.0 + 1.0).astype("float32")
    if kind == "bytes":    # 0..255 stored as float: constant top byte, massive ties
        return rng.randint(0, 256, size=shape).astype("float32")
    if kind == "u8":
        return rng.randint(0, 256, size=shape).astype("uint8")
    if kind == "i16":
        return rng.randint(-3000, 3000, size=shape).astype("int16")
    raise ValueError(kind)


BIG, MID, SMALL = (2, 1, 9, 17, 33), (2, 1, 4, 7, 13), (3, 2, 8, 8)
# name: (kind, data kind, shape, args)
CASES = {
    "norm_all": ("normalize", "normal", BIG, (0,)),
    "norm_sample": ("normalize", "normal", MID, (1,)),
    "norm_channel": ("normalize", "bytes", SMALL, (2,)),
    "pct_all": ("percentile", "uniform", MID, (1.0, 99.0, 0)),
    "pct_sample": ("percentile", "normal", BIG, (1.0, 99.0, 1)),
    "pct_channel": ("percentile", "normal", SMALL, (5.0, 95.0, 2)),
    "pct_bytes": ("percentile", "bytes", (24, 24, 24), (0.1, 99.7, 0)),
    "pct_u8": ("percentile", "u8", SMALL, (1.0, 99.0, 0)),
    "pct_i16": ("percentile", "i16", MID, (2.0, 98.0, 1)),
    "rpn_uniform": ("rpn", "uniform", MID, (42, 0, 0.0, 0.0, 0.0, 5.0, 95.0, 100.0)),
    "rpn_normal": ("rpn", "bytes", SMALL, (7, 1, 2.0, 1.0, 0.0, 5.0, 95.0, 100.0)),
    "contrast": ("contrast", "uniform", MID, (0.5, 2.0, 0.5, 1, 11)),
    "contrast_noclip": ("contrast", "normal", SMALL, (0.5, 2.0, 0.25, 0, 12)),
    "chain": ("chain", "bytes", SMALL, (1.0, 99.0, 0.5, 2.0, 0.5, 13)),
}
SEEDS = {"uniform": 1501, "normal": 1502, "bytes": 1503, "u8": 1504, "i16": 1505}


def make_rpn(raw, a):
    kw = {"distribution": "normal", "distribution_kwargs": {"mean": a[2], "std": a[3]}} if a[1] else {}
    return raw.RandomPercentileNormalization(lower_percentile_bounds=(a[4], a[5]), upper_percentile_bounds=(a[6], a[7]),
                                             seed=int(a[0]), **kw)


def main(checkout):
    import functools
    raw = load_reference(os.path.join(os.path.abspath(checkout), "torch_em"))
    res = {"numpy_version": np.array(np.__version__), "cases": np.array(sorted(CASES))}
    for name, (kind, dkind, shape, args) in CASES.items():
        key = dkind + "_" + "x".join(str(v) for v in shape)
        x = data(dkind, shape, SEEDS[dkind])
        assert x.size <= 24 ** 3, name
        res["input." + key] = x
        xf = x.astype("float32")
        out = {"input": np.array(key), "kind": np.int32(KINDS[kind]), "args": np.asarray(args, dtype=np.float64)}
        if kind == "normalize":
            out["out"] = raw.normalize(xf, axis=axis_of(args[0], x.ndim))
        elif kind == "percentile":
            lo, up, ax = args[0], args[1], axis_of(args[2], x.ndim)
            out["out"] = raw.normalize_percentile(xf, lo, up, axis=ax)
            out["v_lower"] = np.percentile(xf, lo, axis=ax, keepdims=True)
            out["v_upper"] = np.percentile(xf, up, axis=ax, keepdims=True)
            if x.dtype != np.float32:
                out["out_int"] = raw.normalize_percentile(x, lo, up, axis=ax)
        elif kind == "rpn":
            probe = make_rpn(raw, args)
            out["draws"] = np.asarray([probe.sample_percentiles() for _ in range(4)], dtype=np.float64)
            out["out"] = make_rpn(raw, args)(xf)
            one = make_rpn(raw, args)
            out["out_per_sample"] = np.stack([one(s) for s in xf])
        elif kind == "contrast":
            t = raw.RandomContrast(alpha=(args[0], args[1]), mean=args[2],
                                   clip_kwargs={"a_min": 0, "a_max": 1} if args[3] else None)
            np.random.seed(int(args[4]))
            out["out"] = t(xf)
            np.random.seed(int(args[4]))
            out["out_per_sample"] = np.stack([t(s) for s in xf])
        elif kind == "chain":
            t = raw.get_raw_transform(normalizer=functools.partial(raw.normalize_percentile, lower=args[0], upper=args[1]),
                                      augmentation2=raw.RandomContrast(alpha=(args[2], args[3]), mean=args[4]))
            np.random.seed(int(args[5]))
            out["out"] = t(xf)
        assert out["out"].dtype == np.float32, (name, out["out"].dtype)
        res.update({f"{name}.{k}": v for k, v in out.items()})
        print(name, kind, x.dtype, shape, "out range", float(out["out"].min()), float(out["out"].max()))
    np.savez_compressed(FIXTURE, **res)
    print(os.path.getsize(FIXTURE), "bytes, numpy", np.__version__)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(f"usage: {sys.argv[0]} <torch-em checkout>")
    main(sys.argv[1])
