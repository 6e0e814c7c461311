"""The answers of the weight-gradient dispatch queries over a grid of shapes, modes and options, as data:
tests/golden/conv_wgrad_plan_table.json, which tests/test_conv_wgrad_plan_cpu.py recomputes and compares exactly.

    python scripts/conv_wgrad_plan_table.py          # writes the fixture from the library in the tree
    TEM_LIB=<other build> python scripts/...         # ... from another build of the same C-ABI

Needs no GPU: the queries are host code, and without a device tem_device_cus() fails, so the dispatch counts 256 CUs
(the MI355X's own number).  The committed fixture was written by the library as it stood BEFORE the launch and the
queries were put on one plan function (csrc/conv.hip: wgrad_plan); regenerate it only when the dispatch is meant to change.
The workspace answer carries the slab count, the k-split and the sums region of the plan, so it moves with wgrad_zs,
wgrad_zs_persist and wgrad_cus: that pins the geometry without a query of its own.
"""
import itertools
import json
import os
import sys

from conv_fwd_plan_table import pack, unpack   # noqa: F401  (the fixture format is shared)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_wgrad_plan_table.json")

K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
# (N, D, H, W, Cin, Cout, (kd, kh, kw)): each outcome and each boundary of the plan on both sides at least once
SHAPES = [
    (2, 128, 128, 128, 32, 32, K333),   # level 0: persistent segments, sums eligible at 128 MiB
    (2, 8, 16, 16, 32, 32, K333),       # D = TEM_ZS_MIN_D ...
    (2, 7, 16, 16, 32, 32, K333),       # ... and below it
    (1, 16, 16, 16, 64, 96, K333),      # Cout / 4 is no power of two
    (5, 8, 8, 8, 32, 32, K333),         # N > 4
    (1, 8, 8, 8, 32, 256, K333),        # Cout > 128
    (1, 8, 8, 8, 512, 512, K333),       # slabs of 8 MiB and more in the patch plan (wgrad_zs = 0)
    (2, 16, 64, 64, 32, 64, K133),      # 1x3x3 with depth
    (1, 1, 64, 64, 32, 32, K133),       # flat 2-D
    (1, 16, 32, 32, 64, 128, K111),     # four output-channel tiles per workgroup
    (2, 32, 32, 32, 1, 32, K333),       # the small-Cin first layer ...
    (1, 8, 8, 8, 3, 16, K333),
    (1, 8, 8, 8, 5, 16, K333),          # ... and past it
    (1, 16, 32, 32, 64, 2, K111),       # projection and out_bwd ...
    (1, 8, 8, 8, 96, 2, K111),          # ... and their boundaries
    (1, 8, 8, 8, 64, 5, K111),
    (1, 8, 8, 8, 48, 32, K333),         # MFMA modes on channel counts they refuse
    (1, 8, 8, 8, 16, 32, K333),
]
# use_mfma: the arithmetic mode, and 5 / 7 with fp16 / bf16 storage in TEM_MFMA_STX and TEM_MFMA_STY
MODES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 5 | (1 << 8) | (1 << 12), 7 | (2 << 8) | (2 << 12)]
OPTIONS = ["wgrad_zs", "wgrad_zs_persist", "wgrad_sums", "wgrad_sums_min_mb", "wgrad_cus", "fp32_zr"]
OPTION_VALUES = [(0, 1, 2, 3), (1, 0), (1, 0), (0, 128), (256, 64), (1, 0)]
CS = [(st, x_cs) for st in (0, 1, 2) for x_cs in (64, 4)]


def table(lib):
    """{"<options>": [per shape: {"ws" / "sums" / "gmax": [per mode], "gnorm": [per mode], "gscaled": int, "cs": [per CS],
    "out_bwd": [ok, ws]}]} under every combination of OPTION_VALUES; puts the options back as it found them"""
    from torch_em_amd import _lib
    saved = [_lib.get_option(o) for o in OPTIONS]
    out = {}
    try:
        for vals in itertools.product(*OPTION_VALUES):
            for o, v in zip(OPTIONS, vals):
                _lib.set_option(o, v)
            rows = []
            for (N, D, H, W, Cin, Cout, k) in SHAPES:
                s = (N, D, H, W, Cin, Cout, k[0], k[1], k[2])
                row = {"ws": [int(lib.tem_conv3d_wgrad_ws(*s, m)) for m in MODES],
                       "sums": [int(lib.tem_conv3d_wgrad_sums_ok(*s, m)) for m in MODES],
                       "gmax": [int(lib.tem_conv3d_wgrad_gmax_ok(*s, m)) for m in MODES],
                       "gnorm": [int(lib.tem_conv3d_wgrad_gnorm_ok(Cin, Cout, k[0], k[1], k[2], m)) for m in MODES],
                       "gscaled": int(lib.tem_conv3d_wgrad_gscaled_ok(*s)),
                       "cs": [int(lib.tem_conv3d_wgrad_cs_ok(*s, st, x_cs)) for st, x_cs in CS],
                       "out_bwd": [int(lib.tem_conv1x1_out_bwd_ok(Cin, Cout)), int(lib.tem_conv1x1_out_bwd_ws(Cin, Cout))]}
                neg = {k_: v for k_, v in row.items() if min(v if isinstance(v, list) else [v]) < 0}
                if neg:   # a predicate answers 0 or 1 and a size is not negative: a negative value is a leaked error code
                    raise AssertionError(f"a query returned a negative value: {s} {dict(zip(OPTIONS, vals))} {neg}")
                rows.append(row)
            out[",".join(f"{o}={v}" for o, v in zip(OPTIONS, vals))] = rows
    finally:
        for o, v in zip(OPTIONS, saved):
            _lib.set_option(o, v)
    return out


def main():
    sys.path.insert(0, ROOT)
    from torch_em_amd import _lib
    lib = _lib.load()
    cus = lib.tem_device_cus()
    if cus > 0 and cus != 256:
        sys.exit(f"this device has {cus} CUs: the fixture is written for 256 (or no device)")
    t = table(lib)
    with open(FIXTURE, "w") as f:
        fx = pack(t)
        f.write('{"answers": [\n' + ",\n".join(json.dumps(a, separators=(",", ":"), sort_keys=True) for a in fx["answers"]) + '\n],\n"options": {\n'
                + ",\n".join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in fx["options"].items()) + "\n}}\n")
    print(f"wrote {FIXTURE}: {len(t)} option combinations x {len(SHAPES)} shapes, {len(fx['answers'])} distinct answers")


if __name__ == "__main__":
    main()
