"""The answers of the forward-convolution dispatch queries over a grid of shapes, modes, layouts and options, as data:
tests/golden/conv_fwd_plan_table.json, which tests/test_conv_fwd_plan_cpu.py recomputes and compares exactly.

    python scripts/conv_fwd_plan_table.py            # writes the fixture from the library in the tree
    TEM_LIB=<other build> python scripts/...         # ... from another build of the same C-ABI

Needs no GPU: the queries are host code, and without a device tem_device_cus() fails, so the dispatch counts 256 CUs
(the MI355X's own number).  The committed fixture was written by the library as it stood BEFORE the launch and the
queries were put on one plan function; regenerate it only when the dispatch is meant to change.
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_fwd_plan_table.json")

# (N, D, H, W, Cin, Cout, (kd, kh, kw)): the five of tests/test_gpu_conv_layouts.py::SHAPES, then a level-0 and a bottom level of
# the flagship U-Net, a flat 2-D layer, 1x3x3 with depth (Cout % 64 == 0 and not), a Cin = 1 first layer
SHAPES = [
    (2, 8, 16, 16, 32, 32, (3, 3, 3)),
    (1, 16, 16, 16, 256, 256, (3, 3, 3)),
    (2, 8, 16, 16, 32, 64, (3, 3, 3)),
    (2, 12, 24, 24, 128, 64, (3, 3, 3)),
    (1, 16, 32, 32, 64, 32, (1, 1, 1)),
    (2, 128, 128, 128, 32, 32, (3, 3, 3)),
    (1, 8, 8, 8, 256, 256, (3, 3, 3)),
    (1, 1, 64, 64, 32, 32, (1, 3, 3)),
    (2, 16, 64, 64, 32, 64, (1, 3, 3)),
    (2, 16, 64, 64, 32, 96, (1, 3, 3)),
    (2, 32, 32, 32, 1, 32, (3, 3, 3)),
]
# use_mfma: the arithmetic mode, and 5 / 7 with fp16 / bf16 storage in TEM_MFMA_STX and TEM_MFMA_STY
MODES = [0, 1, 2, 3, 4, 5, 6, 7, 5 | (1 << 8) | (1 << 12), 7 | (2 << 8) | (2 << 12)]
OPTIONS = ["conv_fwd_variant", "zr_splitk", "fp32_zr", "team_min_units"]
OPTION_VALUES = [(-1, 0, 1, 2), (1, 0), (1, 0, 2), (0, 1)]


def layouts(H, W, Cin, Cout):
    """(x_ld, y_ld, ref_ld, misaligned) of one shape; ref_ld 0: no ref"""
    # the team kernels address a halo with 32-bit byte offsets: H * W * 32 * ld < 2^31.  A leading dimension on each side
    lim = -(-(1 << 26) // (H * W))          # the smallest ld that is past the limit
    below, above = (lim - 1) // 8 * 8, (lim + 7) // 8 * 8
    out = [(Cin, Cout, 0, 0),               # dense
           (Cin + 8, Cout, 0, 0),           # wide x
           (Cin, Cout + 8, 0, 0),           # wide y
           (Cin, Cout + 3, 0, 0),           # y_ld % 4 != 0
           (Cin, Cout, Cout, 0),            # with a ref
           (Cin, Cout, Cout + 3, 0),        # ... whose ld % 4 != 0
           (Cin, Cout, 0, 1),               # misaligned
           (Cin, Cout, Cout, 1)]
    for ld in (below, above):
        out += [(ld, Cout, 0, 0), (Cin, ld, 0, 0), (Cin, Cout, ld, 0)]
    return out


def table(lib):
    """{"<options>": [per shape: {"ws": [per mode], "plan": [per mode: [family, stat_blocks, family, stat_blocks, ...] over layouts()]}]}
    under every combination of OPTION_VALUES; puts the options back as it found them"""
    from torch_em_amd import _lib
    saved = [_lib.get_option(o) for o in OPTIONS]
    out = {}
    try:
        for vals in itertools.product(*OPTION_VALUES):
            for o, v in zip(OPTIONS, vals):
                _lib.set_option(o, v)
            rows = []
            for (N, D, H, W, Cin, Cout, k) in SHAPES:
                ws, plan = [], []
                for mode in MODES:
                    a = (N, D, H, W, Cin, Cout, k[0], k[1], k[2], mode)
                    ws.append(int(lib.tem_conv3d_fwd_ws(*a)))
                    row = []
                    for lay in layouts(H, W, Cin, Cout):
                        row += [int(lib.tem_conv3d_fwd_kernel_ld(*a, *lay)), int(lib.tem_conv3d_fwd_stat_blocks_ld(*a, *lay))]
                    if (int(lib.tem_conv3d_fwd_kernel(*a)), int(lib.tem_conv3d_fwd_stat_blocks(*a))) != tuple(row[:2]):
                        raise AssertionError(f"the shape-only queries differ from the dense layout: {a}")
                    plan.append(row)
                rows.append({"ws": ws, "plan": plan})
            out[",".join(f"{o}={v}" for o, v in zip(OPTIONS, vals))] = rows
    finally:
        for o, v in zip(OPTIONS, saved):
            _lib.set_option(o, v)
    return out


def pack(t):
    """table() as the fixture stores it: the answers of most shapes do not move with most options, so every distinct per-shape
    answer once ("answers") and, per option combination, the index of each shape's answer ("options")"""
    answers, index = [], {}
    options = {k: [index.setdefault(json.dumps(r, sort_keys=True), len(index)) for r in rows] for k, rows in t.items()}
    for key in index:   # (insertion order = index order)
        answers.append(json.loads(key))
    return {"answers": answers, "options": options}


def unpack(fx):
    return {k: [fx["answers"][i] for i in idx] for k, idx in fx["options"].items()}


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
    print(f"wrote {FIXTURE}: {sum(len(r['plan']) * len(r['plan'][0]) // 2 for rows in t.values() for r in rows)} grid points")


if __name__ == "__main__":
    main()
