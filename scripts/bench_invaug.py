"""Times the per-sample dihedral transform (`ops.dihedral`, csrc/invaug.hip) on the GPU, in one process, alternating the things
compared.

    python scripts/bench_invaug.py [--reps 20] [--warmup 3] [--inner 10] [--out profiles/invaug_bench.txt]

Shapes: 2 x 1 x 128^3 and 2 x 32 x 64^3 (a raw batch and a prediction-sized tensor; both sit in the 256 MiB last-level cache)
and 2 x 32 x 128^3 (beyond it), fp32 and bf16.  Per shape and type:
  * the floor: a plain device copy of the same tensor (`out.copy_(x)`), one read and one write;
  * the kernel alone through the library's entry point (codes already on the device, output allocated), per path:
    vector stream (codes 0, 2, 4, 6), scalar stream (code 6 from a base one element off a 16-byte boundary), tile (code 3;
    for bf16 both variants: packed 64 x 64 tiles, and -- from a base off a dword boundary -- 32 x 32 tiles with one element
    per LDS dword), and a mixed batch (6, 3);
  * `ops.dihedral` as the trainers call it (code upload and output allocation included);
  * what it replaces: the torch composition, a per-sample `flip` / `rot90` loop plus `stack`.
Bytes moved are 2 x the tensor's size for every row; GB/s and the fraction of the copy's rate are printed per path.
Device events around windows of `inner` calls; median and spread over the repetitions.  Without a GPU it fails.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_selftrain import alternate, fmt  # noqa: E402
from torch_em_amd import _lib, ops  # noqa: E402

SHAPES = ((2, 1, 128, 128, 128), (2, 32, 64, 64, 64), (2, 32, 128, 128, 128))
HVK = {0: (0, 0, 0), 2: (0, 1, 0), 4: (1, 0, 0), 6: (0, 0, 2), 3: (0, 0, -1), 5: (0, 0, 1)}   # code -> (h, v, k) of the torch composition


def torch_composition(x, codes):
    out = []
    for sample, c in zip(x, codes):
        h, v, k = HVK[c]
        if h:
            sample = sample.flip(-1)
        if v:
            sample = sample.flip(-2)
        out.append(torch.rot90(sample, k, (-2, -1)) if k else sample)
    return torch.stack(out)


def bench_shape(shape, dtype, reps, warmup, inner, dev, lines):
    lib = _lib.load()
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator().manual_seed(0)
    buf = torch.empty(n + 8, dtype=dtype, device=dev)
    x = buf[:n].view(shape)
    x.copy_(torch.randn(shape[0], shape[1], 8, 8, 8, generator=g).to(dev).to(dtype).repeat(1, 1, *(s // 8 for s in shape[2:])))
    x_off = buf[1:n + 1].view(shape)      # one element off the 16-byte boundary
    out = torch.empty(shape, dtype=dtype, device=dev)
    N, H, W = shape[0], shape[-2], shape[-1]
    planes, eb = n // (N * H * W), x.element_size()

    def launch(src, codes):
        dev_codes = torch.tensor(codes, dtype=torch.int32, device=dev)

        def run():
            _lib.check(lib.tem_dihedral2d(ops._p(src), ops._p(out), ops._p(dev_codes), N, planes, H, W, eb, ops._stream(src)), "tem_dihedral2d")
        return run

    rows = [("device copy (the floor)", lambda: out.copy_(x), None)]
    for code in (0, 2, 4, 6):
        rows.append((f"vector stream, code {code}", launch(x, [code] * N), ops.dihedral_path(x, code, out=out)))
    rows.append(("scalar stream, code 6 (base off by one element)", launch(x_off, [6] * N), ops.dihedral_path(x_off, 6, out=out)))
    tiles = {ops.DH_PATH_TILE: "tile, one element per LDS dword", ops.DH_PATH_TILE_PACKED: "tile, packed"}
    rows.append((tiles[ops.dihedral_path(x, 3, out=out)] + ", code 3", launch(x, [3] * N), ops.dihedral_path(x, 3, out=out)))
    # a base one element off a dword boundary sends the narrow types to the 32 x 32 tile with one element per LDS dword
    rows.append((tiles[ops.dihedral_path(x_off, 3, out=out)] + ", code 3 (base off by one element)", launch(x_off, [3] * N),
                 ops.dihedral_path(x_off, 3, out=out)))
    rows.append(("mixed batch, codes (6, 3)", launch(x, [6, 3]), None))
    rows.append(("ops.dihedral, codes (6, 3), with upload and allocation", lambda: ops.dihedral(x, [6, 3]), None))
    rows.append(("torch composition, codes (6, 3): flip / rot90 per sample + stack", lambda: torch_composition(x, [6, 3]), None))
    want = {"vector": (ops.DH_PATH_VEC,), "scalar": (ops.DH_PATH_SCALAR,), "tile": (ops.DH_PATH_TILE, ops.DH_PATH_TILE_PACKED)}
    for name, _, path in rows:
        assert path is None or path in want[name.split()[0].rstrip(",")], (name, path)
    assert rows[6][2] == (ops.DH_PATH_TILE if eb == 4 else ops.DH_PATH_TILE_PACKED) and rows[7][2] == ops.DH_PATH_TILE
    assert torch.equal(ops.dihedral(x, [6, 3]), torch_composition(x, [6, 3])), "the kernel and the torch composition disagree"
    stats = alternate([r[1] for r in rows], reps, warmup, inner=inner)
    nbytes = 2 * n * eb
    copy_rate = nbytes / (stats[0]["median"] * 1e-3)
    lines.append(f"{'x'.join(str(s) for s in shape)} {str(dtype).split('.')[1]}: {n * eb / 1e6:.1f} MB read + {n * eb / 1e6:.1f} MB written per call, "
                 f"{inner} calls per timed window")
    for (name, _, _), st in zip(rows, stats):
        rate = nbytes / (st["median"] * 1e-3)
        lines.append(f"  {name:<66} {fmt(st)}  {rate / 1e9:8.0f} GB/s  {rate / copy_rate:5.2f} of the copy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_invaug.py needs the GPU: a CPU run gives no timing")
    dev = "cuda:0"
    lines = [f"dihedral transform benchmark; {args.reps} repetitions after {args.warmup} warm-up, device events, alternating",
             f"device: {torch.cuda.get_device_name(0)}"]
    for shape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            bench_shape(shape, dtype, args.reps, args.warmup, args.inner, dev, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
