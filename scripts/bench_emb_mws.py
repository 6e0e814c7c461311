"""Times the two kernels around the embedding mutex watershed (csrc/embmws.hip): `ops.embedding_edges` on 1 x 16 x 1024^2
embeddings with the DSB offset list of the SPOCO experiments, set beside its byte floor (E + 5 C / 4) V 4, and
`ops.merge_background_by_embedding_` on the segmentation of the same image.

    python scripts/bench_emb_mws.py [--reps 9] [--calls 100] [--out profiles/emb_mws_bench.txt]

Inputs are synthetic: Voronoi cells of random points, a centre 3 delta from the others per cell, Gaussian noise of
0.1 delta.  Device events around `--calls` back-to-back calls (one call is tens of microseconds: a window of one would time
the launch); median and spread of the per-call time over the repetitions.  No CPU fallback: without a GPU the script fails."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torch_em_amd import ops  # noqa: E402

DEV = "cuda:0"
OFFSETS = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-9, 0], [0, -9], [-27, 0], [0, -27]]
DELTA, E, SIDE = 0.75, 16, 1024


def per_call_ms(fn, calls, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    s = sorted(out)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_emb_mws.py needs the GPU: a CPU run gives no timing")
    g = torch.Generator(device=DEV).manual_seed(0)
    cells = 48
    pts = torch.rand((cells, 2), generator=g, device=DEV) * SIDE
    yy, xx = torch.meshgrid(torch.arange(SIDE, device=DEV, dtype=torch.float32), torch.arange(SIDE, device=DEV, dtype=torch.float32), indexing="ij")
    lab = ((yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2).argmin(-1)
    centres = 3 * DELTA * torch.randn((cells, E), generator=g, device=DEV)
    emb = centres[lab].permute(2, 0, 1) + 0.1 * DELTA * torch.randn((E, SIDE, SIDE), generator=g, device=DEV)
    emb = emb.reshape(1, E, 1, SIDE, SIDE).contiguous()
    V, C = SIDE * SIDE, len(OFFSETS)
    floor = (E + 5 * C / 4) * V * 4
    lines = [f"embedding mutex watershed kernels (csrc/embmws.hip); {args.reps} repetitions of {args.calls} back-to-back calls, device events",
             f"device: {torch.cuda.get_device_name(0)}",
             f"embedding_edges, 1 x {E} x {SIDE}^2, {C} offsets (reach 1, 3, 9, 27), strides 4, delta {DELTA}; byte floor "
             f"(E + 5 C / 4) V 4 = {floor / 1e6:.1f} MB"]
    for dist in ("l2", "l1"):
        med, lo, hi = per_call_ms(lambda: ops.embedding_edges(emb, OFFSETS, DELTA, 2, [4, 4], dist), args.calls, args.reps)
        lines += [f"  {dist}: median {1e3 * med:.1f} us a call (min {1e3 * lo:.1f}, max {1e3 * hi:.1f}), output allocation included; "
                  f"floor bytes / median = {floor / (med * 1e-3) / 1e12:.2f} TB/s"]
    aff, valid = ops.embedding_edges(emb, OFFSETS, DELTA, 2, [4, 4])
    ids = ops.mutex_watershed(aff, OFFSETS, 2, None, valid)
    n = int(ids.max())
    med, lo, hi = per_call_ms(lambda: ops.merge_background_by_embedding_(ids.clone(), emb, DELTA), max(args.calls // 10, 1), args.reps)
    left = int(ops.merge_background_by_embedding_(ids.clone(), emb, DELTA).max())
    lines += [f"merge_background_by_embedding_ on its {n} segments ({left} left), the clone of the ids included: median {med:.3f} ms a call "
              f"(min {lo:.3f}, max {hi:.3f}); {2 * E + 4} launches and a scan"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
