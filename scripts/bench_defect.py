"""Times EMDefectAugmentation on the GPU against the numpy branch on the same box and against a plain device copy.

    python scripts/bench_defect.py [--reps 10] [--warmup 2] [--inner 5] [--out profiles/defect_bench.txt]

Shape: 2 x 128 x 128 x 128 float32 (per_sample: 256 slices of 128 x 128).  Per deformation mode, one plan drawn under a fixed
seed and replayed, so every row of a block does the same work:
  * the floor: a plain device copy of the tensor (`out.copy_(x)`), one read and one write;
  * `apply_plan` on the device (table upload, artifact-free plan, all launches);
  * its parts through the ops: mean + streaming pass, prefilter, flow, warp;
  * `sample_plan` on the host (numpy draws and the interval tables), for the record;
  * the numpy branch (the reference's algorithm on scipy) on the same two volumes, host clock, `--numpy-reps` calls.
Device events around windows of `inner` calls; median and spread over the repetitions.  Without a GPU it fails.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_selftrain import alternate, fmt  # noqa: E402
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.transform import EMDefectAugmentation  # noqa: E402
from torch_em_amd.transform import defect as D  # noqa: E402

SHAPE = (2, 128, 128, 128)
P = dict(p_drop_slice=0.05, p_low_contrast=0.05, p_deform_slice=0.1)   # the CREMI loader's order of magnitude


def bench_mode(mode, x, reps, warmup, inner, numpy_reps, lines):
    aug = EMDefectAugmentation(**P, deformation_mode=mode, deformation_strength=10.0, per_sample=True)
    N, Z, H, W = x.shape
    np.random.seed(0)
    plan = aug.sample_plan(N * Z, (H, W))
    ptab, rec, tables, chosen = aug.plan_tables(plan)
    tab = ops.DefectTables(ptab, rec, tables, N * Z, H, W, 0, x.device)
    xs = x.reshape(N * Z, H, W)
    out = torch.empty_like(x)
    mean = ops.defect_mean(xs, tab)
    y = ops.defect_apply(xs, tab, mean)
    coef = torch.empty((tab.D, H, W), dtype=torch.float32, device=x.device)
    flow = torch.empty((tab.D, 2, H, W), dtype=torch.float32, device=x.device)
    gw, sw = D.gaussian_weights(), D.spline_fir_weights()
    rows = [("device copy (the floor)", lambda: out.copy_(x)),
            ("apply_plan (upload, all launches)", lambda: aug.apply_plan(x, plan)),
            ("  mean + streaming pass", lambda: ops.defect_apply(xs, tab, ops.defect_mean(xs, tab))),
            ("  prefilter", lambda: ops.defect_prefilter(xs, tab, sw, out=coef))]
    if (rec[:, 1] == 0).any():
        rows.append(("  flow", lambda: ops.defect_flow(tab, plan.seed, 10.0, gw, out=flow)))
    rows.append(("  warp", lambda: ops.defect_warp(coef, flow, y, tab, plan.seed, 10.0 / 8.)))
    stats = alternate([r[1] for r in rows], reps, warmup, inner=inner)
    counts = {a: plan.actions.count(a) for a in (D.DROP, D.LOW_CONTRAST, D.DEFORM)}
    kinds = [plan.deform[s][0] for s in plan.deformed]
    lines.append(f"mode {mode}: {N * Z} slices of {H} x {W}; plan: {counts}, undirected {kinds.count('undirected')}, compress {kinds.count('compress')}")
    for (name, _), st in zip(rows, stats):
        lines.append(f"  {name:<40} {fmt(st)}  {st['median'] / stats[0]['median']:7.2f} x the copy")
    t0 = time.perf_counter()
    for _ in range(20):
        np.random.seed(0)
        aug.sample_plan(N * Z, (H, W))
    lines.append(f"  {'sample_plan on the host':<40} {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms per call (host clock, 20 calls)")
    host = x.cpu().numpy()
    ref = EMDefectAugmentation(**P, deformation_mode=mode, deformation_strength=10.0)
    times = []
    for _ in range(numpy_reps):
        np.random.seed(0)
        t0 = time.perf_counter()
        for vol in host:
            ref(vol)
        times.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"  {'numpy branch, both volumes':<40} median {np.median(times):.1f} ms (min {min(times):.1f}, max {max(times):.1f}; host clock, "
                 f"{numpy_reps} calls) = {np.median(times) / stats[1]['median']:.0f} x apply_plan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--numpy-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_defect.py needs the GPU: a CPU run gives no timing")
    x = torch.rand(SHAPE, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    lines = [f"EM defect augmentation benchmark; {args.reps} repetitions after {args.warmup} warm-up, windows of {args.inner} calls, "
             "device events, alternating", f"device: {torch.cuda.get_device_name(0)}",
             f"tensor: {'x'.join(str(s) for s in SHAPE)} float32, {x.numel() * 4 / 1e6:.1f} MB"]
    for mode in ("undirected", "compress", "all"):
        bench_mode(mode, x, args.reps, args.warmup, args.inner, args.numpy_reps, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
