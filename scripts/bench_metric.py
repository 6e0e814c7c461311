"""Times the instance-segmentation scores on the device: `ops.label_overlaps`, `ops.overlap_scores` and the four score
classes of `torch_em_amd.metric` on one 64^3 and one 128^3 sample with about 200 objects; beside them the same scores by
the numpy oracle (tests/metric_ref.py) including the copy of both label volumes to the host, and the seeded watershed that
produces the segmentation.

    python scripts/bench_metric.py [--reps 10] [--warmup 3] [--out profiles/metric_bench.txt]

Inputs are synthetic (scripts/bench_watershed.py: smoothed noise, about 200 markers): the target is the watershed of one
height map, the segmentation the watershed of another from the same markers, so the objects overlap like a good but not
perfect prediction.  Device events around each call; median and spread over the repetitions; the host figures are wall
clock.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_watershed as BW  # noqa: E402
from torch_em_amd import metric, ops  # noqa: E402

DEV = BW.DEV


def host_scores(seg, target, M):
    """the oracle's scores from device tensors: the copy to the host, the table (np.unique of the pairs), the scores"""
    t0 = time.perf_counter()
    s, t = seg.cpu().numpy(), target.cpu().numpy()
    t1 = time.perf_counter()
    tab = M.table(s, t)
    t2 = time.perf_counter()
    out = {"rand": M.adapted_rand_error(tab), "voi": M.variation_of_information(tab)}
    t3 = time.perf_counter()
    out["matching"] = M.matching(tab, 0.5)
    t4 = time.perf_counter()
    out["sbd"] = M.symmetric_best_dice(tab)[0]
    t5 = time.perf_counter()
    ms = [1e3 * (b - a) for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t4, t5), (t0, t5))]
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_metric.py needs the GPU: a CPU run gives no timing")
    import metric_ref as M
    lines = [f"instance-segmentation scores (csrc/overlap.hip); {args.reps} repetitions after {args.warmup} warm-up, device events",
             f"device: {torch.cuda.get_device_name(0)}"]
    classes = (("AdaptedRandError()", metric.AdaptedRandError()), ("VariationOfInformation()", metric.VariationOfInformation()),
               ("IOUError(0.5)", metric.IOUError(0.5)), ("SymmetricBestDice()", metric.SymmetricBestDice()))
    for size in args.sizes:
        h, markers, fg, n = BW.inputs(size)
        h2 = (0.7 * h + 0.3 * BW.smooth((size,) * 3, 1.5, 5)).contiguous()
        target = ops.seeded_watershed(h, markers, fg)
        seg = ops.seeded_watershed(h2, markers, fg)
        V = h.numel()
        ov = ops.label_overlaps(seg, target)
        s = ops.overlap_scores(ov, 0.5)
        sw = BW.measure(lambda: ops.seeded_watershed(h2, markers, fg), args.warmup, args.reps)
        so = BW.measure(lambda: ops.label_overlaps(seg, target), args.warmup, args.reps)
        sp = BW.measure(lambda: ops.pod_ids(seg, False, 0), args.warmup, args.reps)
        ss = BW.measure(lambda: ops.overlap_scores(ov, 0.5), args.warmup, args.reps)
        lines += [f"{size}^3 ({V} voxels, {n} markers; {int(s.n_pred[0])} seg and {int(s.n_true[0])} target objects, "
                  f"{int(ov.npairs[0])} distinct pairs, tp {int(s.tp[0])}):",
                  f"  ops.label_overlaps                    {BW.fmt(so)}   (two pod_ids, one key sort, flag, scan, table)",
                  f"  of that one ops.pod_ids               {BW.fmt(sp)}   (torch.sort + flag, scan, assign)",
                  f"  ops.overlap_scores                    {BW.fmt(ss)}"]
        for name, fn in classes:
            sc = BW.measure(lambda: fn(seg, target), args.warmup, args.reps)
            lines.append(f"  {name + '(seg, target)':<37} {BW.fmt(sc)}   (table + sums + expression)")
        for _ in range(2):
            want, _ = host_scores(seg[0], target[0], M)
        runs = [host_scores(seg[0], target[0], M)[1] for _ in range(5)]
        med = [sorted(r[k] for r in runs)[len(runs) // 2] for k in range(6)]
        got = {"rand": float(metric.AdaptedRandError()(seg, target)[0]), "voi": float(metric.VariationOfInformation()(seg, target)[0]),
               "sbd": float(metric.SymmetricBestDice()(seg, target)[0]), "tp": int(s.tp[0])}
        lines += [f"  numpy oracle, all four scores, host clock, median of 5: {med[5]:.1f} ms = copy to the host {med[0]:.1f} + table "
                  f"(np.unique of the pairs) {med[1]:.1f} + Rand and VoI {med[2]:.1f} + matching (linear_sum_assignment) {med[3]:.1f} + "
                  f"best Dice {med[4]:.1f}",
                  f"  device against oracle: Rand {got['rand'] == want['rand']}, tp {got['tp'] == want['matching']['tp']}, "
                  f"VoI differs by {abs(got['voi'] - want['voi']):.2e}, SBD by {abs(got['sbd'] - want['sbd']):.2e}"
                  f"  (Rand {got['rand']:.4f}, VoI {got['voi']:.4f}, SBD {got['sbd']:.4f})",
                  f"  for scale: ops.seeded_watershed of the same volume  {BW.fmt(sw)}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
