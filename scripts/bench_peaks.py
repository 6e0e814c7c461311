"""Times peak_local_max on the device: `ops.peak_local_max` / `ops.peak_markers` on one 128^3 volume and one 1 x 1024^2
image at min_distance 3, 10 and 31, the rounds and batches of the spacing pass, the bytes each pass must move against the
HBM peak bench.py uses (8 TB/s), and -- the yardstick -- the same peak mask from a torch composition on the device
(`max_pool3d` with stride 1 on a replicate-padded copy, then `==`).

    python scripts/bench_peaks.py [--reps 7] [--warmup 2] [--out profiles/peaks_bench.txt] [--trace-csv kernel_trace.csv]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o peaks -- python scripts/bench_peaks.py --trace   # one call per case

Inputs are synthetic: uniform noise blurred with sigma 2 (a smoothed distance map has this look: few exact ties), and the
same map quantised to 16 levels (plateaus, so that the spacing pass has work).  Device events around each call; median and
spread over the repetitions.  `--trace-csv`: the kernel trace of a `--trace` run, cut into the cases at every `k_pk_init`
and summed per kernel of csrc/peaks.hip.  The box maximum of the yardstick over the full (2d + 1)^3 cube is only run where
it has at most 4096 taps; beyond that the composition is three 1-D poolings.  There is no CPU fallback: without a GPU the
script fails.
"""
import argparse
import csv
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.transform.defect import gaussian_weights  # noqa: E402

DEV = "cuda:0"
PEAK_HBM_TBS = 8.0
SHAPES = ((128, 128, 128), (1, 1024, 1024))
DISTANCES = (3, 10, 31)
KERNELS = ("k_pk_init", "k_pk_minmax", "k_pk_zmax", "k_pk_xy", "k_pk_batch", "k_pk_round", "k_pk_count", "k_pk_compact", "k_pk_zero",
           "k_pk_seeds")


def stats(ms):
    s = sorted(ms)
    n = len(s)
    return {"median": s[n // 2], "min": s[0], "max": s[-1], "iqr": s[(3 * n) // 4] - s[n // 4]}


def fmt(st):
    return f"median {st['median']:.3f} ms (min {st['min']:.3f}, max {st['max']:.3f}, iqr {st['iqr']:.3f})"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return stats([timed(fn) for _ in range(reps)])


def inputs(shape, seed=0):
    """-> (smooth, quantised): float32 [1, D, H, W]"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.rand((1,) + tuple(shape), generator=g, device=DEV)
    w = gaussian_weights(2.0, 4.0).astype("float32").tolist()
    x = ops.blur2d(x, w, w) if shape[0] == 1 else ops.blur3d(x, w, w, w)
    x = (x - x.min()) / (x.max() - x.min())
    return x.contiguous(), torch.floor(x * 16).clamp_(0, 15).contiguous()


def torch_mask(x, d, separable):
    """the peak mask image == maximum_filter(image, 2d + 1, mode="nearest") by torch ops; x: [1, D, H, W]"""
    D = x.shape[1]
    pz = d if D > 1 else 0
    p = F.pad(x[None], (d, d, d, d, pz, pz), mode="replicate")
    k = (2 * pz + 1, 2 * d + 1, 2 * d + 1)
    if separable:
        for ax in range(3):
            p = F.max_pool3d(p, tuple(k[a] if a == ax else 1 for a in range(3)), stride=1)
    else:
        p = F.max_pool3d(p, k, stride=1)
    return p[0] == x


def pass_bytes(shape):
    """the bytes each pass must move for one sample: name -> bytes"""
    V = shape[0] * shape[1] * shape[2]
    b = {"k_pk_minmax (read the image)": 4 * V}
    if shape[0] > 1:
        b["k_pk_zmax (read the image, write its z maximum)"] = 8 * V
        b["k_pk_xy (read the z maximum and the image, write the states)"] = 9 * V
    else:
        b["k_pk_xy (read the image, write the states)"] = 5 * V
    b["k_pk_round, each (read the states)"] = V
    b["k_pk_count, k_pk_compact, each (read the states)"] = V
    b["k_pk_zero (write the markers)"] = 4 * V
    return b


def trace_tables(path, names):
    """a rocprofv3 kernel trace CSV -> per case (cut at every k_pk_init, the warm-up case dropped) the time per kernel"""
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("KernelName") or row.get("Name") or ""
            t0, t1 = float(row.get("Start_Timestamp") or 0), float(row.get("End_Timestamp") or 0)
            k = next((k for k in KERNELS if k in name), None)
            if k:
                rows.append((t0, k, t1 - t0))
    rows.sort()
    cases, cur = [], None
    for _, k, ns in rows:
        if k == "k_pk_init":
            cur = {}
            cases.append(cur)
        if cur is not None:
            n, t = cur.get(k, (0, 0.0))
            cur[k] = (n + 1, t + ns)
    lines = []
    for name, case in zip(names, cases[1:]):
        total = sum(t for _, t in case.values())
        lines.append(f"  {name}: all kernels of csrc/peaks.hip {1e-3 * total:.1f} us")
        lines += [f"    {k:14s} {1e-3 * t:9.1f} us  ({n} launches)" for k, (n, t) in case.items()]
    if len(cases) != len(names) + 1:
        lines.append(f"  (the trace holds {len(cases)} calls, {len(names) + 1} expected)")
    return lines


def case_names():
    return [f"{'x'.join(str(s) for s in shape)} {kind} d={d} ({fn})" for shape in SHAPES for kind in ("smooth", "16 levels")
            for d in DISTANCES for fn in (("peak_markers",) if kind == "smooth" else ("peak_local_max",))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", action="store_true", help="one call per case and nothing else (for a profiler)")
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_peaks.py needs the GPU: a CPU run gives no timing")
    if args.trace:
        ops.peak_markers(torch.rand(1, 4, 70, 70, device=DEV), 2)        # loads the code objects; the first k_pk_init of the trace
        for shape in SHAPES:
            smooth, quant = inputs(shape)
            for d in DISTANCES:
                ops.peak_markers(smooth, d, exclude_border=False)
            for d in DISTANCES:
                ops.peak_local_max(quant, d, exclude_border=False)
        torch.cuda.synchronize()
        return
    lines = [f"peak_local_max on the device (csrc/peaks.hip); {args.reps} repetitions after {args.warmup} warm-up, device events",
             f"device: {torch.cuda.get_device_name(0)}"]
    for shape in SHAPES:
        smooth, quant = inputs(shape)
        V = smooth.numel()
        name = "x".join(str(s) for s in shape)
        lines += [f"{name} ({V} voxels); the bytes each pass must move, and their time at the {PEAK_HBM_TBS:.0f} TB/s HBM peak:"]
        lines += [f"    {k}: {b / 1e6:.2f} MB = {b / (PEAK_HBM_TBS * 1e6):.2f} us" for k, b in pass_bytes(shape).items()]
        for d in DISTANCES:
            for kind, x in (("smooth", smooth), ("16 levels", quant)):
                peaks, rounds = ops.peak_local_max(x, d, exclude_border=False, return_rounds=True)
                batches = -(-rounds // ops.PEAKS_ROUNDS_PER_BATCH)
                mk = ops.peak_markers(x, d, exclude_border=False)
                yard = {sep: torch_mask(x, d, sep) for sep in (True, False) if sep or (2 * d + 1) ** (3 if shape[0] > 1 else 2) <= 4096}
                # the yardstick computes the candidates before the threshold, the constant rule and the spacing pass
                same = all(bool(((mk > 0) & ~m).sum() == 0) for m in yard.values()) and bool(torch.equal(*yard.values()) if len(yard) == 2 else True)
                lines += [f"  d={d:2d} {kind:9s}: {len(peaks[0])} peaks, {rounds} rounds in {batches} batch(es) of {ops.PEAKS_ROUNDS_PER_BATCH}; "
                          f"{int(yard[True].sum())} voxels equal their box maximum; every peak among them: {same}"]
                lines += [f"    peak_local_max  {fmt(measure(lambda: ops.peak_local_max(x, d, exclude_border=False), args.warmup, args.reps))}",
                          f"    peak_markers    {fmt(measure(lambda: ops.peak_markers(x, d, exclude_border=False), args.warmup, args.reps))}"]
                if kind == "smooth":
                    for sep, label in ((True, "three 1-D max_pool3d"), (False, "one box max_pool3d")):
                        if sep in yard:
                            lines += [f"    torch, {label:21s} + ==  {fmt(measure(lambda: torch_mask(x, d, sep), args.warmup, args.reps))}"]
    if args.trace_csv:
        lines += [f"kernel times of one call per case (rocprofv3 --kernel-trace, a run of its own: {os.path.basename(args.trace_csv)}):"]
        lines += trace_tables(args.trace_csv, case_names())
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
