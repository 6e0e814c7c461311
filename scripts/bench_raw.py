"""Times the raw normalisations of the device input pipeline on a cfg-2 batch (2 x 1 x 128^3 float32, per sample):
`normalize`, `normalize_percentile` (1 / 99) and `standardize`, on uniform [0, 1) data and on 0..255 data stored as float
(constant top byte of the radix key: the contended case of the select's first pass).

    python scripts/bench_raw.py [--size 128] [--reps 50] [--warmup 10] [--out profiles/raw_normalize_bench.txt]

Device events around each call, the ops alternating, median and spread over the repetitions.  Per op: the bytes its passes
move (a model computed from the shapes: 4 B per element per read or write pass) over a device-to-device copy rate measured
in the same run, as the floor -- at the batch's own size (16.8 MB: it sits in the 256 MiB L3) and at 1 GiB (HBM).  Also the
reference's `normalize_percentile` (numpy, one sample) on this host's CPU, the ratio to `standardize`, the slow-down of
0..255 data over uniform data and a same-input agreement check against the numpy branch.
There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.transform import normalize, normalize_percentile, standardize  # noqa: E402

# read + write passes over the batch: (reads, writes)
PASSES = {"normalize": (2, 1), "normalize_percentile": (5, 1), "standardize": (2, 1), "select (4 ranks)": (4, 0)}


def stats(ms):
    s = sorted(ms)
    n = len(s)
    return {"median": s[n // 2], "min": s[0], "max": s[-1], "iqr": s[(3 * n) // 4] - s[n // 4]}


def fmt(st):
    return f"median {st['median'] * 1e3:8.1f} us (min {st['min'] * 1e3:.1f}, max {st['max'] * 1e3:.1f}, iqr {st['iqr'] * 1e3:.1f})"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def copy_rate(nbytes, reps):
    """bytes read + written per second of a device-to-device copy of `nbytes`"""
    a = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda:0").normal_()
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    ms = stats([timed(lambda: b.copy_(a)) for _ in range(reps)])["median"]
    return 2.0 * nbytes / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_raw.py needs the GPU: a CPU run gives no timing")
    dev, S = "cuda:0", args.size
    rng = np.random.RandomState(0)
    data = {"uniform [0,1)": rng.rand(2, 1, S, S, S).astype("float32"),
            "0..255 as float": rng.randint(0, 256, size=(2, 1, S, S, S)).astype("float32")}
    nbytes = 2 * S ** 3 * 4
    rate_l3, rate_hbm = copy_rate(nbytes, args.reps), copy_rate(1 << 30, 10)
    lines = [f"raw normalisation of a batch 2x1x{S}^3 float32 ({nbytes / 1e6:.1f} MB), per sample; {args.reps} repetitions after "
             f"{args.warmup} warm-up, device events, ops alternating", f"device: {torch.cuda.get_device_name(0)}, numpy {np.__version__}",
             f"device-to-device copy, read + written bytes per second: {rate_l3 / 1e12:.2f} TB/s at {nbytes / 1e6:.1f} MB (L3-resident), "
             f"{rate_hbm / 1e12:.2f} TB/s at 1 GiB (HBM; DESIGN.md 6.R5 measured 6.57 TB/s for a dense read)",
             "floor of an op = the bytes of its pass model / the L3-resident copy rate (the batch fits the 256 MiB L3, so that is the "
             "rate a pass over it can reach); 'x the floor' below is against that one, the HBM figure is for reference"]
    medians = {}
    for label, x in data.items():
        xd = torch.from_numpy(x).to(dev)
        L = xd[0].numel()
        ranks = [list(ops.percentile_plan(L, 1.0)[:2]) + list(ops.percentile_plan(L, 99.0)[:2])] * 2
        fns = {"normalize": lambda: normalize(xd, per_sample=True),
               "normalize_percentile": lambda: normalize_percentile(xd, 1.0, 99.0, per_sample=True),
               "standardize": lambda: standardize(xd, per_sample=True),
               "select (4 ranks)": lambda: ops.row_order_statistics(xd.reshape(2, -1), ranks)}
        # same input, same result as the numpy branch (the CPU oracle)
        agree = {k: bool(np.array_equal(fns[k]().cpu().numpy(), f(x, per_sample=True)))
                 for k, f in (("normalize", normalize), ("normalize_percentile", normalize_percentile))}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        lines.append(f"{label}: device result bit-equal to the numpy branch: {agree}")
        for k in fns:
            st = stats(ms[k])
            medians[label, k] = st["median"]
            rd, wr = PASSES[k]
            moved = (rd + wr) * nbytes
            lines.append(f"  {k:22s} {fmt(st)}; model {rd} read + {wr} write passes = {moved / 1e6:.0f} MB -> floor "
                         f"{moved / rate_l3 * 1e6:.1f} us at the L3 copy rate ({moved / rate_hbm * 1e6:.1f} us at the HBM rate), "
                         f"{st['median'] * 1e-3 / (moved / rate_l3):.1f}x the floor")
        lines.append(f"  normalize_percentile / standardize: {medians[label, 'normalize_percentile'] / medians[label, 'standardize']:.2f}x "
                     f"(by pass count (4 + 1 + 1) / (2 + 1) = 2x expected)")
    u, b = "uniform [0,1)", "0..255 as float"
    for k in ("normalize_percentile", "select (4 ranks)"):
        lines.append(f"slow-down of 0..255 data over uniform data, {k}: {medians[b, k] / medians[u, k]:.2f}x")
    x1 = data[u][0]
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        normalize_percentile(x1, 1.0, 99.0)
        t.append(time.perf_counter() - t0)
    cpu_ms = sorted(t)[1] * 1e3
    lines.append(f"CPU reference (numpy branch = the reference's expression, one {S}^3 sample, this host): {cpu_ms:.1f} ms, "
                 f"{2 * cpu_ms:.1f} ms per batch; device batch {medians[u, 'normalize_percentile']:.3f} ms = "
                 f"{2 * cpu_ms / medians[u, 'normalize_percentile']:.0f}x faster")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
