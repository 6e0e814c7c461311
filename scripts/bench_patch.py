"""Times patch supply from a device-resident volume against the host TensorDataset with the same sampler.

    python scripts/bench_patch.py [--reps 10] [--warmup 2] [--inner 5] [--batches 40] [--host-batches 24] [--out profiles/patch_bench.txt]

Workload: batches of 2 x 128^3 patches from one 256^3 volume (uint8 raw, int32 labels: 32^3 blocks with their own ids in the
x >= 96 part, background before it, so that crops differ in foreground, instances and brightness).  Per sampler:
  * the ops on 16 candidate boxes (one round of 2 samples x 8 candidates): device events around windows of `inner` calls;
    bytes are what the boxes hold, the rate is bytes over the median;
  * the batch gather (raw -> float32, labels -> int64);
  * supply per batch through DevicePatchLoader: host clock around `loader.batch(k)`, which ends in a synchronise -- draws,
    table uploads, launches, the read-back of each round and the gather;
  * the host path: TensorDataset with the same sampler in a DataLoader with 16 workers, host clock per batch after a warm-up
    that has every worker started.
The figure to hold against: one training step of the benchmark network takes 7.75 ms in the fp16 mixed mode (BENCH_r06).
Without a GPU it fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_selftrain import alternate, fmt, stats  # noqa: E402
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.data import (DevicePatchLoader, DeviceSegmentationDataset, MinForegroundSampler, MinInstanceSampler,  # noqa: E402
                               MinIntensitySampler, MinTwoInstanceSampler, TensorDataset)

S, P, STEP_MS = 256, 128, 7.75
SAMPLERS = [("none", None),
            ("MinForegroundSampler(0.5)", MinForegroundSampler(0.5)),
            ("MinTwoInstanceSampler()", MinTwoInstanceSampler()),
            ("MinInstanceSampler(40, min_size=1000)", MinInstanceSampler(min_num_instances=40, min_size=1000)),
            ("MinIntensitySampler(100, 'median')", MinIntensitySampler(100, "median"))]


def make_volume():
    blk = np.arange(S) // (S // 8)   # 8 blocks per axis: 32^3 voxels each at S = 256
    z, y, x = np.meshgrid(blk, blk, blk, indexing="ij", sparse=True)
    labels = (1 + z * 64 + y * 8 + x).astype(np.int32) * (np.arange(S) >= 3 * S // 8)[None, None, :]
    rs = np.random.RandomState(0)
    raw = (rs.randint(0, 100, labels.shape) + 100 * (labels > 0)).astype(np.uint8)
    return raw, np.ascontiguousarray(labels, dtype=np.int32)


def host_clock(fn, n, warmup):
    for k in range(warmup):
        fn(k)
    times = []
    for k in range(warmup, warmup + n):
        t0 = time.perf_counter()
        fn(k)
        times.append((time.perf_counter() - t0) * 1e3)
    return stats(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--host-batches", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_patch.py needs the GPU: a CPU run gives no timing")
    dev = "cuda:0"
    raw, labels = make_volume()
    lines = [f"patch supply benchmark; batches of 2 x {P}^3 from one {S}^3 volume (uint8 raw, int32 labels); ops: {args.reps} repetitions after "
             f"{args.warmup} warm-up, windows of {args.inner} calls, device events, alternating; loaders: host clock per batch",
             f"device: {torch.cuda.get_device_name(0)}; the step to fit into: {STEP_MS} ms (fp16 mixed mode, BENCH_r06)"]
    rs = np.random.RandomState(1)
    cand = np.array([[0, *rs.randint(0, S - P, 3), P, P, P] for _ in range(16)])
    vox = 16 * P ** 3
    for name, sampler in SAMPLERS:
        ds = DeviceSegmentationDataset(raw, labels, (P, P, P), sampler=sampler, n_samples=2 * (args.batches + 8), device=dev)
        lines.append(f"{name}:")
        rows = []
        crit = ds.criterion
        if crit is not None and crit.kind.startswith("count"):
            rows.append(("patch_count, 16 boxes", lambda: ops.patch_count(ds.labels, cand, 0), vox * 4))
        elif crit is not None and crit.needs_histogram:
            rows.append((f"patch_hist (n_ids {ds.n_ids}, path {ops.patch_hist_path(ds.n_ids)}) + reduce, 16 boxes",
                         lambda: ops.patch_hist_instances(ops.patch_hist(ds._ids, cand, ds.n_ids), ds._sel, crit.min_size), vox * 4))
        elif crit is not None:
            rows.append(("patch_gather raw -> float32 rows, 16 boxes", lambda: ops.patch_gather(ds.raw, cand, (P, P, P)), vox * 5))
            x = ops.patch_gather(ds.raw, cand, (P, P, P)).view(16, -1)
            L = x.shape[1]
            rows.append(("row_order_statistics (2 ranks), 16 rows", lambda: ops.row_order_statistics(x, [(L - 1) // 2, L // 2]), None))
        rows.append(("batch gather: raw -> float32 and labels -> int64, 2 boxes",
                     lambda: (ops.patch_gather(ds.raw, cand[:2], (P, P, P)), ops.patch_gather(ds.labels, cand[:2], (P, P, P), torch.int64)),
                     2 * P ** 3 * (1 + 4 + 4 + 8)))
        for (label, _, nbytes), st in zip(rows, alternate([r[1] for r in rows], args.reps, args.warmup, inner=args.inner)):
            rate = "" if nbytes is None else f"  {nbytes / 1e6:.0f} MB -> {nbytes / (st['median'] * 1e-3) / 1e12:.2f} TB/s"
            lines.append(f"  {label:<66} {fmt(st)}{rate}")
        loader = DevicePatchLoader(ds, 2, seed=0, candidates_per_round=8)
        attempts = []

        def supply(k):
            loader.batch(k)
            attempts.extend(len(c.starts) for c in loader.last_candidates)
        st = host_clock(supply, args.batches, 4)
        lines.append(f"  {'DevicePatchLoader, supply per batch (8 candidates per round)':<66} {fmt(st)}  = {st['median'] / STEP_MS * 100:.0f} % of the step; "
                     f"{np.mean(attempts):.1f} attempts per sample")
        hds = TensorDataset([raw], [labels], (P, P, P), sampler=sampler, n_samples=2 * (args.host_batches + 40), label_dtype=torch.int64)
        it = iter(torch.utils.data.DataLoader(hds, batch_size=2, num_workers=16, multiprocessing_context="spawn"))  # workers never open the GPU
        hs = host_clock(lambda k: next(it), args.host_batches, 32)
        del it
        lines.append(f"  {'host TensorDataset, 16 loader workers, per batch (before the H2D copy)':<66} {fmt(hs)}  = {hs['median'] / STEP_MS * 100:.0f} % of "
                     f"the step; {hs['median'] / st['median']:.1f} x the device loader")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
