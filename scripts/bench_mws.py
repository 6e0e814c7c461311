"""Times the mutex watershed: `ops.mutex_watershed` on one 128^3 volume and one 1024^2 image, over the batch sizes of its
host loop; for scale the `predict_with_halo` time of the same 128^3 volume with the default `UNet3d`, and the oracle's
sequential Kruskal-with-mutexes on the CPU for 32^3.

    python scripts/bench_mws.py [--reps 7] [--warmup 2] [--out profiles/mws_bench.txt] [--stats-csv kernel_stats.csv]
    rocprofv3 --kernel-trace --stats -d DIR -o mws -- python scripts/bench_mws.py --one 128      # one call, for a trace

Inputs are synthetic: Voronoi cells of random points, the affinity of an edge 1 across two cells and 0 inside one (the
convention of AffinityTransform), blurred (sigma 1), plus uniform noise of 0.1; 3-D offsets -1 / -3 / -9 / -27 an axis
(3 attractive + 9 repulsive), 2-D offsets -1 an axis and nine of reach 3 / 9 / 27 (2 + 9); the repulsive edges subsampled
at random with strides of 2 an axis (`repulsive_edge_subsampling`, seed 0).  Device events around each call; median and
spread over the repetitions.  `--stats-csv`: the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of `--one`,
summed per kernel of csrc/mws.hip into shares.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.transform.defect import gaussian_weights  # noqa: E402
from torch_em_amd.util import mutex_watershed as S  # noqa: E402

DEV = "cuda:0"
OFFS3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-3, 0, 0], [0, -3, 0], [0, 0, -3], [-9, 0, 0], [0, -9, 0], [0, 0, -9],
         [-27, 0, 0], [0, -27, 0], [0, 0, -27]]
OFFS2 = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-9, 0], [0, -9], [-9, -9], [-9, 9], [-27, 0], [0, -27], [-27, -27]]
BATCHES = (1, 2, 4, 8, 16, 32, 64)


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


def inputs(shape, offsets, cells=None, seed=0):
    """-> affinities [1, C, D, H, W], edge_valid of the same shape, n_attractive, the number of cells"""
    nd = len(shape)
    g = torch.Generator(device=DEV).manual_seed(seed)
    cells = cells or max(int(np.prod(shape)) // 20000, 8)
    pts = torch.rand((cells, nd), generator=g, device=DEV) * torch.tensor(shape, device=DEV)
    grid = torch.stack(torch.meshgrid(*[torch.arange(s, device=DEV, dtype=torch.float32) for s in shape], indexing="ij"), -1)
    best = torch.full(shape, float("inf"), device=DEV)
    lab = torch.zeros(shape, dtype=torch.int32, device=DEV)
    for i in range(cells):
        d = ((grid - pts[i]) ** 2).sum(-1)
        lab = torch.where(d < best, i + 1, lab)
        best = torch.minimum(best, d)
    w = gaussian_weights(1.0, 4.0).astype(np.float32).tolist()
    aff = torch.zeros((len(offsets),) + tuple(shape), device=DEV)
    for c, o in enumerate(offsets):
        src = tuple(slice(max(-d, 0), s - max(d, 0)) for d, s in zip(o, shape))
        dst = tuple(slice(max(d, 0), s - max(-d, 0)) for d, s in zip(o, shape))
        aff[c][src] = (lab[src] != lab[dst]).float()
    s3 = (1,) * (3 - nd) + tuple(shape)
    aff = aff.reshape((len(offsets),) + s3)
    aff = ops.blur2d(aff, w, w) if nd == 2 else ops.blur3d(aff, w, w, w)
    aff = (aff + 0.1 * torch.rand(aff.shape, generator=g, device=DEV)).clamp_(0, 1)
    ev = S.repulsive_edge_subsampling(shape, len(offsets), nd, [2] * nd, True, seed=0)
    return aff[None].contiguous(), ev.reshape((1, len(offsets)) + s3).contiguous(), nd, cells


def kernel_shares(path):
    """a rocprofv3 kernel_stats CSV -> lines with the share of each csrc/mws.hip kernel in the time of all of them"""
    groups = {"k_mws_mutex": "mutex set", "k_mws_pick": "pick", "k_mws_veto": "veto", "k_mws_hook": "commit (hook)", "k_mws_flatten": "flatten",
              "k_mws_commit": "commit (comp, resets)", "k_mws_init": "init", "k_mws_clear": "init", "k_mws_batch": "batch begin / end",
              "k_mws_first": "labels", "k_mws_write": "labels"}
    tot, calls = {}, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            for k, gname in groups.items():
                if name.startswith(k):
                    tot[gname] = tot.get(gname, 0.0) + ns
                    calls[gname] = calls.get(gname, 0) + int(float(row.get("Calls") or 0))
    total = sum(tot.values()) or 1.0
    return [f"  {g:24s} {1e-6 * t:9.3f} ms  {100 * t / total:5.1f} %  ({calls[g]} launches)" for g, t in sorted(tot.items(), key=lambda kv: -kv[1])] \
        + [f"  all kernels of csrc/mws.hip {1e-6 * total:.3f} ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", type=int, default=0, help="one call on SIZE^3 and nothing else (for a profiler)")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mws.py needs the GPU: a CPU run gives no timing")
    if args.one:
        aff, ev, na, _ = inputs((args.one,) * 3, OFFS3)
        torch.cuda.synchronize()
        _, r = ops.mutex_watershed(aff, OFFS3, na, None, ev, return_rounds=True)
        torch.cuda.synchronize()
        print(f"{args.one}^3: {r} working rounds")
        return
    import mws_ref as M
    lines = [f"mutex watershed (csrc/mws.hip); {args.reps} repetitions after {args.warmup} warm-up, device events",
             f"device: {torch.cuda.get_device_name(0)}"]

    # the same answer as the oracle at a size its Python loops can still do
    aff, ev, na, cells = inputs((32,) * 3, OFFS3, cells=12)
    got, r = ops.mutex_watershed(aff, OFFS3, na, None, ev, return_rounds=True)
    t0 = time.perf_counter()
    want = M.sequential(aff[0, :, :, :, :].cpu().numpy(), OFFS3, na, None, ev[0].cpu().numpy())
    t_seq = time.perf_counter() - t0
    st = measure(lambda: ops.mutex_watershed(aff, OFFS3, na, None, ev), args.warmup, args.reps)
    lines += [f"32^3, {cells} cells: device result == sequential oracle: {bool(np.array_equal(got[0].cpu().numpy(), want))}; "
              f"{int(want.max())} segments, {r} working rounds",
              f"  the oracle, sequential Kruskal with mutex sets in Python, 32^3 on the CPU: {t_seq:.2f} s; the device: {fmt(st)}"]

    # what one read-back costs when nothing is queued in front of it: the floor of a batch
    probe = torch.zeros(8, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    t = []
    for _ in range(200):
        t0 = time.perf_counter()
        probe.view(torch.int32).tolist()
        t.append((time.perf_counter() - t0) * 1e3)
    lines += [f"read-back of two ints from an idle stream, host clock: {fmt(stats(t))}"]

    for shape, offs in (((128,) * 3, OFFS3), ((1024, 1024), OFFS2)):
        aff, ev, na, cells = inputs(shape, offs)
        seg, r = ops.mutex_watershed(aff, offs, na, None, ev, return_rounds=True)
        name = "x".join(str(s) for s in shape)
        n_edges, n_rep = int(ev.sum()), int(ev[:, na:].sum())
        lines += [f"{name} ({aff[0, 0].numel()} voxels, {len(offs)} channels, {cells} cells; about {n_edges} edges, {n_rep} of them "
                  f"repulsive, before the border is taken off; mutex set of {ops.mws_table_slots(n_rep)} slots): "
                  f"{int(seg.max())} segments, {r} working rounds"]
        res = {}
        for per in BATCHES:
            st = measure(lambda: ops.mutex_watershed(aff, offs, na, None, ev, rounds_per_batch=per), args.warmup, args.reps)
            nb = r // per + 1
            res[per] = (st["median"], nb)
            lines += [f"  rounds_per_batch {per:2d}: {fmt(st)}   {nb} batches, {nb * per} rounds enqueued for {r} working"]
        (t1, b1), (t64, b64) = res[1], res[64]
        lines += [f"  per batch, from 1 against 64 rounds a batch: ({t1:.3f} - {t64:.3f}) ms / ({b1} - {b64}) batches = "
                  f"{1e3 * (t1 - t64) / max(b1 - b64, 1):.1f} us; per working round at 64 a batch: {1e3 * t64 / max(r, 1):.1f} us"]
        if len(shape) == 3:
            fg = torch.ones(shape, device=DEV)

            def end_to_end():
                return S.mutex_watershed_segmentation(fg, aff[0, :, :, :, :], offs, min_size=50, seed=0)
            se = measure(end_to_end, 1, 3)
            lines += [f"  mutex_watershed_segmentation end to end (min_size 50, strides 2, seed 0; {int(end_to_end().max())} segments)  {fmt(se)}"]
            from torch_em_amd.model import UNet3d
            from torch_em_amd.util import predict_with_halo
            model_ = UNet3d(1, 3, final_activation="Sigmoid").to(DEV).eval()
            vol = np.random.RandomState(0).rand(*shape).astype(np.float32)

            def predict():
                predict_with_halo(vol, model_, [0], (64, 64, 64), (16, 16, 16), disable_tqdm=True)
            for _ in range(2):
                predict()
            tp = []
            for _ in range(5):
                t0 = time.perf_counter()
                predict()
                tp.append((time.perf_counter() - t0) * 1e3)
            lines += [f"  for scale: predict_with_halo of the same volume, default UNet3d(1, 3), blocks 64^3 + halo 16, host clock around "
                      f"the call (it ends in a synchronise and the copy to the host)  {fmt(stats(tp))}"]
    if args.stats_csv:
        lines += [f"kernel shares of one 128^3 call (rocprofv3 --kernel-trace --stats, a run of its own: {os.path.basename(args.stats_csv)}):"]
        lines += kernel_shares(args.stats_csv)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
