"""Times the seeded watershed: `ops.seeded_watershed` on one 128^3 and one 256^3 volume, and
`watershed_from_center_and_boundary_distances` end to end on 128^3; for scale the `predict_with_halo` time of the same 128^3
volume with the default `UNet3d` (1 -> 3 channels), and the oracle's sequential priority flood on the CPU for 64^3.

    python scripts/bench_watershed.py [--reps 10] [--warmup 3] [--out profiles/watershed_bench.txt]

Inputs are synthetic: smoothed noise as heights, a smoothed-noise foreground, and about 200 markers: the components of the
lowest heights (the quantile is searched until the count is near 200).  Device events around each call; median and spread
(min, max, inter-quartile range) over the repetitions.  Also: the rounds that did work, the bytes the kernels move per voxel
and round (the model is written out below) with the HBM time they imply, and a check of a 64^3 result against the oracle's
Kruskal.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
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
from torch_em_amd.util import segmentation as S  # noqa: E402

DEV = "cuda:0"
# Bytes per voxel of one working round with ONE flatten pass (csrc/watershed.hip), counting each array once per kernel
# (neighbour reads hit lines the kernel streams anyway; the gathers at roots are counted as one read):
#   pick     comp 4 + rank 4 + lab[root] 4                       = 12   (+ one 8-byte atomic per component border voxel)
#   hook     comp 4 + lab 4 (roots) + nxt 4 written              = 12
#   flatten  nxt 4 + nxt[parent] 4 + nxt 4 written               = 12   (a further pass: + 12)
#   commit   comp 4 + nxt 4 + comp 4 written                     = 12
# and once per call: init (markers 8, mask 1, comp / lab / best 16 written) 25 + write (comp 4, lab 4, out 4) 12
ROUND_BYTES, CALL_BYTES = 48.0, 37.0
HBM_RATE = 6.3e12   # the achievable copy rate of the MI355X (8 TB/s peak)


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


def smooth(shape, sigma, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = gaussian_weights(sigma, 4.0).astype(np.float32).tolist()
    x = ops.blur3d(torch.rand((1,) + shape, generator=g, device=DEV), w, w, w)
    return (x - x.amin()) / (x.amax() - x.amin())


def inputs(size, seed=0, want=200):
    """-> heights, markers (about `want` components of the lowest heights), foreground mask, all [1, S, S, S]"""
    shape = (size,) * 3
    h = smooth(shape, 1.5, seed)
    fg = smooth(shape, 3.0, seed + 1) > 0.4
    lo, hi, best = 0.0, 0.5, None
    for _ in range(14):                     # bisect the quantile: more of the volume below it, more components (up to merging)
        q = 0.5 * (lo + hi)
        thr = torch.quantile(h.flatten()[:: max(h.numel() // 1000000, 1)], q)
        ids = ops.pod_ids(((h < thr) & fg).to(torch.int64), True, 0)
        n = int(ids.max())
        if best is None or abs(n - want) < abs(best[0] - want):
            best = (n, ids)
        if n < want:
            lo = q
        else:
            hi = q
    return h.contiguous(), best[1], fg, best[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_watershed.py needs the GPU: a CPU run gives no timing")
    import watershed_ref as R
    lines = [f"seeded watershed (csrc/watershed.hip); {args.reps} repetitions after {args.warmup} warm-up, device events",
             f"device: {torch.cuda.get_device_name(0)}"]

    # the same answer as the oracle at a size its Python loops can still do
    h, markers, fg, n = inputs(64)
    got = ops.seeded_watershed(h, markers, fg)[0].cpu().numpy()
    t0 = time.perf_counter()
    want = R.kruskal(h[0].cpu().numpy(), markers[0].cpu().numpy(), fg[0].cpu().numpy())
    t_k = time.perf_counter() - t0
    t0 = time.perf_counter()
    flood = R.flood(h[0].cpu().numpy(), markers[0].cpu().numpy(), fg[0].cpu().numpy())
    t_f = time.perf_counter() - t0
    m = fg[0].cpu().numpy()
    lines += [f"64^3, {n} markers: device result == oracle Kruskal: {bool(np.array_equal(got, want))}; agreement of the forest with "
              f"the priority flood on the masked voxels {float((want == flood)[m].mean()):.4f}",
              f"  oracle (c), the sequential priority flood in Python (heapq), 64^3 on the CPU: {t_f:.2f} s (Kruskal (a): {t_k:.2f} s)"]

    for size in args.sizes:
        h, markers, fg, n = inputs(size)
        V = h.numel()
        rounds = torch.zeros(1, dtype=torch.int32, device=DEV)
        st = measure(lambda: ops.seeded_watershed(h, markers, fg, rounds), args.warmup, args.reps)
        sr = measure(lambda: ops.voxel_ranks(h), args.warmup, args.reps)
        r = int(rounds.item())
        kern = st["median"] - sr["median"]
        model = (ROUND_BYTES * r + CALL_BYTES) * V
        lines += [f"{size}^3 ({V} voxels, {n} markers, {100.0 * float(fg.float().mean()):.0f} % inside the mask):",
                  f"  ops.seeded_watershed          {fmt(st)}",
                  f"  of that ops.voxel_ranks       {fmt(sr)}   (torch.sort + scatter)",
                  f"  rounds that did work {r} of {ops.watershed_rounds(V)} enqueued",
                  f"  traffic model {ROUND_BYTES:.0f} B/voxel/round x {r} rounds + {CALL_BYTES:.0f} B/voxel = {model / 1e6:.0f} MB -> "
                  f"{model / HBM_RATE * 1e3:.3f} ms at {HBM_RATE / 1e12:.1f} TB/s; the kernels (call minus ranks) take {kern:.3f} ms = "
                  f"{model / (kern * 1e-3) / 1e12:.2f} TB/s of the model"]
        if size == 128:
            # three prediction-like maps; thresholds at the maps' own 30 % quantiles, so that seeds exist whatever the noise
            cd, bd = smooth((size,) * 3, 2.0, 7), h
            fgmap = smooth((size,) * 3, 3.0, 1)
            tc, tb = (float(torch.quantile(m.flatten()[::2], 0.3)) for m in (cd, bd))

            def end_to_end():
                return S.watershed_from_center_and_boundary_distances(cd[0], bd[0], fgmap[0], tc, tb, 0.4, min_size=50)
            se = measure(end_to_end, args.warmup, args.reps)
            lines += [f"  watershed_from_center_and_boundary_distances end to end (smoothing 1.6, thresholds {tc:.3f} / {tb:.3f} / 0.4, "
                      f"min_size 50; {int(end_to_end().max())} segments)  {fmt(se)}"]
            from torch_em_amd.model import UNet3d
            from torch_em_amd.util import predict_with_halo
            model_ = UNet3d(1, 3, final_activation="Sigmoid").to(DEV).eval()
            vol = np.random.RandomState(0).rand(size, size, size).astype(np.float32)

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
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
