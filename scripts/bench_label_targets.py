"""Times the label transforms that ride on csrc/distance.hip and csrc/label.hip on int64 label batches 2x1x128^3 and
2x1x1024^2 on the device: `DistanceTransform` (three channel settings), `connected_components`, `label_consecutive`,
`MinSizeLabelTransform`, `OneHotTransform`, `NoToBackgroundBoundaryTransform`, `BoundaryTransformWithIgnoreLabel`.

    python scripts/bench_label_targets.py [--reps 10] [--warmup 3] [--out profiles/label_targets_bench.txt]

Per transform: device events around the call, median over the repetitions.  Per kernel of the new ones: the time from one
torch.profiler capture of every transform, and the rate from the bytes the kernel must move (a model from the shapes,
BYTES below).  For `DistanceTransform` the same box's CPU time of the reference's recipe stands next to it:
scipy.ndimage.distance_transform_edt(return_indices=True) plus the numpy post-processing, the samples of the batch spread
over a pool of 16 threads (scipy's transform itself is single-threaded, so a batch of 2 keeps 2 of them busy).
Labels: thresholded smoothed noise, its connected components as instance ids.  There is no CPU fallback: without a GPU the
script fails.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_em_amd.transform import (BoundaryTransformWithIgnoreLabel, DistanceTransform, MinSizeLabelTransform,  # noqa: E402
                                    NoToBackgroundBoundaryTransform, OneHotTransform, connected_components,
                                    label_consecutive)

# bytes per voxel a kernel must move (reads + writes); k_vdt_pass by axis (x reads the int64 labels and writes three offsets
# and the value; y and z read the value and the carried offsets and write them back plus their own)
VDT_BYTES = {2: 8 + 16, 1: 8 + 12, 0: 12 + 16}


def blobs(shape, seed, sigma):
    rng = np.random.default_rng(seed)
    img = ndimage.gaussian_filter(rng.standard_normal(shape).astype("float32"), sigma)
    return img > np.quantile(img, 0.6)


def cpu_distance_transform(lab, directed):
    """the reference's DistanceTransform(distances=True, directed_distances=directed) on one sample, scipy for the EDT"""
    mask = lab == 1
    idx = ndimage.distance_transform_edt(~mask, return_indices=True, return_distances=False)
    vec = (idx - np.indices(lab.shape)).astype("float64")
    d = np.linalg.norm(vec, axis=0)
    d /= d.max() + 1e-7
    if not directed:
        return d
    vec /= np.abs(vec).max(axis=(1, 2), keepdims=True) + 1e-7
    return np.concatenate((d[None], vec), axis=0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_table(fns, NV, ndim, lines):
    """one profiler capture of every transform; new kernels get bytes and a rate"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    except Exception as exc:   # no profiler on this build: the transform-level times above stand alone
        lines.append(f"  per-kernel table unavailable: torch.profiler failed ({type(exc).__name__}: {exc})")
        return
    evs.sort(key=lambda e: e.time_range.start)
    rows, seen = {}, {}
    for e in evs:
        name = e.name.split("(")[0]
        us = e.time_range.end - e.time_range.start
        nbytes = None
        nth = seen[name] = seen.get(name, -1) + 1   # the capture runs the transforms in the order of `fns`
        if name == "k_vdt_pass":
            axis = (2, 1, 0)[nth % ndim]
            name, nbytes = f"k_vdt_pass axis {axis}", VDT_BYTES[axis] * NV
        elif name == "k_dt_write":     # d2 (and the offsets) read, the float channels written
            directed = nth % 3 > 0
            name = f"k_dt_write {1 + ndim if directed else 1} ch"
            nbytes = ((16 + 4 * (1 + ndim)) if directed else 8) * NV
        elif name == "k_boundary_masked":   # the label read once (neighbours from cache), int8 channels written
            name, nbytes = (("k_boundary_masked thick+bin", 10 * NV), ("k_boundary_masked outer", 9 * NV))[nth % 2]
        elif name == "k_dt_max":       # three offsets and the squared distance read
            nbytes = 16 * NV
        elif name == "k_onehot":       # the label read, four float channels written
            nbytes = (8 + 16) * NV
        if not name.startswith(("k_", "void k_")):
            continue
        r = rows.setdefault(name, [0, 0.0, nbytes])
        r[0] += 1
        r[1] += us
    lines.append(f"  {'kernel':28s} {'calls':>5s} {'avg [us]':>10s} {'GB/s':>8s}   (one capture of every transform above)")
    for name, (n, us, nbytes) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        rate = f"{nbytes / (us / n * 1e-6) / 1e9:8.0f}" if nbytes else "        "
        lines.append(f"  {name:28s} {n:5d} {us / n:10.1f} {rate}")


def bench(shape, sigma, args, lines):
    N, ndim = 2, len(shape)
    masks = [blobs(shape, s, sigma) for s in range(N)]
    binary = np.stack(masks).astype("int64")[:, None]
    inst = np.stack([ndimage.label(m)[0] for m in masks]).astype("int64")[:, None]
    NV = binary.size
    dev = "cuda:0"
    yb, yi = torch.from_numpy(binary).to(dev), torch.from_numpy(inst).to(dev)
    ym = yi.clone()
    ym[yi % 11 == 3] = -1
    y4 = yi % 4
    # (callable, bytes of the transform's own streaming kernel: label read + output written, None where several kernels share)
    fns = {
        "DistanceTransform()": lambda: DistanceTransform()(yb),
        "DistanceTransform(directed)": lambda: DistanceTransform(directed_distances=True)(yb),
        "DistanceTransform(directed, invert, max 20)": lambda: DistanceTransform(directed_distances=True, invert=True,
                                                                                  max_distance=20)(yb),
        "connected_components": lambda: connected_components(yb),
        "label_consecutive": lambda: label_consecutive(yi),
        "MinSizeLabelTransform(25)": lambda: MinSizeLabelTransform(25)(yb),
        "OneHotTransform(4)": lambda: OneHotTransform(4)(y4),
        "NoToBackgroundBoundaryTransform(binary)": lambda: NoToBackgroundBoundaryTransform(add_binary_target=True)(ym),
        "BoundaryTransformWithIgnoreLabel(outer)": lambda: BoundaryTransformWithIgnoreLabel(mode="outer")(ym),
    }
    stream_bytes = {"OneHotTransform(4)": (8 + 16) * NV, "NoToBackgroundBoundaryTransform(binary)": (8 + 2) * NV,
                    "BoundaryTransformWithIgnoreLabel(outer)": (8 + 1) * NV}
    lines.append(f"batch 2x1x{'x'.join(str(s) for s in shape)} int64 labels ({NV * 8 / 1e6:.1f} MB), "
                 f"{int(inst.max())} objects in the larger sample; {args.reps} repetitions after {args.warmup} warm-up")
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    for k in fns:
        s = sorted(ms[k])
        med = s[len(s) // 2]
        extra = ""
        if k in stream_bytes:
            extra = (f"; one kernel, {stream_bytes[k] / 1e6:.0f} MB to move -> {stream_bytes[k] / (med * 1e-3) / 1e9:.0f} GB/s "
                     "(launch and allocation included)")
        lines.append(f"  {k:46s} median {med * 1e3:9.1f} us (min {s[0] * 1e3:.1f}, max {s[-1] * 1e3:.1f}){extra}")
    for directed in (False, True):
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda lab: cpu_distance_transform(lab, directed), list(binary[:, 0])))
            cpu = time.perf_counter() - t0
        key = "DistanceTransform(directed)" if directed else "DistanceTransform()"
        med = sorted(ms[key])[len(ms[key]) // 2]
        lines.append(f"  CPU, scipy distance_transform_edt(return_indices=True) + numpy, pool of 16 threads, {key}: "
                     f"{cpu * 1e3:.0f} ms per batch; device {med:.3f} ms = {cpu * 1e3 / med:.0f}x faster")
    kernel_table(fns, NV, ndim, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_label_targets.py needs the GPU: a CPU run gives no timing")
    lines = [f"label transforms on the device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, numpy {np.__version__}",
             "device events around each call (launches, torch glue and output allocation included), ops alternating"]
    bench((128, 128, 128), 4.0, args, lines)
    bench((1024, 1024), 8.0, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
