"""Times the noise and blur raw augmentations of the device input pipeline on a cfg-2 batch (2 x 1 x 128^3 float32, uniform
[0, 1) data, one stream row per sample): `ops.gauss_noise`, `ops.poisson_add`, `ops.poisson_scaled` (row minimum included)
and `ops.blur2d`.  The Poisson ops run at lam / multiplier 10 and 100: at `multiplier = 10` every mean is below 10 (the
inversion), at 100 nine in ten are above (the transformed rejection); `poisson_add` also at the class's default scale.

    python scripts/bench_raw_aug.py [--size 128] [--reps 50] [--warmup 10] [--out profiles/raw_noise_blur_bench.txt]

Device events around each call, the ops alternating, median and spread over the repetitions.  Per op: the bytes of its pass
model (4 B per element per read or write pass) over a device-to-device copy rate measured in the same run, as the floor --
at the batch's own size (16.8 MB: it sits in the 256 MiB L3) and at 1 GiB (HBM).  Also the numpy branch of each class (the
reference's expression) on this host's CPU.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_raw import copy_rate, fmt, stats, timed  # noqa: E402
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.transform import AdditiveGaussianNoise, AdditivePoissonNoise, GaussianBlur, PoissonNoise  # noqa: E402
from torch_em_amd.transform.raw import gaussian_weights  # noqa: E402

SEED = 0x5eed5eed5eed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_raw_aug.py needs the GPU: a CPU run gives no timing")
    dev, S = "cuda:0", args.size
    x = np.random.RandomState(0).rand(2, 1, S, S, S).astype("float32")
    xd = torch.from_numpy(x).to(dev)
    rows = xd.reshape(2, -1)
    nbytes = 2 * S ** 3 * 4
    rate_l3, rate_hbm = copy_rate(nbytes, args.reps), copy_rate(1 << 30, 10)
    w7, w19 = gaussian_weights(1.0).tolist(), gaussian_weights(3.0).tolist()
    clip = (0.0, 1.0)
    # name: (call, read passes, write passes)
    fns = {
        "gauss_noise std 0.15": (lambda: ops.gauss_noise(rows, 0.15, SEED, clip), 1, 1),
        "poisson_add lam 0.05": (lambda: ops.poisson_add(rows, 0.05, SEED, clip), 1, 1),
        "poisson_add lam 10": (lambda: ops.poisson_add(rows, 10.0, SEED, clip), 1, 1),
        "poisson_add lam 100": (lambda: ops.poisson_add(rows, 100.0, SEED, clip), 1, 1),
        "poisson_scaled mult 10": (lambda: ops.poisson_scaled(rows, 10.0, SEED, clip), 2, 1),
        "poisson_scaled mult 100": (lambda: ops.poisson_scaled(rows, 100.0, SEED, clip), 2, 1),
        "blur2d 7 taps (sigma 1)": (lambda: ops.blur2d(xd, w7), 1, 1),
        "blur2d 19 taps (sigma 3)": (lambda: ops.blur2d(xd, w19), 1, 1),
    }
    lines = [f"noise and blur raw augmentations of a batch 2x1x{S}^3 float32 ({nbytes / 1e6:.1f} MB), per sample; {args.reps} repetitions "
             f"after {args.warmup} warm-up, device events, ops alternating", f"device: {torch.cuda.get_device_name(0)}, numpy {np.__version__}",
             f"device-to-device copy, read + written bytes per second: {rate_l3 / 1e12:.2f} TB/s at {nbytes / 1e6:.1f} MB (L3-resident), "
             f"{rate_hbm / 1e12:.2f} TB/s at 1 GiB (HBM)",
             "floor of an op = the bytes of its pass model / the L3-resident copy rate; 'x the floor' below is against that one, the HBM "
             "figure is for reference.  The noise ops are not byte-bound by design: each element costs ten Philox rounds and a "
             "logf / sqrtf / cospif or a sampler loop"]
    for _ in range(args.warmup):
        for fn, _, _ in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, (fn, _, _) in fns.items():
            ms[k].append(timed(fn))
    med = {}
    for k, (_, rd, wr) in fns.items():
        st = stats(ms[k])
        med[k] = st["median"]
        moved = (rd + wr) * nbytes
        lines.append(f"  {k:26s} {fmt(st)}; model {rd} read + {wr} write passes = {moved / 1e6:.0f} MB -> floor "
                     f"{moved / rate_l3 * 1e6:.1f} us at the L3 copy rate ({moved / rate_hbm * 1e6:.1f} us at the HBM rate), "
                     f"{st['median'] * 1e-3 / (moved / rate_l3):.1f}x the floor")
    lines.append(f"poisson_scaled, multiplier 100 over 10 (rejection over inversion): {med['poisson_scaled mult 100'] / med['poisson_scaled mult 10']:.2f}x; "
                 f"poisson_add, lam 100 over 10 (both rejection): {med['poisson_add lam 100'] / med['poisson_add lam 10']:.2f}x")
    # the numpy branch (the reference's expression and np.random draws) on this host, one sample, doubled for the batch
    cpu = {"AdditiveGaussianNoise (scale 0.15)": (AdditiveGaussianNoise(scale=(0.15, 0.15)), "gauss_noise std 0.15"),
           "AdditivePoissonNoise (lam 0.05)": (AdditivePoissonNoise(lam=(0.05, 0.05)), "poisson_add lam 0.05"),
           "PoissonNoise (multiplier 10)": (PoissonNoise(multiplier=(10.0, 10.0)), "poisson_scaled mult 10"),
           "PoissonNoise (multiplier 100)": (PoissonNoise(multiplier=(100.0, 100.0)), "poisson_scaled mult 100"),
           "GaussianBlur (sigma 3, torch CPU)": (GaussianBlur(sigma=(3.0, 3.0)), "blur2d 19 taps (sigma 3)")}
    for name, (t, dev_key) in cpu.items():
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            t(x[0])
            ts.append(time.perf_counter() - t0)
        cpu_ms = sorted(ts)[1] * 1e3
        lines.append(f"CPU, numpy branch of {name}, one {S}^3 sample on this host: {cpu_ms:.1f} ms, {2 * cpu_ms:.1f} ms per batch; "
                     f"device batch {med[dev_key]:.3f} ms = {2 * cpu_ms / med[dev_key]:.0f}x faster")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
