"""Times CombinedclDiceLoss forward + backward on a cfg-2-shaped prediction (2 x 2 x 128^3, channels-last memory, NCDHW
target) for num_iter 3 and 5, against the torch-op restatement of the reference (loss/cldice.py with loss/dice.py's
dice_score; fp32, autograd) on the same GPU, in the same process, alternating the two.

    python scripts/bench_cldice.py [--size 128] [--reps 30] [--warmup 5] [--out profiles/cldice_bench.txt]

Device events around each forward + backward; median and spread (min, max, inter-quartile range) over the repetitions.
Also: the forward skeleton alone against its traffic model (16 B / voxel / round: read e_j and skel, write e_{j+1} and
skel), the loss's share of a 15 ms training step (README.md, cfg 2), and a same-input agreement check of the two paths.
There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_em_amd.loss import CombinedclDiceLoss, SoftSkeletonize  # noqa: E402


# ---- the reference restated with torch ops (what a user of torch_em runs on this GPU) ----
def erode(x):
    p1 = -F.max_pool3d(-x, (3, 1, 1), 1, (1, 0, 0))
    p2 = -F.max_pool3d(-x, (1, 3, 1), 1, (0, 1, 0))
    p3 = -F.max_pool3d(-x, (1, 1, 3), 1, (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def soft_skel(x, num_iter):
    x1 = F.max_pool3d(erode(x), 3, 1, 1)
    skel = F.relu(x - x1)
    for _ in range(num_iter):
        x = erode(x)
        delta = F.relu(x - F.max_pool3d(erode(x), 3, 1, 1))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def restated_loss(x, y, num_iter, alpha=0.5, eps=1e-7):
    dice = 1.0 - 2.0 * (x * y).sum() / ((x * x).sum() + (y * y).sum()).clamp(min=eps)
    sx, sy = soft_skel(x, num_iter), soft_skel(y, num_iter)
    tp = (sx * y).sum() / sx.sum().clamp(min=eps)
    ts = (sy * x).sum() / sy.sum().clamp(min=eps)
    cl = 1.0 - 2.0 * (tp * ts) / (tp + ts).clamp(min=eps)
    return (1.0 - alpha) * dice + alpha * cl


def stats(ms):
    s = sorted(ms)
    n = len(s)
    return {"median": s[n // 2], "min": s[0], "max": s[-1], "iqr": s[(3 * n) // 4] - s[n // 4]}


def fmt(st):
    return f"median {st['median']:.3f} ms (min {st['min']:.3f}, max {st['max']:.3f}, iqr {st['iqr']:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cldice.py needs the GPU: a CPU run gives no timing")
    dev = "cuda:0"
    S = args.size
    g = torch.Generator().manual_seed(0)
    # a sigmoid-like prediction of smooth structures and a binary target
    field = F.avg_pool3d(torch.randn(2, 2, S, S, S, generator=g), 5, 1, 2)
    field = field / field.std()
    pred = torch.sigmoid(3.0 * field).to(dev).contiguous(memory_format=torch.channels_last_3d)
    target = (field > 0.3).float().to(dev)
    voxels = pred.numel()
    lines = [f"CombinedclDiceLoss forward + backward, prediction 2x2x{S}^3 channels-last fp32 ({voxels * 4 / 1e6:.1f} MB), "
             f"target NCDHW; {args.reps} repetitions after {args.warmup} warm-up, device events, fused and restated "
             f"alternating", f"device: {torch.cuda.get_device_name(0)}"]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for num_iter in (3, 5):
        loss_fn = CombinedclDiceLoss(num_iter=num_iter)
        x = pred.clone(memory_format=torch.preserve_format).requires_grad_(True)

        def fused():
            x.grad = None
            loss_fn(x, target).backward()

        def restated():
            x.grad = None
            restated_loss(x, target, num_iter).backward()

        sk = SoftSkeletonize(num_iter)

        def skel_fwd():
            with torch.no_grad():
                sk(pred)

        # same inputs, same result (the restatement is the comparison target, so it must compute the same thing)
        fused()
        gf, lf = x.grad.clone(), float(loss_fn(x, target).detach())
        restated()
        gr, lr = x.grad.clone(), float(restated_loss(x, target, num_iter).detach())
        agree = float((gf - gr).abs().max() / gr.abs().max())
        for _ in range(args.warmup):
            fused(), restated(), skel_fwd()
        torch.cuda.synchronize()
        tf, tr, ts = [], [], []
        for _ in range(args.reps):
            tf.append(timed(fused))
            tr.append(timed(restated))
            ts.append(timed(skel_fwd))
        sf, sr, ss = stats(tf), stats(tr), stats(ts)
        rounds = num_iter + 1
        model_bytes = 16.0 * voxels * rounds
        lines += [f"num_iter={num_iter}:",
                  f"  fused    {fmt(sf)}",
                  f"  restated {fmt(sr)}",
                  f"  ratio restated / fused (medians) {sr['median'] / sf['median']:.2f}x",
                  f"  loss fused {lf:.7f}, restated {lr:.7f}; max |grad difference| / max |grad| {agree:.2e}",
                  f"  fused loss share of a 15 ms step: {100.0 * sf['median'] / 15.0:.1f} % (restated: "
                  f"{100.0 * sr['median'] / 15.0:.1f} %)",
                  f"  forward skeleton alone ({rounds} rounds, no grad) {fmt(ss)}: traffic model 16 B/voxel/round = "
                  f"{model_bytes / 1e6:.0f} MB -> {model_bytes / (ss['median'] * 1e-3) / 1e12:.2f} TB/s achieved "
                  f"(a {voxels * 4 / 1e6:.0f} MB tensor sits in the 256 MiB L3: the HBM copy rate is an upper reference, "
                  f"not a roofline, at this size)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
