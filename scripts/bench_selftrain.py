"""Times the self-training additions on the GPU, in one process, alternating the things compared.

    python scripts/bench_selftrain.py [--size 128] [--reps 20] [--warmup 3] [--out profiles/selftrain_bench.txt]

1. `ops.pseudo_label` (sigmoid, both-sided mask; csrc/selftrain.hip) against the reference's composition as torch ops on the
   same device -- sigmoid, two compares, an add, a cast (self_training/pseudo_labeling.py:39-72) -- on a 2 x 2 x size^3
   channels-last prediction, fp32 and fp16.  The kernel moves (read + label write + mask write) bytes once; its achieved
   bytes/s stands beside the 6.29 TB/s float4 copy rate of the MI355X (a 67 MB tensor sits in the 256 MiB last-level cache:
   the copy rate is a reference point at this size, not a roofline).
2. Step times at cfg 2's shape (UNet3d(1 -> 2, 32 features, depth 4, sigmoid), 2 x 1 x size^3): the unsupervised step
   (teacher forward, labeler, student forward + backward, AdamW, EMA) against one supervised step plus one inference forward
   measured in the same run; the difference is the self-training overhead.
3. The optimizer phase of the semi-supervised step (two gradient nodes: FusedAdamW's per-tensor path) against that of the
   unsupervised step (one node: one launch).

Device events around each item; median and spread over the repetitions.  There is no CPU fallback: without a GPU it fails.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_em_amd import ops  # noqa: E402

COPY_RATE = 6.29e12   # float4 copy, measured on the MI355X (bytes/s)


def stats(ms):
    s = sorted(ms)
    n = len(s)
    return {"median": s[n // 2], "min": s[0], "max": s[-1], "iqr": s[(3 * n) // 4] - s[n // 4]}


def fmt(st):
    return f"median {st['median']:.3f} ms (min {st['min']:.3f}, max {st['max']:.3f}, iqr {st['iqr']:.3f})"


def timed(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fns, reps, warmup, inner=1):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            out[i].append(timed(fn, inner))
    return [stats(o) for o in out]


def bench_labeler(S, reps, warmup, dev, lines):
    t = 0.9
    g = torch.Generator().manual_seed(0)
    base = (2.0 * torch.randn(2, 2, S, S, S, generator=g)).to(dev).contiguous(memory_format=torch.channels_last_3d)
    for dtype in (torch.float32, torch.float16):
        x = base.to(dtype)

        def kernel():
            return ops.pseudo_label(x, "sigmoid", t, True)

        def composition():
            labels = torch.sigmoid(x)
            return labels, ((labels >= t) + (labels <= 1.0 - t)).to(dtype=torch.float32)

        (lk, mk), (lc, mc) = kernel(), composition()
        same_mask = bool(torch.equal(mk, ((lk >= t) + (lk <= 1.0 - t)).to(torch.float32)))
        differ = float((mk != mc).float().mean())
        sk, sc = alternate([kernel, composition], reps, warmup, inner=20)
        nbytes = x.numel() * (2 * x.element_size() + 4)
        rate = nbytes / (sk["median"] * 1e-3)
        lines += [f"pseudo_label {str(dtype).split('.')[1]}, 2x2x{S}^3 channels-last ({x.numel() * x.element_size() / 1e6:.1f} MB in), "
                  f"sigmoid + both-sided mask, 20 calls per timed window:",
                  f"  kernel      {fmt(sk)}",
                  f"  composition {fmt(sc)}   (torch: sigmoid, two compares, add, cast)",
                  f"  ratio composition / kernel (medians) {sc['median'] / sk['median']:.2f}x",
                  f"  kernel traffic {nbytes / 1e6:.1f} MB (read + label write + mask write) -> {rate / 1e12:.2f} TB/s achieved, "
                  f"{100 * rate / COPY_RATE:.0f} % of the {COPY_RATE / 1e12:.2f} TB/s float4 copy rate",
                  f"  kernel mask == compare of the kernel's labels: {same_mask}; mask voxels that differ from the composition's: {differ:.2e}"]


def bench_steps(S, reps, warmup, dev, lines):
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.model import UNet3d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.self_training import (DefaultPseudoLabeler, DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric,
                                            MeanTeacherTrainer)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    xs = torch.randn(2, 1, S, S, S, generator=g).to(dev)
    ys = (torch.rand(2, 2, S, S, S, generator=g) > 0.5).float().to(dev)
    xu1 = torch.randn(2, 1, S, S, S, generator=g).to(dev)
    xu2 = xu1 + 0.5 * torch.randn(2, 1, S, S, S, generator=g).to(dev)
    loaders = [(xu1, xu2)], [(xs, ys)]   # the trainer only asks them for their length here

    def make(semi):
        model = UNet3d(1, 2, initial_features=32, depth=4, final_activation="Sigmoid").to(dev)
        kw = dict(supervised_train_loader=loaders[1], supervised_loss=DefaultSelfTrainingLoss()) if semi else {}
        tr = MeanTeacherTrainer(name="bench", model=model, optimizer=FusedAdamW(model.parameters(), lr=1e-4),
                                pseudo_labeler=DefaultPseudoLabeler(confidence_threshold=0.6), unsupervised_loss=DefaultSelfTrainingLoss(),
                                unsupervised_train_loader=loaders[0], unsupervised_val_loader=loaders[0],
                                unsupervised_loss_and_metric=DefaultSelfTrainingLossAndMetric(), momentum=0.999,
                                reinit_teacher=False, mixed_precision=False, device=dev, **kw)
        tr.teacher.to(dev)
        tr.model.train()
        return tr

    unsup, semi = make(False), make(True)
    sup_model = UNet3d(1, 2, initial_features=32, depth=4, final_activation="Sigmoid").to(dev)
    sup_opt, dice = FusedAdamW(sup_model.parameters(), lr=1e-4), DiceLoss()

    def supervised_step():
        sup_opt.zero_grad()
        dice(sup_model(xs), ys).backward()
        sup_opt.step()

    def inference():
        with torch.no_grad():
            sup_model(xu1)

    def unsupervised_step():
        unsup._unsupervised_step(xu1, xu2)
        with torch.no_grad():
            unsup._momentum_update()

    def semisupervised_step():
        semi._semisupervised_step(xs, ys, xu1, xu2)
        with torch.no_grad():
            semi._momentum_update()

    s_sup, s_inf, s_unsup, s_semi = alternate([supervised_step, inference, unsupervised_step, semisupervised_step], reps, warmup)
    base = s_sup["median"] + s_inf["median"]
    lines += [f"steps at cfg 2's shape (UNet3d 1->2, 32 features, depth 4, sigmoid; 2x1x{S}^3; fp32-class arithmetic):",
              f"  supervised step (zero_grad, forward, DiceLoss, backward, AdamW) {fmt(s_sup)}",
              f"  inference forward (no grad)                                     {fmt(s_inf)}",
              f"  unsupervised step (teacher, labeler, student fwd+bwd, AdamW, EMA) {fmt(s_unsup)}",
              f"  self-training overhead: unsupervised - (supervised + inference) = {s_unsup['median'] - base:+.3f} ms "
              f"({100 * (s_unsup['median'] - base) / base:+.1f} %)",
              f"  semi-supervised step (two student passes, one backward)         {fmt(s_semi)}"]

    # ---- optimizer phase: per-tensor path (two gradient nodes) against the one-launch path (one node) ----
    def opt_phase(tr, prepare):
        def run():
            prepare()
            return timed(tr.optimizer.step)
        return run

    def one_node():
        unsup.optimizer.zero_grad()
        unsup.unsupervised_loss(unsup.model, xu2, ys, None).backward()

    def two_nodes():
        semi.optimizer.zero_grad()
        ((semi.supervised_loss(semi.model, xs, ys) + semi.unsupervised_loss(semi.model, xu2, ys, None)) / 2).backward()

    runs = [opt_phase(unsup, one_node), opt_phase(semi, two_nodes)]
    for r in runs:
        r()
    one, two = [], []
    for _ in range(max(reps // 2, 5)):
        one.append(runs[0]())
        flat_one = unsup.optimizer._arena.grads_flat() is not None
        two.append(runs[1]())
        flat_two = semi.optimizer._arena.grads_flat() is not None
    s_one, s_two = stats(one), stats(two)
    lines += ["optimizer phase (FusedAdamW.step alone, device events):",
              f"  one gradient node  (flat arena found: {flat_one})  {fmt(s_one)}",
              f"  two gradient nodes (flat arena found: {flat_two}) {fmt(s_two)}",
              f"  per-tensor path costs {s_two['median'] - s_one['median']:+.3f} ms per semi-supervised step "
              f"({100 * (s_two['median'] - s_one['median']) / s_semi['median']:.1f} % of it)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_selftrain.py needs the GPU: a CPU run gives no timing")
    dev = "cuda:0"
    lines = [f"self-training benchmark; {args.reps} repetitions after {args.warmup} warm-up, device events, alternating",
             f"device: {torch.cuda.get_device_name(0)}"]
    bench_labeler(args.size, args.reps, args.warmup, dev, lines)
    bench_steps(args.size, args.reps, args.warmup, dev, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
