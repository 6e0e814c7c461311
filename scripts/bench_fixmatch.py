"""Times the FixMatch additions on the GPU, in one process, alternating the things compared.

    python scripts/bench_fixmatch.py [--size 128] [--step-size 64] [--reps 20] [--warmup 3] [--out profiles/fixmatch_bench.txt]
                                     [--alignment-only]   (part 1 alone: the command to put under a kernel trace for kernel times)

1. Distribution alignment (`ops.distribution_align`: count + align, csrc/selftrain.hip) against the reference's composition
   as torch ops on the same device -- a compare, a `where`, `torch.unique(..., return_counts=True)`, the ratio, two scaled
   copies, a second `where` and a `clip` (self_training/fix_match.py:164-181) -- on 2 x 2 x size^3 labels, fp32 and fp16.
   The two launches are also timed one by one through the library's entry points: the count reads n * b bytes, the align
   launch reads n * b and writes n * b.  Their achieved bytes/s stand beside the dense read and write rates that
   profiles/r05_halfline.txt found reachable on the MI355X (a 34 MB tensor sits in the 256 MiB last-level cache: the rates are
   reference points at this size, not a roofline).
2. One semi-supervised FixMatch step (supervised forward, the labeler's no_grad forward of the same model, alignment,
   unsupervised forward, one backward, AdamW) of UNet3d(1 -> 2, 32 features, depth 4, sigmoid) at 2 x 1 x step-size^3, with
   and without `source_distribution`; the difference is what the alignment costs in a step.

Device events around each item; median and spread over the repetitions.  There is no CPU fallback: without a GPU it fails.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_selftrain import alternate, fmt  # noqa: E402
from torch_em_amd import _lib, ops  # noqa: E402

READ_RATE, WRITE_RATE = 6.57e12, 4.01e12   # dense 128-byte lines, profiles/r05_halfline.txt rows 1 and 7 (bytes/s)
SOURCE = (0.7, 0.3)


def composition(x, source, label_threshold=0.5):
    """the reference's lines, on the device"""
    binary = torch.where(x >= label_threshold, 1, 0)
    _, target = torch.unique(binary, return_counts=True)
    target = target / target.sum()
    ratio = source / target
    return torch.where(x < label_threshold, x * ratio[0], x * ratio[1]).clip(0, 1)


def bench_alignment(S, reps, warmup, dev, lines):
    g = torch.Generator().manual_seed(0)
    base = (torch.rand(2, 2, S, S, S, generator=g) ** 2).to(dev)
    source = torch.FloatTensor(SOURCE).to(dev)
    lib = _lib.load()
    for dtype in (torch.float32, torch.float16):
        x = base.to(dtype)
        n, st = x.numel(), ops._st(x)
        thr = ops.round_to(0.5, dtype)
        partials, out = ops.label_count_partials(x), torch.empty_like(x)

        def kernels():
            return ops.distribution_align(x, SOURCE)

        def torch_ops():
            return composition(x, source)

        def count_launch():
            _lib.check(lib.tem_label_count_st(ops._p(x), n, thr, ops._p(partials), partials.numel(), st, ops._stream(x)), "count")

        def align_launch():
            _lib.check(lib.tem_distribution_align_st(ops._p(x), ops._p(out), n, thr, SOURCE[0], SOURCE[1], ops._p(partials),
                                                     partials.numel(), st, ops._stream(x)), "align")

        # the kernels are pinned bit for bit to the reference on the CPU (tests/golden/g18_fixmatch.npz); torch's device
        # composition need not agree with torch's CPU one in the 16-bit types, so the difference is reported, not asserted
        yk, yc = kernels().float(), torch_ops().float()
        differ = float((yk != yc).float().mean())
        ulp = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -10
        worst = float(((yk - yc).abs() / (yc.abs().clamp_min(2.0 ** -14) * ulp)).max())
        sk, sc, s1, s2 = alternate([kernels, torch_ops, count_launch, align_launch], reps, warmup, inner=20)
        nb = n * x.element_size()
        r1, r2 = nb / (s1["median"] * 1e-3), 2 * nb / (s2["median"] * 1e-3)
        verdict = "the two launches are faster" if sk["median"] <= sc["median"] else "THE TWO LAUNCHES ARE SLOWER"
        lines += [f"distribution_align {str(dtype).split('.')[1]}, 2x2x{S}^3 ({nb / 1e6:.1f} MB of labels), source {list(SOURCE)}, "
                  f"20 calls per timed window:",
                  f"  count + align (ops.distribution_align) {fmt(sk)}",
                  f"  torch composition                      {fmt(sc)}   (compare, where, unique + counts, ratio, 2 products, where, clip)",
                  f"  ratio composition / kernels (medians) {sc['median'] / sk['median']:.2f}x: {verdict}",
                  f"  count launch alone {fmt(s1)}: {nb / 1e6:.1f} MB read -> {r1 / 1e12:.2f} TB/s, "
                  f"{100 * r1 / READ_RATE:.0f} % of the {READ_RATE / 1e12:.2f} TB/s dense read rate",
                  f"  align launch alone {fmt(s2)}: {nb / 1e6:.1f} MB read + {nb / 1e6:.1f} MB written -> {r2 / 1e12:.2f} TB/s, "
                  f"{100 * r2 / WRITE_RATE:.0f} % of the {WRITE_RATE / 1e12:.2f} TB/s dense write rate "
                  f"({100 * r2 / READ_RATE:.0f} % of the read rate)",
                  f"  elements that differ from the device composition's: {differ:.2e} of all, by at most {worst:.2f} relative "
                  f"units of 2^{-23 if dtype == torch.float32 else -10}"]


def bench_steps(S, reps, warmup, dev, lines):
    from torch_em_amd.model import UNet3d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.self_training import (DefaultPseudoLabeler, DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric,
                                            FixMatchTrainer)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    xs = torch.randn(2, 1, S, S, S, generator=g).to(dev)
    ys = (torch.rand(2, 2, S, S, S, generator=g) > 0.5).float().to(dev)
    xu1 = torch.randn(2, 1, S, S, S, generator=g).to(dev)
    xu2 = xu1 + 0.5 * torch.randn(2, 1, S, S, S, generator=g).to(dev)
    loaders = [(xu1, xu2)], [(xs, ys)]   # the trainer only asks them for their length here

    def make(source):
        model = UNet3d(1, 2, initial_features=32, depth=4, final_activation="Sigmoid").to(dev)
        tr = FixMatchTrainer(name="bench", model=model, optimizer=FusedAdamW(model.parameters(), lr=1e-4),
                             pseudo_labeler=DefaultPseudoLabeler(confidence_threshold=0.6), unsupervised_loss=DefaultSelfTrainingLoss(),
                             unsupervised_train_loader=loaders[0], unsupervised_val_loader=loaders[0],
                             unsupervised_loss_and_metric=DefaultSelfTrainingLossAndMetric(),
                             supervised_train_loader=loaders[1], supervised_loss=DefaultSelfTrainingLoss(),
                             source_distribution=source, mixed_precision=False, device=dev)
        tr.model.train()
        return tr

    plain, aligned = make(None), make(list(SOURCE))
    s_plain, s_aligned = alternate([lambda: plain._semisupervised_step(xs, ys, xu1, xu2),
                                    lambda: aligned._semisupervised_step(xs, ys, xu1, xu2)], reps, warmup)
    d = s_aligned["median"] - s_plain["median"]
    lines += [f"semi-supervised FixMatch step (UNet3d 1->2, 32 features, depth 4, sigmoid; 2x1x{S}^3; fp32-class arithmetic; "
              f"supervised forward, no_grad labeler forward, unsupervised forward, one backward, AdamW):",
              f"  without source_distribution {fmt(s_plain)}",
              f"  with source_distribution    {fmt(s_aligned)}",
              f"  alignment in the step: {d:+.3f} ms ({100 * d / s_plain['median']:+.2f} %)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--step-size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--alignment-only", action="store_true", help="skip the training steps (for a run under a kernel profiler)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fixmatch.py needs the GPU: a CPU run gives no timing")
    dev = "cuda:0"
    lines = [f"FixMatch benchmark; {args.reps} repetitions after {args.warmup} warm-up, device events, alternating",
             f"device: {torch.cuda.get_device_name(0)}"]
    bench_alignment(args.size, args.reps, args.warmup, dev, lines)
    if not args.alignment_only:
        bench_steps(args.step_size, args.reps, args.warmup, dev, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
