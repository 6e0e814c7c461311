"""Times ops.attention (csrc/attention.hip) on the attention shapes of the SAM vision transformers, with relative-position
tables, beside two yardsticks from outside the code under test: the plain torch composition that materialises the logits
(what segment_anything runs) and torch.nn.functional.scaled_dot_product_attention with the bias passed as attn_mask.

    python scripts/bench_attention.py [--reps 9] [--warmup 3] [--out profiles/attention_bench.txt]

  ViT-B global   B=1  nH=12 64x64 D=64        ViT-B windows  B=25 nH=12 14x14 D=64        ViT-H global   B=1 nH=16 64x64 D=80
each in float16, bfloat16 and float32.  q, k, v are the views of a packed qkv-linear output, as the module passes them.
Device events around each call; median and spread over the repetitions.  The flop count is 4 B nH N^2 D (both products; the
bias pre-pass adds 2 B nH N (H + W) D); the fraction is of the chip's sustained 16-bit MFMA rate with random operands
(profiles/r03_mfma_sustained.txt), a call-time figure: the pre-pass launch is inside it.  The yardsticks get their bias
tensor [B, nH, N, N] prebuilt outside the timed window for SDPA (its construction is timed separately) and build it inside
for the plain composition, as segment_anything does.  There is no CPU fallback: without a GPU the script fails.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torch_em_amd import ops  # noqa: E402

DEV = "cuda:0"
SUSTAINED_MFMA16_TFLOPS = 1700.0      # profiles/r03_mfma_sustained.txt: 1622 .. 1742 TF with random operands
SHAPES = (("ViT-B global", 1, 12, 64, 64, 64), ("ViT-B windows", 25, 12, 14, 14, 64), ("ViT-H global", 1, 16, 64, 64, 80))
DTYPES = (torch.float16, torch.bfloat16, torch.float32)


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


def rel_bias(q, H, W, Rh, Rw):
    """segment_anything's add_decomposed_rel_pos as a bias tensor [B, nH, N, N]"""
    B, nH, N, D = q.shape
    ih = torch.arange(H, device=q.device)[:, None] - torch.arange(H, device=q.device)[None, :] + H - 1
    iw = torch.arange(W, device=q.device)[:, None] - torch.arange(W, device=q.device)[None, :] + W - 1
    r = q.reshape(B, nH, H, W, D)
    rel_h = torch.einsum("bahwc,hkc->bahwk", r, Rh[ih])
    rel_w = torch.einsum("bahwc,wkc->bahwk", r, Rw[iw])
    return (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, nH, N, N)


def composition(q, k, v, H, W, Rh, Rw, scale):
    attn = (q * scale) @ k.transpose(-2, -1)
    attn = (attn + rel_bias(q, H, W, Rh, Rw)).softmax(dim=-1)
    return attn @ v


def backward_mode(args):
    """forward + backward of one attention call (gradients of q, k, v and both tables), device events; peak allocated memory
    above what is resident before the call, for ops.attention plus its cached workspace.  Yardsticks: the plain composition (logits materialised in both passes) and SDPA
    with a prebuilt bias leaf [B, nH, N, N] as attn_mask (autograd produces its gradient; building the bias is timed apart)."""
    lines = [f"ops.attention forward + backward (csrc/attention.hip, csrc/attention_bwd.hip) with relative-position tables; {args.reps} "
             f"repetitions after {args.warmup} warm-up, device events", f"device: {torch.cuda.get_device_name(0)}"]
    g = torch.Generator(device=DEV).manual_seed(0)
    for name, B, nH, H, W, D in SHAPES:
        N = H * W
        lines.append(f"{name}: B={B} nH={nH} {H}x{W} D={D}; logits [B, nH, N, N] in fp32: {4e-6 * B * nH * N * N:.0f} MB; backward workspace "
                     f"(tem_attention_bwd_ws): {ops._lib.load().tem_attention_bwd_ws(B, nH, H, W, D, 1) / 1e6:.0f} MB")
        for dt in DTYPES:
            qkv = torch.randn((B, N, 3, nH, D), generator=g, device=DEV).to(dt).requires_grad_()
            views = lambda: tuple(qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))      # fresh view nodes for every backward
            Rh, Rw = ((0.5 * torch.randn((2 * s - 1, D), generator=g, device=DEV)).to(dt).requires_grad_() for s in (H, W))
            dO = torch.randn((B, nH, N, D), generator=g, device=DEV).to(dt)
            scale = D ** -0.5
            bias = rel_bias(views()[0], H, W, Rh, Rw).detach().requires_grad_()
            leaves = (qkv, Rh, Rw, bias)

            def step(fn):
                for t in leaves:
                    t.grad = None
                fn().backward(dO)

            def run(fn):
                st = measure(lambda: step(fn), args.warmup, args.reps)
                for t in leaves:
                    t.grad = None
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                step(fn)
                torch.cuda.synchronize()
                return st, (torch.cuda.max_memory_allocated() - base) / 1e6

            ours, m0 = run(lambda: ops.attention(*views(), (H, W), rel_pos=(Rh, Rw)))
            # ops.workspace() is a cached per-stream buffer the warm-up already allocated: it is inside the baseline, so its size
            # (the backward's query, the larger of the two passes, at least the cache's 1 MiB) is added to the peak
            ws_mb = max(ops._lib.load().tem_attention_bwd_ws(B, nH, H, W, D, 1), 1 << 20) / 1e6
            m0 += ws_mb
            comp, m1 = run(lambda: composition(*views(), H, W, Rh, Rw, scale))
            sdpa, m2 = run(lambda: F.scaled_dot_product_attention(*views(), attn_mask=bias, scale=scale))
            with torch.no_grad():
                mask = measure(lambda: rel_bias(views()[0], H, W, Rh, Rw), args.warmup, args.reps)
            verdict = ", ".join(f"{'faster' if ours['median'] < o['median'] else 'SLOWER'} than {n} x{o['median'] / ours['median']:.2f}"
                                for n, o in (("the composition", comp), ("SDPA", sdpa)))
            lines += [f"  {str(dt).split('.')[-1]:8s} ops.attention            {fmt(ours)}; peak {m0:.0f} MB (of which workspace {ws_mb:.0f} MB)",
                      f"           torch composition        {fmt(comp)}; peak {m1:.0f} MB",
                      f"           SDPA, bias as attn_mask  {fmt(sdpa)}; peak {m2:.0f} MB (+ building the bias: {mask['median']:.3f} ms)",
                      f"           -> {verdict}"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true", help="time forward + backward (with gradients of the tables) instead of the forward")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention.py needs the GPU: a CPU run gives no timing")
    if args.backward:
        text = "\n".join(backward_mode(args))
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    lines = [f"ops.attention (csrc/attention.hip) with relative-position tables; {args.reps} repetitions after {args.warmup} warm-up, device events",
             f"device: {torch.cuda.get_device_name(0)}; fraction: of {SUSTAINED_MFMA16_TFLOPS:.0f} TF, the sustained 16-bit MFMA rate"]
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for name, B, nH, H, W, D in SHAPES:
            N = H * W
            flop = 4.0 * B * nH * N * N * D + 2.0 * B * nH * N * (H + W) * D
            lines.append(f"{name}: B={B} nH={nH} {H}x{W} D={D}; {flop / 1e9:.2f} GFLOP; logits [B, nH, N, N] in fp32: {4e-6 * B * nH * N * N:.0f} MB")
            for dt in DTYPES:
                qkv = torch.randn((B, N, 3, nH, D), generator=g, device=DEV).to(dt)
                q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
                Rh, Rw = (0.5 * torch.randn((2 * s - 1, D), generator=g, device=DEV).to(dt) for s in (H, W))
                scale = D ** -0.5
                y = torch.empty((B, H, W, nH * D), dtype=dt, device=DEV)
                out = y.view(B, N, nH, D).permute(0, 2, 1, 3)
                bias = rel_bias(q, H, W, Rh, Rw)
                want = composition(q.float(), k.float(), v.float(), H, W, Rh.float(), Rw.float(), scale)
                ops.attention(q, k, v, (H, W), rel_pos=(Rh, Rw), out=out)
                err = float((out.float() - want).abs().max())
                ours = measure(lambda: ops.attention(q, k, v, (H, W), rel_pos=(Rh, Rw), out=out), args.warmup, args.reps)
                comp = measure(lambda: composition(q, k, v, H, W, Rh, Rw, scale), args.warmup, args.reps)
                sdpa = measure(lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=scale), args.warmup, args.reps)
                mask = measure(lambda: rel_bias(q, H, W, Rh, Rw), args.warmup, args.reps)
                tf = flop / (ours["median"] * 1e9)
                verdict = ", ".join(f"{'faster' if ours['median'] < o['median'] else 'SLOWER'} than {n} x{o['median'] / ours['median']:.2f}"
                                    for n, o in (("the composition", comp), ("SDPA", sdpa)))
                lines += [f"  {str(dt).split('.')[-1]:8s} ops.attention            {fmt(ours)}; {tf:.1f} TFLOP/s = {tf / SUSTAINED_MFMA16_TFLOPS:.3f} of the rate; "
                          f"max |out - fp32 composition| {err:.2e}",
                          f"           torch composition        {fmt(comp)}",
                          f"           SDPA, bias as attn_mask  {fmt(sdpa)} (+ building the bias: {mask['median']:.3f} ms)",
                          f"           -> {verdict}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
