"""Times model.vit.Block against the same block composed from torch ops around the same vit.Attention, and each new op of
csrc/vit_block.hip against the bytes it must move.  Device events; versions alternate inside one loop.

    python scripts/bench_vit_block.py --out profiles/vit_block_bench.txt
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_em_amd import ops  # noqa: E402
from torch_em_amd.model import Block  # noqa: E402

# device-to-device copy, read + written bytes per second, measured on this chip (profiles/raw_normalize_bench.txt)
HBM_RATE, L3_RATE = 5.16e12, 4.09e12
SHAPES = [("ViT-B global", 768, 12, 0), ("ViT-B windowed", 768, 12, 14), ("ViT-H global", 1280, 16, 0)]
GRID = 64


class TorchBlock(torch.nn.Module):
    """the same parameters and the same Attention, everything else torch ops"""

    def __init__(self, blk):
        super().__init__()
        self.b = blk

    def forward(self, x):
        b, ws = self.b, self.b.window_size
        B, H, W, C = x.shape
        t = F.layer_norm(x, (C,), b.norm1.weight, b.norm1.bias, b.norm1.eps)
        if ws:
            Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
            t = F.pad(t, (0, 0, 0, Wp - W, 0, Hp - H)).view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)
        t = b.attn(t)
        if ws:
            t = t.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, C)[:, :H, :W].contiguous()
        x = x + t
        return x + b.mlp.lin2(F.gelu(b.mlp.lin1(F.layer_norm(x, (C,), b.norm2.weight, b.norm2.bias, b.norm2.eps))))


def timed(fns, reps, warmup):
    """median / min / max time in us of each callable, alternating them; one event pair per call"""
    times = [[] for _ in fns]
    for it in range(warmup + reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[i].append(a.elapsed_time(b) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = "cuda:0"
    lines = [f"model.vit.Block against the torch composition around the same vit.Attention; B = 1, {GRID} x {GRID} tokens; {args.reps} repetitions "
             f"after {args.warmup} warm-up, device events, versions alternating; times in us: median (min - max)",
             f"device: {torch.cuda.get_device_name(0)}; byte floors at the measured device-to-device copy rates: {HBM_RATE / 1e12:.2f} TB/s (HBM, 1 GiB) "
             f"and {L3_RATE / 1e12:.2f} TB/s (L3-resident, 16.8 MB) of profiles/raw_normalize_bench.txt; every tensor here fits the 256 MiB L3"]
    fmt = lambda t: f"{t[0]:8.1f} ({t[1]:.1f} - {t[2]:.1f})"
    for dtype in (torch.float16, torch.float32):
        for name, C, heads, ws in SHAPES:
            torch.manual_seed(0)
            blk = Block(C, heads, use_rel_pos=True, window_size=ws, input_size=(GRID, GRID)).to(dev).to(dtype).train()
            ref = TorchBlock(blk)
            x = torch.randn(1, GRID, GRID, C, device=dev, dtype=dtype)
            g = torch.randn_like(x)
            xg = x.clone().requires_grad_()

            def fwd(m):
                with torch.no_grad():
                    m(x)

            def fwd_bwd(m):
                m(xg).backward(g)
                xg.grad = None
                blk.zero_grad(set_to_none=True)

            with torch.no_grad():
                diff = float((blk(x).float() - ref(x).float()).abs().max())
            t = timed([lambda: fwd(blk), lambda: fwd(ref), lambda: fwd_bwd(blk), lambda: fwd_bwd(ref)], args.reps, args.warmup)
            lines.append(f"{name} C={C} {str(dtype)[6:]}: max |Block - torch| = {diff:.2e}")
            lines.append(f"  forward             Block {fmt(t[0])}   torch {fmt(t[1])}   torch / Block {t[1][0] / t[0][0]:.2f}x")
            lines.append(f"  forward + backward  Block {fmt(t[2])}   torch {fmt(t[3])}   torch / Block {t[3][0] / t[2][0]:.2f}x")

            # ---- the ops alone: call times (launch, allocation and, in the backward, the k_col_sum launch included)
            E, T = x.element_size(), GRID * GRID
            Td = T if ws == 0 else (-(-GRID // ws) * ws) ** 2
            w, b_ = blk.norm1.weight.detach(), blk.norm1.bias.detach()
            leaf = lambda t_: t_.detach().clone().requires_grad_()
            l1, l3 = [leaf(x), leaf(w), leaf(b_)], [leaf(torch.randn(T, 4 * C, device=dev, dtype=dtype)), leaf(blk.mlp.lin1.bias)]
            xw = ops.layer_norm_windows(*l1, 1e-6, ws)
            y = torch.randn_like(xw).detach()
            l2 = [leaf(y), leaf(x), leaf(w), leaf(b_)]
            x1, xn = ops.window_merge_norm(*l2, 1e-6, ws)
            z = ops.bias_gelu(*l3)
            h, b1 = l3[0].detach(), l3[1].detach()
            gw, gz = torch.randn_like(xw), torch.randn_like(z)
            back = lambda outs, leaves, gs: (lambda: torch.autograd.grad(outs, leaves, gs, retain_graph=True))
            cases = [("k_ln_win_fwd", (T + Td) * C * E, lambda: ops.layer_norm_windows(x, w, b_, 1e-6, ws)),
                     ("k_win_merge_ln_fwd", 4 * T * C * E, lambda: ops.window_merge_norm(y, x, w, b_, 1e-6, ws)),
                     ("k_ln_win_bwd + k_col_sum", 3 * T * C * E, back([xw], l1, [gw])),
                     ("k_win_merge_ln_bwd + k_col_sum", (4 * T + Td) * C * E, back([x1, xn], l2, [g, g])),
                     ("k_bias_gelu_fwd", 2 * T * 4 * C * E, lambda: ops.bias_gelu(h, b1)),
                     ("k_bias_gelu_bwd + k_col_sum", 3 * T * 4 * C * E, back([z], l3, [gz]))]
            with torch.no_grad():
                fwd_t = timed([c[2] for c in cases if "bwd" not in c[0]], args.reps, args.warmup)
            bwd_t = timed([c[2] for c in cases if "bwd" in c[0]], args.reps, args.warmup)
            ts = [fwd_t[0], fwd_t[1], bwd_t[0], bwd_t[1], fwd_t[2], bwd_t[2]]
            for (kname, nbytes, _), tt in zip(cases, ts):
                lines.append(f"  {kname:32s} {fmt(tt)}   {nbytes / 1e6:6.1f} MB -> floor {nbytes / HBM_RATE * 1e6:5.1f} us HBM, {nbytes / L3_RATE * 1e6:5.1f} us L3; "
                             f"{tt[0] / (nbytes / L3_RATE * 1e6):.1f}x the L3 floor")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
