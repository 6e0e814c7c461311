"""Golden vectors of the clDice losses by IMPORTING THE REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cldice.py <torch-em checkout>

Loads the reference's loss/dice.py and loss/cldice.py by path from the checkout's `torch_em` package (the loader recipe
of gen_golden_distance.py) and writes g13_cldice.npz: per case `<case>.x` (prediction [N, C, *spatial]), `.y` (target),
`.num_iter`, `.alpha`, `.exclude_background`, `.kind` (0 SoftclDiceLoss, 1 CombinedclDiceLoss), `.skel_x` / `.skel_y`
(SoftSkeletonize(num_iter) of x / y, the reference's fp32 run), `.loss` and `.grad` (d loss / d x) from the reference run
in FLOAT64, `.loss32` (its fp32 loss) and `.grad32_dev` (the reference's own fp32-vs-float64 gradient deviation: max abs
difference over max |grad|).  Data only.

The generator asserts, for every case it writes, that the set of voxels with a non-zero gradient is the same in fp32 and
float64; a random case where a ReLU decision differs between the two precisions is drawn again with the next seed, so no
voxel has to be excluded from any comparison.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref):
    for name, path in (("torch_em", ref), ("torch_em.loss", ref + "/loss")):
        mod = types.ModuleType(name)
        mod.__path__ = [path]
        sys.modules[name] = mod
    out = {}
    for name, rel in (("torch_em.loss.dice", "loss/dice.py"), ("torch_em.loss.cldice", "loss/cldice.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        out[name.split(".")[-1]] = mod
    return out


def smooth(g, shape, passes=3):
    """box-filtered noise, standardised (smooth blobs without scipy)"""
    nd = len(shape) - 2
    a = torch.randn(shape, generator=g)
    pool = F.avg_pool3d if nd == 3 else F.avg_pool2d
    for _ in range(passes):
        a = pool(a, 3, 1, 1, count_include_pad=False)
    return (a - a.mean()) / a.std()


def make(kind, g, shape):
    if kind == "random":
        return torch.rand(shape, generator=g), (torch.rand(shape, generator=g) > 0.6).float()
    if kind == "blob":     # smooth blobs through a sigmoid against a noisy binary target
        field = smooth(g, shape)
        y = ((field + 0.3 * torch.randn(shape, generator=g)) > 0.2).float()
        return torch.sigmoid(4.0 * field), y
    if kind == "quant":    # multiples of 1/8: ties between distinct voxels everywhere
        return torch.round(torch.rand(shape, generator=g) * 8) / 8, (torch.rand(shape, generator=g) > 0.5).float()
    if kind == "plateau":  # saturated sigmoid: exact 0 / 1 plateaus with a thin graded rim
        field = smooth(g, shape)
        x = torch.round(torch.clamp(2.0 * field + 0.5, 0, 1) * 4) / 4
        return x, (smooth(g, shape) > 0.1).float()
    raise ValueError(kind)


def lines(a, b):
    x = torch.zeros(1, 1, 32, 32)
    x[0, 0, a:a + 4, :] = 1.0
    y = torch.zeros(1, 1, 32, 32)
    y[0, 0, b:b + 4, :] = 1.0
    return x, y


# name: (data kind, shape, loss kind (0 soft, 1 combined), num_iter, alpha, exclude_background)
CASES = {
    "rand3d": ("random", (2, 2, 8, 12, 20), 1, 5, 0.5, False),
    "blob3d": ("blob", (1, 1, 12, 16, 20), 1, 5, 0.5, False),
    "blob3d_soft": ("blob", (1, 2, 8, 10, 12), 0, 5, 0.5, False),
    "quant3d": ("quant", (1, 2, 8, 10, 12), 1, 5, 0.5, False),
    "plateau3d": ("plateau", (1, 1, 10, 12, 14), 1, 5, 0.3, False),
    "rand2d": ("random", (1, 2, 20, 24), 1, 5, 0.5, False),
    "rand2d_soft": ("random", (2, 1, 12, 16), 0, 5, 0.5, False),
    "blob2d": ("blob", (1, 1, 32, 36), 1, 5, 0.5, False),
    "quant2d": ("quant", (2, 1, 16, 20), 1, 5, 0.5, False),
    "plateau2d": ("plateau", (1, 1, 24, 28), 0, 5, 0.5, False),
    "odd3d": ("random", (1, 1, 9, 11, 37), 1, 5, 0.5, False),
    "odd2d": ("quant", (1, 1, 17, 35), 1, 5, 0.7, False),
    "iter0": ("random", (1, 1, 8, 10, 12), 1, 0, 0.5, False),
    "iter3": ("blob", (1, 2, 8, 10, 12), 1, 3, 0.5, False),
    "exbg3d": ("random", (1, 3, 8, 10, 12), 1, 5, 0.5, True),
    "exbg2d_soft": ("quant", (1, 3, 12, 16), 0, 2, 0.5, True),
    "line_overlap": ("lines", (14, 14), 1, 5, 0.5, False),
    "line_apart": ("lines", (4, 24), 1, 5, 0.5, False),
}


def run(cl, x, y, kind, num_iter, alpha, exbg, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    y = y.to(dtype)
    loss_fn = (cl.CombinedclDiceLoss(num_iter=num_iter, alpha=alpha, exclude_background=exbg) if kind == 1
               else cl.SoftclDiceLoss(num_iter=num_iter, exclude_background=exbg))
    loss = loss_fn(x, y)
    loss.backward()
    return loss.detach(), x.grad.detach()


def main(checkout):
    cl = load_reference(os.path.join(os.path.abspath(checkout), "torch_em"))["cldice"]
    res = {}
    for idx, (name, (data, shape, kind, num_iter, alpha, exbg)) in enumerate(CASES.items()):
        for attempt in range(20):
            g = torch.Generator().manual_seed(1300 + 100 * idx + attempt)
            x, y = lines(*shape) if data == "lines" else make(data, g, shape)
            l32, g32 = run(cl, x, y, kind, num_iter, alpha, exbg, torch.float32)
            l64, g64 = run(cl, x, y, kind, num_iter, alpha, exbg, torch.float64)
            if torch.equal(g32 != 0, g64 != 0):
                break
            assert data != "lines", name
            print(f"{name}: a ReLU decision differs between fp32 and float64 with seed offset {attempt}; drawing again")
        else:
            raise AssertionError(f"{name}: no draw with identical non-zero gradient sets")
        assert torch.equal(g32 != 0, g64 != 0), name
        dev = float((g32.double() - g64).abs().max() / g64.abs().max().clamp(min=1e-300))
        sk = cl.SoftSkeletonize(num_iter=num_iter)
        res.update({f"{name}.x": x.numpy(), f"{name}.y": y.numpy(), f"{name}.num_iter": np.int32(num_iter),
                    f"{name}.alpha": np.float64(alpha), f"{name}.exclude_background": np.int32(exbg),
                    f"{name}.kind": np.int32(kind), f"{name}.skel_x": sk(x).numpy(), f"{name}.skel_y": sk(y).numpy(),
                    f"{name}.loss": np.float64(l64.item()), f"{name}.loss32": np.float32(l32.item()),
                    f"{name}.grad": g64.numpy(), f"{name}.grad32_dev": np.float64(dev)})
        print(f"{name}: loss {l64.item():.6f}, grad32_dev {dev:.2e}, non-zero grads {int((g64 != 0).sum())}/{g64.numel()}")
    np.savez_compressed(os.path.join(OUT, "g13_cldice.npz"), **res)
    print(sorted({k.split(".")[0] for k in res}))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(f"usage: {sys.argv[0]} <torch-em checkout>")
    main(sys.argv[1])
