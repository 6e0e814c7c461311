"""Golden vectors of the distance-based losses by IMPORTING THE REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_distance.py <torch-em checkout>

Loads the reference's loss/dice.py and loss/distance_based.py by path from the checkout's `torch_em` package (the
loader recipe of gen_golden.py) and writes
g12_distance_loss.npz: per case `<case>.x` (prediction [N, 3, *spatial]), `.y` (target), `.loss`, `.grad` (d loss /
d x), `.kind` (0 DistanceLoss, 1 DiceBasedDistanceLoss), `.mask` (mask_distances_in_bg).  Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref):
    for name, path in (("torch_em", ref), ("torch_em.loss", ref + "/loss")):
        mod = types.ModuleType(name)
        mod.__path__ = [path]
        sys.modules[name] = mod
    out = {}
    for name, rel in (("torch_em.loss.dice", "loss/dice.py"), ("torch_em.loss.distance_based", "loss/distance_based.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        out[name.split(".")[-1]] = mod
    return out


def case(g, shape, frac_fg):
    x = torch.rand(shape, generator=g)
    fg = torch.rand((shape[0], 1) + shape[2:], generator=g)
    fg = fg if frac_fg else (fg > 0.45).float()
    dist = torch.rand((shape[0], 2) + shape[2:], generator=g) * (fg > 0).float()
    return x, torch.cat([fg, dist], 1)


def main(checkout):
    db = load_reference(os.path.join(os.path.abspath(checkout), "torch_em"))["distance_based"]
    g = torch.Generator().manual_seed(12)
    res = {}
    for kind, cls in ((0, db.DistanceLoss), (1, db.DiceBasedDistanceLoss)):
        for mask in (True, False):
            for frac, shape in ((False, (2, 3, 8, 10, 12)), (True, (1, 3, 24, 20))):
                if frac and not mask:
                    continue
                name = f"{'dl' if kind == 0 else 'dbdl'}_{'mask' if mask else 'nomask'}_{'frac' if frac else 'bin'}"
                x, y = case(g, shape, frac)
                x.requires_grad_(True)
                loss = cls(mask_distances_in_bg=mask)(x, y)
                loss.backward()
                res.update({f"{name}.x": x.detach().numpy(), f"{name}.y": y.numpy(),
                            f"{name}.loss": np.float32(loss.item()), f"{name}.grad": x.grad.numpy(),
                            f"{name}.kind": np.int32(kind), f"{name}.mask": np.int32(mask)})
    np.savez_compressed(os.path.join(OUT, "g12_distance_loss.npz"), **res)
    print(sorted({k.split(".")[0] for k in res}))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(f"usage: {sys.argv[0]} <torch-em checkout>")
    main(sys.argv[1])
