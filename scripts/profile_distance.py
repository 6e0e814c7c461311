"""Workload for a kernel census of the distance-based targets and losses (run under rocprofv3 --kernel-trace --stats):
PerObjectDistanceTransform on a 2x1x128^3 label batch with a few hundred objects, and DiceBasedDistanceLoss /
DistanceLoss forward + backward at the 2x3x128^3 prediction shape of the cfg-2 network with three output channels."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_em_amd.loss import DiceBasedDistanceLoss, DistanceLoss  # noqa: E402
from torch_em_amd.transform import PerObjectDistanceTransform  # noqa: E402


def voronoi(seed, shape, n):
    rng = np.random.default_rng(seed)
    pts = torch.from_numpy(rng.uniform(0, 1, (n, 3)) * np.array(shape)).float().cuda()
    grid = torch.stack(torch.meshgrid(*[torch.arange(s, device="cuda") for s in shape], indexing="ij"), -1).float()
    lab = torch.empty(shape, dtype=torch.int64, device="cuda")
    for z in range(shape[0]):
        lab[z] = torch.cdist(grid[z].reshape(-1, 3), pts).argmin(-1).reshape(shape[1:]) + 1
    lab[lab % 7 == 0] = 0
    return lab


def main(reps=5):
    labs = torch.stack([voronoi(s, (128, 128, 128), 300) for s in (0, 1)])[:, None]
    tt = PerObjectDistanceTransform(min_size=25)
    for _ in range(reps):
        y = tt(labs)
    torch.cuda.synchronize()
    pred = torch.rand(2, 3, 128, 128, 128, device="cuda", requires_grad=True)
    for loss_fn in (DiceBasedDistanceLoss(True), DistanceLoss(True)):
        for _ in range(reps):
            loss = loss_fn(pred, y)
            loss.backward()
    torch.cuda.synchronize()
    print("targets", tuple(y.shape), "foreground fraction", float(y[:, 0].mean()), "loss", float(loss.detach()))


if __name__ == "__main__":
    main()
