"""GPU: PerObjectDistanceTransform against the per-object oracle (tests/test_distance_cpu.py: pod_oracle), and
DistanceLoss / DiceBasedDistanceLoss against the reference's values (g12_distance_loss.npz), end to end in the
DefaultTrainer."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_distance_cpu import fixtures_2d, fixtures_3d, oracle_ids, pod_oracle, voronoi_3d

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the channel combinations of the reference's test (test/transform/test_label_transforms.py:171-226) and the rest of
# the constructor's surface
CONFIGS = [
    dict(),
    dict(distances=True, boundary_distances=False),
    dict(distances=False, boundary_distances=True),
    dict(foreground=False),
    dict(directed_distances=True),
    dict(distances=False, boundary_distances=False, directed_distances=True, foreground=False),
    dict(instances=True, directed_distances=True),
    dict(min_size=25, instances=True),
    dict(apply_label=False, instances=True),
    dict(distance_fill_value=0.0, apply_label=False, min_size=25),
]


def _compare(got, exp, cfg):
    got = np.asarray(got, dtype="float64")
    exp = np.asarray(exp, dtype="float64")
    assert got.shape == exp.shape, (got.shape, exp.shape)
    n_exact = int(cfg.get("instances", False)) + int(cfg.get("foreground", True))
    np.testing.assert_array_equal(got[:n_exact], exp[:n_exact])
    # distance channels: a different center or arg-max would move whole objects by far more than this
    err = np.abs(got[n_exact:] - exp[n_exact:]).max() if got.shape[0] > n_exact else 0.0
    assert err <= 1e-6, err


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
@pytest.mark.parametrize("name", sorted(fixtures_2d()))
def test_transform_2d_matches_oracle(name, ci):
    from torch_em_amd.transform import PerObjectDistanceTransform
    lab = fixtures_2d()[name]
    cfg = CONFIGS[ci]
    out = PerObjectDistanceTransform(**cfg)(torch.from_numpy(lab).to(DEV))
    assert out.is_cuda and out.dtype == torch.float32
    _compare(out.cpu().numpy(), pod_oracle(lab, **cfg), cfg)


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
@pytest.mark.parametrize("name", sorted(fixtures_3d()))
def test_transform_3d_matches_oracle(name, ci):
    from torch_em_amd.transform import PerObjectDistanceTransform
    lab = fixtures_3d()[name]
    cfg = CONFIGS[ci]
    out = PerObjectDistanceTransform(**cfg)(torch.from_numpy(lab).to(DEV))
    _compare(out.cpu().numpy(), pod_oracle(lab, **cfg), cfg)


@pytest.mark.parametrize("sampling,name", [((2.5, 1.0, 1.0), "voronoi0"), ((2.5, 1.0, 1.0), "rings"),
                                           ((1.0, 2.5), "blobs0"), ((1.0, 2.5), "rings")])
@pytest.mark.parametrize("directed", [False, True])
def test_transform_sampling(sampling, name, directed):
    from torch_em_amd.transform import PerObjectDistanceTransform
    lab = (fixtures_3d() if len(sampling) == 3 else fixtures_2d())[name]
    cfg = dict(sampling=sampling, directed_distances=directed)
    out = PerObjectDistanceTransform(**cfg)(torch.from_numpy(lab).to(DEV))
    _compare(out.cpu().numpy(), pod_oracle(lab, **cfg), cfg)


@pytest.mark.parametrize("instances", [False, True])
def test_numpy_path_dtypes(instances):
    from torch_em_amd.transform import PerObjectDistanceTransform
    lab = fixtures_2d()["rings"].astype("uint32")
    out = PerObjectDistanceTransform(instances=instances)(lab)
    assert isinstance(out, np.ndarray) and out.dtype == (np.float64 if instances else np.float32)
    exp = pod_oracle(lab.astype("int64"), instances=instances)
    assert exp.dtype == out.dtype
    _compare(out, exp, dict(instances=instances))


def test_degenerate_samples():
    from torch_em_amd.transform import PerObjectDistanceTransform
    t = PerObjectDistanceTransform(directed_distances=True, instances=True)
    empty = t(torch.zeros(6, 7, 8, dtype=torch.int64, device=DEV)).cpu()
    assert (empty[:2] == 0).all() and (empty[2:] == 1.0).all()           # fill value everywhere, foreground 0
    single = torch.zeros(6, 7, 8, dtype=torch.int64, device=DEV)
    single[2, 3, 4] = 9
    out = t(single).cpu()
    assert out[0, 2, 3, 4] == 1 and out[1, 2, 3, 4] == 1 and (out[2:, 2, 3, 4] == 0).all()
    full = t(torch.full((6, 7, 8), 4, dtype=torch.int64, device=DEV)).cpu()
    assert (full[1] == 1).all() and (full[-1] == 0).all()              # no boundary voxel: boundary channel 0
    assert torch.isfinite(full).all()


def test_batched_call_matches_per_sample_oracle():
    """one [2, 1, 64, 96, 80] call, samples independent"""
    from torch_em_amd.transform import PerObjectDistanceTransform
    labs = np.stack([voronoi_3d(5, shape=(64, 96, 80), n=60), voronoi_3d(6, shape=(64, 96, 80), n=90)])[:, None]
    cfg = dict(instances=True, directed_distances=True)
    out = PerObjectDistanceTransform(**cfg)(torch.from_numpy(labs).to(DEV))
    assert out.shape == (2, 1 + 1 + 1 + 3 + 1, 64, 96, 80)
    for n in range(2):
        _compare(out[n].cpu().numpy(), pod_oracle(labs[n, 0], **cfg), cfg)
    lab2d = np.stack([fixtures_2d()["blobs0"], fixtures_2d()["blobs1"]])[:, None]
    out2 = PerObjectDistanceTransform(**cfg)(torch.from_numpy(lab2d).to(DEV))
    for n in range(2):
        _compare(out2[n].cpu().numpy(), pod_oracle(lab2d[n, 0], **cfg), cfg)


def test_transform_and_loss_make_no_host_sync():
    from torch_em_amd.loss import DiceBasedDistanceLoss
    from torch_em_amd.transform import PerObjectDistanceTransform
    labs = torch.from_numpy(voronoi_3d(2, shape=(16, 24, 20), n=10)[None, None]).to(DEV)
    pred = torch.rand(1, 3, 16, 24, 20, device=DEV, requires_grad=True)
    t = PerObjectDistanceTransform(min_size=10)
    t2 = PerObjectDistanceTransform(apply_label=False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = t(labs)
        t2(labs)
        loss = DiceBasedDistanceLoss(True)(pred, y)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()


def _golden_cases():
    g = np.load(os.path.join(GOLDEN, "g12_distance_loss.npz"))
    return g, sorted({k.split(".")[0] for k in g.files})


@pytest.mark.parametrize("case", _golden_cases()[1])
def test_loss_matches_reference_golden(case):
    from torch_em_amd.loss import DiceBasedDistanceLoss, DistanceLoss
    g = _golden_cases()[0]
    cls = DiceBasedDistanceLoss if int(g[f"{case}.kind"]) else DistanceLoss
    loss_fn = cls(mask_distances_in_bg=bool(g[f"{case}.mask"]))
    res = []
    for _ in range(2):
        x = torch.from_numpy(g[f"{case}.x"]).to(DEV).requires_grad_(True)
        y = torch.from_numpy(g[f"{case}.y"]).to(DEV)
        loss = loss_fn(x, y)
        loss.backward()
        res.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
    loss, grad = res[0]
    ref_l, ref_g = g[f"{case}.loss"], g[f"{case}.grad"]
    assert abs(float(loss) - float(ref_l)) <= 1e-5 * abs(float(ref_l)), (float(loss), float(ref_l))
    assert np.abs(grad - ref_g).max() <= 1e-5 * np.abs(ref_g).max()
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()


def test_loss_accepts_channels_last_and_half_inputs():
    from torch_em_amd.loss import DistanceLoss
    g = np.load(os.path.join(GOLDEN, "g12_distance_loss.npz"))
    x = torch.from_numpy(g["dl_mask_bin.x"]).to(DEV)
    y = torch.from_numpy(g["dl_mask_bin.y"]).to(DEV)
    xc = x.to(memory_format=torch.channels_last_3d).requires_grad_(True)
    loss = DistanceLoss(True)(xc, y)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["dl_mask_bin.loss"])) <= 1e-5 * abs(float(g["dl_mask_bin.loss"]))
    assert np.abs(xc.grad.cpu().numpy() - g["dl_mask_bin.grad"]).max() <= 1e-5 * np.abs(g["dl_mask_bin.grad"]).max()
    xh = x.half().requires_grad_(True)
    lh = DistanceLoss(True)(xh, y)
    lh.backward()
    assert xh.grad.dtype == torch.float16 and abs(float(lh.detach()) - float(g["dl_mask_bin.loss"])) < 1e-2


def test_trainer_end_to_end_with_distance_targets(tmp_path):
    from torch_em_amd.loss import DiceBasedDistanceLoss
    from torch_em_amd.model import UNet3d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.trainer import DefaultTrainer
    from torch_em_amd.transform import PerObjectDistanceTransform
    xs = torch.randn(2, 1, 64, 64, 64, generator=torch.Generator().manual_seed(0))
    labs = torch.from_numpy(np.stack([voronoi_3d(s, shape=(64, 64, 64), n=40) for s in (7, 8)])[:, None])
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(xs, labs), batch_size=1)
    seen = []
    tt = PerObjectDistanceTransform(distances=True, boundary_distances=True, foreground=True, min_size=25)
    torch.manual_seed(0)
    model = UNet3d(1, 3, depth=2, initial_features=8, final_activation="Sigmoid")
    trainer = DefaultTrainer(name="dist", train_loader=loader, val_loader=loader, model=model,
                             loss=DiceBasedDistanceLoss(mask_distances_in_bg=True),
                             optimizer=FusedAdamW(model.parameters(), lr=1e-3), metric=DiceBasedDistanceLoss(True),
                             device=DEV, save_root=str(tmp_path), logger=None, target_transform=tt)
    losses = []
    orig = trainer.loss.forward

    def record(pred, y):
        val = orig(pred, y)
        seen.append(y.detach().clone())
        losses.append(val.detach())
        return val
    trainer.loss.forward = record
    trainer.fit(iterations=4)
    assert losses and all(torch.isfinite(v).item() for v in losses)
    exp = [tt(labs[i:i + 1].to(DEV)) for i in range(2)]
    assert seen and all(any(torch.equal(s, e) for e in exp) for s in seen)
    back = DefaultTrainer.from_checkpoint(trainer.checkpoint_folder, name="latest")
    assert type(back.loss) is DiceBasedDistanceLoss and back.loss.init_kwargs == {"mask_distances_in_bg": True}
    assert type(back.metric) is DiceBasedDistanceLoss
