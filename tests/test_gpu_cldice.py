"""GPU: the clDice kernels (csrc/cldice.hip) against the reference's recorded runs (tests/golden/g13_cldice.npz) and the
CPU oracle of tests/test_cldice_cpu.py (torch-op restatement, hand-written gather-form gradient).

Forward: SoftSkeletonize and soft_erode / soft_dilate / soft_open are BIT-EQUAL to the fixture and to the restatement.

Gradient bound (fixed before the kernels ran): per case, max |grad - grad64| <= GRAD_MULT * max(grad32_dev, 2^-23) *
max |grad64|, with grad64 the reference's float64 gradient and grad32_dev the reference's own fp32-vs-float64 deviation
recorded in the fixture.  GRAD_MULT = 8: the kernels sum the same fp32 terms in another order (gather, fixed) and take
the score's coefficients from a double reduction, so they may sit a small multiple of the reference's own fp32 error
away from float64; the floor is one fp32 ulp (2^-23), below which an fp32 result cannot be expected to agree (the line
cases record a deviation of exactly 0).  A wrong tie rule moves single voxels by O(1) of max |grad| -- 10^6 bounds.
Worst ratio error / (max(grad32_dev, 2^-23) * max |grad64|) observed on the MI355X: 1.26 (plateau3d; all others
<= 1.00), i.e. the kernels are as close to float64 as the reference's own fp32 run.

Loss bound: |loss - loss64| <= 2e-6 absolute (the loss lies in [0, 1]; 16 fp32 ulps of 1 for the fp32 skeletons, the
fp32 products under the double sums and the fp32 Dice / combination arithmetic).
"""
import numpy as np
import pytest
import torch

from test_cldice_cpu import (case_names, dilate, erode, load_case, np_dilate_bwd, np_erode, np_erode_bwd,
                             np_skel_bwd, skel_restate)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_MULT = 8.0
FLOOR = 2.0 ** -23


def _layouts(x):
    """the tensor as the loader gives it (NCDHW) and as the engine gives predictions (channels-last memory)"""
    out = [("planar", x.contiguous())]
    if x.shape[1] > 1:
        out.append(("channels_last", x.contiguous(memory_format=torch.channels_last_3d if x.dim() == 5
                                                  else torch.channels_last)))
    return out


def _loss_of(c):
    from torch_em_amd.loss import CombinedclDiceLoss, SoftclDiceLoss
    if int(c["kind"]) == 1:
        return CombinedclDiceLoss(num_iter=int(c["num_iter"]), alpha=float(c["alpha"]),
                                  exclude_background=bool(c["exclude_background"]))
    return SoftclDiceLoss(num_iter=int(c["num_iter"]), exclude_background=bool(c["exclude_background"]))


@pytest.mark.parametrize("name", case_names())
def test_skeleton_is_bit_equal_to_reference(name):
    from torch_em_amd.loss import SoftSkeletonize
    c = load_case(name)
    sk = SoftSkeletonize(num_iter=int(c["num_iter"]))
    for key in ("x", "y"):
        for layout, t in _layouts(torch.from_numpy(c[key]).to(DEV)):
            out = sk(t)
            assert out.shape == t.shape and out.dtype == torch.float32
            assert torch.equal(out.cpu(), torch.from_numpy(c[f"skel_{key}"])), (name, key, layout)


@pytest.mark.parametrize("name", ["rand3d", "quant3d", "plateau3d", "odd3d", "rand2d", "quant2d", "odd2d", "blob2d"])
def test_erode_dilate_open_are_bit_equal_to_restatement(name):
    from torch_em_amd.loss import SoftSkeletonize
    c = load_case(name)
    sk = SoftSkeletonize()
    x = torch.from_numpy(c["x"])
    for layout, t in _layouts(x.to(DEV)):
        assert torch.equal(sk.soft_erode(t).cpu(), erode(x)), (name, layout, "erode")
        assert torch.equal(sk.soft_dilate(t).cpu(), dilate(x)), (name, layout, "dilate")
        assert torch.equal(sk.soft_open(t).cpu(), dilate(erode(x))), (name, layout, "open")


def test_channel_sliced_view_is_read_in_place():
    from torch_em_amd.loss import SoftSkeletonize
    c = load_case("exbg3d")
    x = torch.from_numpy(c["x"])
    for layout, t in _layouts(x.to(DEV)):
        view = t[:, 1:]
        assert view.storage_offset() > 0 and view.shape[1] == 2   # a view into the 3-channel tensor, no copy
        assert torch.equal(SoftSkeletonize(3)(view).cpu(), skel_restate(x[:, 1:], 3)), layout
        assert torch.equal(SoftSkeletonize().soft_erode(view).cpu(), erode(x[:, 1:])), layout
    c = load_case("exbg2d_soft")
    x = torch.from_numpy(c["x"])
    assert torch.equal(SoftSkeletonize(2)(x.to(DEV)[:, 1:]).cpu(), skel_restate(x[:, 1:], 2))


def test_larger_volume_64_cubed():
    from torch_em_amd.loss import SoftSkeletonize
    g = torch.Generator().manual_seed(64)
    x = torch.rand(1, 2, 64, 64, 64, generator=g)
    x[:, 1] = torch.round(x[:, 1] * 16) / 16          # one continuous, one quantised channel
    ref = skel_restate(x, 5)
    for layout, t in _layouts(x.to(DEV)):
        assert torch.equal(SoftSkeletonize(5)(t).cpu(), ref), layout
    # a shape that is no multiple of the tile, W not a multiple of 4
    x = torch.rand(2, 1, 19, 21, 70, generator=g)
    assert torch.equal(SoftSkeletonize(4)(x.to(DEV)).cpu(), skel_restate(x, 4))
    x = torch.rand(1, 3, 45, 131, generator=g)
    assert torch.equal(SoftSkeletonize(5)(x.to(DEV)).cpu(), skel_restate(x, 5))


@pytest.mark.parametrize("name", case_names())
def test_loss_and_gradient_match_reference_float64(name):
    c = load_case(name)
    loss_fn = _loss_of(c)
    y = torch.from_numpy(c["y"]).to(DEV)
    gmax = float(np.abs(c["grad"]).max())
    bound = GRAD_MULT * max(float(c["grad32_dev"]), FLOOR) * gmax
    for layout, x0 in _layouts(torch.from_numpy(c["x"]).to(DEV)):
        res = []
        for _ in range(2):
            x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
            loss = loss_fn(x, y)
            loss.backward()
            res.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
        loss, grad = res[0]
        err = float(np.abs(grad - c["grad"]).max())
        print(f"cldice {name} {layout}: loss {float(loss):.7f} (float64 {float(c['loss']):.7f}), grad err / max|grad| "
              f"{err / gmax:.3e}, grad32_dev {float(c['grad32_dev']):.3e}, ratio to max(dev, 2^-23) "
              f"{err / gmax / max(float(c['grad32_dev']), FLOOR):.2f}")
        assert abs(float(loss) - float(c["loss"])) <= 2e-6, (name, layout, float(loss), float(c["loss"]))
        assert err <= bound, (name, layout, err / gmax, bound / gmax)
        assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes(), (name, layout)


@pytest.mark.parametrize("name", ["rand3d", "quant3d", "plateau3d", "odd3d", "iter0", "rand2d", "quant2d", "plateau2d",
                                  "odd2d", "line_apart"])
def test_skeleton_gradient_with_random_upstream(name):
    """d / d x of sum(SoftSkeletonize(x) * g) for a random g against the hand-written float64 gather gradient"""
    from torch_em_amd.loss import SoftSkeletonize
    c = load_case(name)
    k = int(c["num_iter"])
    g = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(3))
    ref = np_skel_bwd(c["x"].astype(np.float64), k, g.numpy().astype(np.float64))
    scale = float(np.abs(ref).max())
    for layout, x0 in _layouts(torch.from_numpy(c["x"]).to(DEV)):
        grads = []
        for _ in range(2):
            x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
            produced = []
            x.register_hook(lambda gr: produced.append(gr.stride()))
            SoftSkeletonize(k)(x).backward(g.to(DEV))
            grads.append(x.grad.cpu().numpy())
            assert produced == [x.stride()], (layout, produced)   # written in the prediction's own layout
        err = float(np.abs(grads[0] - ref).max())
        print(f"skeleton gradient {name} {layout}: err / max|grad| {err / scale:.3e}")
        assert err <= GRAD_MULT * max(float(c["grad32_dev"]), FLOOR) * scale, (name, layout, err / scale)
        assert grads[0].tobytes() == grads[1].tobytes()


@pytest.mark.parametrize("name", ["quant3d", "plateau3d", "odd3d", "quant2d", "odd2d"])
def test_erode_dilate_open_gradients(name):
    from torch_em_amd.loss import SoftSkeletonize
    c = load_case(name)
    sk = SoftSkeletonize()
    nd = c["x"].ndim - 2
    x64 = c["x"].astype(np.float64)
    g = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(4))
    g64 = g.numpy().astype(np.float64)
    refs = {"erode": np_erode_bwd(x64, g64, nd), "dilate": np_dilate_bwd(x64, g64, nd),
            "open": np_erode_bwd(x64, np_dilate_bwd(np_erode(x64, nd), g64, nd), nd)}
    for layout, x0 in _layouts(torch.from_numpy(c["x"]).to(DEV)):
        for op, ref in refs.items():
            x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
            getattr(sk, f"soft_{op}")(x).backward(g.to(DEV))
            err = float(np.abs(x.grad.cpu().numpy() - ref).max())
            assert err <= GRAD_MULT * FLOOR * float(np.abs(ref).max()), (name, layout, op, err)


def test_half_and_mixed_inputs_are_cast_to_fp32():
    from torch_em_amd.loss import CombinedclDiceLoss
    c = load_case("blob3d")
    x = torch.from_numpy(c["x"]).to(DEV).half().requires_grad_(True)
    y = torch.from_numpy(c["y"]).to(DEV).half()
    loss = CombinedclDiceLoss()(x, y)
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == torch.float16
    assert abs(float(loss.detach()) - float(c["loss"])) < 1e-2 and torch.isfinite(x.grad).all().item()


def test_loss_makes_no_host_sync():
    from torch_em_amd.loss import CombinedclDiceLoss
    c = load_case("rand3d")
    x = torch.from_numpy(c["x"]).to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    y = torch.from_numpy(c["y"]).to(DEV)
    loss_fn = CombinedclDiceLoss()
    loss_fn(x, y).backward()                  # sizes the workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = loss_fn(x, y)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()


def _tube_batches(n, seed, size=32):
    """noisy raw volumes with a few axis-aligned tubes; target channels: tubes, background"""
    g = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for _ in range(n):
        t = torch.zeros(size, size, size)
        for _ in range(4):
            a, b = (int(v) for v in torch.randint(3, size - 6, (2,), generator=g))
            ax = int(torch.randint(0, 3, (1,), generator=g))
            idx = [slice(a, a + 3), slice(b, b + 3)]
            idx.insert(ax, slice(None))
            t[tuple(idx)] = 1.0
        xs.append((t + 0.3 * torch.randn(size, size, size, generator=g))[None])
        ys.append(torch.stack([t, 1.0 - t]))
    return torch.utils.data.TensorDataset(torch.stack(xs), torch.stack(ys))


def _trainer(tmp_path, name, loss, hip_graph):
    from torch_em_amd.model import UNet3d
    from torch_em_amd.optim import FusedAdamW
    from torch_em_amd.trainer import DefaultTrainer
    torch.manual_seed(0)
    model = UNet3d(1, 2, depth=2, initial_features=4, final_activation="Sigmoid")
    train = torch.utils.data.DataLoader(_tube_batches(4, 0), batch_size=1, shuffle=False)
    val = torch.utils.data.DataLoader(_tube_batches(2, 1), batch_size=1, shuffle=False)
    return DefaultTrainer(name=name, train_loader=train, val_loader=val, model=model, loss=loss,
                          optimizer=FusedAdamW(model.parameters(), lr=1e-3), metric=loss, device=DEV,
                          save_root=str(tmp_path), logger=None, mixed_precision=False, hip_graph=hip_graph)


def test_trainer_with_combined_cldice_loss_eager_graph_and_checkpoint(tmp_path):
    from torch_em_amd.loss import CombinedclDiceLoss
    from torch_em_amd.trainer import DefaultTrainer
    trainers = []
    for hip_graph in (False, True):
        t = _trainer(tmp_path, f"cld{int(hip_graph)}", CombinedclDiceLoss(num_iter=3, alpha=0.4), hip_graph)
        sd0 = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
        t.fit(iterations=6)
        assert any(not torch.equal(v.cpu(), sd0[k].cpu()) for k, v in t.model.state_dict().items())
        assert all(torch.isfinite(v).all().item() for v in t.model.state_dict().values())
        trainers.append(t)
    t0, t1 = trainers
    assert t0._graphed is None and t1._graphed is not None and t1._graph_why is None and t1._graphed.replays == 6
    for (k, a), b in zip(t0.model.state_dict().items(), t1.model.state_dict().values()):
        assert torch.equal(a, b), k
    back = DefaultTrainer.from_checkpoint(t0.checkpoint_folder, name="latest")
    assert type(back.loss) is CombinedclDiceLoss
    assert back.loss.init_kwargs == {"num_iter": 3, "alpha": 0.4, "eps": 1e-7, "exclude_background": False}
    assert back.loss.num_iter == 3 and back.loss.alpha == 0.4


def test_trainer_with_combined_loss_of_dice_and_cldice(tmp_path):
    from torch_em_amd.loss import CombinedLoss, DiceLoss, SoftclDiceLoss
    loss = CombinedLoss(DiceLoss(), SoftclDiceLoss(num_iter=2))
    t = _trainer(tmp_path, "comb", loss, False)
    seen = []
    orig = t.loss.forward

    def record(pred, y):
        val = orig(pred, y)
        seen.append(val.detach())
        return val
    t.loss.forward = record
    t.fit(iterations=4)
    assert len(seen) >= 4 and all(torch.isfinite(v).item() for v in seen)
    # the weighted sum of its parts
    x, y = next(iter(t.train_loader))
    with torch.no_grad():
        pred = t.model(x.to(DEV))
        parts = 0.5 * DiceLoss()(pred, y.to(DEV)) + 0.5 * SoftclDiceLoss(num_iter=2)(pred, y.to(DEV))
        assert torch.equal(orig(pred, y.to(DEV)), parts)
