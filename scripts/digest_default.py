"""SHA-256 digests of one training step in the DEFAULT (fp32-class) arithmetic: prediction, loss, flat parameter gradient.

Every kernel of the library is deterministic (no floating-point atomics, fixed reduction orders), so the digests are a
property of the source tree and the chip, not of the run.  tests/golden/default_step_digest.json holds the digests of the
tree at the end of round 4; tests/test_gpu_unet.py::test_default_arithmetic_is_bit_identical_to_round4 recomputes them --
the 16-bit activation storage of round 5 must not move a single bit of the fp32-class path.
usage: python scripts/digest_default.py [--write tests/golden/default_step_digest.json]   (TEM_LIB=<older .so> for an A/B)

ENGINE_CASES / run_engine_case: a second table for the host side of the step (model/engine.py, model/pack.py) -- the other
precision modes, norms, topologies and the no-grad forward -- with, next to the digests of TWO steps (the parameters are
scaled in place in between, so the second one runs on the batched weight re-pack), the ordered list of `ops` functions
the engine called.  tests/golden/engine_step_digest.json was written by the tree BEFORE the engine's state became named
records; tests/test_gpu_unet.py::test_engine_steps_and_op_calls_are_identical_to_the_fixture recomputes it.
usage: python scripts/digest_default.py --engine [--write tests/golden/engine_step_digest.json]"""
import hashlib
import inspect
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CASES = {
    # name: (model kwargs, input shape, pooling note)
    "cfg2_2x128": (dict(in_channels=1, out_channels=2, depth=4, initial_features=32), (2, 1, 128, 128, 128)),
    "gn_depth3_1x32x48x40": (dict(in_channels=1, out_channels=2, depth=3, initial_features=32, norm="GroupNorm"), (1, 1, 32, 48, 40)),
    "depth2_2x16": (dict(in_channels=1, out_channels=3, depth=2, initial_features=16), (2, 1, 16, 16, 16)),
}


def digest(t):
    return hashlib.sha256(t.detach().float().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(kw, shape):
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.model import UNet3d
    torch.manual_seed(11)
    model = UNet3d(**kw).to("cuda")
    g = torch.Generator().manual_seed(12)
    x = torch.randn(*shape, generator=g).to("cuda")
    y = (torch.rand(shape[0], kw["out_channels"], *shape[2:], generator=g) > 0.5).float().to("cuda")
    out = {}
    for rep in range(2):   # the second step runs on the batched weight re-pack: both must agree
        model.zero_grad(set_to_none=True)
        pred = model(x)
        loss = DiceLoss()(pred, y)
        loss.backward()
        torch.cuda.synchronize()
        grads = torch.cat([p.grad.flatten() for p in model.parameters()])
        cur = {"pred": digest(pred), "loss": float(loss).hex(), "grads": digest(grads)}
        assert rep == 0 or cur == out, "two identical steps differ"
        out = cur
    return out


ENGINE_CASES = {
    # name: (model class, positional arguments, keywords, input shape, options: mode / check_shape / no_grad_first)
    "amp": ("UNet3d", (1, 2), dict(depth=4, initial_features=32), (1, 1, 64, 64, 64), dict(mode="amp")),
    "amp_bf16": ("UNet3d", (1, 2), dict(depth=4, initial_features=32), (1, 1, 64, 64, 64), dict(mode="amp_bf16")),
    "fp32": ("UNet3d", (1, 2), dict(depth=4, initial_features=32), (1, 1, 64, 64, 64), dict(mode="fp32")),
    "batchnorm": ("UNet3d", (1, 2), dict(depth=2, initial_features=32, norm="BatchNorm"), (2, 1, 16, 32, 32), {}),
    "no_norm_sigmoid": ("UNet3d", (1, 2), dict(depth=2, initial_features=32, norm=None, final_activation="Sigmoid"),
                        (1, 1, 16, 32, 32), {}),
    "anisotropic": ("AnisotropicUNet", (1, 2, [[1, 2, 2], [2, 2, 2]]), dict(initial_features=32, anisotropic_kernel=True),
                    (1, 1, 8, 64, 64), {}),
    # the factor-2 upsampling kernel writes the statistics of its output itself; any other factor leaves them to
    # ops.upsample_stats, which needs the skip half's rows too (the 32-channel conv delivers them from 8 x 128 x 128 upward)
    "anisotropic_f4": ("AnisotropicUNet", (1, 2, [[1, 4, 4], [2, 2, 2]]), dict(initial_features=32, anisotropic_kernel=True),
                       (1, 1, 8, 128, 128), {}),
    "unet2d": ("UNet2d", (1, 2), dict(depth=2, initial_features=32), (1, 1, 128, 128), {}),
    "side_outputs": ("UNet3d", (1, 2), dict(depth=2, initial_features=32, return_side_outputs=True), (1, 1, 16, 32, 32), {}),
    "crop_floor": ("AnisotropicUNet", (1, 2, [[3, 3, 3], [2, 2, 2]]), dict(initial_features=4), (2, 1, 14, 14, 14),
                   dict(check_shape=False)),
    "no_grad_then_train": ("UNet3d", (1, 2), dict(depth=2, initial_features=32), (1, 1, 16, 32, 32), dict(no_grad_first=True)),
}
# every one of these must appear in the call list of at least one case (the routes this table exists for)
ENGINE_MUST_REACH = ("conv_fwd_refnorm", "conv_wgrad_gscaled", "conv_wgrad_gnorm", "conv1x1_out_bwd", "norm_bwd_coef",
                     "norm_stats_from_partials", "norm_stats_from_partials2", "upsample_stats", "absmax", "pack_weights_batch")


class OpsRecorder:
    """stands in for the `ops` module: appends the name of every FUNCTION called through it and forwards the call"""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not inspect.isfunction(v):
            return v

        def call(*a, **k):
            self._calls.append(name)
            return v(*a, **k)
        return call


def run_engine_case(cls, args, kw, shape, opt):
    import contextlib
    import importlib
    import torch_em_amd.model as tm
    from torch_em_amd import _lib, ops
    from torch_em_amd.loss import DiceLoss
    from torch_em_amd.model import engine
    mods = [engine]
    with contextlib.suppress(ImportError):   # a tree from before the weight-pack cache had a module of its own
        mods.append(importlib.import_module("torch_em_amd.model.pack"))
    torch.manual_seed(21)
    model = getattr(tm, cls)(*args, **kw)
    if "check_shape" in opt:
        model.check_shape = opt["check_shape"]
    model.to("cuda")
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*shape, generator=g).to("cuda")
    cat = lambda ts: torch.cat([t.detach().float().flatten() for t in ts])  # noqa: E731
    calls, res, ys = [], {}, None
    old = _lib.get_option("wgrad_sums_min_mb")
    _lib.set_option("wgrad_sums_min_mb", 0)    # as under tests/conftest.py: the norm sums on every layer that qualifies
    for m in mods:
        m.ops = OpsRecorder(ops, calls)
    try:
        with engine.precision_scope(opt.get("mode", engine.PRECISION)):
            if opt.get("no_grad_first"):
                with torch.no_grad():
                    pred = model(x)
                torch.cuda.synchronize()
                res["no_grad"] = {"pred": digest(pred), "calls": list(calls)}
            for rep in range(2):
                del calls[:]
                model.zero_grad(set_to_none=True)
                pred = model(x)
                preds = pred if isinstance(pred, (list, tuple)) else [pred]
                if ys is None:   # one target per output (side outputs: one per decoder level), drawn once
                    ys = [(torch.rand(*p.shape, generator=g) > 0.5).float().to("cuda") for p in preds]
                loss = sum(DiceLoss()(p, y) for p, y in zip(preds, ys))
                loss.backward()
                torch.cuda.synchronize()
                res[f"step{rep}"] = {"pred": digest(cat(preds)), "loss": float(loss).hex(),
                                     "grads": digest(cat([p.grad for p in model.parameters()])), "calls": list(calls)}
                with torch.no_grad():   # same storage, new values and versions: the next step re-packs in one launch
                    for p in model.parameters():
                        p.mul_(1 + 2.0 ** -10)
    finally:
        for m in mods:
            m.ops = ops
        _lib.set_option("wgrad_sums_min_mb", old)
    return res


def main():
    if "--engine" in sys.argv:
        sys.argv.remove("--engine")
        res = {name: run_engine_case(*case) for name, case in ENGINE_CASES.items()}
        reached = {c for r in res.values() for s in r.values() for c in s["calls"]}
        print(json.dumps({n: {s: dict(v, calls=len(v["calls"])) for s, v in r.items()} for n, r in res.items()}, indent=1))
        for name in ENGINE_MUST_REACH:
            print(f"{name}: {[n for n, r in res.items() if any(name in s['calls'] for s in r.values())]}")
        assert not set(ENGINE_MUST_REACH) - reached, set(ENGINE_MUST_REACH) - reached
    else:
        res = {name: run_case(kw, shape) for name, (kw, shape) in CASES.items()}
        print(json.dumps(res, indent=1))
    if len(sys.argv) > 2 and sys.argv[1] == "--write":
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
