"""The REFERENCE's own `torch_em.util.load_model` (util/util.py:408-460) and `DefaultTrainer.from_checkpoint`
(trainer/default_trainer.py:288-330) read a checkpoint that THIS repo's trainer wrote on an MI355X (tests/golden/ckpt_tiny,
made by scripts/make_tiny_checkpoint.py) -- SURVEY.md 8(f)-4, checkpoint wire-format compatibility.  What the reference
returned for exactly these files is recorded in tests/golden/g11_reference_reads_ckpt.npz
(tests/golden/gen_golden_checkpoint_read.py); this repo's side -- the model class and kwargs named by the checkpoint's
`init` record -- is rebuilt here and must reproduce the reference's prediction: on the CPU through the oracle
(oracle/unet_ref.py, the engine has no CPU path), on the GPU through the rebuilt model itself."""
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CKPT = os.path.join(GOLDEN, "ckpt_tiny", "checkpoints", "tiny")


def _sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_reference_loads_our_checkpoint():
    g = np.load(os.path.join(GOLDEN, "g11_reference_reads_ckpt.npz"))
    # the record belongs to these very files
    assert _sha256(os.path.join(CKPT, "latest.pt")) == str(g["latest_sha256"])
    assert _sha256(os.path.join(CKPT, "io.pt")) == str(g["io_sha256"])
    ck = torch.load(os.path.join(CKPT, "latest.pt"), weights_only=False, map_location="cpu")
    # load_model: class + kwargs from the `init` record, then the state
    assert str(g["model_class"]) == "UNet2d" and str(g["model_module"]).startswith("torch_em_amd"), (g["model_class"], g["model_module"])
    assert bool(g["state_equal"]) and sorted(str(k) for k in g["state_keys"]) == sorted(ck["model_state"])
    mod, _, cls = ck["init"]["model_class"].rpartition(".")
    assert mod == str(g["model_module"]) and cls == str(g["model_class"])
    model = getattr(importlib.import_module(mod), cls)(**ck["init"]["model_kwargs"])
    model.load_state_dict(ck["model_state"])
    sd = model.state_dict()
    assert sorted(sd) == sorted(ck["model_state"]) and all(torch.equal(sd[k], ck["model_state"][k].cpu()) for k in sd)
    # the same state in the REFERENCE's UNet2d reproduces the prediction our engine stored next to the checkpoint ...
    io = torch.load(os.path.join(CKPT, "io.pt"), weights_only=False)
    ref_pred = torch.from_numpy(g["ref_pred"])
    err = float((ref_pred - io["pred"]).abs().max() / io["pred"].abs().max())
    assert err < 1e-4, err
    # ... and so does the rebuilt model's state in the oracle's UNet2d (fp32 CPU: round-off of the host's kernels only)
    from oracle import unet_ref
    with torch.no_grad():
        pred = unet_ref.unet_forward(sd, io["x"], [2] * (ck["init"]["model_kwargs"]["depth"]), training=False)
    err = float((pred - ref_pred).abs().max() / ref_pred.abs().max())
    assert err < 1e-5, err
    # DefaultTrainer.from_checkpoint: counters and the optimizer (class named by the record, one state per parameter)
    assert int(g["trainer_iteration"]) == ck["iteration"] == 4 and int(g["trainer_epoch"]) == ck["epoch"]
    assert str(g["optimizer_class"]) == "FusedAdamW" and int(g["optimizer_n_state"]) == len(sd)


@pytest.mark.gpu
def test_model_rebuilt_from_our_checkpoint_reproduces_the_reference_prediction():
    """The model this repo rebuilds from the checkpoint's `init` record, run on the MI355X in eval mode, reproduces the
    prediction the reference's own UNet2d computed from the same state (g11 `ref_pred`)."""
    g = np.load(os.path.join(GOLDEN, "g11_reference_reads_ckpt.npz"))
    ck = torch.load(os.path.join(CKPT, "latest.pt"), weights_only=False, map_location="cpu")
    mod, _, cls = ck["init"]["model_class"].rpartition(".")
    model = getattr(importlib.import_module(mod), cls)(**ck["init"]["model_kwargs"])
    model.load_state_dict(ck["model_state"])
    model.to("cuda").eval()
    io = torch.load(os.path.join(CKPT, "io.pt"), weights_only=False)
    with torch.no_grad():
        pred = model(io["x"].cuda()).cpu()
    ref_pred = torch.from_numpy(g["ref_pred"])
    err = float((pred - ref_pred).abs().max() / ref_pred.abs().max())
    assert err < 1e-4, err
