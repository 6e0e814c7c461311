"""G11: what the REFERENCE reads from the checkpoint THIS repo's trainer wrote (tests/golden/ckpt_tiny, made on an MI355X by
scripts/make_tiny_checkpoint.py), recorded as data for tests/test_reference_reads_checkpoint.py.  Run it where the
reference checkout is available (gen_golden_trainer.REF_ROOT), from outside the repository root:

    PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen_golden_checkpoint_read.py

The reference's `torch_em.util.load_model` (util/util.py:408-460) and `DefaultTrainer.from_checkpoint`
(trainer/default_trainer.py:288-330) load the checkpoint on the CPU; the fixture keeps the SHA-256 of the files they read,
the class / state / counters they returned, and the prediction of the reference's own UNet2d with the loaded state on
io.pt's input.  The reference is imported through the stand-in modules of gen_golden_trainer.py (route B).
The fixture is data (what the reference returned); no reference source is copied.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import gen_golden_trainer as gg  # noqa: E402

CKPT = os.path.join(HERE, "ckpt_tiny", "checkpoints", "tiny")


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    torch.set_num_threads(4)
    torch_em = gg.import_reference()
    from torch_em.model import UNet2d
    from torch_em.trainer import DefaultTrainer
    from torch_em.util import load_model
    ck = torch.load(os.path.join(CKPT, "latest.pt"), weights_only=False, map_location="cpu")
    model = load_model(CKPT, name="latest", device="cpu")
    model = getattr(model, "_orig_mod", model)   # the reference wraps the model in torch.compile (compile_model=None: auto)
    sd = model.state_dict()
    state_equal = sorted(sd) == sorted(ck["model_state"]) and all(torch.equal(sd[k].cpu(), ck["model_state"][k].cpu())
                                                                   for k in sd)
    kw = {k: v for k, v in ck["init"]["model_kwargs"].items() if not k.endswith("_impl")}   # the reference's own block classes
    ref_model = UNet2d(**kw)
    ref_model.load_state_dict(ck["model_state"])
    ref_model.eval()
    io = torch.load(os.path.join(CKPT, "io.pt"), weights_only=False)
    with torch.no_grad():
        ref_pred = ref_model(io["x"])
    trainer = DefaultTrainer.from_checkpoint(CKPT, name="latest", device="cpu")
    out = dict(latest_sha256=np.array(sha256(os.path.join(CKPT, "latest.pt"))),
               io_sha256=np.array(sha256(os.path.join(CKPT, "io.pt"))),
               model_class=np.array(type(model).__name__), model_module=np.array(type(model).__module__),
               state_keys=np.array(sorted(sd)), state_equal=np.bool_(state_equal),
               ref_pred=ref_pred.numpy().astype(np.float32),
               trainer_iteration=np.int64(trainer._iteration), trainer_epoch=np.int64(trainer._epoch),
               optimizer_class=np.array(type(trainer.optimizer).__name__),
               optimizer_n_state=np.int64(len(trainer.optimizer.state_dict()["state"])))
    np.savez_compressed(os.path.join(HERE, "g11_reference_reads_ckpt.npz"), **out)
    print("G11:", out["model_module"], out["model_class"], "state_equal", state_equal, "iteration", out["trainer_iteration"],
          "optimizer", out["optimizer_class"], out["optimizer_n_state"])


if __name__ == "__main__":
    main()
