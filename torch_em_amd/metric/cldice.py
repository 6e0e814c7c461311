"""The clDice score as a metric, on the device (reference torch_em/metric/cldice.py; clDice: https://arxiv.org/abs/2003.07311)."""
import numpy as np
import torch

from ..loss.cldice import SoftSkeletonize


def cl_score(img: torch.Tensor, skel: torch.Tensor) -> torch.Tensor:
    """The skeleton volume intersection sum(img * skel) / sum(skel), accumulated in float64"""
    skel = skel.to(torch.float64)
    return (img.to(torch.float64) * skel).sum() / skel.sum()


def _image(x, what: str) -> torch.Tensor:
    t = torch.as_tensor(np.ascontiguousarray(x)) if not torch.is_tensor(x) else x
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("torch_em_amd.metric.clDice runs on MI355X only; there is no CPU fallback")
        t = t.cuda()
    if t.dim() in (2, 3):     # one image: batch and channel axes for SoftSkeletonize, as the reference adds them
        t = t[None, None]
    if t.dim() not in (4, 5):
        raise ValueError(f"clDice: expected a 2-D or 3-D {what} or a batch [N, C, *spatial], got shape {tuple(x.shape)}")
    return t.to(torch.float32).contiguous()


def clDice(input_, target, skeletonize_method="soft", num_iter=5):
    """The clDice score between a binary input and target: 2 * Tprec * Tsens / max(Tprec + Tsens, 1e-7) with
    Tprec = |skel(input) * target| / |skel(input)| and Tsens = |skel(target) * input| / |skel(target)| (the reference's
    formula and guard), over `loss.SoftSkeletonize(num_iter)` on the device; the sums of the float32 skeletons and the
    formula are float64.  One image (2-D or 3-D) or a batch [N, C, *spatial] scored as a whole; numpy arrays are moved to
    the device.  Returns a 0-dim float64 device tensor; nothing is read back.  Like the reference's, an empty skeleton
    gives nan.  `skeletonize_method="skimage"` (topological thinning) is not provided."""
    if tuple(input_.shape) != tuple(target.shape):
        raise ValueError(f"Expect input and target of same shape, got: {tuple(input_.shape)}, {tuple(target.shape)}.")
    if skeletonize_method == "skimage":
        raise NotImplementedError("clDice: skeletonize_method='skimage' needs topological thinning, which is not provided; use 'soft'")
    if skeletonize_method != "soft":
        raise ValueError("Unknown option for `skeletonize_method`. Valid options are `skimage` and `soft`.")
    x, t = _image(input_, "input"), _image(target, "target")
    soft_skeletonize = SoftSkeletonize(num_iter=num_iter)
    with torch.no_grad():
        skel_input, skel_target = soft_skeletonize(x), soft_skeletonize(t)
    t_prec = cl_score(t, skel_input)
    t_sens = cl_score(x, skel_target)
    return 2.0 * (t_prec * t_sens) / torch.clamp(t_prec + t_sens, min=1e-7)
