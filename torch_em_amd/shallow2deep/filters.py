"""The five filters of the Shallow2Deep feature bank on the device, under the names the reference resolves: the snake_case
ones of `bioimage_cpp.filters` and the legacy CamelCase ones of `_FILTER_NAMES`.

`f(x, sigma)` takes a 2-D or 3-D sample, numpy or a device tensor, and returns what it was given; sigma is a float or one
per axis.  The eigenvalue filters return the eigenvalues (descending) on a trailing axis, as the reference's
`response[..., c]` expects.  The definitions are scipy's (DESIGN.md "Shallow2Deep front end"): J_o = `scipy.ndimage.
gaussian_filter(x, sigma, order=o, mode="mirror", truncate=4.0)`.  Parity with `bioimage_cpp.filters` -- where it truncates
its windows and what it does at the border -- is not pinned: it is not installed where this was written.
"""
import numpy as np
import torch

from .. import ops

_FILTER_NAMES = {
    "gaussianSmoothing": "gaussian_smoothing",
    "laplacianOfGaussian": "laplacian_of_gaussian",
    "gaussianGradientMagnitude": "gaussian_gradient_magnitude",
    "hessianOfGaussianEigenvalues": "hessian_of_gaussian_eigenvalues",
    "structureTensorEigenvalues": "structure_tensor_eigenvalues",
}


def as_batch(x, device="cuda"):
    """a 2-D or 3-D sample, numpy or tensor -> (float32 device tensor [1, D, H, W], was it numpy)"""
    is_np = not torch.is_tensor(x)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device) if is_np else x.float()
    if t.dim() not in (2, 3):
        raise ValueError(f"expected a 2-D or 3-D sample, got shape {tuple(t.shape)}")
    return t.reshape((1,) * (4 - t.dim()) + tuple(t.shape)), is_np


def _wrap(name):
    op = getattr(ops, name)

    def filt(x, sigma, **kw):
        t, is_np = as_batch(x)
        out = op(t, sigma, **kw)[0]                      # [F, D, H, W]
        out = out.reshape((out.shape[0],) + tuple(x.shape))
        out = out[0] if ops.FILTER_NAMES.index(name) < 3 else out.movedim(0, -1)
        return out.cpu().numpy() if is_np else out
    filt.tem_filter = name
    filt.__name__ = filt.__qualname__ = name
    filt.__doc__ = op.__doc__
    return filt


for _camel, _snake in _FILTER_NAMES.items():
    globals()[_snake] = globals()[_camel] = _wrap(_snake)
