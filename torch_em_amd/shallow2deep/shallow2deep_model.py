"""Shallow2Deep inference without leaving the device (reference torch_em/shallow2deep/shallow2deep_model.py): the ilastik
feature bank (ops.feature_bank), the random forest (ops.forest_predict) and the enhancer network.

Out of scope here: training forests (`prepare_shallow2deep*`) and their sampling strategies, `Shallow2DeepDataset`, the
`shallow2deep.transform` label transforms, `IlastikPredicter` and the bioimageio fallback of `load_model`.
"""
import os
import pickle
from functools import partial
from typing import Dict, Optional, Tuple, Union

import torch

from .. import ops
from . import filters
from .filters import _FILTER_NAMES, as_batch


def _get_filters(ndim, filters_and_sigmas):
    """The reference's filter list (prepare_shallow2deep.py:205-227): None gives the subset of the ilastik default
    features -- five filters at four scales, the structure tensor with outer_sigma = 0.5 * sigma; a list is validated."""
    if filters_and_sigmas is None:
        filts = [filters.gaussian_smoothing, filters.laplacian_of_gaussian, filters.gaussian_gradient_magnitude,
                 filters.hessian_of_gaussian_eigenvalues, filters.structure_tensor_eigenvalues]
        sigmas = [0.7, 1.6, 3.5, 5.0]
        filters_and_sigmas = [
            (filt, sigma) if i != len(filts) - 1 else (partial(filt, outer_sigma=0.5 * sigma), sigma)
            for i, filt in enumerate(filts) for sigma in sigmas
        ]
    assert isinstance(filters_and_sigmas, (list, tuple))
    for filt_and_sig in filters_and_sigmas:
        filt, sig = filt_and_sig
        assert callable(filt) or (isinstance(filt, str) and hasattr(filters, _FILTER_NAMES.get(filt, filt)))
        assert isinstance(sig, (float, tuple))
        if isinstance(sig, tuple):
            assert ndim is not None and len(sig) == ndim
            assert all(isinstance(sigg, float) for sigg in sig)
    return filters_and_sigmas


class RFWithFilters:
    """Feature computation and random-forest prediction on the device.

    Args:
        rf_path: The path to the pickled random forest (a fitted sklearn `RandomForestClassifier`).
        ndim: The dimensionality of the input data.
        filter_config: The configuration of the filters (None: the default bank).
        output_channel: The output channel(s) of the random forest prediction to keep.
    """
    def __init__(self, rf_path: str, ndim: int, filter_config: Dict,
                 output_channel: Optional[Union[Tuple[int, ...], int]] = None):
        with open(rf_path, "rb") as f:
            self.rf = pickle.load(f)
        self.filters_and_sigmas = [(_FILTER_NAMES.get(f, f) if isinstance(f, str) else f, s)
                                   for f, s in _get_filters(ndim, filter_config)]
        self.output_channel = output_channel
        self.forest = ops.pack_forest(self.rf)

    def __call__(self, x):
        """x: a 2-D or 3-D sample, numpy or a device tensor -> the forest's probabilities, numpy or a tensor on x's device:
        `(C,) + x.shape`, `x.shape` for an int `output_channel`, `(len(output_channel),) + x.shape` for a tuple."""
        t, is_np = as_batch(x)
        bank = ops.feature_bank(t, self.filters_and_sigmas)
        out = ops.forest_predict(bank, self.forest, self.output_channel)[0]
        out = out.reshape(tuple(out.shape[:out.dim() - 3]) + tuple(x.shape))
        return out.cpu().numpy() if is_np else out


class Shallow2DeepModel:
    """The enhancer applied to the random forest's prediction of the raw data.

    Args:
        checkpoint: The checkpoint of the enhancer model (a trainer checkpoint folder or a pickled module).
        rf_config: (rf_path, ndim, filter_config).  The two-element ilastik form is not supported.
        device: The device.
        rf_channel: The channel of the random forest prediction the enhancer takes.
    """
    @staticmethod
    def load_model(checkpoint, device):
        from ..util import load_model
        model = load_model(checkpoint, device=device)
        model.eval()
        return model

    @staticmethod
    def load_rf(rf_config, rf_channel=1, ilastik_multi_thread=False):
        if len(rf_config) == 3:
            rf_path, ndim, filter_config = rf_config
            assert os.path.exists(rf_path)
            return RFWithFilters(rf_path, ndim, filter_config, rf_channel)
        if len(rf_config) == 2:
            raise NotImplementedError("Shallow2DeepModel: ilastik projects (IlastikPredicter) are not supported on the device")
        raise ValueError(f"Invalid rf config: {rf_config}")

    def __init__(self, checkpoint: str, rf_config, device: str, rf_channel: Optional[int] = 1, ilastik_multi_thread: bool = False):
        self.model = self.load_model(checkpoint, device)
        self.rf_predicter = self.load_rf(rf_config, rf_channel, ilastik_multi_thread)
        self.checkpoint = checkpoint
        self.rf_config = rf_config
        self.device = device

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """x: [1, 1, *spatial] -> the enhancer's prediction; x[0, 0] goes through the bank, the forest and the enhancer on
        the device."""
        with torch.no_grad():
            out = self.rf_predicter(x[0, 0].detach().to(self.device))
        return self.model(out[None, None])

    def __getstate__(self):
        state = self.__dict__.copy()
        del state["rf_predicter"]
        return state

    def __setstate__(self, state):
        state["rf_predicter"] = self.load_rf(state["rf_config"])
        self.__dict__.update(state)
