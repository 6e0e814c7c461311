"""In-memory datasets for the MI355X path (harness; reference torch_em/data/tensor_dataset.py), the rejection samplers
(reference data/sampler.py) and the device-resident patch dataset that judges them with HIP kernels."""
from .device_dataset import DevicePatchLoader, DeviceSegmentationDataset
from .sampler import (MinForegroundSampler, MinInstanceSampler, MinIntensitySampler, MinNoToBackgroundBoundarySampler,
                      MinSemanticLabelForegroundSampler, MinTwoInstanceSampler)
from .tensor_dataset import TensorDataset
