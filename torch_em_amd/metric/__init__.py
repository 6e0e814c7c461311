"""Validation metrics on the device (reference torch_em/metric/)."""
from .cldice import clDice
from .instance_segmentation_metric import (AdaptedRandError, BaseInstanceSegmentationMetric, ComponentsWatershed,
                                           DistanceWatershed, IOUError, SymmetricBestDice, VariationOfInformation,
                                           WatershedIOUMetric, WatershedRandMetric, WatershedSBDMetric, WatershedVOIMetric)
