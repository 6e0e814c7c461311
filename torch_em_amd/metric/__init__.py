"""Validation metrics on the device (reference torch_em/metric/)."""
from .cldice import clDice
from .instance_segmentation_metric import (MWS, AdaptedRandError, BaseInstanceSegmentationMetric, ComponentsWatershed,
                                           DistanceWatershed, EmbeddingMWS, EmbeddingMWSIOUMetric, EmbeddingMWSRandMetric,
                                           EmbeddingMWSSBDMetric, EmbeddingMWSVOIMetric, IOUError, MWSIOUMetric, MWSRandMetric,
                                           MWSSBDMetric, MWSVOIMetric, SymmetricBestDice, VariationOfInformation,
                                           WatershedIOUMetric, WatershedRandMetric, WatershedSBDMetric, WatershedVOIMetric)
