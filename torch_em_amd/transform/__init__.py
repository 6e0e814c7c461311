"""Transforms of the MI355X path that belong to the hot path (reference torch_em/transform/)."""
from .label import (AffinityTransform, BoundaryTransform, BoundaryTransformWithIgnoreLabel, DistanceTransform,
                    MinSizeLabelTransform, NoToBackgroundBoundaryTransform, OneHotTransform, PerObjectDistanceTransform,
                    connected_components, label_consecutive, labels_to_binary)
from .raw import (AdditiveGaussianNoise, AdditivePoissonNoise, GaussianBlur, PoissonNoise, RandomContrast,
                  RandomPercentileNormalization, RawTransform, get_default_mean_teacher_augmentations, get_raw_transform, normalize,
                  normalize_percentile, standardize)
from .augmentation import (KorniaAugmentationPipeline, RandomAffine, RandomAffine3D, RandomElasticDeformation, RandomRotation,
                           RandomElasticDeformationStacked, RandomRotation3D, get_augmentations)
from .defect import EMDefectAugmentation
