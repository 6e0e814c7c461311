"""Self-training (reference torch_em/self_training): mean-teacher, FixMatch and UniMatch v2 training with pseudo labels.

Built: `MeanTeacherTrainer`, `FixMatchTrainer`, their `*WithInvertibleAugmentations` variants and `UniMatchv2Trainer` (the
augmenters are in `torch_em_amd.transform.invertible_augmentations`), `DefaultPseudoLabeler`, `ScheduledPseudoLabeler`,
`DefaultSelfTrainingLoss`, `DefaultSelfTrainingLossAndMetric`, `SelfTrainingLossWithInvertibleAugmentations`,
`SelfTrainingLossAndMetricWithInvertibleAugmentations`, `UniMatchv2Loss`, `UniMatchv2LossAndMetric`.  Not built:
UniMatch v2's complementary dropout (it needs the UNETR decoder), the probabilistic U-Net labeler / losses / trainer and the
tensorboard logger classes.  Importable without a GPU; running anything on CPU tensors raises, as everywhere in this package.
"""
from .fix_match import FixMatchTrainer, FixMatchTrainerWithInvertibleAugmentations
from .loss import (DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric, SelfTrainingLossAndMetricWithInvertibleAugmentations,
                   SelfTrainingLossWithInvertibleAugmentations, UniMatchv2Loss, UniMatchv2LossAndMetric)
from .mean_teacher import MeanTeacherTrainer, MeanTeacherTrainerWithInvertibleAugmentations
from .pseudo_labeling import DefaultPseudoLabeler, ScheduledPseudoLabeler
from .uni_match_v2 import UniMatchv2Trainer

__all__ = ["DefaultPseudoLabeler", "DefaultSelfTrainingLoss", "DefaultSelfTrainingLossAndMetric", "FixMatchTrainer",
           "FixMatchTrainerWithInvertibleAugmentations", "MeanTeacherTrainer", "MeanTeacherTrainerWithInvertibleAugmentations",
           "ScheduledPseudoLabeler", "SelfTrainingLossAndMetricWithInvertibleAugmentations",
           "SelfTrainingLossWithInvertibleAugmentations", "UniMatchv2Loss", "UniMatchv2LossAndMetric", "UniMatchv2Trainer"]
