"""Self-training (reference torch_em/self_training): mean-teacher training with pseudo labels.

Built: `MeanTeacherTrainer`, `DefaultPseudoLabeler`, `ScheduledPseudoLabeler`, `DefaultSelfTrainingLoss`,
`DefaultSelfTrainingLossAndMetric`.  Not built: FixMatch / UniMatchv2 trainers, the variants with invertible augmentations,
the probabilistic U-Net labeler / losses / trainer and the tensorboard logger classes.  Importable without a GPU; running
anything on CPU tensors raises, as everywhere in this package.
"""
from .loss import DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric
from .mean_teacher import MeanTeacherTrainer
from .pseudo_labeling import DefaultPseudoLabeler, ScheduledPseudoLabeler

__all__ = ["DefaultPseudoLabeler", "DefaultSelfTrainingLoss", "DefaultSelfTrainingLossAndMetric", "MeanTeacherTrainer",
           "ScheduledPseudoLabeler"]
