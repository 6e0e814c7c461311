"""Self-training (reference torch_em/self_training): mean-teacher and FixMatch training with pseudo labels.

Built: `MeanTeacherTrainer`, `FixMatchTrainer`, `DefaultPseudoLabeler`, `ScheduledPseudoLabeler`, `DefaultSelfTrainingLoss`,
`DefaultSelfTrainingLossAndMetric`.  Not built: the UniMatchv2 trainer, the variants with invertible augmentations,
the probabilistic U-Net labeler / losses / trainer and the tensorboard logger classes.  Importable without a GPU; running
anything on CPU tensors raises, as everywhere in this package.
"""
from .fix_match import FixMatchTrainer
from .loss import DefaultSelfTrainingLoss, DefaultSelfTrainingLossAndMetric
from .mean_teacher import MeanTeacherTrainer
from .pseudo_labeling import DefaultPseudoLabeler, ScheduledPseudoLabeler

__all__ = ["DefaultPseudoLabeler", "DefaultSelfTrainingLoss", "DefaultSelfTrainingLossAndMetric", "FixMatchTrainer",
           "MeanTeacherTrainer", "ScheduledPseudoLabeler"]
