"""Instance-segmentation validation metrics on the device (reference torch_em/metric/instance_segmentation_metric.py).

The reference copies prediction and target to the host, segments there and scores with `elf.evaluation`.  Here the
prediction is segmented by the watersheds of `torch_em_amd.util.segmentation`, the contingency table of segmentation and
target is built once per sample in device memory (`ops.label_overlaps`) and every score is a fixed float64 expression of the
sums `ops.overlap_scores` takes from it -- no copy to the host and no host synchronisation, so a metric can sit in
`DefaultTrainer(metric=...)` without stalling the validation loop.

The definitions (DESIGN.md "Instance segmentation scores") follow `elf.evaluation` as its maintainers document it:
`rand_index` (adapted Rand error; label 0 is a label like any other), `variation_of_information` (split + merge, in bits,
nothing ignored), `matching` (label 0 ignored on both sides, objects matched one to one at an IoU threshold) and
`symmetric_best_dice_score`.  Parity with elf is NOT pinned: elf is not installed where this was written, so no value here
was compared with its output.  IoU thresholds below 0.5 are refused: there the matches no longer are isolated pairs and
counting them needs an assignment solver.

Not provided: the reference's `MWS*`, `EmbeddingMWS*`, `Multicut*` and `HDBScan*` classes (and their segmenters): the
mutex watershed exists as a segmenter (util/mutex_watershed.py: `mutex_watershed_segmentation`) but its metric classes are not
written, and there is no multicut solver and no HDBSCAN here.
The prefab classes sit on the two watershed segmenters that exist: `Watershed{IOU,SBD,VOI,Rand}Metric`."""
import torch
import torch.nn as nn

from .. import ops
from ..util import segmentation as useg

_STATS = ("precision", "recall", "segmentation_accuracy", "f1")


def _label_batch(x: torch.Tensor, what: str) -> torch.Tensor:
    """[N, D, H, W] or one 2-D / 3-D sample -> [N, D, H, W]; a batch of 2-D samples is [N, 1, H, W]"""
    if not torch.is_tensor(x):
        raise ValueError(f"{what}: expected a device tensor of integer labels, got {type(x).__name__}")
    if x.dim() == 4:
        return x
    if x.dim() in (2, 3):
        return x.reshape((1,) * (4 - x.dim()) + tuple(x.shape))
    raise ValueError(f"{what}: expected labels [N, D, H, W] or one 2-D / 3-D sample, got shape {tuple(x.shape)}")


def _scores(seg, target, threshold=0.5):
    what = "instance segmentation score"
    single = torch.is_tensor(seg) and seg.dim() in (2, 3)
    ov = ops.label_overlaps(_label_batch(seg, what), _label_batch(target, what))
    return ops.overlap_scores(ov, threshold), single


def _out(score: torch.Tensor, single: bool) -> torch.Tensor:
    return score[0] if single else score


class AdaptedRandError:
    """1 - 2 sum n_ab^2 / (sum n_a^2 + sum n_b^2): the adapted Rand error; label 0 counts as a label like any other.
    (seg, target): integer device tensors [N, D, H, W] or one sample -> float64 per-sample scores on the device.  Exact
    integer sums and one fixed expression: the result is the correctly rounded one."""
    def __call__(self, seg, target):
        s, single = _scores(seg, target)
        return _out(1.0 - (2.0 * s.sum_ab.to(torch.float64)) / (s.sum_a + s.sum_b).to(torch.float64), single)


class VariationOfInformation:
    """H(seg | target) + H(target | seg) in bits = (sum n_a log2 n_a + sum n_b log2 n_b - 2 sum n_ab log2 n_ab) / n;
    nothing is ignored."""
    def __call__(self, seg, target):
        s, single = _scores(seg, target)
        return _out((s.s_a + s.s_b - 2.0 * s.s_ab) / float(s.n), single)


def matching_stats(s: "ops.OverlapScores") -> dict:
    """precision, recall, segmentation_accuracy and f1 of a matching (float64 [N] each; 0 where nothing matched)"""
    tp, n_pred, n_true = (t.to(torch.int64) for t in (s.tp, s.n_pred, s.n_true))
    fp, fn = n_pred - tp, n_true - tp
    zero = torch.zeros((), dtype=torch.float64, device=tp.device)

    def ratio(num, den):
        return torch.where(tp > 0, num.to(torch.float64) / den.clamp(min=1).to(torch.float64), zero)

    return {"precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn),
            "segmentation_accuracy": ratio(tp, tp + fp + fn), "f1": ratio(2 * tp, 2 * tp + fp + fn)}


class IOUError:
    """1 - a statistic of the one-to-one matching of seg and target objects at an IoU threshold in [0.5, 1]; label 0 is
    ignored on both sides.  metric: precision | recall | segmentation_accuracy | f1."""
    def __init__(self, threshold=0.5, metric="precision"):
        if metric not in _STATS:
            raise ValueError(f"IOUError: metric must be one of {_STATS}, got {metric!r}")
        self.threshold = ops._ov_threshold(threshold)
        self.metric = metric

    def __call__(self, seg, target):
        s, single = _scores(seg, target, self.threshold)
        return _out(1.0 - matching_stats(s)[self.metric], single)


class SymmetricBestDice:
    """1 - min(best Dice of the seg objects against the target's, best Dice of the target objects against the seg's);
    label 0 is ignored, a side without objects scores 0."""
    def __call__(self, seg, target):
        s, single = _scores(seg, target)
        return _out(1.0 - torch.minimum(s.dice_pred, s.dice_true), single)


#
# Segmenters: a prediction batch [N, C, *spatial] on the device -> int32 ids [N, D, H, W]
#

def _ids4(seg: torch.Tensor) -> torch.Tensor:
    return seg if seg.dim() == 4 else seg[:, 0]   # [N, 1, H, W] is [N, D = 1, H, W] already


class ComponentsWatershed:
    """channels [foreground, boundaries] -> `util.segmentation.watershed_from_components`"""
    def __init__(self, min_size=50, threshold1=0.5, threshold2=0.5):
        self.kwargs = {"min_size": min_size, "threshold1": threshold1, "threshold2": threshold2}

    def __call__(self, input_):
        if input_.dim() not in (4, 5) or input_.shape[1] != 2:
            raise ValueError(f"ComponentsWatershed: expected [N, 2, *spatial] (foreground, boundaries), got {tuple(input_.shape)}")
        return _ids4(useg.watershed_from_components(input_[:, 1:2], input_[:, 0:1], **self.kwargs))


class DistanceWatershed:
    """channels [foreground, center distances, boundary distances] ->
    `util.segmentation.watershed_from_center_and_boundary_distances`, with its keyword arguments and defaults"""
    def __init__(self, center_distance_threshold=0.5, boundary_distance_threshold=0.5, foreground_threshold=0.5,
                 distance_smoothing=1.6, min_size=0):
        self.kwargs = {"center_distance_threshold": center_distance_threshold,
                       "boundary_distance_threshold": boundary_distance_threshold, "foreground_threshold": foreground_threshold,
                       "distance_smoothing": distance_smoothing, "min_size": min_size}

    def __call__(self, input_):
        if input_.dim() not in (4, 5) or input_.shape[1] != 3:
            raise ValueError("DistanceWatershed: expected [N, 3, *spatial] (foreground, center distances, boundary distances), "
                             f"got {tuple(input_.shape)}")
        return _ids4(useg.watershed_from_center_and_boundary_distances(input_[:, 1:2], input_[:, 2:3], input_[:, 0:1],
                                                                       **self.kwargs))


_SEGMENTERS = {"distances": DistanceWatershed, "components": ComponentsWatershed}


def _segmenter(name, kwargs):
    if name not in _SEGMENTERS:
        raise ValueError(f"segmenter must be one of {sorted(_SEGMENTERS)}, got {name!r}")
    return _SEGMENTERS[name](**kwargs)


class BaseInstanceSegmentationMetric(nn.Module):
    """segmenter: prediction batch [N, C, *spatial] -> ids; metric: (seg, target ids) -> per-sample scores.  forward
    segments the whole batch on the device, takes the ids from `target[:, -1]` (the reference's convention) and returns
    the mean of the per-sample scores as a 0-dim float64 device tensor.  The whole forward runs with host synchronisation
    forbidden (`torch.cuda.set_sync_debug_mode("error")`).  `to_numpy` is kept for the signature and ignored."""
    def __init__(self, segmenter, metric, to_numpy=False):
        super().__init__()
        self.segmenter = segmenter
        self.metric = metric
        self.to_numpy = to_numpy

    def forward(self, input_, target):
        if input_.dim() != target.dim() or input_.dim() not in (4, 5) or len(input_) != len(target):
            raise ValueError(f"expected a prediction [N, C, *spatial] and a target [N, Ct, *spatial], got {tuple(input_.shape)} and "
                             f"{tuple(target.shape)}")
        ops._req_cuda(input_, target)
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            seg = self.segmenter(input_.detach())
            ids = target.detach()[:, -1]
            if ids.dtype not in ops._OV_LABELS:
                ids = ids.to(torch.int64)
            return self.metric(seg, ids.reshape(seg.shape)).mean()
        finally:
            torch.cuda.set_sync_debug_mode(before)


#
# Prefab metrics
#

class WatershedIOUMetric(BaseInstanceSegmentationMetric):
    """1 - precision of the matching at `iou_threshold` of a watershed segmentation of the prediction.

    Args:
        segmenter: "distances" (channels foreground, center distances, boundary distances) or "components" (foreground,
            boundaries).
        iou_threshold: the IoU from which two objects match, in [0.5, 1].
        segmenter_kwargs: keyword arguments of `DistanceWatershed` / `ComponentsWatershed`."""
    def __init__(self, segmenter="distances", iou_threshold=0.5, **segmenter_kwargs):
        super().__init__(_segmenter(segmenter, segmenter_kwargs), IOUError(iou_threshold))
        self.init_kwargs = {"segmenter": segmenter, "iou_threshold": iou_threshold, **segmenter_kwargs}


class WatershedSBDMetric(BaseInstanceSegmentationMetric):
    """1 - symmetric best Dice of a watershed segmentation of the prediction (arguments: `WatershedIOUMetric`)."""
    def __init__(self, segmenter="distances", **segmenter_kwargs):
        super().__init__(_segmenter(segmenter, segmenter_kwargs), SymmetricBestDice())
        self.init_kwargs = {"segmenter": segmenter, **segmenter_kwargs}


class WatershedVOIMetric(BaseInstanceSegmentationMetric):
    """Variation of information of a watershed segmentation of the prediction (arguments: `WatershedIOUMetric`)."""
    def __init__(self, segmenter="distances", **segmenter_kwargs):
        super().__init__(_segmenter(segmenter, segmenter_kwargs), VariationOfInformation())
        self.init_kwargs = {"segmenter": segmenter, **segmenter_kwargs}


class WatershedRandMetric(BaseInstanceSegmentationMetric):
    """Adapted Rand error of a watershed segmentation of the prediction (arguments: `WatershedIOUMetric`)."""
    def __init__(self, segmenter="distances", **segmenter_kwargs):
        super().__init__(_segmenter(segmenter, segmenter_kwargs), AdaptedRandError())
        self.init_kwargs = {"segmenter": segmenter, **segmenter_kwargs}
