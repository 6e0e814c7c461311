"""Rejection samplers (reference torch_em/data/sampler.py): callables `sampler(x, y) -> bool` that a dataset asks whether
a crop is worth training on.  Two faces per class:

* `__call__(x, y)` on numpy arrays is the reference's decision, quirks included: the rejection coin is
  `np.random.rand() > p_reject`, drawn only when the criterion fails and drawn also at `p_reject=1.0`;
  `MinSemanticLabelForegroundSampler(min_fraction_per_id=False)` compares a voxel COUNT with `min_fraction`.
* `device_criterion()` describes the criterion to the device-resident path (`data/device_dataset.py`) as a
  `DeviceCriterion` record: which box statistic the kernels of csrc/patch.hip have to produce and how the host turns it into
  "criterion met".  The coin stays on the host.  A sampler the kernels cannot judge raises `NotImplementedError` there.
"""
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import numpy as np

# statistics of a box the device path can produce (DeviceCriterion.kind)
COUNT_NOT_VALUE = "count_not_value"   # voxels of the label box != ids[0]                       (tem_patch_count, word 0)
COUNT_NOT_FIRST = "count_not_first"   # voxels of the label box != its first voxel               (tem_patch_count, word 1)
ID_COUNTS = "id_counts"               # voxels per listed label id                               (tem_patch_hist + _reduce)
INSTANCE_COUNT = "instance_count"     # label ids with >= max(min_size, 1) voxels, not excluded  (tem_patch_hist + _reduce)
ORDER_STATISTIC = "order_statistic"   # "median" / "max" / "min" of the raw box                  (tem_patch_gather + row select)

_ON_HOST = "use TensorDataset (the host path) with this sampler"


@dataclass(frozen=True)
class DeviceCriterion:
    """What the device has to compute for one sampler, and the host's rule on the numbers it reads back."""
    kind: str
    ids: tuple = ()                 # label ids (original values): the background id, the listed ids, the excluded ids
    threshold: float = 0.0          # min_fraction / min_intensity / min_num_instances
    min_size: int = 1               # INSTANCE_COUNT
    per_id: bool = False            # ID_COUNTS: every id's fraction against the threshold (else: the summed count)
    complement: bool = False        # ID_COUNTS: the statistic is the fraction of voxels NOT in `ids`
    function: str = ""              # ORDER_STATISTIC

    @property
    def needs_histogram(self) -> bool:
        return self.kind in (ID_COUNTS, INSTANCE_COUNT)

    def met(self, stat, size: int) -> bool:
        """The criterion on the statistic of one box of `size` label voxels: an int (counts), a sequence of ints (ID_COUNTS) or
        the intensity (ORDER_STATISTIC).  Written with the reference's own expressions, so float rounding agrees."""
        if self.kind == COUNT_NOT_VALUE:
            return int(stat) / float(size) > self.threshold
        if self.kind == COUNT_NOT_FIRST:
            return int(stat) > 0
        if self.kind == INSTANCE_COUNT:
            return int(stat) >= self.threshold
        if self.kind == ID_COUNTS:
            counts = [int(c) for c in stat]
            if self.complement:
                return (size - sum(counts)) / float(size) > self.threshold
            if self.per_id:
                return all(c / float(size) > self.threshold for c in counts)
            return sum(counts) > self.threshold
        if self.kind == ORDER_STATISTIC:
            return bool(stat > self.threshold)
        raise ValueError(self.kind)


def _coin(p_reject: float) -> bool:
    return bool(np.random.rand() > p_reject)


class MinForegroundSampler:
    """Accept when more than `min_fraction` of the label voxels are foreground (not `background_id`, an int or a list)."""

    def __init__(self, min_fraction: float, background_id: int = 0, p_reject: float = 1.0):
        self.min_fraction, self.background_id, self.p_reject = min_fraction, background_id, p_reject

    def __call__(self, x: np.ndarray, y: Optional[np.ndarray] = None) -> bool:
        y = x if y is None else y   # usable on raw data alone, to skip regions that were not imaged
        if isinstance(self.background_id, int):
            foreground = np.sum(y != self.background_id)
        else:
            foreground = np.sum(~np.isin(y, self.background_id))
        return True if foreground / float(y.size) > self.min_fraction else _coin(self.p_reject)

    def device_criterion(self) -> DeviceCriterion:
        if isinstance(self.background_id, (int, np.integer)):
            return DeviceCriterion(COUNT_NOT_VALUE, ids=(int(self.background_id),), threshold=self.min_fraction)
        return DeviceCriterion(ID_COUNTS, ids=tuple(int(i) for i in self.background_id), threshold=self.min_fraction, complement=True)


class MinSemanticLabelForegroundSampler:
    """Accept when the voxels of `semantic_ids` exceed `min_fraction`: per id as a fraction (`min_fraction_per_id`), or --
    the reference's behaviour, kept -- all of them together as a COUNT."""

    def __init__(self, semantic_ids: List[int], min_fraction: float, min_fraction_per_id: bool = False, p_reject: float = 1.0):
        self.semantic_ids, self.min_fraction = semantic_ids, min_fraction
        self.p_reject, self.min_fraction_per_id = p_reject, min_fraction_per_id

    def __call__(self, x: np.ndarray, y: np.ndarray) -> bool:
        if self.min_fraction_per_id:
            values = [np.sum(np.isin(y, i)) / float(y.size) for i in self.semantic_ids]
        else:
            values = [np.sum(np.isin(y, self.semantic_ids))]
        return True if all(v > self.min_fraction for v in values) else _coin(self.p_reject)

    def device_criterion(self) -> DeviceCriterion:
        return DeviceCriterion(ID_COUNTS, ids=tuple(int(i) for i in self.semantic_ids), threshold=self.min_fraction,
                               per_id=bool(self.min_fraction_per_id))


class MinIntensitySampler:
    """Accept when `function(x)` of the raw crop exceeds `min_intensity`; `function` is a callable or the name of a numpy one."""

    def __init__(self, min_intensity: int, function: Union[str, Callable] = "median", p_reject: float = 1.0):
        self.min_intensity = min_intensity
        self.function = getattr(np, function) if isinstance(function, str) else function
        assert callable(self.function)
        self.p_reject = p_reject

    def __call__(self, x: np.ndarray, y: Optional[np.ndarray] = None) -> bool:
        return True if self.function(x) > self.min_intensity else _coin(self.p_reject)

    def device_criterion(self) -> DeviceCriterion:
        for name in ("median", "max", "min"):   # order statistics: exact on the device
            if self.function is getattr(np, name):
                return DeviceCriterion(ORDER_STATISTIC, threshold=self.min_intensity, function=name)
        raise NotImplementedError("MinIntensitySampler on the device judges order statistics only (function 'median', 'max' or "
                                  f"'min'), not {getattr(self.function, '__name__', self.function)!r}; {_ON_HOST}")


class MinInstanceSampler:
    """Accept when the labels hold at least `min_num_instances` ids (background counts as one) that have at least `min_size`
    voxels and are not in `exclude_ids`."""

    def __init__(self, min_num_instances: int = 2, p_reject: float = 1.0, min_size: Optional[int] = None,
                 exclude_ids: Optional[List[int]] = None):
        self.min_num_instances, self.p_reject, self.min_size, self.exclude_ids = min_num_instances, p_reject, min_size, exclude_ids
        if exclude_ids is not None:
            assert isinstance(exclude_ids, list)

    def __call__(self, x: np.ndarray, y: np.ndarray) -> bool:
        ids, sizes = np.unique(y, return_counts=True)
        if self.min_size is not None:
            ids = ids[sizes >= self.min_size]
        if self.exclude_ids is not None:
            ids = [i for i in ids if i not in self.exclude_ids]
        return True if len(ids) >= self.min_num_instances else _coin(self.p_reject)

    def device_criterion(self) -> DeviceCriterion:
        return DeviceCriterion(INSTANCE_COUNT, ids=tuple(int(i) for i in (self.exclude_ids or ())), threshold=self.min_num_instances,
                               min_size=max(int(self.min_size or 0), 1))


class MinTwoInstanceSampler:
    """Accept when the labels hold two different values: any voxel differs from the first (no `np.unique`)."""

    def __init__(self, p_reject: float = 1.0):
        self.p_reject = p_reject

    def __call__(self, x: np.ndarray, y: np.ndarray) -> bool:
        return True if (y != y.flat[0]).any() else _coin(self.p_reject)

    def device_criterion(self) -> DeviceCriterion:
        return DeviceCriterion(COUNT_NOT_FIRST)


class MinNoToBackgroundBoundarySampler:
    """Accept when more than `min_fraction` of `trafo(y)` is boundary after its mask label is folded into the background
    (for training on pseudo labels with boundaries to the background ignored).  Host only: `trafo` is arbitrary code."""

    def __init__(self, trafo, min_fraction: float = 0.01, p_reject: float = 1.0):
        self.trafo, self.bg_label, self.mask_label = trafo, trafo.bg_label, trafo.mask_label
        self.min_fraction, self.p_reject = min_fraction, p_reject

    def __call__(self, x: np.ndarray, y: np.ndarray) -> bool:
        boundaries = self.trafo(y)
        boundaries[boundaries == self.mask_label] = self.bg_label
        fraction = np.sum(boundaries != self.bg_label) / float(boundaries.size)
        return True if fraction > self.min_fraction else _coin(self.p_reject)

    def device_criterion(self) -> DeviceCriterion:
        raise NotImplementedError(f"MinNoToBackgroundBoundarySampler runs a label transform per candidate; {_ON_HOST}")


def device_criterion(sampler) -> Optional[DeviceCriterion]:
    """The record of `sampler` (None for no sampler); anything that cannot describe itself is refused."""
    if sampler is None:
        return None
    describe = getattr(sampler, "device_criterion", None)
    if describe is None:
        raise NotImplementedError(f"{type(sampler).__name__} is an arbitrary callable the device cannot judge; {_ON_HOST}")
    return describe()
