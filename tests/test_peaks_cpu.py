"""CPU: the oracle of peak_local_max (tests/peaks_ref.py) on hand-worked cases written out, the host-side argument checks of
ops.peak_local_max / ops.peak_markers, and where watershed_from_maxima lives."""
import numpy as np
import pytest
import torch

import peaks_ref as P


def ridge():
    a = np.zeros((1, 5, 12), np.float32)
    a[0, 2, 1:11] = 1                                    # ten equal voxels: every third survives, the walk starts at x = 1
    return a


def pair(offset):
    a = np.zeros((8, 16, 16), np.float32)
    a[2, 4, 4] = a[2 + offset[0], 4 + offset[1], 4 + offset[2]] = 1
    return a


HAND = {
    "ridge": (ridge(), dict(min_distance=3, exclude_border=False), [[0, 2, 1], [0, 2, 4], [0, 2, 7], [0, 2, 10]]),
    "at_distance": (pair((0, 3, 4)), dict(min_distance=5, exclude_border=False), [[2, 4, 4], [2, 7, 8]]),   # 9 + 16 = 25: not below
    "below_distance": (pair((2, 3, 3)), dict(min_distance=5, exclude_border=False), [[2, 4, 4]]),   # 4 + 9 + 9 = 22
    "constant": (np.full((1, 6, 6), 2.5, np.float32), dict(min_distance=1, threshold_abs=0.0, exclude_border=False), []),
    "heights_first": (np.float32([[[0, 3, 0, 0, 0, 0, 5, 0, 0, 4, 0]]]), dict(min_distance=2, exclude_border=False),
                      [[0, 0, 6], [0, 0, 9], [0, 0, 1]]),
    "border": (np.float32([[[9, 0, 0, 0, 7, 0, 0, 0, 8]]]), dict(min_distance=2), [[0, 0, 4]]),
    "threshold_rel": (np.float32([[[0, 3, 0, 0, 0, 0, 5, 0, 0, 4, 0]]]), dict(min_distance=2, exclude_border=False, threshold_rel=0.7),
                      [[0, 0, 6], [0, 0, 9]]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_on_hand_worked_cases(name):
    image, kw, want = HAND[name]
    assert P.peak_local_max(image, **kw).tolist() == want
    assert P.peak_local_max(image, num_peaks=1, **kw).tolist() == want[:1]
    assert P.markers(P.peak_local_max(image, **kw), image.shape).sum() == len(want) * (len(want) + 1) // 2


def test_argument_checks_run_on_the_host():
    from torch_em_amd import ops
    x = torch.zeros(1, 1, 8, 8)
    for fn in (ops.peak_local_max, ops.peak_markers):
        for bad in (x.double(), x[0], torch.zeros(0, 1, 8, 8)):
            with pytest.raises(ValueError, match="float32 image"):
                fn(bad)
        for d in (0, 32, 1.5, True):
            with pytest.raises(ValueError, match="min_distance"):
                fn(x, min_distance=d)
        with pytest.raises(ValueError, match="exclude_border"):
            fn(x, exclude_border=-1)
        with pytest.raises(ValueError, match="num_peaks"):
            fn(x, num_peaks=0)
        with pytest.raises(ValueError, match="threshold_abs"):
            fn(x, threshold_abs="high")
        with pytest.raises(ValueError, match="rounds_per_batch"):
            fn(x, rounds_per_batch=65)
        for extra in ("footprint", "labels", "p_norm"):
            with pytest.raises(TypeError, match="not offered"):
                fn(x, **{extra: 1})
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, min_distance=2)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.peak_local_max(torch.zeros(1).expand(1, 2 ** 11, 2 ** 10, 2 ** 10))


def test_watershed_from_maxima_is_exported_by_util_only():
    import torch_em_amd.util as U
    from torch_em_amd.util import peak_watershed, segmentation
    assert U.watershed_from_maxima is peak_watershed.watershed_from_maxima and not hasattr(segmentation, "watershed_from_maxima")
    with pytest.raises(ValueError, match="one shape"):
        U.watershed_from_maxima(np.zeros((4, 4), np.float32), np.zeros((4, 5), np.float32), 2)
