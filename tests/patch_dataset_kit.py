"""Shared by test_patch_dataset_cpu.py and test_gpu_patch_dataset.py: the G21 fixture (tests/golden/gen_golden_patch_dataset.py)
and the numpy side of every comparison.  Nothing here touches a device."""
import json
import os

import numpy as np

from conftest import GOLDEN

_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        z = np.load(os.path.join(GOLDEN, "g21_patch_dataset.npz"))
        _FIX = {k: z[k] for k in z.files}
        _FIX["configs"] = json.loads(str(_FIX["configs"]))
    return _FIX


def sampler_of(cfg):
    from torch_em_amd.data import sampler as S
    return None if cfg["sampler"] is None else getattr(S, cfg["sampler"])(**cfg["args"])


def volumes_of(cfg):
    """(raw, labels, roi as a tuple of slices or None, the two after the roi)"""
    fx = fixture()
    raw, labels = fx[f"vol/{cfg['vol']}/raw"], fx[f"vol/{cfg['vol']}/labels"]
    roi = None if cfg.get("roi") is None else tuple(slice(a, b) for a, b in cfg["roi"])
    if roi is None:
        return raw, labels, None, raw, labels
    return raw, labels, roi, raw[((slice(None),) if cfg.get("with_channels") else ()) + roi], labels[roi]


def runs_of(name):
    """per sample of a stored configuration: (starts [attempts, rank], coins, raw crop, label crop)"""
    fx = fixture()
    counts, out, a0, c0 = fx[f"{name}/counts"], [], 0, 0
    for s, (na, nc) in enumerate(counts):
        out.append((fx[f"{name}/starts"][a0:a0 + na].astype(np.int64), fx[f"{name}/coins"][c0:c0 + nc], fx[f"{name}/raw"][s],
                    fx[f"{name}/labels"][s]))
        a0, c0 = a0 + na, c0 + nc
    return out


def crop(raw, labels, start, patch, with_channels=False):
    bb = tuple(slice(int(s), int(s) + int(p)) for s, p in zip(start, patch))
    return raw[((slice(None),) if with_channels else ()) + bb], labels[bb]


def numpy_stat(crit, raw_crop, label_crop):
    """the statistic of data/sampler.py's DeviceCriterion computed in numpy on the unpadded crop"""
    from torch_em_amd.data import sampler as S
    if crit.kind == S.COUNT_NOT_VALUE:
        return int((label_crop != crit.ids[0]).sum())
    if crit.kind == S.COUNT_NOT_FIRST:
        return int((label_crop != label_crop.flat[0]).sum())
    if crit.kind == S.INSTANCE_COUNT:
        ids, sizes = np.unique(label_crop, return_counts=True)
        return int(sum(1 for i, n in zip(ids, sizes) if n >= crit.min_size and int(i) not in crit.ids))
    if crit.kind == S.ID_COUNTS:
        listed = crit.ids if crit.per_id else tuple(dict.fromkeys(crit.ids))
        return [int((label_crop == i).sum()) for i in listed]
    if crit.kind == S.ORDER_STATISTIC:
        return getattr(np, crit.function)(raw_crop)
    raise ValueError(crit.kind)


def numpy_judge(cfg):
    """judge(items) of data/device_dataset.py's speculate() made of numpy"""
    _, _, _, raw, labels = volumes_of(cfg)
    crit = sampler_of(cfg).device_criterion()

    def judge(items):
        out = []
        for _, _, start in items:
            r, l = crop(raw, labels, start, cfg["patch"], cfg.get("with_channels", False))
            out.append(crit.met(numpy_stat(crit, r, l), l.size))
        return out
    return judge


def pad_to(a, patch):
    """np.pad constant mode to the patch on the trailing axes (the reference's ensure_patch_shape)"""
    lead = a.ndim - len(patch)
    return np.pad(a, [(0, 0)] * lead + [(0, max(0, p - s)) for p, s in zip(patch, a.shape[lead:])])
