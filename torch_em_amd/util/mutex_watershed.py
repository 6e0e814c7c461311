"""The mutex watershed on the device: instances from affinities (reference torch_em/util/segmentation.py:
`mutex_watershed_segmentation`, there through elf / affogato), composed without a copy to the host.

It is `ops.mutex_watershed` (DESIGN.md "Mutex watershed"): Kruskal with mutex constraints over the affinity graph -- edges by
priority descending (1 - affinity for the attractive channels, the affinity for the repulsive ones), ties by the lower edge
id; an attractive edge merges two clusters unless they are mutually exclusive, a repulsive one makes them so.  The device
runs rounds that commit, in parallel, the edges whose sequential decision is already certain, so the labels are the
sequential algorithm's bit for bit; the number of rounds depends on the data (tens for noise; 135 for cell-like affinities
at 1024^2 and 2457 at 128^3, profiles/mws_bench.txt), so the host reads two ints back per batch of rounds.  Parity with
affogato / elf is not pinned (neither is installed where this was written, and affogato's `std::sort` leaves the order of
equal weights open); the random subsampling of the repulsive edges is a device draw, not affogato's.

Inputs and results follow `torch_em_amd.util.segmentation`: numpy arrays or device tensors, one sample or a batch
`[N, 1, *spatial]`, int32 ids.  The functions live here and not in that module because its test pins that it has no
`mutex_watershed_segmentation`; `torch_em_amd.util` exports them."""
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..transform.label import _from_batch
from ..transform.raw import _check_seed, _field_seed
from .segmentation import _as_float_batch, _spatial, _thr, size_filter

__all__ = ["mutex_watershed_segmentation", "repulsive_edge_subsampling"]


def repulsive_edge_subsampling(shape: Sequence[int], n_channels: int, n_attractive: int, strides: Optional[Sequence[int]] = None,
                               randomize_strides: bool = True, seed: Optional[int] = None, batch: Optional[int] = None,
                               device="cuda") -> torch.Tensor:
    """The `edge_valid` of `ops.mutex_watershed` that subsamples the repulsive edges: bool `[n_channels, *shape]` on the
    device (`[batch, n_channels, *shape]` with `batch`) for a 2-D or 3-D `shape`.  The `n_attractive` leading channels are
    kept whole.  A repulsive edge (c, v) is kept where every coordinate of v is a multiple of its stride (`strides`, one per
    axis; default 2 each) -- or, with `randomize_strides`, with probability 1 / prod(strides), drawn from a device
    generator seeded with `seed`; `seed=None` takes a 64-bit seed from numpy's global state, so `np.random.seed` pins the
    draw.  (affogato draws with the host's `std::mt19937`: the same rate, not the same edges.)"""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"repulsive_edge_subsampling: expected a 2-D or 3-D shape, got {shape}")
    strides = [2] * len(shape) if strides is None else [int(s) for s in strides]
    if len(strides) != len(shape) or min(strides) < 1:
        raise ValueError(f"repulsive_edge_subsampling: expected {len(shape)} strides >= 1, got {strides}")
    if not 0 <= int(n_attractive) <= int(n_channels):
        raise ValueError(f"repulsive_edge_subsampling: n_attractive {n_attractive} outside 0..{n_channels}")
    seed = _check_seed(seed)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("torch_em_amd.util.mutex_watershed runs on MI355X only; there is no CPU fallback")
    lead = (int(n_channels),) if batch is None else (int(batch), int(n_channels))
    valid = torch.zeros(lead + shape, dtype=torch.bool, device=dev)
    whole = (slice(None),) * len(shape)
    att = (Ellipsis, slice(None, int(n_attractive)))
    rep = (Ellipsis, slice(int(n_attractive), None))
    valid[att + whole] = True
    if randomize_strides:
        gen = torch.Generator(device=dev)
        gen.manual_seed(_field_seed() if seed is None else seed)
        draw = torch.rand(valid[rep + whole].shape, generator=gen, device=dev, dtype=torch.float32)
        valid[rep + whole] = draw < 1.0 / float(np.prod(strides))
    else:
        valid[rep + tuple(slice(None, None, s) for s in strides)] = True
    return valid


def mutex_watershed_segmentation(foreground, affinities, offsets, min_size: int = 50, threshold: float = 0.5,
                                 strides: Optional[Sequence[int]] = None, randomize_strides: bool = True,
                                 seed: Optional[int] = None):
    """Instances from affinities by the mutex watershed inside `foreground >= threshold` (reference `:52-80`): the first
    `ndim` channels of `affinities` are attractive, the others repulsive and subsampled by `strides` (default 2 per axis)
    through `repulsive_edge_subsampling(..., randomize_strides, seed)`; the result goes through
    `size_filter(seg, min_size, hmap=affinities, with_background=True)`.  `foreground`: 2-D or 3-D, with `affinities`
    `[C, *spatial]`, or a batch `[N, 1, *spatial]` with `[N, C, *spatial]`; `offsets`: C integer vectors of length ndim.
    `randomize_strides` and `seed` are this package's: the reference always draws at random (affogato, from the host's
    generator), so its segmentation is not reproducible from a seed."""
    what = "mutex_watershed_segmentation"
    batched, sp = _spatial(foreground, what)
    sp = tuple(sp)
    lead = (int(foreground.shape[0]),) if batched else ()
    ashape = tuple(affinities.shape)
    if len(ashape) != len(lead) + 1 + len(sp) or ashape[:len(lead)] != lead or ashape[len(lead) + 1:] != sp:
        raise ValueError(f"{what}: affinities {ashape} do not match the foreground {tuple(foreground.shape)} "
                         "([C, *spatial], or [N, C, *spatial] for a batch [N, 1, *spatial])")
    C = ashape[-len(sp) - 1]
    if len(offsets) != C:
        raise ValueError(f"{what}: {len(offsets)} offsets do not match the {C} affinity channels")
    if C > ops.MWS_MAX_CHANNELS:
        raise ValueError(f"{what}: {C} channels, at most {ops.MWS_MAX_CHANNELS} supported")
    if any(len(o) != len(sp) for o in offsets):
        raise ValueError(f"{what}: offsets must have {len(sp)} entries each")
    fg, is_np = _as_float_batch(foreground)
    N = fg.shape[0]
    aff = torch.as_tensor(np.ascontiguousarray(affinities)) if not torch.is_tensor(affinities) else affinities
    aff = aff.to(fg.device).to(torch.float32)
    aff5 = aff.reshape((N, C) + (1,) * (3 - len(sp)) + sp).contiguous()
    valid = repulsive_edge_subsampling(sp, C, len(sp), strides, randomize_strides, seed, batch=N, device=fg.device)
    seg = ops.mutex_watershed(aff5, offsets, len(sp), fg >= _thr(threshold), valid.reshape(aff5.shape))
    seg = _from_batch(seg, False, batched, sp, channels=False)
    seg = size_filter(seg, min_size, hmap=aff if batched else aff.reshape((C,) + sp), with_background=True)
    return seg.cpu().numpy() if is_np else seg
