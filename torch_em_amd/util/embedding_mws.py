"""Instances from pixel embeddings by the mutex watershed, on the device (the reference's validation path
torch_em/metric/instance_segmentation_metric.py `EmbeddingMWS`, there through elf's `segment_embeddings_mws` on the host).

`ops.embedding_edges` turns the embeddings into the edge weights of every offset and the strided repulsive-edge mask in one
kernel (DESIGN.md "Embedding mutex watershed"), `ops.mutex_watershed` segments, `ops.merge_background_by_embedding_` merges
the segments whose mean embedding is close to the largest one's into the background, `ops.size_filter_` drops the small
ones -- no copy to the host in between.  Parity with elf is not pinned: elf is not installed where this was written."""
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..transform.label import _from_batch
from .mutex_watershed import repulsive_edge_subsampling

__all__ = ["segment_embeddings_mws"]


def segment_embeddings_mws(embeddings, offsets, delta: float, strides: Optional[Sequence[int]] = None, distance_type: str = "l2",
                           with_background: bool = False, min_size: int = 0, randomize_strides: bool = False,
                           seed: Optional[int] = None):
    """Instances from `embeddings` -- numpy or a device tensor, one sample `[E, *spatial]` or a batch `[N, E, *spatial]`, 2-D
    or 3-D as the length of the `offsets` says -- as int32 ids, `[*spatial]` or `[N, 1, *spatial]`.  The first `ndim` offsets
    are attractive, the others repulsive; the weight of an edge is `1 - (max(2 delta - d, 0) / (2 delta))^2` of the distance
    d (`distance_type` "l2" or "l1") of its ends' embeddings.  The repulsive edges are kept where every coordinate is a
    multiple of its stride (`strides`, default 4 per axis as in the reference) or, with `randomize_strides`, at that rate at
    random (`repulsive_edge_subsampling(..., seed)`).  `with_background`: the largest segment and every segment whose mean
    embedding lies within the hinge of it (p > 0.5) become 0, the others are renumbered.  `min_size > 0`: segments with fewer
    voxels become 0, the others are renumbered."""
    what = "segment_embeddings_mws"
    try:
        ndim = len(offsets[0])
    except (TypeError, IndexError):
        raise ValueError(f"{what}: offsets must be integer vectors of length 2 or 3") from None
    if ndim not in (2, 3) or len(offsets) < ndim:
        raise ValueError(f"{what}: expected at least ndim offsets of length 2 or 3 (the first ndim are attractive), got "
                         f"{len(offsets)} of length {ndim}")
    shape = tuple(embeddings.shape)
    if len(shape) not in (ndim + 1, ndim + 2):
        raise ValueError(f"{what}: expected embeddings [E, *spatial] or [N, E, *spatial] with {ndim} spatial axes, got shape {shape}")
    batched = len(shape) == ndim + 2
    sp = shape[-ndim:]
    is_np = not torch.is_tensor(embeddings)
    emb = torch.as_tensor(np.ascontiguousarray(embeddings)) if is_np else embeddings
    if not emb.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("torch_em_amd.util.embedding_mws runs on MI355X only; there is no CPU fallback")
        emb = emb.cuda()
    N = shape[0] if batched else 1
    emb5 = emb.to(torch.float32).reshape((N, shape[-ndim - 1]) + (1,) * (3 - ndim) + sp).contiguous()
    strides = [4] * ndim if strides is None else list(strides)
    aff, valid = ops.embedding_edges(emb5, offsets, delta, ndim, strides, distance_type)
    if randomize_strides:
        valid = repulsive_edge_subsampling(sp, len(offsets), ndim, strides, True, seed, batch=N, device=emb5.device).reshape(aff.shape)
    ids = ops.mutex_watershed(aff, offsets, ndim, None, valid)
    if with_background:
        ops.merge_background_by_embedding_(ids, emb5, delta)
    if min_size > 0:
        ops.size_filter_(ids, int(min_size))
    return _from_batch(ids, is_np, batched, sp, channels=False)
