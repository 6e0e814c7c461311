"""Random patches of volumes that live in HBM (the reference's `SegmentationDataset` use: random crops of one large volume,
data/segmentation_dataset.py:155-216), with the rejection samplers of `data/sampler.py` judged by HIP kernels
(csrc/patch.hip) and the accepted boxes gathered straight into the device batch the trainer's pre-pass consumes.

The sampling contract (DESIGN.md "Device-resident patches"):

* global sample number `s = (batch_index * world_size + rank) * batch_size + i`; sample `s` owns
  `np.random.RandomState([seed, s])`;
* its crop is exactly what the reference's `SegmentationDataset._get_sample` returns with `np.random` in that state: with more
  than one volume first `randint(0, n_volumes)`; per attempt one `randint(0, sh - psh)` per axis where `sh - psh > 0`; after a
  failed criterion one `rand()` coin, accepted when `> p_reject`; the first accepted attempt wins; more than
  `max_sampling_attempts = 500` re-draws raise the reference's RuntimeError.

It is implemented by speculation (`speculate`): per round every unresolved sample draws `candidates_per_round` attempts as if
each one failed (box, then coin) -- up to the first accepted attempt that IS the true stream --, all candidates of the batch
are judged in one set of launches, the criteria are read back once (the round's only synchronisation), and the host picks each
sample's first accepted attempt.  Unresolved samples go on with their streams where the round left them.

Out of scope (use `TensorDataset` on the host, or the trainer's on-device arguments): `z_ext`, `pre_label_transform`,
`patch_shape=None`, label channels, 4-D data, file readers, and `raw_transform` / `label_transform` / `transform` inside the
dataset -- those are `DefaultTrainer(raw_transform=..., target_transform=..., augmentation=...)`, which run on the device batch.
"""
from math import ceil
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .sampler import COUNT_NOT_FIRST, COUNT_NOT_VALUE, ID_COUNTS, INSTANCE_COUNT, ORDER_STATISTIC, device_criterion

MAX_SAMPLING_ATTEMPTS = 500


def sample_state(seed: int, s: int) -> np.random.RandomState:
    """the random stream sample number `s` owns (seed and s below 2^32)"""
    return np.random.RandomState([int(seed), int(s)])


class Candidate:
    """One sample of a batch while it is being resolved: its stream, its volume, the `sh - psh` of every axis, and the record of
    what was tried (`starts`, and `coins`: the ones a failed criterion consumed)."""
    __slots__ = ("rs", "volume", "spans", "starts", "coins", "accepted")

    def __init__(self, rs, volume: int, spans: Sequence[int]):
        self.rs, self.volume, self.spans = rs, int(volume), tuple(int(s) for s in spans)
        self.starts, self.coins, self.accepted = [], [], None

    def draw(self, n: int, with_coins: bool):
        """n attempts as if every one failed: per attempt the box, then the coin"""
        starts, coins = [], []
        for _ in range(n):
            starts.append(tuple(self.rs.randint(0, sp) if sp > 0 else 0 for sp in self.spans))
            coins.append(self.rs.rand() if with_coins else 0.0)
        return starts, coins


def speculate(candidates: List[Candidate], judge, p_reject: Optional[float], candidates_per_round: int = 8,
              max_sampling_attempts: int = MAX_SAMPLING_ATTEMPTS) -> List[Tuple[int, ...]]:
    """Resolve every candidate to the start of its first accepted attempt and return those starts.

    `judge(items) -> sequence of bool` tells for a list of `(candidate index, volume, start)` whether the criterion is met; it
    is called once per round with the attempts of all unresolved candidates.  `p_reject=None`: no sampler -- the first box is
    taken, no coin exists.  Pure host logic: the device path passes a judge that launches kernels, a test one made of numpy."""
    if p_reject is None:
        for c in candidates:
            c.starts, _ = c.draw(1, False)
            c.accepted = c.starts[0]
        return [c.accepted for c in candidates]
    if candidates_per_round < 1:
        raise ValueError("candidates_per_round must be at least 1")
    allowed = max_sampling_attempts + 1   # the reference evaluates the first draw and max_sampling_attempts re-draws before it raises
    open_ = list(range(len(candidates)))
    while open_:
        items, drawn = [], []
        for ci in open_:
            c = candidates[ci]
            n = min(candidates_per_round, allowed - len(c.starts))
            if n <= 0:
                raise RuntimeError(f"Could not sample a valid batch in {max_sampling_attempts} attempts")
            starts, coins = c.draw(n, True)
            drawn.append((ci, starts, coins))
            items += [(ci, c.volume, st) for st in starts]
        met = list(judge(items))
        assert len(met) == len(items)
        pos, still = 0, []
        for ci, starts, coins in drawn:
            c = candidates[ci]
            for k, st in enumerate(starts):
                c.starts.append(st)
                if met[pos + k]:
                    c.accepted = st
                    break
                c.coins.append(coins[k])
                if coins[k] > p_reject:
                    c.accepted = st
                    break
            pos += len(starts)
            if c.accepted is None:
                still.append(ci)
        open_ = still
    return [c.accepted for c in candidates]


_RAW_NATIVE = (torch.uint8, torch.uint16, torch.int16, torch.float32)
_LABEL_NATIVE = (torch.uint8, torch.uint16, torch.int32, torch.int64)
_NP_OF = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.int16: np.int16, torch.float32: np.float32}


def _as_tensor(a) -> torch.Tensor:
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


class DeviceSegmentationDataset:
    """Raw and label volumes resident on `device`; a sample is a random crop of `patch_shape` that `sampler` accepts.

    raw / labels: an array or tensor, or equally long lists of them (a sample of several volumes first draws
        `randint(0, n_volumes)`); 2-D or 3-D data, raw with a leading channel axis if `with_channels`.  Raw is kept as uint8 /
        uint16 / int16 / float32 (anything else is cast to float32 once), labels as uint8 / uint16 / int32 / int64 (other
        integer types are widened; float labels are refused).
    patch_shape: one entry per data axis; with `ndim` one less than that, the leading entry must be 1 and is squeezed from the
        batch (reference :211-214).
    sampler: one of `data/sampler.py` that the device can judge (`device_criterion()`); others raise NotImplementedError.
    roi: a tuple of plain slices (step 1) applied to every volume before it is copied.
    with_padding: a volume axis shorter than the patch is filled with ZEROS (`np.pad` constant mode, the reference's
        `ensure_patch_shape`; `TensorDataset` reflects instead).  False is refused: a batch needs one shape.
    Batches come from `DevicePatchLoader`: raw `dtype` [B, C, ...], labels `label_dtype` [B, 1, ...], on the device.

    Not supported (see the module docstring): z_ext, pre_label_transform, patch_shape=None, label channels, 4-D data, file
    readers, transforms inside the dataset.  With a histogram sampler (MinInstanceSampler, MinSemanticLabelForegroundSampler,
    list background ids) the labels are renumbered densely once (`ops.pod_ids`), which costs one synchronisation here."""
    max_sampling_attempts = MAX_SAMPLING_ATTEMPTS

    @staticmethod
    def compute_len(shape, patch_shape):
        return 1 if patch_shape is None else ceil(np.prod([float(sh / csh) for sh, csh in zip(shape, patch_shape)]))

    def __init__(self, raw, labels, patch_shape, sampler=None, n_samples=None, roi=None, with_channels=False, with_padding=True,
                 dtype=torch.float32, label_dtype=torch.int64, device="cuda", ndim=None):
        from .. import ops
        if patch_shape is None:
            raise NotImplementedError("DeviceSegmentationDataset needs a patch_shape (whole-volume samples: TensorDataset)")
        if not with_padding:
            raise NotImplementedError("DeviceSegmentationDataset pads to the patch (a batch has one shape); with_padding=False: TensorDataset")
        raws = list(raw) if isinstance(raw, (list, tuple)) else [raw]
        labs = list(labels) if isinstance(labels, (list, tuple)) else [labels]
        if len(raws) != len(labs) or not raws:
            raise ValueError(f"Number of raw and label volumes does not match: {len(raws)}, {len(labs)}")
        self.patch_shape = tuple(int(p) for p in patch_shape)
        rank = len(self.patch_shape)
        self._ndim = rank if ndim is None else int(ndim)
        if rank not in (2, 3) or self._ndim not in (rank, rank - 1) or self._ndim < 2:
            raise ValueError(f"2-D or 3-D data only: patch_shape {self.patch_shape}, ndim {self._ndim}")
        if self._ndim == rank - 1 and self.patch_shape[0] != 1:
            raise ValueError(f"the extra leading entry of patch_shape {self.patch_shape} must be 1")
        self.sampler, self.criterion = sampler, device_criterion(sampler)
        self.with_channels, self.with_padding, self.roi = with_channels, with_padding, roi
        self.dtype, self.label_dtype, self.device = dtype, label_dtype, torch.device(device)
        if roi is not None:
            roi = tuple(roi)
            if len(roi) != rank or any(not isinstance(s, slice) or s.step not in (None, 1) for s in roi):
                raise ValueError(f"roi must be a tuple of {rank} plain slices")
        rv, lv = [], []
        for r, l in zip(raws, labs):
            r, l = _as_tensor(r), _as_tensor(l)
            if r.dim() != rank + (1 if with_channels else 0) or l.dim() != rank:
                raise ValueError(f"expected {rank}-D volumes (raw with a channel axis: {with_channels}); label channels and 4-D data are not supported")
            if roi is not None:
                r, l = r[((slice(None),) if with_channels else ()) + roi], l[roi]
            if tuple(r.shape[-rank:]) != tuple(l.shape) or l.numel() == 0:
                raise ValueError(f"Image and label shape does not match: {tuple(r.shape)}, {tuple(l.shape)}")
            if l.dtype.is_floating_point or l.dtype == torch.bool:
                raise ValueError(f"integer labels expected, got {l.dtype}")
            if r.dtype not in _RAW_NATIVE:
                r = r.to(torch.float32)
            if l.dtype not in _LABEL_NATIVE:
                l = l.to(torch.int32 if l.dtype in (torch.int8, torch.int16) else torch.int64)
            r = r if with_channels else r[None]
            shape4 = (1,) * (3 - rank) + tuple(l.shape)
            rv.append(r.reshape(r.shape[0], *shape4).contiguous().to(self.device))
            lv.append(l.reshape(1, *shape4).contiguous().to(self.device))
        if len({v.dtype for v in rv}) != 1 or len({v.dtype for v in lv}) != 1 or len({v.shape[0] for v in rv}) != 1:
            raise ValueError("all raw volumes share one dtype and channel count, all label volumes one dtype")
        self.shapes = [tuple(v.shape[1:]) for v in lv]          # (D, H, W) per volume, D = 1 for 2-D data
        self._patch3 = (1,) * (3 - rank) + self.patch_shape
        self.shape = tuple(lv[0].shape[4 - rank:])
        self._len = self.compute_len(self.shape, self.patch_shape) if n_samples is None else int(n_samples)
        self.raw, self.labels = ops.PatchVolumes(rv), ops.PatchVolumes(lv)
        self._raw_np = _NP_OF[rv[0].dtype]
        self._ids = self._sel = None
        if self.criterion is not None and self.criterion.needs_histogram:
            self._build_ids(ops, lv)
        torch.cuda.synchronize(self.device)

    # ---- construction of the dense ids (histogram samplers only) ----
    def _build_ids(self, ops, label_volumes):
        dense, origs = [], []
        for l in label_volumes:
            ids = ops.pod_ids(l.to(torch.int64), False, 0)                   # [1, D, H, W] int32: 0 -> 0, the rest 1..n ascending
            orig = torch.zeros((int(ids.max()) + 1,), dtype=torch.int64, device=l.device)   # the synchronisation
            orig[ids.view(-1).long()] = l.view(-1).to(torch.int64)
            dense.append(ids)
            origs.append(orig.cpu().numpy())
        if len(dense) > 1:   # one numbering for all volumes: 0, then the union of the original ids in ascending order
            union = np.unique(np.concatenate([o[1:] for o in origs]))
            union = np.concatenate([[0], union[union != 0]])
            for v, (ids, orig) in enumerate(zip(dense, origs)):
                lut = torch.from_numpy(np.searchsorted(union[1:], orig[1:]).astype(np.int32) + 1)
                lut = torch.cat([torch.zeros(1, dtype=torch.int32), lut]).to(ids.device)
                dense[v] = lut[ids.long()].contiguous()
            origs = [union]
        self.original_ids = origs[0]                                         # dense id -> original label id (host)
        self.n_ids = int(len(self.original_ids))
        self._ids = ops.PatchVolumes(dense)
        crit, dense_of = self.criterion, {int(o): d for d, o in enumerate(self.original_ids)}
        if crit.kind == INSTANCE_COUNT:
            sel = np.zeros(self.n_ids, dtype=np.int32)
            sel[[dense_of[i] for i in crit.ids if i in dense_of]] = 1
        else:
            listed = crit.ids if crit.per_id else tuple(dict.fromkeys(crit.ids))   # np.isin counts a repeated id once
            if not listed:
                raise ValueError("the sampler lists no ids")
            sel = np.array([dense_of.get(i, -1) for i in listed], dtype=np.int32)
        self._sel = torch.from_numpy(sel).to(self.device)

    # ---- the reference's dataset interface ----
    def __len__(self):
        return self._len

    @property
    def ndim(self):
        return self._ndim

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in ("raw", "labels", "_ids", "_sel"):   # the volumes stay behind: a checkpoint holds the configuration only
            state[k] = None
        return state

    def _check_alive(self):
        if self.raw is None or self.labels is None:
            raise RuntimeError("DeviceSegmentationDataset has not been properly deserialized.")

    # ---- sampling ----
    def candidate(self, seed: int, s: int) -> Candidate:
        rs = sample_state(seed, s)
        v = int(rs.randint(0, len(self.shapes))) if len(self.shapes) > 1 else 0
        rank = len(self.patch_shape)
        return Candidate(rs, v, [sh - p for sh, p in zip(self.shapes[v][3 - rank:], self.patch_shape)])

    def _boxes(self, volumes, starts) -> np.ndarray:
        """int64 [M, 7]: the starts (one entry per data axis) as boxes clipped to their volumes"""
        out = np.zeros((len(starts), 7), dtype=np.int64)
        rank = len(self.patch_shape)
        for m, (v, st) in enumerate(zip(volumes, starts)):
            st3 = (0,) * (3 - rank) + tuple(int(s) for s in st)
            out[m, 0], out[m, 1:4] = v, st3
            out[m, 4:7] = [min(p, sh - s0) for p, sh, s0 in zip(self._patch3, self.shapes[v], st3)]
        return out

    def judge(self, items) -> List[bool]:
        """criterion met? for `(candidate index, volume, start)` items: one set of launches, one read-back"""
        from .. import ops
        self._check_alive()
        crit = self.criterion
        boxes = self._boxes([it[1] for it in items], [it[2] for it in items])
        sizes = (boxes[:, 4] * boxes[:, 5] * boxes[:, 6]).tolist()
        if crit.kind in (COUNT_NOT_VALUE, COUNT_NOT_FIRST):
            value = crit.ids[0] if crit.kind == COUNT_NOT_VALUE else 0
            stats = ops.patch_count(self.labels, boxes, value).cpu().numpy()[:, 0 if crit.kind == COUNT_NOT_VALUE else 1]
        elif crit.kind == INSTANCE_COUNT:
            hist = ops.patch_hist(self._ids, boxes, self.n_ids)
            stats = ops.patch_hist_instances(hist, self._sel, crit.min_size).cpu().numpy()
        elif crit.kind == ID_COUNTS:
            hist = ops.patch_hist(self._ids, boxes, self.n_ids)
            stats = ops.patch_hist_listed(hist, self._sel).cpu().numpy()
        elif crit.kind == ORDER_STATISTIC:
            stats = self._intensities(ops, boxes, crit.function)
        else:
            raise ValueError(crit.kind)
        return [crit.met(st, n) for st, n in zip(stats, sizes)]

    def _intensities(self, ops, boxes, function):
        """np.median / np.max / np.min of every raw box, exactly: the boxes are gathered unpadded (grouped by their shape), the
        ranks come from `ops.row_order_statistics`, and numpy averages the two middle values of an even count on the host in
        the volume's dtype, as `np.median` would."""
        groups = {}
        for m, b in enumerate(boxes):
            groups.setdefault(tuple(b[4:7].tolist()), []).append(m)
        parts, order = [], []
        for dims, rows in groups.items():
            x = ops.patch_gather(self.raw, boxes[rows], dims, torch.float32)
            L = x[0].numel()
            ranks = {"max": [L - 1, L - 1], "min": [0, 0], "median": [(L - 1) // 2, L // 2]}[function]
            parts.append(ops.row_order_statistics(x.view(len(rows), L), ranks))
            order += rows
        vals = torch.cat(parts).cpu().numpy().astype(self._raw_np)   # float32 holds every raw dtype exactly
        out = [None] * len(order)
        for row, m in zip(vals, order):
            out[m] = np.mean(row) if function == "median" else row[0]
        return out

    def gather(self, volumes, starts):
        """the batch (raw [B, C, ...] `dtype`, labels [B, 1, ...] `label_dtype`) of the boxes at `starts`: two launches"""
        from .. import ops
        self._check_alive()
        boxes = self._boxes(volumes, starts)
        direct = self.label_dtype in (torch.float32, torch.int32, torch.int64)
        x = ops.patch_gather(self.raw, boxes, self._patch3, torch.float32)
        y = ops.patch_gather(self.labels, boxes, self._patch3, self.label_dtype if direct else torch.int64)
        if len(self.patch_shape) == 2:
            x, y = x[:, :, 0], y[:, :, 0]
        elif self._ndim == 2:
            x, y = x.squeeze(2), y.squeeze(2)
        return (x if self.dtype == torch.float32 else x.to(self.dtype)), (y if direct else y.to(self.label_dtype))


class DevicePatchLoader:
    """Yields device batches `(x, y)` of a `DeviceSegmentationDataset`; takes the place of a `torch.utils.data.DataLoader` as
    `DefaultTrainer(train_loader=...)` (`DevicePrefetcher` passes device tensors through, the trainer's `raw_transform`,
    `target_transform` and `augmentation` then run on them).  Batch `batch_index` of rank `rank` holds the samples
    `(batch_index * world_size + rank) * batch_size + i`; `batch_index` counts on over the epochs, so every epoch sees new
    crops and a run is reproducible from `seed` alone.  The work runs on a stream of the loader's own and the batch is complete
    when it is yielded: any stream may consume it."""
    shuffle = True

    def __init__(self, dataset: DeviceSegmentationDataset, batch_size: int, seed: int, candidates_per_round: int = 8, rank: int = 0,
                 world_size: int = 1):
        if batch_size < 1 or candidates_per_round < 1 or not 0 <= rank < world_size:
            raise ValueError("batch_size, candidates_per_round >= 1 and 0 <= rank < world_size")
        self.dataset, self.batch_size, self.seed = dataset, int(batch_size), int(seed)
        self.candidates_per_round, self.rank, self.world_size = int(candidates_per_round), int(rank), int(world_size)
        self.batch_index = 0
        self.last_candidates = None   # the Candidate records of the batch yielded last (what was tried): for tests and logs
        self._stream = None

    def __len__(self):
        return ceil(len(self.dataset) / (self.batch_size * self.world_size))

    def batch(self, batch_index: int):
        ds = self.dataset
        ds._check_alive()
        s0 = (batch_index * self.world_size + self.rank) * self.batch_size
        cands = [ds.candidate(self.seed, s0 + i) for i in range(self.batch_size)]
        if self._stream is None:
            self._stream = torch.cuda.Stream(ds.device)
        caller = torch.cuda.current_stream(ds.device)
        with torch.cuda.stream(self._stream):
            p_reject = None if ds.criterion is None else float(ds.sampler.p_reject)
            starts = speculate(cands, ds.judge, p_reject, self.candidates_per_round, ds.max_sampling_attempts)
            x, y = ds.gather([c.volume for c in cands], starts)
            self._stream.synchronize()
        for t in (x, y):
            t.record_stream(caller)
        self.last_candidates = cands
        return x, y

    def __iter__(self):
        for _ in range(len(self)):
            index = self.batch_index
            self.batch_index += 1
            yield self.batch(index)
