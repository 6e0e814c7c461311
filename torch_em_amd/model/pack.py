"""Packed convolution weights: one `PackEntry` per conv module, cached until the parameter changes.

The entry hangs on the conv (`_tem_pack`) and the conv is registered in `_PACKED_CONVS`; an optimizer step changes the
values in place (same storage, new version), and `repack_stale` then refreshes every registered entry in ONE
tem_conv_pack_weights_batch launch, written into the existing buffers (HIP-graph capture bakes their addresses in)."""
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import torch

from .. import ops
from ..arith import Arith, PackKind, pack_is_tiled

_PACKED_CONVS = weakref.WeakSet()
_PACK_BATCH = os.environ.get("TEM_PACK_BATCH", "1") != "0"
_PACK_TABLES = {}

# slot -> `transpose` of ops.pack_weights, in the order repack_stale visits them (the order of the job table)
_SLOTS = {"fwd": False, "dgrad": True, "fwd_inf": False}


def k3(k):
    k = tuple(int(v) for v in k)
    return (1,) * (3 - len(k)) + k


@dataclass(slots=True)
class Pack:
    buf: Optional[torch.Tensor]   # None: packed on first use
    mode: Arith
    used: bool = False            # since the last refresh


@dataclass(slots=True)
class PackEntry:
    weight: torch.Tensor   # the parameter the packs were made from (not the conv: no reference cycle through its attribute)
    version: int
    ptr: int
    prec: str
    wgrad: Arith      # mode of the weight gradient (which reads the parameter itself: no buffer)
    fwd: Pack
    dgrad: Pack
    fwd_inf: Pack     # no-grad forward passes in bf16x3 (engine._INFER_BF16X3)

    def get(self, slot: str) -> Pack:
        """the pack of `slot` ("fwd" / "dgrad" / "fwd_inf"), packed on first use and marked used"""
        p = getattr(self, slot)
        if p.buf is None:
            p.buf = ops.pack_weights(self.weight, transpose=_SLOTS[slot], mfma=p.mode)
        p.used = True
        return p

    def fresh(self, w, prec: str, values: bool = True) -> bool:
        """packed from the storage of `w` under `prec` (values: and from its current values)"""
        return self.ptr == w.data_ptr() and self.prec == prec and (not values or self.version == w._version)


def packed(conv, prec: str, modes) -> PackEntry:
    """The entry of `conv` under the precision mode `prec`; modes() -> (forward, data-gradient, weight-gradient) mode."""
    w = conv.weight
    ent = getattr(conv, "_tem_pack", None)
    if ent is not None and ent.fresh(w, prec):
        return ent
    if _PACK_BATCH and ent is not None and ent.fresh(w, prec, values=False):
        # only the values changed (an optimizer step): refresh EVERY stale registered conv in one launch
        repack_stale(prec)
        if ent.version == w._version:
            return ent
    mf, md, mw = modes()
    ent = PackEntry(w, w._version, w.data_ptr(), prec, mw, Pack(None, mf), Pack(None, md), Pack(None, Arith.BF16X3))
    ent.fwd.buf = ops.pack_weights(w, transpose=False, mfma=mf)
    ent.dgrad.buf = ops.pack_weights(w, transpose=True, mfma=md)
    object.__setattr__(conv, "_tem_pack", ent)
    _PACKED_CONVS.add(conv)
    return ent


def _generic_batchable(conv, k) -> bool:
    """k_pack_weights_batch writes the generic layout in items of 8 elements"""
    return _PACK_BATCH and (conv.out_channels * conv.in_channels * k[0] * k[1] * k[2]) % 8 == 0 and conv.weight.is_contiguous()


def _pack_job(conv, p: Pack, k, transpose):
    """The job (ops.pack_table) that re-packs `p` in the batched launch, or None when the tensor needs a
    tem_conv_pack_weights launch of its own."""
    planes, kind = Arith(p.mode).pack
    cout, cin = conv.out_channels, conv.in_channels
    if kind == PackKind.FP32:
        # exact fp32 (TEM_WL_MFMA): two 64-lane groups per 16-channel chunk, written by the tile kernel only
        batched = _PACK_BATCH and pack_is_tiled(planes, k, cout, cin)
    elif planes == 0:
        # the generic fp32 layout (first conv, out_conv) rides along in the batched launch
        batched = _generic_batchable(conv, k)
    else:
        batched = True
    return (conv.weight, p.buf, cout, cin, k, int(transpose), planes, kind) if batched else None


def repack_stale(prec: str, prepare_only: bool = False):
    """Re-pack the weights of every registered conv whose parameter changed in place (same storage, new version):
    all split-layout packs go into ONE tem_conv_pack_weights_batch launch, written into the existing buffers.
    prepare_only: build (and upload) the job table for the currently stale set without launching or marking anything
    fresh -- HIP-graph capture cannot upload it, so torch_em_amd/graph.py does that just before capturing."""
    jobs, rest = [], []
    # a WeakSet has no stable order: sort, so that the same stale set always gives the same table
    for conv in sorted(_PACKED_CONVS, key=lambda c: c.weight.data_ptr()):
        ent = getattr(conv, "_tem_pack", None)
        w = conv.weight
        if ent is None or not w.is_cuda or not ent.fresh(w, prec, values=False) or ent.version == w._version:
            continue
        k = k3(conv.kernel_size)
        for slot, transpose in _SLOTS.items():
            p = getattr(ent, slot)
            if p.buf is None:
                continue
            if slot == "fwd_inf" and not p.used:
                # not used since the last refresh (a model that went back to training): drop it, it is re-packed lazily
                if not prepare_only:
                    p.buf = None
                continue
            if not prepare_only:
                p.used = False
            job = _pack_job(conv, p, k, transpose)
            if job is not None:
                jobs.append(job)
            elif not prepare_only:
                rest.append((p, w, transpose))
        if not prepare_only:
            ent.version = w._version
    for p, w, transpose in rest:
        p.buf = ops.pack_weights(w, transpose=transpose, mfma=p.mode)
    by_dev = {}
    for j in jobs:  # one table / launch per device (a process normally drives one GPU)
        by_dev.setdefault(j[0].device, []).append(j)
    for dev, dj in by_dev.items():
        sig = tuple((j[0].data_ptr(), j[1].data_ptr()) for j in dj)
        tab = _PACK_TABLES.get(dev)
        if tab is None or tab[0] != sig:
            tab = _PACK_TABLES[dev] = (sig, ops.pack_table(dj))
        if prepare_only:
            continue
        with torch.cuda.device(dev):
            ops.pack_weights_batch(tab[1])


def keepalive():
    """Every device buffer a captured launch may point to: the job tables and the packed weights of all registered convs."""
    ents = [getattr(c, "_tem_pack", None) for c in list(_PACKED_CONVS)]
    return [dict(_PACK_TABLES), [(e.fwd.buf, e.dgrad.buf, e.fwd_inf.buf) for e in ents if e is not None]]


def forget(module):
    """Drop the packs of every conv under `module` (a deep copy shares the device buffers of its source: it builds its own)."""
    for mod in module.modules():
        mod.__dict__.pop("_tem_pack", None)
