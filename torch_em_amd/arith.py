"""The arithmetic modes of the convolutions -- the `use_mfma` integer of the C-ABI (include/tem_hip.h: TEM_ARITH_*) -- and the
per-mode facts the Python side needs.  The C++ side keeps the same table in csrc/conv_arith.h; tests/test_cabi.py holds the two
and the header together."""
from enum import IntEnum
from typing import NamedTuple, Optional


class PackKind(IntEnum):
    """How a packed weight stores its planes: the `kind` word of a pack descriptor (csrc/conv_arith.h: TemPackKind)"""
    BF16 = 0
    F16 = 1
    F16_LO12 = 2   # fp16, lo plane x 2^12
    F16_PRE = 3    # fp16 of the weight x 2^7
    FP32 = 4       # the fp32 values in MFMA fragment order: written by the tile kernel only


class _Facts(NamedTuple):
    planes: int                 # 16-bit planes per packed weight (FP32: 64-lane groups); 0: the generic fp32 layout
    pack_kind: PackKind
    zr: str                     # profiler-tag fragment on the z-reuse kernel
    fwd: Optional[str]          # ... of the patch kernel (None: the exact-fp32 / VALU names)
    wgrad: Optional[str]        # ... of the split-precision weight gradient (None: exact fp32 / VALU)


class Arith(IntEnum):
    VALU = 0
    FP32 = 1      # exact fp32
    BF16X3 = 2
    BF16X6 = 3
    F16X3 = 4
    F16 = 5       # one fp16 term
    F16X3S = 6    # fp16x3 with prescaled operands
    BF16 = 7      # one bf16 term
    F16X2 = 8     # fp16 2x1: weight gradient only

    @property
    def facts(self) -> _Facts:
        return _FACTS[self]

    @property
    def pack(self):
        """(planes, pack kind) of the mode's weight layout"""
        return self.facts.planes, self.facts.pack_kind


_FACTS = {
    Arith.VALU: _Facts(0, PackKind.BF16, "bf16x3", None, None),
    Arith.FP32: _Facts(2, PackKind.FP32, "fp32", None, None),
    Arith.BF16X3: _Facts(2, PackKind.BF16, "bf16x3", "bf16x3", "bf16x3"),
    Arith.BF16X6: _Facts(3, PackKind.BF16, "bf16x3", "bf16x6", None),
    Arith.F16X3: _Facts(2, PackKind.F16_LO12, "f16x3", "f16x3", None),
    Arith.F16: _Facts(1, PackKind.F16, "f16", "f16", "f16"),
    Arith.F16X3S: _Facts(2, PackKind.F16_PRE, "bf16x3", "f16x3", None),
    Arith.BF16: _Facts(1, PackKind.BF16, "bf16", "bf16", "bf16"),
    Arith.F16X2: _Facts(0, PackKind.F16, "bf16x3", None, "f16x2"),   # no weight layout of its own
}


def pack_is_tiled(planes: int, k, cout: int, cin: int) -> bool:
    """Does tem_conv_pack_weights_tiles (one workgroup per 32 x 32 x taps tile) write this pack?  The gather kernel
    (tem_conv_pack_weights_batch) takes the rest -- and has no PackKind.FP32 branch."""
    return planes != 0 and k[0] * k[1] * k[2] <= 27 and cout % 16 == 0 and cin % 16 == 0
