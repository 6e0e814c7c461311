"""The forward-convolution dispatch queries, pinned without a GPU.

tem_conv3d_fwd_kernel[_ld], tem_conv3d_fwd_stat_blocks[_ld] and tem_conv3d_fwd_ws are host code that print the launch
plan (csrc/conv.hip: fwd_plan).  tests/golden/conv_fwd_plan_table.json holds their answers over the grid of
scripts/conv_fwd_plan_table.py -- shapes x arithmetic modes and storage types x layouts (wide / odd leading
dimensions, ref, misaligned, either side of the 32-bit plane limit) x dispatch options -- written by the library as it
stood before launch and queries shared one plan function.  Recomputed here and compared exactly: the engine sizes its
statistics buffers and picks its layouts from these answers, so a change is a change of what a training step computes.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))


def test_conv_fwd_plan_table():
    import conv_fwd_plan_table as gen
    from torch_em_amd import _lib
    lib = _lib.load()
    cus = lib.tem_device_cus()
    if cus > 0 and cus != 256:
        pytest.skip(f"the table is written for 256 compute units (or no device: the dispatch then counts 256), this device has {cus}")
    with open(gen.FIXTURE) as f:
        want = gen.unpack(json.load(f))
    before = [_lib.get_option(o) for o in gen.OPTIONS]
    got = gen.table(lib)
    assert [_lib.get_option(o) for o in gen.OPTIONS] == before
    assert sorted(got) == sorted(want)
    bad = []
    for opts, rows in got.items():
        for shape, g, w in zip(gen.SHAPES, rows, want[opts]):
            lays = gen.layouts(shape[2], shape[3], shape[4], shape[5])
            for mi, mode in enumerate(gen.MODES):
                if g["ws"][mi] != w["ws"][mi]:
                    bad.append((opts, shape, hex(mode), "ws", g["ws"][mi], w["ws"][mi]))
                for li, lay in enumerate(lays):
                    a, b = tuple(g["plan"][mi][2 * li:2 * li + 2]), tuple(w["plan"][mi][2 * li:2 * li + 2])
                    if a != b:
                        bad.append((opts, shape, hex(mode), lay, a, b))
    assert not bad, f"{len(bad)} grid points differ; (options, shape, use_mfma, layout | ws, got, want): {bad[:10]}"
    assert got == want
