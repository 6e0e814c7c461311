"""The weight-gradient dispatch queries, pinned without a GPU.

tem_conv3d_wgrad_ws, _sums_ok, _gmax_ok, _gscaled_ok, _cs_ok, _gnorm_ok and tem_conv1x1_out_bwd_ok / _ws are host code
that print the launch plan (csrc/conv.hip: wgrad_plan).  tests/golden/conv_wgrad_plan_table.json holds their answers
over the grid of scripts/conv_wgrad_plan_table.py -- shapes on both sides of every boundary of the plan x arithmetic
modes and storage types x dispatch options -- written by the library as it stood before launch and queries shared one
plan function.  Recomputed here and compared exactly: the engine sizes its workspace and decides which by-products a
weight gradient delivers from these answers, so a change is a change of what a training step computes.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))


def test_conv_wgrad_plan_table():
    import conv_wgrad_plan_table as gen
    from torch_em_amd import _lib
    lib = _lib.load()
    cus = lib.tem_device_cus()
    if cus > 0 and cus != 256:
        pytest.skip(f"the table is written for 256 compute units (or no device: the dispatch then counts 256), this device has {cus}")
    with open(gen.FIXTURE) as f:
        want = gen.unpack(json.load(f))
    before = [_lib.get_option(o) for o in gen.OPTIONS]
    got = gen.table(lib)   # (asserts that no query answered with a negative value)
    assert [_lib.get_option(o) for o in gen.OPTIONS] == before
    assert sorted(got) == sorted(want)
    bad = []
    for opts, rows in got.items():
        for shape, g, w in zip(gen.SHAPES, rows, want[opts]):
            for col in w:
                if g[col] != w[col]:
                    bad.append((opts, shape, col, g[col], w[col]))
    assert not bad, f"{len(bad)} grid points differ; (options, shape, query, got, want): {bad[:10]}"
    assert got == want
