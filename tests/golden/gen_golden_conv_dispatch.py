"""Fixture for tests/test_cabi.py::test_conv_dispatch_matches_the_recorded_table: what the convolution dispatch QUERIES of
libtem_hip.so answer over a grid of arithmetic modes, storage types, volumes, channel counts, kernels and layouts.  The
queries are host logic (256 CUs are assumed without a device), so this runs on a CPU.

The committed g14_conv_dispatch.npz was recorded from the library BEFORE the arithmetic modes got their one table
(csrc/conv_arith.h): the table, the predicates and the kernel selectors must reproduce it exactly.  Regenerate it only when a
dispatch decision changes on purpose:

    python tests/golden/gen_golden_conv_dispatch.py            # the in-tree library
    TEM_LIB=/path/to/other/libtem_hip.so python tests/golden/gen_golden_conv_dispatch.py
"""
import os
import sys

os.environ.setdefault("TEM_OPT_WGRAD_SUMS_MIN_MB", "0")   # as tests/conftest.py
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

FIXTURE = os.path.join(HERE, "g14_conv_dispatch.npz")

MODES = range(9)
STORAGE = (0, 1, 2)                                         # TEM_ST_F32 / _F16 / _BF16
VOLUMES = [(2, s, s, s) for s in (128, 64, 32, 16, 8)] + [(1, 1, 256, 256), (1, 6, 12, 12), (1, 4, 16, 8)]
CHANNELS = [(1, 32), (32, 32), (64, 32), (32, 64), (256, 512), (48, 32), (32, 2), (16, 32)]
KERNELS = [(3, 3, 3), (1, 3, 3), (1, 1, 1)]
# every option a dispatch decision reads: the test pins them to the recorded values
OPTIONS = ["wgrad_zs", "wgrad_zs_persist", "wgrad_sums", "wgrad_sums_min_mb", "fwd_persistent", "conv_fwd_variant",
           "conv1x1_stream", "fwd_ksplit_chunks", "wgrad_cus", "team_min_units", "zr_splitk", "zr_wide", "fp32_zr"]
NOT_ASKED = -2   # a query the grid leaves out (see wgrad_asked)


def layouts(cin, cout):
    """(x_ld, y_ld, ref_ld, misaligned): dense / padded ld with a ref / ld % 4 != 0 / a pointer off 16 bytes"""
    return [(cin, cout, 0, 0), (cin + 32, cout + 64, cout + 32, 0), (cin + 2, cout + 2, 0, 0), (cin, cout, 0, 1)]


def wgrad_asked(mode, cin, cout):
    """The weight-gradient queries of an MFMA mode are recorded for the channel counts its launch takes only: before the
    table, tem_conv3d_wgrad_ws divided by zero on the others (tests/test_cabi.py::test_wgrad_ws_answers_for_refused_channels)."""
    return mode == 0 or (cin % 32 == 0 and cout % 32 == 0)


def sweep(lib):
    """-> dict of int64 arrays, one row per (mode, storage, volume, channels, kernel)"""
    key, fam, blocks, fwd_ws, wgrad = [], [], [], [], []
    for mode in MODES:
        for st in STORAGE:
            um = mode | (st << 8) | (st << 12)
            for (n, d, h, w) in VOLUMES:
                for (cin, cout) in CHANNELS:
                    for k in KERNELS:
                        shape = (n, d, h, w, cin, cout) + k
                        key.append((mode, st) + shape)
                        fam.append([lib.tem_conv3d_fwd_kernel_ld(*shape, um, *lay) for lay in layouts(cin, cout)])
                        blocks.append([lib.tem_conv3d_fwd_stat_blocks_ld(*shape, um, *lay) for lay in layouts(cin, cout)])
                        fwd_ws.append(lib.tem_conv3d_fwd_ws(*shape, um))
                        if wgrad_asked(mode, cin, cout):
                            mfma_ch = cin % 32 == 0 and cout % 32 == 0
                            wgrad.append([lib.tem_conv3d_wgrad_ws(*shape, um), lib.tem_conv3d_wgrad_sums_ok(*shape, um),
                                          lib.tem_conv3d_wgrad_gmax_ok(*shape, um),
                                          lib.tem_conv3d_wgrad_gscaled_ok(*shape) if mfma_ch else NOT_ASKED,
                                          lib.tem_conv3d_wgrad_cs_ok(*shape, st, 64)])
                        else:
                            wgrad.append([NOT_ASKED] * 5)
    return {"key": np.asarray(key, np.int64), "fwd_kernel_ld": np.asarray(fam, np.int64),
            "fwd_stat_blocks_ld": np.asarray(blocks, np.int64), "fwd_ws": np.asarray(fwd_ws, np.int64),
            "wgrad": np.asarray(wgrad, np.int64)}   # wgrad columns: ws, sums_ok, gmax_ok, gscaled_ok, cs_ok


def main():
    from torch_em_amd import _lib
    lib = _lib.load()
    out = sweep(lib)
    out["options"] = np.asarray([_lib.get_option(o) for o in OPTIONS], np.int64)
    np.savez_compressed(FIXTURE, **out)
    fam = out["fwd_kernel_ld"]
    print(f"{FIXTURE}: {len(out['key'])} grid points, {fam.size + out['fwd_stat_blocks_ld'].size + out['fwd_ws'].size + int((out['wgrad'] != NOT_ASKED).sum())} answers; "
          f"families 0..4: {[int((fam == f).sum()) for f in range(5)]}")


if __name__ == "__main__":
    main()
