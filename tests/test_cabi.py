"""CPU: the C-ABI shared library loads and exports every symbol include/tem_hip.h declares
(no compute calls -- there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "tem_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tem_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_entry_points():
    syms = _declared_symbols()
    assert "tem_conv3d_fwd" in syms and "tem_dice_sums" in syms and len(syms) >= 25


def test_library_exports_every_declared_symbol():
    from torch_em_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in _declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"not exported: {missing}"


def test_ctypes_signatures_cover_the_header():
    from torch_em_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared_symbols()


def _header_defines(prefix):
    text = open(os.path.join(ROOT, "include", "tem_hip.h")).read()
    return dict(re.findall(r"^#define (%s\w+) (\w+)" % prefix, text, flags=re.M))


def test_arith_enum_matches_the_header():
    """One numbering of the arithmetic modes: arith.Arith == TEM_ARITH_* of the header, and every TEM_WL_* layout is
    DEFINED as the mode it serves."""
    from torch_em_amd.arith import Arith
    modes = {k[len("TEM_ARITH_"):]: int(v) for k, v in _header_defines("TEM_ARITH_").items()}
    assert modes == {m.name: int(m) for m in Arith} and sorted(modes.values()) == list(range(9))
    layouts = _header_defines("TEM_WL_")
    assert layouts == {"TEM_WL_GENERIC": "TEM_ARITH_VALU", "TEM_WL_MFMA": "TEM_ARITH_FP32", "TEM_WL_BF16X3": "TEM_ARITH_BF16X3",
                       "TEM_WL_BF16X6": "TEM_ARITH_BF16X6", "TEM_WL_F16X3": "TEM_ARITH_F16X3", "TEM_WL_F16": "TEM_ARITH_F16",
                       "TEM_WL_F16X3S": "TEM_ARITH_F16X3S", "TEM_WL_BF16": "TEM_ARITH_BF16"}


def test_arith_pack_facts():
    """(planes, pack kind) per mode, as literals; the C++ column is the same table (csrc/conv_arith.h), read back as text."""
    from torch_em_amd.arith import Arith, PackKind
    want = {0: (0, 0), 1: (2, 4), 2: (2, 0), 3: (3, 0), 4: (2, 2), 5: (1, 1), 6: (2, 3), 7: (1, 0)}
    assert {int(m): tuple(int(v) for v in m.pack) for m in Arith if m is not Arith.F16X2} == want
    text = open(os.path.join(ROOT, "torch_em_amd", "csrc", "conv_arith.h")).read()
    kinds = {k: int(v) for k, v in re.findall(r"^\s+(TEM_PK_\w+) = (\d),", text, flags=re.M)}
    assert kinds == {"TEM_PK_" + k.name: int(k) for k in PackKind}
    rows = re.findall(r"^\s+/\* (\w+)\s*\*/ \{(\d), (TEM_PK_\w+),", text, flags=re.M)
    assert [r[0] for r in rows] == [m.name for m in Arith]
    assert {int(Arith[n]): (int(p), kinds[k]) for n, p, k in rows if n != "F16X2"} == want


# (mode, family) -> tags for Cout 32 and 64, kernel 3x3x3; family 0: patch kernel, 1 / 2: ping-pong teams, 3 / 4: z-reuse kernel
FWD_TAGS = {
    (0, 0): ('k_conv_fwd_valu<3,3,3>', 'k_conv_fwd_valu<3,3,3>'),
    (0, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (0, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (0, 3): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (0, 4): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (1, 0): ('k_conv_fwd_mfma<3,3,3,NR=1>', 'k_conv_fwd_mfma<3,3,3,NR=2>'),
    (1, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (1, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (1, 3): ('k_conv_zr_fp32<3,3,3>', 'k_conv_zr_fp32<3,3,3>'),
    (1, 4): ('k_conv_zr_fp32<3,3,3>', 'k_conv_zr_fp32<3,3,3>'),
    (2, 0): ('k_conv_fwd_bf16x3<3,3,3,NR=1>', 'k_conv_fwd_bf16x3<3,3,3,NR=2>'),
    (2, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (2, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (2, 3): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (2, 4): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (3, 0): ('k_conv_fwd_bf16x6<3,3,3,NR=1>', 'k_conv_fwd_bf16x6<3,3,3,NR=2>'),
    (3, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (3, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (3, 3): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (3, 4): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (4, 0): ('k_conv_fwd_f16x3<3,3,3,NR=1>', 'k_conv_fwd_f16x3<3,3,3,NR=2>'),
    (4, 1): ('k_conv_pp_f16x3<3,3,3,CT=1>', 'k_conv_pp_f16x3<3,3,3,CT=2>'),
    (4, 2): ('k_conv_pp_f16x3<3,3,3,CT=1>', 'k_conv_pp_f16x3<3,3,3,CT=2>'),
    (4, 3): ('k_conv_zr_f16x3<3,3,3>', 'k_conv_zr_f16x3<3,3,3>'),
    (4, 4): ('k_conv_zr_f16x3<3,3,3>', 'k_conv_zr_f16x3<3,3,3>'),
    (5, 0): ('k_conv_fwd_f16<3,3,3,NR=1>', 'k_conv_fwd_f16<3,3,3,NR=2>'),
    (5, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (5, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (5, 3): ('k_conv_zr_f16<3,3,3>', 'k_conv_zr_f16<3,3,3>'),
    (5, 4): ('k_conv_zr_f16<3,3,3>', 'k_conv_zr_f16<3,3,3>'),
    (6, 0): ('k_conv_fwd_f16x3<3,3,3,NR=1>', 'k_conv_fwd_f16x3<3,3,3,NR=2>'),
    (6, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (6, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (6, 3): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (6, 4): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (7, 0): ('k_conv_fwd_bf16<3,3,3,NR=1>', 'k_conv_fwd_bf16<3,3,3,NR=2>'),
    (7, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (7, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (7, 3): ('k_conv_zr_bf16<3,3,3>', 'k_conv_zr_bf16<3,3,3>'),
    (7, 4): ('k_conv_zr_bf16<3,3,3>', 'k_conv_zr_bf16<3,3,3>'),
    (8, 0): ('k_conv_fwd_mfma<3,3,3,NR=1>', 'k_conv_fwd_mfma<3,3,3,NR=2>'),
    (8, 1): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (8, 2): ('k_conv_pp_bf16x3<3,3,3,CT=1>', 'k_conv_pp_bf16x3<3,3,3,CT=2>'),
    (8, 3): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
    (8, 4): ('k_conv_zr_bf16x3<3,3,3>', 'k_conv_zr_bf16x3<3,3,3>'),
}
# mode -> tags for (3x3x3, Cout 32), (3x3x3, Cout 64), (1x1x1, Cout 32), (1x1x1, Cout 64)
WGRAD_TAGS = {
    0: ('k_conv_wgrad_valu<3,3,3>(+reduce)', 'k_conv_wgrad_valu<3,3,3>(+reduce)', 'k_conv_wgrad_valu<1,1,1>(+reduce)', 'k_conv_wgrad_valu<1,1,1>(+reduce)'),
    1: ('k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)'),
    2: ('k_conv_wgrad_bf16x3<3,3,3,NCO=1>(+reduce)', 'k_conv_wgrad_bf16x3<3,3,3,NCO=2>(+reduce)', 'k_conv_wgrad_bf16x3<1,1,1>(+reduce)', 'k_conv_wgrad_bf16x3<1,1,1>(+reduce)'),
    3: ('k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)'),
    4: ('k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)'),
    5: ('k_conv_wgrad_f16<3,3,3,NCO=1>(+reduce)', 'k_conv_wgrad_f16<3,3,3,NCO=2>(+reduce)', 'k_conv_wgrad_f16<1,1,1>(+reduce)', 'k_conv_wgrad_f16<1,1,1>(+reduce)'),
    6: ('k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<3,3,3>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)', 'k_conv_wgrad_mfma<1,1,1>(+reduce)'),
    7: ('k_conv_wgrad_bf16<3,3,3,NCO=1>(+reduce)', 'k_conv_wgrad_bf16<3,3,3,NCO=2>(+reduce)', 'k_conv_wgrad_bf16<1,1,1>(+reduce)', 'k_conv_wgrad_bf16<1,1,1>(+reduce)'),
    8: ('k_conv_wgrad_f16x2<3,3,3,NCO=1>(+reduce)', 'k_conv_wgrad_f16x2<3,3,3,NCO=2>(+reduce)', 'k_conv_wgrad_f16x2<1,1,1>(+reduce)', 'k_conv_wgrad_f16x2<1,1,1>(+reduce)'),
}


def test_profiler_tags_are_unchanged():
    """bench.py parses these strings (RP_NAMES, the split detection): pinned as they were before the modes got names."""
    from torch_em_amd import ops
    for (mode, fam), tags in FWD_TAGS.items():
        assert tuple(ops._fwd_tag(mode, (3, 3, 3), cout, fam) for cout in (32, 64)) == tags, (mode, fam)
    for mode, tags in WGRAD_TAGS.items():
        assert tuple(ops._wgrad_tag(mode, k, cout) for k in ((3, 3, 3), (1, 1, 1)) for cout in (32, 64)) == tags, mode
    assert ops._fwd_tag(False, (1, 3, 3), 32) == "k_conv_fwd_valu<1,3,3>" and ops._fwd_tag(True, (1, 3, 3), 64) == "k_conv_fwd_mfma<1,3,3,NR=2>"


def test_version_and_error_string():
    from torch_em_amd import _lib
    lib = _lib.load()
    assert lib.tem_version() >= 100
    assert isinstance(lib.tem_last_error(), bytes)
    # argument validation happens before any HIP call: exercise the error path on CPU
    rc = lib.tem_conv3d_fwd(None, 0, None, None, None, None, None, 0, None, 0, None, 0, 1, 1, 1, 1, 1, 1, 3, 3, 3, 0, 0,
                            None)
    assert rc == -1 and b"null pointer" in lib.tem_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "tem_conv3d_fwd")


def test_cfg2_layers_select_the_team_kernels():
    """Dispatch guard (no GPU needed: tem_conv3d_fwd_kernel is host logic, 256 CUs assumed without a device): every 3x3x3
    forward / data-gradient convolution of the benchmark network (UNet3d(1->2, 32 features, depth 4) on 2x1x128^3,
    BASELINE.json cfg 2) runs on the z-reuse team kernel -- family 3 with fused statistics at the 128^3 ... 32^3 levels,
    family 4 (split input channels, statistics from the split-K epilogue) where there are too few tiles: a change that silently sends one of
    them back to the one-patch-per-workgroup kernel costs 0.1-1 ms per step."""
    from torch_em_amd import _lib
    lib = _lib.load()
    # (size, features) per level; each block has cin->f and f->f convs, the decoder's first conv reads 2f channels
    levels = [(128, 32), (64, 64), (32, 128), (16, 256)]
    layers = []
    for i, (s, f) in enumerate(levels):
        layers += [(s, f, f), (s, 2 * f, f)]                       # conv2 of both blocks / decoder conv1
        if i:
            layers.append((s, f // 2, f))                          # encoder conv1 (level 0 has Cin = 1: the row kernel)
    layers += [(8, 256, 512), (8, 512, 512)]                       # base block
    for s, cin, cout in layers:
        for a, b in ((cin, cout), (cout, cin)):                    # forward and its data gradient (transposed channels)
            for mode in (2, 4, 5, 7):
                fam = lib.tem_conv3d_fwd_kernel(2, s, s, s, a, b, 3, 3, 3, mode)
                units = 2 * (s // 4) * max(s // 16, 1) * (s // 8) * (b // 32)
                assert fam == (3 if units >= 512 else 4), (s, a, b, mode, fam)
                blocks = lib.tem_conv3d_fwd_stat_blocks(2, s, s, s, a, b, 3, 3, 3, mode)
                # statistics partials come from the team kernel's epilogue or, round 4, from the split-K epilogue (blocks of
                # 4 rows of 256 / (Cout / 4) voxels)
                vb = 4 * (256 // (b // 4))
                assert blocks > 0 and (fam == 3 or blocks == (s ** 3 + vb - 1) // vb), (s, a, b, mode, blocks)


def test_error_buffer_is_the_only_thread_local():
    """Per-call state of the library travels in arguments (csrc/conv_internal.h: TemConvCall), never in globals that an entry
    point installs for its launchers to find: the only `thread_local` under csrc/ is the buffer behind tem_last_error()."""
    csrc = os.path.join(ROOT, "torch_em_amd", "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h", ".inc", ".cpp", ".hpp")):
            continue
        text = open(os.path.join(csrc, name)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for no, line in enumerate(text.splitlines(), 1):
            if re.search(r"\bthread_local\b", line.split("//")[0]):
                found.append((name, no, line.strip()))
    assert len(found) == 1 and found[0][0] == "capi.hip" and re.match(r"static thread_local char g_err\[\d+\]", found[0][2]), found


def test_conv_dispatch_matches_the_recorded_table(golden_dir):
    """What the dispatch queries answer -- kernel family, statistics rows, workspaces, the weight gradient's by-product
    queries -- over modes x storage types x volumes x channel counts x kernels x layouts equals the table recorded before the
    arithmetic modes got their one definition (tests/golden/gen_golden_conv_dispatch.py; host logic: no device needed)."""
    import importlib.util

    import numpy as np
    from torch_em_amd import _lib
    spec = importlib.util.spec_from_file_location("gen_golden_conv_dispatch", os.path.join(golden_dir, "gen_golden_conv_dispatch.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(gen.FIXTURE)
    lib = _lib.load()
    before = [_lib.get_option(o) for o in gen.OPTIONS]
    try:
        for o, v in zip(gen.OPTIONS, want["options"]):
            _lib.set_option(o, int(v))
        got = gen.sweep(lib)
    finally:
        for o, v in zip(gen.OPTIONS, before):
            _lib.set_option(o, v)
    fam = want["fwd_kernel_ld"]
    assert all(int((fam == f).sum()) > 0 for f in (1, 2, 3, 4)), "the grid must reach every kernel family"
    assert int((want["wgrad"][:, 1:] > 0).sum()) > 0 and int((want["fwd_stat_blocks_ld"] > 0).sum()) > 0
    for name in ("key", "fwd_kernel_ld", "fwd_stat_blocks_ld", "fwd_ws", "wgrad"):
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, (name, len(bad), [(want["key"][b[0]].tolist(), b.tolist(), int(want[name][tuple(b)]), int(got[name][tuple(b)]))
                                                for b in bad[:5]])


def test_wgrad_ws_answers_for_refused_channels():
    """A public query must not abort: an MFMA mode asked about channel counts its launch refuses (Cin or Cout % 32 != 0) gets
    the size of the VALU path (the plans behind the MFMA answer divide by Cin / 32)."""
    from torch_em_amd import _lib
    lib = _lib.load()
    valu = lib.tem_conv3d_wgrad_ws(2, 128, 128, 128, 1, 32, 3, 3, 3, 0)
    assert valu > 0
    for mode in range(1, 9):
        assert lib.tem_conv3d_wgrad_ws(2, 128, 128, 128, 1, 32, 3, 3, 3, mode) == valu, mode
        assert lib.tem_conv3d_wgrad_ws(2, 16, 16, 16, 16, 32, 3, 3, 3, mode) > 0 and lib.tem_conv3d_wgrad_ws(2, 16, 16, 16, 32, 48, 1, 1, 1, mode) > 0
    assert lib.tem_conv3d_wgrad_gscaled_ok(2, 128, 128, 128, 1, 32, 3, 3, 3) == 0
