"""The paired z-reuse kernel (k_conv_zr<..., PAIR>, csrc/conv_zr.hip; option "zr_pair") against the unpaired one, bit for bit.

Where Cout % 64 == 0 the two teams of a workgroup hold sibling output-channel tiles of one input tile; paired, they stage each
halo chunk once between them (team 0 halo planes 0-2, team 1 planes 3-5, into a double buffer of chunks) instead of once each.
Every accumulator sees the same operands in the same order, so output, statistics rows and the output-amax word must be EQUAL
to those of option zr_pair = 0, which is the kernel as it was before the pairing existed.  The forward / data-gradient
convolutions of ConvBlock (reference model/unet.py:417-438) are what the kernel computes; their accuracy against F.conv3d is
tests/test_gpu_ops.py's subject, not this file's."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = (3, 3, 3)


def _ops():
    from torch_em_amd import ops
    return ops


@contextlib.contextmanager
def _options(**kw):
    from torch_em_amd import _lib
    old = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def _inputs(N, D, H, W, Cin, Cout, seed):
    """Activations NDHWC, weights, bias, pre-norm, a reference tensor for the masks and norm-backward coefficients"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)  # noqa: E731
    return dict(x=r(N, D, H, W, Cin), w=r(Cout, Cin, *K) * 0.1, b=r(Cout), scale=torch.rand(N, Cin, generator=g, device=DEV) + 0.5,
                shift=r(N, Cin), ref=r(N, D, H, W, Cout), coef=r(N, Cout, 4), gbig=r(N, D, H, W, Cin) * 3e-4)


def _epilogues(t, dims, Cin, Cout, mode):
    """One launch per epilogue of the kernel -> {name: tensors to compare}.  The weight is used as it is for every call (a data
    gradient is the same kernel on another pack: what matters here is which instantiation runs)."""
    ops = _ops()
    N, D, H, W = dims
    wp = ops.pack_weights(t["w"], transpose=False, mfma=mode)
    new = lambda: torch.full((N, D, H, W, Cout), 7.0, device=DEV)  # noqa: E731
    out = {}
    y = new()                                                                     # MODE 0: plain
    ops.conv_fwd(t["x"], wp, None, y, K, Cin, Cout, mfma=mode)
    out["plain"] = (y,)
    y = new()                                                                     # MODE 1: pre-norm on load, bias, ReLU, statistics rows
    st = ops.conv_fwd(t["x"], wp, t["b"], y, K, Cin, Cout, scale=t["scale"], shift=t["shift"], act="relu", mfma=mode, want_stats=True)
    assert st is not None
    out["stats"] = (y, st[0])
    y, amax = new(), torch.zeros(1, dtype=torch.int32, device=DEV)                # MODE 2: ReLU mask of ref, output amax
    bp = ops.Byproducts(out_amax=amax)
    ops.conv_fwd(t["x"], wp, None, y, K, Cin, Cout, ref=t["ref"], mfma=mode, bp=bp)
    assert bp.amax
    out["mask"] = (y, amax)
    y, amax = new(), torch.zeros(1, dtype=torch.int32, device=DEV)                # MODE 3: mask + norm backward
    bp = ops.Byproducts(out_amax=amax)
    ops.conv_fwd_refnorm(t["x"], wp, y, K, Cin, Cout, t["ref"], t["coef"], mode, bp=bp)
    assert bp.amax
    out["refnorm"] = (y, amax)
    if mode == 4:                                                                 # in_amax prescale of a small raw gradient
        y, amax = new(), torch.zeros(1, dtype=torch.int32, device=DEV)
        bp = ops.Byproducts(out_amax=amax)
        ops.conv_fwd_gscaled(t["gbig"], wp, y, K, Cin, Cout, ops.absmax(t["gbig"]), ref=t["ref"], bp=bp)
        out["gscaled"] = (y, amax)
    torch.cuda.synchronize()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        for i, (u, v) in enumerate(zip(a[name], b[name])):
            assert torch.equal(u, v), f"{what}: {name}[{i}] differs between zr_pair 0 and 1"


def _pair_vs_unpaired(dims, Cin, Cout, mode, family=3):
    from torch_em_amd import _lib
    lib = _lib.load()
    N, D, H, W = dims
    t = _inputs(N, D, H, W, Cin, Cout, seed=Cin + Cout + D)
    res = {}
    for pair in (0, 1):
        with _options(zr_pair=pair):
            assert lib.tem_conv3d_fwd_kernel(N, D, H, W, Cin, Cout, 3, 3, 3, mode) == family
            res[pair] = _epilogues(t, dims, Cin, Cout, mode)
    _assert_same(res[0], res[1], f"{dims} {Cin}->{Cout} mode {mode}")
    return res[1]


# volumes: every tile a border tile / interior and border tiles / partial tiles in z, y and x (D % 4, H % 16, W % 8 all nonzero)
@pytest.mark.parametrize("dims", [(1, 8, 32, 16), (2, 12, 40, 24), (1, 6, 20, 12)])
@pytest.mark.parametrize("Cout", [64, 128])
def test_paired_kernel_is_bit_identical(dims, Cout):
    """Cin 16 / 32 / 48: one, two, three chunks per unit; both two-term arithmetics (bf16x3: the data gradients' kernel, fp16x3: the
    forward's); every epilogue.  These shapes have at most 216 units, one per team on a device with 108 or more CUs: what happens
    when a team moves from one unit to the next is test_several_units_per_team's subject."""
    with _options(team_min_units=1):
        for Cin in (16, 32, 48):
            for mode in (2, 4):
                _pair_vs_unpaired(dims, Cin, Cout, mode)


@pytest.mark.parametrize("Cin", [16, 48])
def test_one_unit_per_team(Cin):
    """One 4 x 16 x 8 tile, Cout 64: one workgroup whose teams have exactly one unit each -- the prologue runs straight into the drain"""
    with _options(team_min_units=1):
        for mode in (2, 4):
            _pair_vs_unpaired((1, 4, 16, 8), Cin, 64, mode)


@pytest.mark.parametrize("Cin", [16, 32, 48])
def test_several_units_per_team(Cin):
    """More units than the device has teams (the grid is capped at one workgroup per CU): teams walk through several units, the
    stage cursor of team 0 crosses into the next unit one chunk before its tap cursor does.  One chunk per unit: team 0 decodes a
    new unit in every iteration and stages a whole unit ahead of its taps; three: the tile that holds a unit's first chunk
    alternates from unit to unit (the tile follows the pair's chunk count, not the chunk's place in its unit)."""
    from torch_em_amd import _lib
    N, D, H, W, Cout = 4, 5, 33, 41, 128
    units = N * ((D + 3) // 4) * ((H + 15) // 16) * ((W + 7) // 8) * (Cout // 32)
    assert units > 2 * _lib.load().tem_device_cus(), "the shape must give some team a second unit"
    with _options(team_min_units=1):
        for mode in (2, 4):
            _pair_vs_unpaired((N, D, H, W), Cin, Cout, mode)


@pytest.mark.parametrize("case", [(2, 16, 16, 16, 256, 256), (2, 8, 8, 8, 256, 512), (2, 16, 16, 16, 160, 256)])
def test_paired_split_k(case):
    """Family 4: paired launches enumerate the column tile fastest and the K-slice next; every unit still writes the same partial
    sums into the same workspace slice, so the summing epilogue's output and statistics do not move.  The first two shapes split
    into 512 units (one per team on 256 CUs); 160 -> 256 splits its ten chunks five ways into 640, so some teams move on from
    one (tile, slice) to the next."""
    from torch_em_amd import _lib
    ops = _ops()
    lib = _lib.load()
    N, D, H, W, Cin, Cout = case
    if Cin == 160:
        # tem_zr_splitk_ks: the smallest divisor of the chunk count that gives every team a unit
        tiles, nch, teams = N * ((D + 3) // 4) * ((H + 15) // 16) * ((W + 7) // 8) * (Cout // 32), Cin // 16, 2 * lib.tem_device_cus()
        ks = next(d for d in range(2, nch // 2 + 1) if nch % d == 0 and tiles * d >= teams)
        assert tiles * ks > teams, "the shape must give some team a second unit"
    t = _inputs(N, D, H, W, Cin, Cout, seed=5)
    res = {}
    for pair in (0, 1):
        with _options(zr_pair=pair):
            out = {}
            for mode in (2, 4):
                assert lib.tem_conv3d_fwd_kernel(N, D, H, W, Cin, Cout, 3, 3, 3, mode) == 4
                wp = ops.pack_weights(t["w"], transpose=False, mfma=mode)
                y = torch.full((N, D, H, W, Cout), 7.0, device=DEV)
                st = ops.conv_fwd(t["x"], wp, t["b"], y, K, Cin, Cout, scale=t["scale"], shift=t["shift"], act="relu", mfma=mode,
                                  want_stats=True)
                assert st is not None
                out[f"stats{mode}"] = (y, st[0])
                y = torch.full((N, D, H, W, Cout), 7.0, device=DEV)
                ops.conv_fwd(t["x"], wp, None, y, K, Cin, Cout, ref=t["ref"], mfma=mode)
                out[f"mask{mode}"] = (y,)
            torch.cuda.synchronize()
            res[pair] = out
    _assert_same(res[0], res[1], f"split-K {case}")


@pytest.mark.parametrize("Cout", [32, 96])
def test_odd_tile_counts_stay_unpaired(Cout):
    """No sibling for every tile: the option must not reach these launches"""
    with _options(team_min_units=1):
        for mode in (2, 4):
            _pair_vs_unpaired((2, 12, 40, 24), 32, Cout, mode)


def test_exact_fp32_is_untouched():
    """use_mfma 1 on the z-reuse kernel keeps its own schedule (its epilogue runs behind the tap phase)"""
    from torch_em_amd import _lib
    ops = _ops()
    lib = _lib.load()
    N, D, H, W, Cin, Cout = 2, 12, 40, 24, 32, 64
    t = _inputs(N, D, H, W, Cin, Cout, seed=9)
    res = {}
    with _options(team_min_units=1):
        for pair in (0, 1):
            with _options(zr_pair=pair):
                assert lib.tem_conv3d_fwd_kernel(N, D, H, W, Cin, Cout, 3, 3, 3, 1) == 3
                y = torch.full((N, D, H, W, Cout), 7.0, device=DEV)
                st = ops.conv_fwd(t["x"], ops.pack_weights(t["w"], transpose=False, mfma=1), t["b"], y, K, Cin, Cout, scale=t["scale"],
                                  shift=t["shift"], act="relu", mfma=1, want_stats=True)
                assert st is not None
                torch.cuda.synchronize()
                res[pair] = {"stats": (y, st[0])}
    _assert_same(res[0], res[1], "exact fp32")
