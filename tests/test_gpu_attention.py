"""GPU: ops.attention (csrc/attention.hip) and model.vit.Attention against the float64 definition of tests/attention_ref.py,
on the values the tensors store.  Per element, A = sum_j P |v_j| and scale = A (1 + max_j sum_c |q_c| (s |k_jc| + |Rh.| + |Rw.|)):
  f32     judge.within(judge.units(got, ref, scale), e32), e32 the figure of the float32 restatement
  16-bit  stored element in [round16(ref - d), round16(ref + d)], d = 3 * 2^-p * A + judge.band(e32) * scale (p = 11 fp16, 8 bf16:
          one 2^-p for rounding P, one for a row sum taken on the other side of that rounding, one margin)
Grids: the issue's four, and 256 x 2 -- the workgroup shape of large H + W (two waves, more than 64 KB of LDS), H at its limit."""
import numpy as np
import pytest
import torch

import attention_ref as R
from oracle import judge

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
B, NH = 2, 3
GRIDS = [(5, 3), (8, 8), (14, 14), (20, 13), (256, 2)]
CASES = [(g, D, dt, rel, "normal") for g in GRIDS for D in (64, 80) for dt in TORCH for rel in (False, True)] \
    + [((20, 13), D, dt, True, "ramp") for D in (64, 80) for dt in TORCH]


def make_inputs(grid, D, dt, rel, kind, seed=0):
    """float64 arrays of values the storage type holds exactly"""
    H, W = grid
    N = H * W
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((B, NH, N, D)) for _ in range(3))
    if kind == "ramp":          # q, k > 0 and |k_j| growing with j: the row maximum rises in every key tile
        q, k = np.abs(q), np.abs(k) * (0.2 + 1.8 * np.arange(N) / N)[:, None]
    tables = (0.5 * rng.standard_normal((2 * H - 1, D)), 0.5 * rng.standard_normal((2 * W - 1, D))) if rel else None
    st = lambda x: judge.stored(x.astype(np.float32), dt)
    return st(q), st(k), st(v), None if tables is None else tuple(st(t) for t in tables)


def dev(x, dt):
    return torch.from_numpy(x).to("cuda:0").to(TORCH[dt])


def assert_close(tag, got, dt, q, k, v, grid, scale, rel, ref=None, ref32=None, extra=1.0):
    """the rule of the module docstring; ref / ref32: the reference when it is more than the attention itself"""
    A = R.attention(q, k, np.abs(v), grid, scale, rel)
    absrel = None if rel is None else tuple(np.abs(t) for t in rel)
    sc = A * (1.0 + R.logits(np.abs(q), np.abs(k), grid, scale, absrel).max(-1, keepdims=True)) * extra
    ref = R.attention(q, k, v, grid, scale, rel) if ref is None else ref
    e32 = judge.units(R.attention32(q, k, v, grid, scale, rel) if ref32 is None else ref32, ref, sc)
    units = judge.units(got, ref, sc)
    if dt == "f32":
        print(f"ATTN_ERR {tag}: kernel {units:.2f} f32 {e32:.2f}")
        assert judge.within(units, e32), f"{tag}: {units:.2f} units from float64, plain fp32 arithmetic {e32:.2f}"
    else:
        d = 3.0 * 2.0 ** -judge.FMT[dt][0] * A + judge.band(e32) * sc
        bad = judge.outside16_abs(got, ref, d, dt)
        print(f"ATTN_ERR {tag}: kernel {units:.2f} f32 {e32:.2f}; {bad} of {got.size} outside, worst |err| / d {np.max(np.abs(got - ref) / d):.3f}")
        assert bad == 0, f"{tag}: {bad} stored elements outside [round16(ref - d), round16(ref + d)]"


@pytest.mark.parametrize("grid,D,dt,rel,kind", CASES, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else str(p))
def test_attention_against_float64(grid, D, dt, rel, kind):
    from torch_em_amd import ops
    q, k, v, tables = make_inputs(grid, D, dt, rel, kind)
    got = ops.attention(dev(q, dt), dev(k, dt), dev(v, dt), grid, rel_pos=None if tables is None else tuple(dev(t, dt) for t in tables))
    assert got.shape == (B, NH, grid[0] * grid[1], D) and got.dtype == TORCH[dt]
    assert_close(f"{grid[0]}x{grid[1]} D={D} {dt} rel={int(rel)} {kind}", got.double().cpu().numpy(), dt, q, k, v, grid, None, tables)


def test_packed_views_and_strided_out_give_the_same_bits():
    from torch_em_amd import ops
    grid, D, dt = (14, 14), 64, "f16"
    q, k, v, tables = make_inputs(grid, D, dt, True, "normal", seed=1)
    tables = tuple(dev(t, dt) for t in tables)
    want = ops.attention(dev(q, dt), dev(k, dt), dev(v, dt), grid, rel_pos=tables)
    qkv = torch.stack([dev(t, dt).permute(0, 2, 1, 3) for t in (q, k, v)], dim=2)            # [B, N, 3, nH, D], as the qkv linear writes
    views = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    assert not views[0].is_contiguous()
    y = torch.zeros((B, 14, 14, NH * D), dtype=TORCH[dt], device="cuda:0")
    for _ in range(2):                                                                        # the second call: the same bits again
        ops.attention(*views, grid, rel_pos=tables, out=y.view(B, 196, NH, D).permute(0, 2, 1, 3))
        assert torch.equal(y.view(B, 196, NH, D).permute(0, 2, 1, 3).contiguous().view(torch.int16), want.view(torch.int16))
        y.zero_()


def test_vit_attention_module_loads_sam_keys_and_resamples():
    from torch_em_amd.model import Attention
    H = W = 14
    dim, heads, D = 128, 2, 64
    rng = np.random.default_rng(2)
    f32 = lambda *s, a=1.0: (a * rng.standard_normal(s)).astype(np.float32)
    sd = {"qkv.weight": f32(3 * dim, dim, a=dim ** -0.5), "qkv.bias": f32(3 * dim, a=0.1), "proj.weight": f32(dim, dim, a=dim ** -0.5),
          "proj.bias": f32(dim, a=0.1), "rel_pos_h": f32(13, D, a=0.5), "rel_pos_w": f32(41, D, a=0.5)}     # 27 rows needed: both resampled
    m = Attention(dim, heads, use_rel_pos=True, input_size=(7, 21))
    m.load_state_dict({k_: torch.from_numpy(v_) for k_, v_ in sd.items()})
    m = m.to("cuda:0").eval()
    x = f32(B, H, W, dim)
    with torch.no_grad():
        got = m(torch.from_numpy(x).to("cuda:0"))
    with pytest.raises(NotImplementedError, match="backward"):
        m(torch.from_numpy(x).to("cuda:0"))

    def resample(t, dtype):      # get_rel_pos: F.interpolate(mode="linear", align_corners=False) to 2 * 14 - 1 rows
        L, n = t.shape[0], 2 * H - 1
        src = np.clip((np.arange(n, dtype=dtype) + dtype(0.5)) * dtype(L / n) - dtype(0.5), 0, None)
        i0 = np.minimum(src.astype(np.int64), L - 1)
        lam = (src - i0).astype(dtype)[:, None]
        return (1 - lam) * t[i0].astype(dtype) + lam * t[np.minimum(i0 + 1, L - 1)].astype(dtype)

    def compose(dtype):
        qkv = (x.astype(dtype).reshape(B, H * W, dim) @ sd["qkv.weight"].astype(dtype).T + sd["qkv.bias"].astype(dtype))
        q, k, v = qkv.reshape(B, H * W, 3, heads, D).transpose(2, 0, 3, 1, 4)
        rel = (resample(sd["rel_pos_h"], dtype), resample(sd["rel_pos_w"], dtype))
        o = R.attention(q, k, v, (H, W), None, rel, dtype=dtype)
        return (q, k, v, rel), o.transpose(0, 2, 1, 3).reshape(B, H * W, dim) @ sd["proj.weight"].astype(dtype).T + sd["proj.bias"].astype(dtype)

    (q, k, v, rel), ref = compose(np.float64)
    _, ref32 = compose(np.float32)
    # per-element scale: |proj.weight| applied to the attention's scale, plus the linears' own sum of magnitudes
    A = R.attention(q, k, np.abs(v), (H, W), None, rel)
    s_att = A * (1.0 + R.logits(np.abs(q), np.abs(k), (H, W), None, tuple(np.abs(t) for t in rel)).max(-1, keepdims=True))
    sc = s_att.transpose(0, 2, 1, 3).reshape(B, H * W, dim) @ np.abs(sd["proj.weight"].astype(np.float64)).T + np.abs(sd["proj.bias"]) + 1.0
    got = got.double().cpu().numpy().reshape(B, H * W, dim)
    units, e32 = judge.units(got, ref, sc), judge.units(ref32, ref, sc)
    print(f"ATTN_ERR vit.Attention 14x14 f32: kernel {units:.2f} f32 {e32:.2f}")
    assert judge.within(units, e32), (units, e32)


def test_refusals():
    from torch_em_amd import ops
    t = lambda *s: torch.zeros(s, device="cuda:0")
    with pytest.raises(ValueError, match="head width"):
        ops.attention(t(1, 1, 4, 48), t(1, 1, 4, 48), t(1, 1, 4, 48), (2, 2))
    wide = t(1, 1, 4, 128)[..., ::2]
    with pytest.raises(ValueError, match="unit stride"):
        ops.attention(wide, t(1, 1, 4, 64), t(1, 1, 4, 64), (2, 2))
    with pytest.raises(ValueError, match="exceeds"):
        ops.attention(t(1, 1, 257, 64), t(1, 1, 257, 64), t(1, 1, 257, 64), (257, 1))
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attention(*(torch.zeros(1, 1, 4, 64) for _ in range(3)), (2, 2))
