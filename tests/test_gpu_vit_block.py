"""GPU: ops.layer_norm_windows, ops.window_merge_norm, ops.bias_gelu (csrc/vit_block.hip) and model.vit.Block against the float64
definitions of tests/vit_block_ref.py (scales: its docstring).  Inputs are values every storage type holds exactly, so one
reference serves the three types.
  f32     judge.within(judge.units(got, ref, scale), e32), e32 the figure of the float32 restatement
  16-bit  every stored element inside judge.interval16(ref, scale, e32, dt); no extra 16-bit rounding on the paths of xw, x1, xn, y,
          dh, dx and the parameter gradients of layer_norm_windows.  The gradients of window_merge_norm recompute xhat from the
          stored x1 (one rounding): dy, dshortcut and dgamma get d = 2^-p * stored_x1_sensitivity + judge.band(e32) * scale.
The slab case: 2 x 40 x 37 tokens, window 14, are 2960 source and 3528 window tokens -- 92.5 and 110.25 slabs of 32."""
import functools

import numpy as np
import pytest
import torch

import vit_block_ref as R
from oracle import judge

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GRIDS = [(2, 5, 3, 4), (1, 14, 14, 14), (1, 16, 15, 7), (2, 9, 6, 0)]
ROW_CASES = [(g, C) for g in GRIDS for C in (40, 768, 1280)] + [((1, 16, 15, 7), 512), ((1, 16, 15, 7), 2048)]
EPS = 1e-6
bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0").to(TORCH[dt])
host = lambda t: t.detach().double().cpu().numpy()


def judge_one(tag, got, ref, ref32, scale, dt, extra=None):
    """the rule of the module docstring; extra: the absolute allowance of the one documented rounding (16-bit only)"""
    e32, units = judge.units(ref32, ref, scale), judge.units(got, ref, scale)
    print(f"VIT_BLOCK_ERR {tag} {dt}: kernel {units:.2f} f32 {e32:.2f}")
    if dt == "f32":
        assert judge.within(units, e32), f"{tag}: {units:.2f} units from float64, plain fp32 arithmetic {e32:.2f}"
    elif extra is None:
        lo, hi = judge.interval16(ref, scale, e32, dt)
        assert judge.outside_interval(got, lo, hi) == 0, f"{tag}: stored elements outside interval16"
    else:
        d = 2.0 ** -judge.FMT[dt][0] * extra + judge.band(e32) * scale
        assert judge.outside16_abs(got, ref, d, dt) == 0, f"{tag}: stored elements outside [round16(ref - d), round16(ref + d)]"


@functools.lru_cache(maxsize=None)
def row_case(grid, C):
    """inputs, float64 / float32 references and scales of both row ops on one grid, computed once"""
    B, H, W, ws = grid
    rng = np.random.default_rng(C + H)
    c16 = lambda a: judge.round_common16(a)
    x, s = c16(rng.standard_normal((B, H, W, C)) + 0.5), c16(rng.standard_normal((B, H, W, C)))
    gamma, beta = c16(1 + 0.3 * rng.standard_normal(C)), c16(0.2 * rng.standard_normal(C))
    wshape = R.partition(x, ws).shape
    y, g = c16(rng.standard_normal(wshape)), c16(rng.standard_normal(wshape))          # pad tokens hold values: never read / dropped
    d1, dn = c16(rng.standard_normal((B, H, W, C))), c16(rng.standard_normal((B, H, W, C)))
    inp = dict(x=x, s=s, gamma=gamma, beta=beta, y=y, g=g, d1=d1, dn=dn)
    ref, ref32, sc = {}, {}, {}
    for out, dtype in ((ref, np.float64), (ref32, np.float32)):
        out["xw"] = R.layer_norm_windows(x, gamma, beta, EPS, ws, dtype)
        out["dx"], out["dgamma1"], out["dbeta1"] = R.layer_norm_windows_bwd(g, x, gamma, EPS, ws, dtype)
        out["x1"], out["xn"] = R.window_merge_norm(y, s, gamma, beta, EPS, ws, dtype)
        out["dy"], out["ds"], out["dgamma2"], out["dbeta2"] = R.window_merge_norm_bwd(d1, dn, y, s, gamma, EPS, ws, dtype)
    (sc["dx"], sc["dgamma1"], sc["dbeta1"]), (_, rstd, _) = R.ln_bwd_scales(R.merge(g, ws, B, H, W), x, gamma, EPS)
    sc["xw"] = R.partition(R.forward_scale(np.abs(x), gamma, beta, rstd), ws)
    sc["x1"] = np.abs(s) + R.merge(np.abs(y), ws, B, H, W)
    (sds, sc["dgamma2"], sc["dbeta2"]), (_, rstd1, _) = R.ln_bwd_scales(dn, ref["x1"], gamma, EPS)
    sc["xn"] = R.forward_scale(sc["x1"], gamma, beta, rstd1)
    sc["ds"] = sds + np.abs(d1)
    sc["dy"] = R.partition(sc["ds"], ws)
    a, ag = R.stored_x1_sensitivity(dn, ref["x1"], gamma, EPS)
    return inp, ref, ref32, sc, {"ds": a, "dy": R.partition(a, ws), "dgamma2": ag}


def run_row_ops(grid, C, dt):
    """both ops under grad -> every output and gradient as tensors, and what a second evaluation needs"""
    from torch_em_amd import ops
    ws = grid[3]
    inp = row_case(grid, C)[0]
    t = {k: dev(v, dt) for k, v in inp.items()}
    l1 = [t[k].clone().requires_grad_() for k in ("x", "gamma", "beta")]
    xw = ops.layer_norm_windows(*l1, EPS, ws)
    l2 = [t[k].clone().requires_grad_() for k in ("y", "s", "gamma", "beta")]
    x1, xn = ops.window_merge_norm(*l2, EPS, ws)
    grads = lambda: list(torch.autograd.grad(xw, l1, t["g"], retain_graph=True)) + list(torch.autograd.grad([x1, xn], l2, [t["d1"], t["dn"]], retain_graph=True))
    names = ["xw", "x1", "xn", "dx", "dgamma1", "dbeta1", "dy", "ds", "dgamma2", "dbeta2"]
    return dict(zip(names, [xw, x1, xn] + grads())), grads, t


@pytest.mark.parametrize("dt", list(TORCH))
@pytest.mark.parametrize("grid,C", ROW_CASES, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else str(p))
def test_row_ops_against_float64(grid, C, dt):
    from torch_em_amd import ops
    _, ref, ref32, sc, extra = row_case(grid, C)
    got, grads, t = run_row_ops(grid, C, dt)
    for name, val in got.items():
        assert val.dtype == TORCH[dt] and tuple(val.shape) == ref[name].shape, name
        judge_one(f"{'x'.join(map(str, grid))} C={C} {name}", host(val), ref[name], ref32[name], sc[name], dt, extra.get(name))
    pad = torch.from_numpy(R.pad_mask(grid[3], *grid[:3])).to("cuda:0")
    for name in ("xw", "dy"):                                                                # pad tokens: +0.0 in every bit
        assert int(bits(got[name].detach())[pad].count_nonzero()) == 0, name
    again = grads()                                                                           # the same bits a second time
    assert all(torch.equal(bits(a), bits(got[n])) for a, n in zip(again, list(got)[3:]))
    with torch.no_grad():                                                                     # under grad: the no-grad bits
        plain = [ops.layer_norm_windows(t["x"], t["gamma"], t["beta"], EPS, grid[3])] \
            + list(ops.window_merge_norm(t["y"], t["s"], t["gamma"], t["beta"], EPS, grid[3]))
    assert all(torch.equal(bits(a), bits(got[n].detach())) for a, n in zip(plain, ("xw", "x1", "xn")))


def test_parameter_gradients_across_slab_boundaries():
    grid, C = (2, 40, 37, 14), 40
    _, ref, ref32, sc, _ = row_case(grid, C)
    got, _, _ = run_row_ops(grid, C, "f32")
    for name in ("dgamma1", "dbeta1", "dgamma2", "dbeta2"):
        judge_one(f"slabs {name}", host(got[name]), ref[name], ref32[name], sc[name], "f32")


@pytest.mark.parametrize("dt", ("f32", "f16"))
def test_one_whole_window_gives_the_bits_of_no_windows(dt):
    a, _, _ = run_row_ops((1, 14, 14, 14), 768, dt)                                           # the seed is C + H: the same inputs
    b, _, _ = run_row_ops((1, 14, 14, 0), 768, dt)
    assert all(torch.equal(bits(a[n].detach()), bits(b[n].detach())) for n in a)


@functools.lru_cache(maxsize=None)
def gelu_case(M, C4):
    rng = np.random.default_rng(M)
    c16 = lambda a: judge.round_common16(a)
    h, b, dy = c16(rng.uniform(-5.5, 5.5, (M, C4))), c16(rng.uniform(-0.5, 0.5, C4)), c16(rng.standard_normal((M, C4)))   # z in [-6, 6]
    ref = (R.bias_gelu(h, b),) + R.bias_gelu_bwd(dy, h, b)
    ref32 = (R.bias_gelu(h, b, np.float32),) + R.bias_gelu_bwd(dy, h, b, np.float32)
    return (h, b, dy), ref, ref32, R.gelu_scales(dy, h, b)


@pytest.mark.parametrize("dt", list(TORCH))
@pytest.mark.parametrize("M,C4", [(3, 40), (70, 3072), (257, 5120)])
def test_bias_gelu_against_float64(M, C4, dt):
    from torch_em_amd import ops
    (h, b, dy), ref, ref32, sc = gelu_case(M, C4)
    leaves = [dev(h, dt).requires_grad_(), dev(b, dt).requires_grad_()]
    y = ops.bias_gelu(*leaves)
    got = [y] + list(torch.autograd.grad(y, leaves, dev(dy, dt), retain_graph=True))
    for name, val, r, r32, s in zip(("y", "dh", "db"), got, ref, ref32, sc):
        judge_one(f"gelu {M}x{C4} {name}", host(val), r, r32, s, dt)
    again = torch.autograd.grad(y, leaves, dev(dy, dt))
    assert all(torch.equal(bits(a), bits(g)) for a, g in zip(again, got[1:]))
    with torch.no_grad():
        assert torch.equal(bits(ops.bias_gelu(*leaves)), bits(y.detach()))


SAM_BLOCK_KEYS = ["norm1.weight", "norm1.bias", "attn.rel_pos_h", "attn.rel_pos_w", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                  "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.lin1.weight", "mlp.lin1.bias", "mlp.lin2.weight", "mlp.lin2.bias"]


def torch_block(sd, x, g, ws, heads, dtype):
    """segment_anything's Block composed from torch ops on the CPU -> (out, gradients of x and of every parameter)"""
    F = torch.nn.functional
    p = {k: v.to(dtype).requires_grad_() for k, v in sd.items()}
    xt = x.to(dtype).requires_grad_()
    B, H, W, dim = x.shape
    D = dim // heads
    t = F.layer_norm(xt, (dim,), p["norm1.weight"], p["norm1.bias"], EPS)
    Hp, Wp = (H, W) if ws == 0 else (-(-H // ws) * ws, -(-W // ws) * ws)
    if ws:
        t = F.pad(t, (0, 0, 0, Wp - W, 0, Hp - H)).view(B, Hp // ws, ws, Wp // ws, ws, dim).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, dim)
    Bw, h, w, _ = t.shape
    qkv = (t.reshape(Bw, h * w, dim) @ p["attn.qkv.weight"].T + p["attn.qkv.bias"]).reshape(Bw, h * w, 3, heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    idx = lambda n: torch.arange(n)[:, None] - torch.arange(n)[None, :] + n - 1
    r = q.reshape(Bw, heads, h, w, D)
    S = (D ** -0.5 * (q @ k.transpose(-1, -2))).reshape(Bw, heads, h, w, h, w) \
        + torch.einsum("bahwc,hkc->bahwk", r, p["attn.rel_pos_h"][idx(h)])[..., :, None] + torch.einsum("bahwc,wkc->bahwk", r, p["attn.rel_pos_w"][idx(w)])[..., None, :]
    o = (torch.softmax(S.reshape(Bw, heads, h * w, h * w), -1) @ v).permute(0, 2, 1, 3).reshape(Bw, h, w, dim)
    t = o @ p["attn.proj.weight"].T + p["attn.proj.bias"]
    if ws:
        t = t.view(B, Hp // ws, Wp // ws, ws, ws, dim).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, dim)[:, :H, :W]
    x1 = xt + t
    m = F.gelu(F.layer_norm(x1, (dim,), p["norm2.weight"], p["norm2.bias"], EPS) @ p["mlp.lin1.weight"].T + p["mlp.lin1.bias"])
    out = x1 + m @ p["mlp.lin2.weight"].T + p["mlp.lin2.bias"]
    (out * g.to(dtype)).sum().backward()
    return [out.detach().numpy(), xt.grad.numpy()] + [p[k].grad.numpy() for k in SAM_BLOCK_KEYS]


@pytest.mark.parametrize("H,W,ws", [(16, 15, 7), (9, 6, 0)])
def test_block_wiring(H, W, ws):
    from torch_em_amd.model import Block
    dim, heads, B = 128, 2, 2
    side = (ws, ws) if ws else (H, W)
    gen = torch.Generator().manual_seed(H)
    rnd = lambda *s, a=1.0: a * torch.randn(*s, generator=gen)
    sd = {"norm1.weight": 1 + rnd(dim, a=0.2), "norm1.bias": rnd(dim, a=0.1), "attn.rel_pos_h": rnd(2 * side[0] - 1, 64, a=0.5),
          "attn.rel_pos_w": rnd(2 * side[1] - 1, 64, a=0.5), "attn.qkv.weight": rnd(3 * dim, dim, a=dim ** -0.5), "attn.qkv.bias": rnd(3 * dim, a=0.1),
          "attn.proj.weight": rnd(dim, dim, a=dim ** -0.5), "attn.proj.bias": rnd(dim, a=0.1), "norm2.weight": 1 + rnd(dim, a=0.2),
          "norm2.bias": rnd(dim, a=0.1), "mlp.lin1.weight": rnd(4 * dim, dim, a=dim ** -0.5), "mlp.lin1.bias": rnd(4 * dim, a=0.1),
          "mlp.lin2.weight": rnd(dim, 4 * dim, a=(4 * dim) ** -0.5), "mlp.lin2.bias": rnd(dim, a=0.1)}
    assert list(sd) == SAM_BLOCK_KEYS
    x, g = rnd(B, H, W, dim), rnd(B, H, W, dim)
    m = Block(dim, heads, norm_layer=lambda d: torch.nn.LayerNorm(d, eps=EPS), use_rel_pos=True, window_size=ws, input_size=(H, W))
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda:0").train()
    xg = x.to("cuda:0").requires_grad_()
    out = m(xg)
    (out * g.to("cuda:0")).sum().backward()
    params = dict(m.named_parameters())
    got = [out, xg.grad] + [params[k].grad for k in SAM_BLOCK_KEYS]
    ref, ref32 = torch_block(sd, x, g, ws, heads, torch.float64), torch_block(sd, x, g, ws, heads, torch.float32)
    for name, a, r64, r32 in zip(["out", "dx"] + SAM_BLOCK_KEYS, got, ref, ref32):
        sc = np.abs(r64).max()                                                               # per tensor: a statement about wiring
        units, e32 = judge.units(host(a), r64, sc), judge.units(r32, r64, sc)
        print(f"VIT_BLOCK_ERR Block {H}x{W} ws={ws} {name}: kernel {units:.2f} f32 {e32:.2f}")
        assert judge.within(units, e32), (name, units, e32)
    with pytest.raises(ValueError, match="GELU"):
        Block(dim, heads, act_layer=torch.nn.ReLU)
    with pytest.raises(ValueError, match="LayerNorm"):
        Block(dim, heads, norm_layer=torch.nn.BatchNorm1d)
