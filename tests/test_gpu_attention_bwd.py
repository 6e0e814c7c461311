"""GPU: the backward of ops.attention (csrc/attention_bwd.hip) and the training path of model.vit.Attention against the float64
gradients of tests/attention_bwd_ref.py, on the values the tensors store.  Per element, A = the gradient formula on magnitudes
(A_dS = P (|dO| . |v| + |dO| . (P |v|)) for dS, |q|, |k|, |R| for the operands) and scale = the same with every row i of P and
A_dS multiplied by the forward's factor 1 + max_j logits(|q|, |k|, |R|)[i] (the relative error of row i of P grows with it):
  f32     judge.within(judge.units(got, ref, scale), e32), e32 the figure of the float32 restatement
  16-bit  stored element in [round16(ref - d), round16(ref + d)], d = c * 2^-p * A + judge.band(e32) * scale, c = the 16-bit
          roundings on the element's path (the count of the kernel file's header) plus one margin:
          dv: P, + 1 = 2;   dq, dk: dS, the stored O inside delta, + 1 = 3;   dRh, dRw: the stored O inside delta, + 1 = 2 (dB is
          summed from the fp32 dS and stays fp32);   the final store is the interval's own."""
import numpy as np
import pytest
import torch

import attention_bwd_ref as RB
import attention_ref as R
from oracle import judge
from test_gpu_attention import B, GRIDS, NH, TORCH, dev, make_inputs

pytestmark = pytest.mark.gpu
NAMES = ("dq", "dk", "dv", "dRh", "dRw")
ROUNDINGS = {"dq": 3, "dk": 3, "dv": 2, "dRh": 2, "dRw": 2}
bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_dout(grid, D, dt, seed):
    return judge.stored(np.random.default_rng(100 + seed).standard_normal((B, NH, grid[0] * grid[1], D)).astype(np.float32), dt)


def gradients(q, k, v, g, tables, grid, dt, scale=None):
    """ops.attention under grad -> (out, [dq, dk, dv, dRh, dRw] as tensors)"""
    from torch_em_amd import ops
    leaves = [dev(t, dt).requires_grad_() for t in (q, k, v) + (tables or ())]
    out = ops.attention(*leaves[:3], grid, scale=scale, rel_pos=tuple(leaves[3:]) or None)
    return out, list(torch.autograd.grad(out, leaves, dev(g, dt), retain_graph=True)), (out, leaves)


def assert_grads(tag, got, dt, q, k, v, g, grid, tables):
    ref, ref32 = RB.backward(q, k, v, g, grid, None, tables), RB.backward(q, k, v, g, grid, None, tables, dtype=np.float32)
    A, sc = RB.magnitudes(q, k, v, g, grid, None, tables), RB.magnitudes(q, k, v, g, grid, None, tables, logit_factor=True)
    for i, t in enumerate(got):
        x, name = t.double().cpu().numpy(), NAMES[i]
        e32, units = judge.units(ref32[i], ref[i], sc[i]), judge.units(x, ref[i], sc[i])
        if dt == "f32":
            print(f"ATTN_BWD_ERR {tag} {name}: kernel {units:.2f} f32 {e32:.2f}")
            assert judge.within(units, e32), f"{tag} {name}: {units:.2f} units from float64, plain fp32 arithmetic {e32:.2f}"
        else:
            d = ROUNDINGS[name] * 2.0 ** -judge.FMT[dt][0] * A[i] + judge.band(e32) * sc[i]
            bad = judge.outside16_abs(x, ref[i], d, dt)
            print(f"ATTN_BWD_ERR {tag} {name}: kernel {units:.2f} f32 {e32:.2f}; {bad} of {x.size} outside, worst |err| / d "
                  f"{np.max(np.abs(x - ref[i]) / d):.3f}")
            assert bad == 0, f"{tag} {name}: {bad} stored elements outside [round16(ref - d), round16(ref + d)]"


@pytest.mark.parametrize("rel", (False, True), ids=("norel", "rel"))
@pytest.mark.parametrize("dt", list(TORCH))
@pytest.mark.parametrize("D", (64, 80))
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_attention_backward_against_float64(grid, D, dt, rel):
    from torch_em_amd import ops
    q, k, v, tables = make_inputs(grid, D, dt, rel, "normal")
    g = make_dout(grid, D, dt, 0)
    out, got, (o2, leaves) = gradients(q, k, v, g, tables, grid, dt)
    assert out.grad_fn is not None and all(t.dtype == TORCH[dt] and t.shape == l.shape for t, l in zip(got, leaves))
    assert_grads(f"{grid[0]}x{grid[1]} D={D} {dt} rel={int(rel)}", got, dt, q, k, v, g, grid, tables)
    again = torch.autograd.grad(o2, leaves, dev(g, dt))                                      # the same bits a second time
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again))
    with torch.no_grad():                                                                    # the forward under grad: the no-grad bits
        plain = ops.attention(*leaves[:3], grid, rel_pos=tuple(leaves[3:]) or None)
    assert torch.equal(bits(out.detach()), bits(plain))


def test_packed_gradient_buffer_and_strided_dout_give_the_same_bits():
    from torch_em_amd.model.vit import _PackedAttention
    grid, D, dt = (14, 14), 64, "f16"
    q, k, v, tables = make_inputs(grid, D, dt, True, "normal", seed=1)
    g = make_dout(grid, D, dt, 1)
    out, want, _ = gradients(q, k, v, g, tables, grid, dt)
    qkv = torch.stack([dev(t, dt).permute(0, 2, 1, 3) for t in (q, k, v)], dim=2).requires_grad_()   # [B, N, 3, nH, D], the module's route
    tabs = [dev(t, dt).requires_grad_() for t in tables]
    dy = dev(g, dt).permute(0, 2, 1, 3).reshape(B, 14, 14, NH * D).contiguous()               # [B, H, W, nH D]: dO is its strided view
    assert not dy.view(B, 196, NH, D).permute(0, 2, 1, 3).is_contiguous()
    y = _PackedAttention.apply(qkv, *tabs, 14, 14, None)
    assert torch.equal(bits(y.detach().view(B, 196, NH, D).permute(0, 2, 1, 3)), bits(out.detach()))
    dqkv, dRh, dRw = torch.autograd.grad(y, [qkv] + tabs, dy)
    for a, b in zip([dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)] + [dRh, dRw], want):
        assert torch.equal(bits(a), bits(b))


def test_vit_attention_trains():
    from torch_em_amd.model import Attention
    H = W = 14
    dim, heads, D = 128, 2, 64
    rng = np.random.default_rng(3)
    f32 = lambda *s, a=1.0: (a * rng.standard_normal(s)).astype(np.float32)
    sd = {"qkv.weight": f32(3 * dim, dim, a=dim ** -0.5), "qkv.bias": f32(3 * dim, a=0.1), "proj.weight": f32(dim, dim, a=dim ** -0.5),
          "proj.bias": f32(dim, a=0.1), "rel_pos_h": f32(13, D, a=0.5), "rel_pos_w": f32(41, D, a=0.5)}
    x, g = f32(B, H, W, dim), f32(B, H, W, dim)
    names = ["qkv.weight", "qkv.bias", "proj.weight", "rel_pos_h", "rel_pos_w"]
    m = Attention(dim, heads, use_rel_pos=True, input_size=(7, 21))
    m.load_state_dict({k_: torch.from_numpy(v_) for k_, v_ in sd.items()})
    m = m.to("cuda:0").train()
    xg = torch.from_numpy(x).to("cuda:0").requires_grad_()
    (m(xg) * torch.from_numpy(g).to("cuda:0")).sum().backward()
    got = [xg.grad] + [dict(m.named_parameters())[n].grad for n in names]

    def compose(dtype, mag=False):
        """the module in plain torch ops on the CPU; mag: the same graph on magnitudes, softmax rows as constants, every product
        of the backward positive -- the per-element scale"""
        p = {n: torch.from_numpy(t).to(dtype).requires_grad_() for n, t in sd.items()}
        xt = torch.from_numpy(x).to(dtype).requires_grad_()
        res = lambda t, n: torch.nn.functional.interpolate(t.reshape(1, t.shape[0], -1).permute(0, 2, 1), size=n, mode="linear") \
            .reshape(-1, n).permute(1, 0)
        qkv = (xt.reshape(B, H * W, dim) @ p["qkv.weight"].T + p["qkv.bias"]).reshape(B, H * W, 3, heads, D).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        Rh, Rw = res(p["rel_pos_h"], 2 * H - 1), res(p["rel_pos_w"], 2 * W - 1)
        idx = torch.arange(H)[:, None] - torch.arange(H)[None, :] + H - 1
        r = q.reshape(B, heads, H, W, D)
        S = (D ** -0.5 * (q @ k.transpose(-1, -2))).reshape(B, heads, H, W, H, W) \
            + torch.einsum("bahwc,hkc->bahwk", r, Rh[idx])[..., :, None] + torch.einsum("bahwc,wkc->bahwk", r, Rw[idx])[..., None, :]
        o = torch.softmax(S.reshape(B, heads, H * W, H * W), -1) @ v
        y = o.permute(0, 2, 1, 3).reshape(B, H * W, dim) @ p["proj.weight"].T + p["proj.bias"]
        (y.reshape(B, H, W, dim) * torch.from_numpy(g).to(dtype)).sum().backward()
        return [xt.grad.numpy()] + [p[n].grad.numpy() for n in names], (q, k, v, (Rh, Rw))

    ref, (q, k, v, rel) = compose(torch.float64)
    ref32, _ = compose(torch.float32)
    # scale: the attention's own (magnitudes with the logit factor, dO = |g| |proj.weight|) pushed through the magnitudes of the linears
    # and of the interpolation; proj.weight: |g|^T applied to the forward's scale
    n64 = lambda t: t.detach().numpy().astype(np.float64)
    q, k, v, rel = n64(q), n64(k), n64(v), tuple(n64(t) for t in rel)
    aW, aP, ax, ag = np.abs(sd["qkv.weight"]).astype(np.float64), np.abs(sd["proj.weight"]).astype(np.float64), np.abs(x.reshape(-1, dim)), \
        np.abs(g.reshape(B, H * W, dim)).astype(np.float64)
    dO = (ag @ aP).reshape(B, H * W, heads, D).transpose(0, 2, 1, 3)
    sq, sk, sv, sRh, sRw = RB.magnitudes(q, k, v, dO, (H, W), None, rel, logit_factor=True)
    sqkv = np.stack([t.transpose(0, 2, 1, 3) for t in (sq, sk, sv)], axis=2).reshape(B * H * W, 3 * dim)
    s_att = R.attention(q, k, np.abs(v), (H, W), None, rel) * (1.0 + R.logits(np.abs(q), np.abs(k), (H, W), None, tuple(np.abs(t) for t in rel)).max(-1, keepdims=True))

    def interp_T(s, L):      # the adjoint of the (non-negative) interpolation weights applied to a scale
        t = torch.zeros(L, D, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.interpolate(t.reshape(1, L, -1).permute(0, 2, 1), size=s.shape[0], mode="linear").reshape(-1, s.shape[0]) \
            .permute(1, 0).backward(torch.from_numpy(s))
        return t.grad.numpy()

    scales = [(sqkv @ aW).reshape(B, H, W, dim) + 1.0, sqkv.T @ ax + 1.0, sqkv.sum(0) + 1.0,
              ag.reshape(-1, dim).T @ s_att.transpose(0, 2, 1, 3).reshape(B * H * W, dim) + 1.0, interp_T(sRh, 13) + 1.0, interp_T(sRw, 41) + 1.0]
    for name, a, r64, r32, sc in zip(["x"] + names, got, ref, ref32, scales):
        units, e32 = judge.units(a.double().cpu().numpy(), r64, sc), judge.units(r32, r64, sc)
        print(f"ATTN_BWD_ERR vit.Attention 14x14 f32 d{name}: kernel {units:.2f} f32 {e32:.2f}")
        assert judge.within(units, e32), (name, units, e32)


def test_refusals():
    from torch_em_amd import ops
    t = lambda *s: torch.zeros(s, device="cuda:0")
    with pytest.raises(ValueError, match="out="):
        ops.attention(t(1, 1, 4, 64).requires_grad_(), t(1, 1, 4, 64), t(1, 1, 4, 64), (2, 2), out=t(1, 1, 4, 64))
    big = t(1, 1, 256 * 65, 64)
    with pytest.raises(ValueError, match="exceeds"):
        ops.attention(big.requires_grad_(), big, big, (256, 65))
