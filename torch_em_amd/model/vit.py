"""Building blocks of the SAM vision transformer on the MI355X path (reference: torch_em/model/vit.py, which wraps
segment_anything's ImageEncoderViT): the attention layer and the transformer block.  Their hot paths are ops.attention and the
fused row kernels of csrc/vit_block.hip; the linears are torch's."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def resample_rel_pos(table: torch.Tensor, size: int, keep_graph: bool = False) -> torch.Tensor:
    """A relative-position table [L, D] at the length 2 * size - 1 a grid side of `size` tokens needs: itself, or its linear
    interpolation along L (segment_anything's get_rel_pos).  `keep_graph`: differentiable with respect to `table`."""
    need = 2 * size - 1
    if table.shape[0] == need:
        return table
    src = table if keep_graph else table.detach()
    res = F.interpolate(src.float().reshape(1, table.shape[0], -1).permute(0, 2, 1), size=need, mode="linear")
    return res.reshape(-1, need).permute(1, 0).to(table.dtype).contiguous()


class _PackedAttention(torch.autograd.Function):
    """ops.attention on the three views of a packed qkv-linear output [B, N, 3, nH, D] -> [B, H, W, nH D]; the backward
    writes dq, dk, dv through strides into ONE packed buffer, the single gradient of the qkv output."""

    @staticmethod
    def forward(ctx, qkv, rel_h, rel_w, H, W, scale):
        B, N, _, nH, D = qkv.shape
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        y = torch.empty((B, H, W, nH * D), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B, nH, N), dtype=torch.float32, device=qkv.device)
        ops._attn_fwd(q, k, v, H, W, scale, (rel_h, rel_w), y.view(B, N, nH, D).permute(0, 2, 1, 3), lse)
        ctx.save_for_backward(qkv, y, lse, rel_h, rel_w)
        ctx.conf = (H, W, scale)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        qkv, y, lse, rel_h, rel_w = ctx.saved_tensors
        B, N, _, nH, D = qkv.shape
        heads = lambda t: t.reshape(B, N, nH, D).permute(0, 2, 1, 3)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        want = rel_h is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        drh, drw = ops._attn_bwd(q, k, v, heads(y), heads(dy), lse, *ctx.conf, (rel_h, rel_w), dq, dk, dv, want)
        if want:
            drh, drw = drh.to(rel_h.dtype), drw.to(rel_w.dtype)
        return dqkv, drh, drw, None, None, None


class Attention(nn.Module):
    """segment_anything's multi-head attention block with decomposed relative position embeddings: same signature, same
    state_dict keys (qkv.weight/bias, proj.weight/bias, rel_pos_h, rel_pos_w).  forward(x [B, H, W, C]) -> [B, H, W, C]:
    the qkv linear, ops.attention on the three views of its packed output, writing [B, H, W, heads * D] in place for the
    proj linear.  In training mode (module.train()) under grad the fused backward of ops.attention runs: one packed gradient
    for the qkv output, and rel_pos_h / rel_pos_w get theirs through the resampling (no table cache in that path).  In eval
    mode the module is inference only: under grad it raises NotImplementedError; call it under torch.no_grad()."""

    def __init__(self, dim, num_heads=8, qkv_bias=True, use_rel_pos=False, rel_pos_zero_init=True, input_size=None):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.use_rel_pos = use_rel_pos
        if use_rel_pos:
            assert input_size is not None, "Input size must be provided if using relative positional encoding."
            self.rel_pos_h = nn.Parameter(torch.zeros(2 * input_size[0] - 1, head_dim))
            self.rel_pos_w = nn.Parameter(torch.zeros(2 * input_size[1] - 1, head_dim))
        self._tables = None   # (key, (Rh, Rw)): the tables resampled for the grid last seen

    def _rel_pos(self, H, W, dtype):
        src = (self.rel_pos_h, self.rel_pos_w)
        key = (H, W, dtype) + tuple((t.data_ptr(), t._version, t.device) for t in src)
        if self._tables is None or self._tables[0] != key:
            self._tables = (key, tuple(resample_rel_pos(t.detach(), s).to(dtype) for t, s in zip(src, (H, W))))
        return self._tables[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, H, W, C = x.shape
        nH, D = self.num_heads, C // self.num_heads
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if not self.training:
                raise NotImplementedError("model.vit.Attention in eval mode is inference only: the backward pass runs in training mode "
                                          "(module.train()); call it under torch.no_grad()")
            qkv = self.qkv(x).reshape(B, H * W, 3, nH, D)
            tables = (None, None)
            if self.use_rel_pos:
                tables = tuple(resample_rel_pos(t, s, keep_graph=True).to(qkv.dtype).contiguous()
                               for t, s in zip((self.rel_pos_h, self.rel_pos_w), (H, W)))
            ops._attn_ws_bytes("tem_attention_bwd_ws", qkv[:, :, 0].permute(0, 2, 1, 3), H, W, self.use_rel_pos)   # refuse before the forward
            return self.proj(_PackedAttention.apply(qkv.contiguous(), tables[0], tables[1], H, W, self.scale))
        qkv = self.qkv(x).reshape(B, H * W, 3, nH, D)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [B, nH, N, D] views, read in place
        y = torch.empty((B, H, W, C), dtype=qkv.dtype, device=qkv.device)
        ops.attention(q, k, v, (H, W), scale=self.scale, rel_pos=self._rel_pos(H, W, qkv.dtype) if self.use_rel_pos else None,
                      out=y.view(B, H * W, nH, D).permute(0, 2, 1, 3))
        return self.proj(y)


class MLPBlock(nn.Module):
    """segment_anything's MLPBlock (lin1, GELU, lin2; state_dict keys lin1.weight/bias, lin2.weight/bias).  lin1 runs without
    its bias, which ops.bias_gelu adds in the same pass as the exact GELU; `act` must be nn.GELU in its erf form."""

    def __init__(self, embedding_dim, mlp_dim, act=nn.GELU):
        super().__init__()
        self.lin1 = nn.Linear(embedding_dim, mlp_dim)
        self.lin2 = nn.Linear(mlp_dim, embedding_dim)
        self.act = act()
        if not isinstance(self.act, nn.GELU) or self.act.approximate != "none":
            raise ValueError("MLPBlock: the fused kernel computes the exact (erf) nn.GELU; other activations are not supported")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.lin2(ops.bias_gelu(F.linear(x, self.lin1.weight), self.lin1.bias))


class Block(nn.Module):
    """segment_anything's transformer block: same signature, same state_dict keys (norm1.*, attn.*, norm2.*, mlp.lin1.*,
    mlp.lin2.*).  forward(x [B, H, W, C]) -> [B, H, W, C]:
        xw = ops.layer_norm_windows(x, norm1, window_size)        LayerNorm + pad + window partition, one pass
        a = attn(xw)                                              on the windows, or on the whole grid for window_size 0
        x1, xn = ops.window_merge_norm(a, x, norm2, window_size)  un-partition + crop + residual add + LayerNorm, one pass
        out = x1 + lin2(ops.bias_gelu(lin1_without_bias(xn), lin1.bias))
    Padded windows carry their zero tokens through attention unmasked, as SAM does.  norm_layer must build an affine
    nn.LayerNorm and act_layer the exact nn.GELU (ValueError otherwise).  Training: as Attention (module.train() under grad)."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, norm_layer=nn.LayerNorm, act_layer=nn.GELU, use_rel_pos=False,
                 rel_pos_zero_init=True, window_size=0, input_size=None):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, use_rel_pos=use_rel_pos, rel_pos_zero_init=rel_pos_zero_init,
                              input_size=input_size if window_size == 0 else (window_size, window_size))
        self.norm2 = norm_layer(dim)
        for n in (self.norm1, self.norm2):
            if not isinstance(n, nn.LayerNorm) or not n.elementwise_affine or n.bias is None or tuple(n.normalized_shape) != (dim,):
                raise ValueError("Block: norm_layer must build an affine nn.LayerNorm over the channels")
        self.mlp = MLPBlock(embedding_dim=dim, mlp_dim=int(dim * mlp_ratio), act=act_layer)
        self.window_size = window_size

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        ws = self.window_size
        xw = ops.layer_norm_windows(x, self.norm1.weight, self.norm1.bias, self.norm1.eps, ws)
        x1, xn = ops.window_merge_norm(self.attn(xw), x, self.norm2.weight, self.norm2.bias, self.norm2.eps, ws)
        return x1 + self.mlp(xn)
