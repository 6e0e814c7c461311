"""Building blocks of the SAM vision transformer on the MI355X path (reference: torch_em/model/vit.py, which wraps
segment_anything's ImageEncoderViT).  So far the attention layer: its hot path is ops.attention, the linears are torch's."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def resample_rel_pos(table: torch.Tensor, size: int) -> torch.Tensor:
    """A relative-position table [L, D] at the length 2 * size - 1 a grid side of `size` tokens needs: itself, or its linear
    interpolation along L (segment_anything's get_rel_pos)."""
    need = 2 * size - 1
    if table.shape[0] == need:
        return table
    res = F.interpolate(table.detach().float().reshape(1, table.shape[0], -1).permute(0, 2, 1), size=need, mode="linear")
    return res.reshape(-1, need).permute(1, 0).to(table.dtype).contiguous()


class Attention(nn.Module):
    """segment_anything's multi-head attention block with decomposed relative position embeddings: same signature, same
    state_dict keys (qkv.weight/bias, proj.weight/bias, rel_pos_h, rel_pos_w).  forward(x [B, H, W, C]) -> [B, H, W, C]:
    the qkv linear, ops.attention on the three views of its packed output, writing [B, H, W, heads * D] in place for the
    proj linear.  Inference only."""

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
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("model.vit.Attention is inference only: the backward kernel of ops.attention (k_attn_bwd) does "
                                      "not exist yet; call it under torch.no_grad()")
        B, H, W, C = x.shape
        nH, D = self.num_heads, C // self.num_heads
        qkv = self.qkv(x).reshape(B, H * W, 3, nH, D)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [B, nH, N, D] views, read in place
        y = torch.empty((B, H, W, C), dtype=qkv.dtype, device=qkv.device)
        ops.attention(q, k, v, (H, W), scale=self.scale, rel_pos=self._rel_pos(H, W, qkv.dtype) if self.use_rel_pos else None,
                      out=y.view(B, H * W, nH, D).permute(0, 2, 1, 3))
        return self.proj(y)
