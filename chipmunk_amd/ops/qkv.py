"""Projection output -> attention operands (caller-side glue of the attention ops, SURVEY 8f "callers either side of the path").

The reference's blocks do this in model code (``examples/hunyuan/hyvideo/modules/models.py:188-193, 376-381``):
``rearrange(qkv, "B L (K H D) -> K B L H D")``, ``RMSNorm(head_dim)`` on q and k (``norm_layers.py:43-58``), the rotary embedding of
the image tokens (``posemb_layers.py:133-172``), then the transposes to the ``[B, H, L, D]`` operands of ``chipmunk.*`` attention.  ``qkv_split_norm`` is that sequence as one HBM pass on the GPU
(``chipmunk_qkv_split_norm``); on CPU tensors it is the reference's op sequence itself.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch


def _rms_norm_reference(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """norm_layers.py:43-58: normalise in fp32, cast back, multiply by the weight in the tensor's dtype."""
    xf = x.float()
    out = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).type_as(x)
    return out if weight is None else out * weight


def _rotary_reference(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """posemb_layers.py:133-172, (cos, sin) form, on ``x [1, H, rows, 128]`` with ``cos, sin [rows, 128]``."""
    xf = x.float()
    re, im = xf.reshape(*xf.shape[:-1], -1, 2).unbind(-1)
    rot = torch.stack([-im, re], dim=-1).flatten(-2)
    return (xf * cos + rot * sin).type_as(x)


def qkv_split_norm(qkv: torch.Tensor, q_weight: Optional[torch.Tensor], k_weight: Optional[torch.Tensor], heads: int,
                   eps: float = 1e-6, freqs_cos: Optional[torch.Tensor] = None,
                   freqs_sin: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """``qkv [n, >= 3*heads*128]`` (one batch element's projection rows) -> ``[q, k, v]``, each ``[1, heads, n, 128]``, q and k
    RMS-normalised over the head dimension and -- with ``freqs_cos / freqs_sin`` fp32 ``[rows, 128]`` -- rotated (rotary
    embedding of the first ``rows`` tokens: the image tokens; the text tokens behind them carry none)."""
    if qkv.is_cuda:
        return torch.ops.chipmunk.qkv_split_norm(qkv, q_weight, k_weight, heads, eps, freqs_cos, freqs_sin)
    n = qkv.shape[0]
    q, k, v = qkv[:, :3 * heads * 128].reshape(n, 3, heads, 128).permute(1, 2, 0, 3).unsqueeze(1)   # [3][1, H, n, 128]
    q, k = _rms_norm_reference(q, q_weight, eps).contiguous(), _rms_norm_reference(k, k_weight, eps).contiguous()
    if freqs_cos is not None:
        r = freqs_cos.shape[0]
        q[:, :, :r] = _rotary_reference(q[:, :, :r], freqs_cos, freqs_sin)
        k[:, :, :r] = _rotary_reference(k[:, :, :r], freqs_cos, freqs_sin)
    return [q, k, v.contiguous()]


# ------------------------------------------------------------------------------------------------ Wan: row-wide norm + rotary
def _wan_rms_norm_reference(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """``WanRMSNorm.forward`` (``examples/wan/wan/modules/model.py:89-97``) over the whole row: ``_norm(x.float()).type_as(x) * weight``
    -- a bf16 weight gives a bf16 product, an fp32 weight (Wan's parameters under its bf16 autocast) an fp32 one."""
    xf = x.float()
    out = (xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)).type_as(x)
    return out if weight is None else out * weight


def _wan_rope_reference(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """``rope_apply`` (``model.py:49-78``) on ``x [B, L, H, 128]`` with the multipliers of the first ``rows`` tokens given as the
    operator's tables (``cos, sin [rows, 128]``, the pair's angle in both entries): complex product in float64, the tokens behind
    ``rows`` appended unchanged (``:74``), ``.float()`` (``:78``)."""
    B, L, H, D = x.shape
    rows = cos.shape[0]
    freqs = torch.complex(cos[:, 0::2].to(torch.float64), sin[:, 0::2].to(torch.float64)).view(1, rows, 1, D // 2)
    xi = torch.view_as_complex(x[:, :rows].to(torch.float64).reshape(B, rows, H, D // 2, 2))
    out = torch.view_as_real(xi * freqs).flatten(3)
    return torch.cat([out, x[:, rows:].to(torch.float64)], dim=1).float()


def split_heads_rownorm(x: torch.Tensor, heads: int, weights: Sequence[Optional[torch.Tensor]] = (None, None, None),
                        norm: Sequence[bool] = (True, True, False), rope: Sequence[bool] = (False, False, False), eps: float = 1e-6,
                        freqs_cos: Optional[torch.Tensor] = None, freqs_sin: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """Wan's attention operands in one pass (``chipmunk_split_heads_rownorm``).  ``x [B, n, >= parts*heads*128]`` or ``[n, ...]`` bf16
    holds ``parts = len(norm)`` (1 .. 3) consecutive blocks of ``heads*128`` columns; part ``p`` comes back as ``[B, heads, n, 128]``
    bf16.  ``norm[p]``: ``WanRMSNorm`` over the whole row of the part (``model.py:81-97``), then ``weights[p]`` (``None``, bf16 or fp32
    ``[heads*128]``; an fp32 weight keeps the product in fp32, as torch does); ``rope[p]``: the rotation of ``rope_apply``
    (``:49-78``) for the first ``freqs_cos.shape[0]`` tokens, tables fp32 ``[rows, 128]`` as :func:`wan_rope_table` builds them;
    every value is rounded once to bf16 at the end (``:164``).  A part with neither is a bit copy (v).  Self-attention:
    ``norm=(True, True, False), rope=(True, True, False)`` on the q | k | v projection; the cross-attention keys
    (``:195-197``): ``norm=(True, False)`` on k | v without tables.  On CPU tensors: the reference's op sequence, float64 rotation included."""
    parts = len(norm)
    weights, rope = tuple(weights)[:parts] + (None,) * max(0, parts - len(weights)), tuple(rope)[:parts] + (False,) * max(0, parts - len(rope))
    if not 1 <= parts <= 3 or not 1 <= heads <= 64:
        raise ValueError("split_heads_rownorm: 1 .. 3 parts and 1 .. 64 heads")
    if any(w is not None and not nm for w, nm in zip(weights, norm)):
        raise ValueError("split_heads_rownorm: a weight belongs to a part that is not normalised")
    if (freqs_cos is None) != (freqs_sin is None) or (any(rope) and freqs_cos is None):
        raise ValueError("split_heads_rownorm: a rotated part needs freqs_cos and freqs_sin, and they come together")
    if x.is_cuda:
        w = list(weights) + [None] * (3 - parts)
        return torch.ops.chipmunk.split_heads_rownorm(x, heads, parts, w[0], w[1], w[2], sum(1 << p for p in range(parts) if norm[p]),
                                                      sum(1 << p for p in range(parts) if rope[p]), eps, freqs_cos, freqs_sin)
    xb = x if x.dim() == 3 else x.unsqueeze(0)
    B, n, C = xb.shape[0], xb.shape[1], heads * 128
    if x.dtype != torch.bfloat16 or xb.shape[2] < parts * C or (freqs_cos is not None and freqs_cos.shape[0] > n):
        raise ValueError("split_heads_rownorm: x must be bfloat16 [B, n, >= parts*heads*128] and the tables no longer than n")
    out = []
    for p in range(parts):
        t = xb[:, :, p * C:(p + 1) * C]
        if norm[p]:
            t = _wan_rms_norm_reference(t, weights[p], eps)
        t = t.reshape(B, n, heads, 128)                                               # .view(b, s, n, d), model.py:155-157
        if rope[p]:
            t = _wan_rope_reference(t, freqs_cos, freqs_sin)
        out.append(t.permute(0, 2, 1, 3).to(torch.bfloat16).contiguous())             # model.py:164
    return out


_ROPE_TABLES: Dict[Tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def wan_rope_table(grid: Sequence[int], voxel_shape: Optional[Sequence[int]] = (4, 6, 8), head_dim: int = 128, theta: float = 10000,
                   device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(cos, sin)`` fp32 ``[f*h*w, head_dim]`` for :func:`split_heads_rownorm`: Wan's three-axis rotary multipliers of a
    ``grid = (f, h, w)`` latent.  ``rope_params`` (``model.py:37-44``) with the split of ``:501-503`` -- ``d - 4*(d//6)`` channels
    (22 complex frequencies at 128) turn with the frame, ``2*(d//6)`` (21) with the height and as many with the width -- taken per
    token as ``rope_apply`` does (``:53, 63-68``), computed in float64 and rounded once; each pair's value sits in both of its
    entries.  Rows are in raster order, or -- with a ``voxel_shape`` -- in the token order of ``voxel_chunk_no_padding`` (``:69-70``:
    the order Wan's tokens are in when they reach the attention).  Host code, cached per arguments like ``_reorder.index_map``."""
    f, h, w = (int(v) for v in grid)
    vs = None if voxel_shape is None else tuple(int(v) for v in voxel_shape)
    dev = torch.device("cpu") if device is None else torch.device(device)
    key = (f, h, w, vs, int(head_dim), float(theta), str(dev))
    hit = _ROPE_TABLES.get(key)
    if hit is None:
        d = int(head_dim)
        if d % 2:
            raise ValueError("wan_rope_table: head_dim must be even")

        def angles(length, dim):                                                      # rope_params, model.py:39-42
            return torch.outer(torch.arange(length), 1.0 / torch.pow(theta, torch.arange(0, dim, 2).to(torch.float64).div(dim)))
        ang = torch.cat([angles(f, d - 4 * (d // 6)).view(f, 1, 1, -1).expand(f, h, w, -1),      # model.py:63-67
                         angles(h, 2 * (d // 6)).view(1, h, 1, -1).expand(f, h, w, -1),
                         angles(w, 2 * (d // 6)).view(1, 1, w, -1).expand(f, h, w, -1)], dim=-1)  # [f, h, w, d/2] float64
        fr = torch.polar(torch.ones_like(ang), ang)                                  # model.py:43
        tab = torch.stack([fr.real, fr.imag]).repeat_interleave(2, dim=-1).float()    # [2, f, h, w, d]: both entries of a pair
        if vs is not None:
            from .voxel import _voxel_chunk_torch
            tab = _voxel_chunk_torch(tab.unsqueeze(0), vs).squeeze(0)                 # [b=1, ah=2, f, h, w, d] -> [2, f*h*w, d]
        tab = tab.reshape(2, f * h * w, d).contiguous().to(dev)
        hit = _ROPE_TABLES[key] = (tab[0], tab[1])
    return hit


__all__ = ["qkv_split_norm", "split_heads_rownorm", "wan_rope_table"]


def residual_ln_modulate(x: torch.Tensor, y: Optional[torch.Tensor], gate: Optional[torch.Tensor], shift: torch.Tensor,
                         scale: torch.Tensor, eps: float = 1e-6):
    """The block's row-wise chain between two GEMMs as one HBM pass (``chipmunk_residual_ln_modulate``): with ``y`` and ``gate``
    ``x = x + gate * y`` first (``models.py:262-275, 431``), then ``xm = LayerNorm(x) * (1 + scale) + shift`` (``modulate(norm(x))``,
    ``models.py:184-186``; LayerNorm without affine).  Returns ``(x, xm)``.  On CPU tensors: the reference's torch sequence."""
    if x.is_cuda:
        out = torch.ops.chipmunk.residual_ln_modulate(x, y, gate, shift, scale, eps)
        return (out[0], out[1]) if y is not None else (x, out[0])      # (the operator never returns its own input)
    if y is not None:
        x = torch.addcmul(x, gate, y)
    xn = torch.nn.functional.layer_norm(x, (x.shape[-1],), eps=eps)
    return x, torch.addcmul(shift, xn, 1 + scale)


def _per_sequence(v: torch.Tensor, name: str, B: int, C: int) -> torch.Tensor:
    """A per-sequence vector as ``[1 or B, 1, C]``: fp32 ``[C]``, ``[B, C]`` or ``[B, 1, C]`` with a batch dimension of 1 or B."""
    if v.dtype != torch.float32:
        raise ValueError(f"residual_ln_modulate_f32: {name} must be float32 (Wan's modulation is, model.py:317)")
    ok = (v.dim() == 1 and v.shape[0] == C) or (v.dim() == 2 and v.shape[1] == C) or (v.dim() == 3 and v.shape[1] == 1 and v.shape[2] == C)
    if not ok or (v.dim() > 1 and v.shape[0] not in (1, B)):
        raise ValueError(f"residual_ln_modulate_f32: {name} must be [C], [B, C] or [B, 1, C] with a batch dimension of 1 or B = {B} "
                         f"(got {tuple(v.shape)})")
    return v.reshape(-1, 1, C)


def _wan_block_glue_reference(x, y, gate, shift, scale, weight, bias, eps):
    """The reference's torch sequence for one use of the block glue, on ``x [B, L, C]`` with vectors ``[1 or B, 1, C]``: ``x + y * e``
    (``model.py:327, 334``; fp32 by promotion, what the fp32 autocast around those lines leaves) or ``x + y`` (``:331``), ``WanLayerNorm``
    (``:110``), then the modulation in fp32 (``:324, :332``) or the affine ``norm3`` (``:283-285``), bf16 as the next Linear takes it."""
    C = x.shape[-1]
    if y is not None:
        x = x + (y * gate if gate is not None else y)
    norm = lambda w, b: torch.nn.functional.layer_norm(x.float(), (C,), w, b, eps).type_as(x)      # noqa: E731
    if weight is not None:
        return x, norm(weight.float(), bias.float()).to(torch.bfloat16)
    return x, (norm(None, None).float() * (1 + scale) + shift).to(torch.bfloat16)


def residual_ln_modulate_f32(x: torch.Tensor, y: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
                             shift: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                             weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, eps: float = 1e-6):
    """A Wan block's row-wise chain between two GEMMs as one HBM pass (``chipmunk_residual_ln_modulate_f32``): the residual stream
    is fp32 and the vectors are fp32, one set per sequence (``examples/wan/wan/modules/model.py:317-334``).

    ``x [B, L, C]`` or ``[L, C]``, fp32 or (before the first block) bf16; ``y`` bf16 of that shape or ``None``; ``gate`` and the pair
    ``shift`` / ``scale`` fp32 ``[C]``, ``[B, C]`` or ``[B, 1, C]``; or, instead of the modulation, ``weight`` / ``bias`` ``[C]``
    (``norm3``, ``:283-285``).  With ``y``: ``x_out = x.float() + y.float() * gate`` (``:327, :334``; without a gate ``x + y``, ``:331``),
    fp32.  Then ``xm = bf16(norm(x_out).float() * (1 + scale) + shift)`` (``:324, :332``) or ``bf16(norm3(x_out))``, where ``norm`` is
    ``WanLayerNorm`` (``:100-110``): statistics in fp32, ``.type_as(x)`` -- a rounding only for a bf16 ``x``.  Returns ``(x_out, xm)``;
    without ``y`` the caller's ``x`` comes back as ``x_out``.  On CPU tensors: the reference's torch sequence."""
    if x.dim() not in (2, 3) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise ValueError("residual_ln_modulate_f32: x must be a contiguous float32 or bfloat16 [B, L, C] or [L, C]")
    B, C = (x.shape[0] if x.dim() == 3 else 1), x.shape[-1]
    if C % 8 or C > 8192:
        raise ValueError(f"residual_ln_modulate_f32: C must be a multiple of 8, at most 8192 (got {C})")
    if y is None and gate is not None:
        raise ValueError("residual_ln_modulate_f32: a gate without y")
    if y is not None and (y.dtype != torch.bfloat16 or y.shape != x.shape):
        raise ValueError("residual_ln_modulate_f32: y must be bfloat16 of x's shape")
    if y is not None and gate is None and x.dtype == torch.bfloat16:
        raise ValueError("residual_ln_modulate_f32: a bfloat16 x takes its residual with a gate (torch would keep x + y in bfloat16)")
    if (shift is None) != (scale is None) or (weight is None) != (bias is None) or (shift is None) == (weight is None):
        raise ValueError("residual_ln_modulate_f32: exactly one pair of (shift, scale) and (weight, bias)")
    vecs = {n: _per_sequence(v, n, B, C) for n, v in (("gate", gate), ("shift", shift), ("scale", scale)) if v is not None}
    if weight is not None and (weight.shape != (C,) or bias.shape != (C,)):
        raise ValueError("residual_ln_modulate_f32: weight / bias must be [C]")
    if x.is_cuda:
        out = torch.ops.chipmunk.residual_ln_modulate_f32(x, y, gate, shift, scale, weight, bias, eps)
        return (out[0], out[1]) if y is not None else (x, out[0])      # (the operator never returns its own input)
    x_out, xm = _wan_block_glue_reference(x if x.dim() == 3 else x.unsqueeze(0), None if y is None else y.reshape(B, -1, C), vecs.get("gate"),
                                          vecs.get("shift"), vecs.get("scale"), weight, bias, eps)
    return (x_out.reshape(x.shape) if y is not None else x), xm.reshape(x.shape)
