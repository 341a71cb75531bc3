"""Weight-only fp8 linear layer for few rows (``chipmunk_w8_linear``; DESIGN 4.2, "Weight-only forward for few rows"; not in the reference).

    S[m, i] = sum_k x[m, k] * f(weight[i, k])            f widens e4m3 exactly; fp32, from zero
    y[m, i] = bf16(bf16(S[m, i] * scale[i]) + bias[i])    (without a bias: bf16(S[m, i] * scale[i]))

On the GPU the e4m3 weight is streamed once and widened in registers; on CPU tensors the same definition runs in torch.
"""
from __future__ import annotations

from typing import Optional

import torch


def w8_linear_torch(x2: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The definition in torch on ``x2 [M, K]``: an fp32 matmul with the widened weight, then the two roundings."""
    s = scale.reshape(-1).float()
    t = ((x2.float() @ weight.float().T) * (s if s.numel() > 1 else s[0])).to(torch.bfloat16)
    return t if bias is None else (t.float() + bias.float()).to(torch.bfloat16)


def w8_linear(x: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x [..., K]`` bf16, ``weight [F, K]`` ``float8_e4m3fn``, ``scale`` fp32 with one element or ``F`` (the weight's reciprocal
    quantisation scale: ``W8Linear.scale_reciprocal``), ``bias`` bf16 ``[F]`` or None -> ``[..., F]`` bf16.  The rows of ``x`` are flattened;
    the bits of an output row depend on its input row only, not on the row count.  GPU: ``K % 64 == 0`` and ``F % 8 == 0``."""
    if weight.dtype != torch.float8_e4m3fn or weight.dim() != 2:
        raise ValueError(f"w8_linear: weight must be a float8_e4m3fn [F, K] tensor (got {weight.dtype}, {weight.dim()} dimensions)")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"w8_linear: x must be bfloat16 (got {x.dtype})")
    F, K = weight.shape
    if x.dim() < 1 or x.shape[-1] != K:
        raise ValueError(f"w8_linear: x must be [..., K] with K = {K}, the weight's in_features (got {tuple(x.shape)})")
    if scale.dtype != torch.float32 or scale.numel() not in (1, F):
        raise ValueError(f"w8_linear: scale must be float32 with one element or F = {F} (got {scale.dtype}, {scale.numel()} elements)")
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.numel() != F):
        raise ValueError(f"w8_linear: bias must be bfloat16 with F = {F} elements (got {bias.dtype}, {bias.numel()} elements)")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K)
    if not x.is_cuda:
        return w8_linear_torch(x2, weight, scale, bias).view(*lead, F)
    if K % 64 != 0 or F % 8 != 0 or x2.shape[0] < 1:
        raise ValueError(f"w8_linear: on the GPU K must be a multiple of 64, F a multiple of 8 and x hold at least one row "
                         f"(got K = {K}, F = {F}, {x2.shape[0]} rows)")
    if x2.stride(1) != 1 or x2.stride(0) % 8 != 0 or x2.data_ptr() % 16 != 0:
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], F), dtype=torch.bfloat16, device=x.device)
    torch.ops.chipmunk.w8_linear(x2, weight.contiguous(), scale.reshape(-1).contiguous(), None if bias is None else bias.contiguous(), y)
    return y.view(*lead, F)


__all__ = ["w8_linear", "w8_linear_torch"]
