"""Weight-only MXFP4 linear layer for few rows (``chipmunk_w4_linear``; DESIGN 4.2, "MXFP4 forward for few rows"; not in the reference).

    S[m, i] = sum_k x[m, k] * wide(weight)[i, k]      wide = W4Linear.widened(): e2m1 * 2^(block_scale - 127), exact in bf16; fp32, from zero
    y[m, i] = bf16(S[m, i] + float(bias[i]))          one rounding (without a bias: bf16(S[m, i]))

On the GPU the packed weight and its e8m0 bytes are streamed once and widened in registers; on CPU tensors the same definition runs in torch.
"""
from __future__ import annotations

from typing import Optional

import torch

from .mlp import MXFP4_SCALES, MXFP4_WEIGHTS


def widen_mxfp4(weight: torch.Tensor, block_scale: torch.Tensor) -> torch.Tensor:
    """fp32 ``[F, K]`` of uint8 ``weight [F, K / 2]`` (element ``2j`` in bits 0 .. 3 of byte ``j``) and ``block_scale [F, K / 32]``: exact,
    the values of ``W4Linear.widened()``."""
    from ..modules.mlp_fp8 import E2M1_VALUES
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=weight.device)
    nib = torch.stack((weight & 15, weight >> 4), dim=2).reshape(weight.shape[0], -1)
    return torch.ldexp(table[nib.long()], (block_scale.to(torch.int32) - 127).repeat_interleave(32, dim=1))


def w4_linear_torch(x2: torch.Tensor, weight: torch.Tensor, block_scale: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The definition in torch on ``x2 [M, K]``: an fp32 matmul with the widened weight, the bias added in fp32, one rounding."""
    s = x2.float() @ widen_mxfp4(weight, block_scale).T
    return (s if bias is None else s + bias.float()).to(torch.bfloat16)


def w4_linear(x: torch.Tensor, weight: torch.Tensor, block_scale: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x [..., K]`` bf16, ``weight [F, K / 2]`` uint8 / ``float4_e2m1fn_x2``, ``block_scale [F, K / 32]`` uint8 / ``float8_e8m0fnu``
    (``W4Linear.weight`` / ``.block_scale``), ``bias`` bf16 ``[F]`` or None -> ``[..., F]`` bf16.  The rows of ``x`` are flattened; the bits
    of an output row depend on its input row only, not on the row count.  GPU: ``K % 128 == 0`` and ``F % 8 == 0``."""
    if weight.dtype not in MXFP4_WEIGHTS or weight.dim() != 2:
        raise ValueError(f"w4_linear: weight must be a uint8 or float4_e2m1fn_x2 [F, K / 2] tensor (got {weight.dtype}, {weight.dim()} dimensions)")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"w4_linear: x must be bfloat16 (got {x.dtype})")
    F, K = weight.shape[0], weight.shape[1] * 2
    if x.dim() < 1 or x.shape[-1] != K:
        raise ValueError(f"w4_linear: x must be [..., K] with K = {K}, twice the weight's bytes per row (got {tuple(x.shape)})")
    if block_scale.dtype not in MXFP4_SCALES or K % 32 or tuple(block_scale.shape) != (F, K // 32):
        raise ValueError(f"w4_linear: block_scale must be uint8 or float8_e8m0fnu [F, K / 32] = {(F, K // 32)} with K a multiple of 32 "
                         f"(got {block_scale.dtype} {tuple(block_scale.shape)})")
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.numel() != F):
        raise ValueError(f"w4_linear: bias must be bfloat16 with F = {F} elements (got {bias.dtype}, {bias.numel()} elements)")
    weight, block_scale = weight.view(torch.uint8), block_scale.view(torch.uint8)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K)
    if not x.is_cuda:
        return w4_linear_torch(x2, weight, block_scale, bias).view(*lead, F)
    if K % 128 != 0 or F % 8 != 0 or x2.shape[0] < 1:
        raise ValueError(f"w4_linear: on the GPU K must be a multiple of 128, F a multiple of 8 and x hold at least one row "
                         f"(got K = {K}, F = {F}, {x2.shape[0]} rows)")
    if x2.stride(1) != 1 or x2.stride(0) % 8 != 0 or x2.data_ptr() % 16 != 0:
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], F), dtype=torch.bfloat16, device=x.device)
    torch.ops.chipmunk.w4_linear(x2, weight.contiguous(), block_scale.contiguous(), None if bias is None else bias.contiguous(), y)
    return y.view(*lead, F)


__all__ = ["w4_linear", "w4_linear_torch"]
