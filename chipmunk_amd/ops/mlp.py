"""Sparse-MLP op wrappers (mirror of reference ``src/chipmunk/ops/mlp.py:7-92``).

``run_e2e`` (exported as ``chipmunk_amd.ops.mlp``) = packed GEMM1 with fused bias+GeLU+cache-subtract, then
scatter-add of the deltas into the column-major activation cache and GEMM2 accumulating into the output cache.
Both GEMMs are native HIP kernels here; the reference's GEMM2 is a Triton kernel whose CUfunction pointer is passed
through the op as an int (``ops/mlp.py:42``) -- the argument is kept (value 0) and ignored.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..util.config import GLOBAL_CONFIG, amd_key
from .indexed_io import scatter_add

USE_FUSED_MLP_MATMUL_2 = True
csp_mlp_mm2_function_ptr = 0  # placeholder for the reference's Triton kernel pointer (triton/csp_mlp_mm2.py:131-138)


GLU_ACTS = ("gelu_tanh", "silu", "gelu")


def _default_form(who: str, act: str, fc1b: Optional[torch.Tensor]) -> bool:
    """True for tanh-GELU with a bias -- the operators GEMM1 always had, untouched; every other (activation, bias | None) pair takes
    ``csp_mlp_mm1_act`` / ``csp_mlp_mm1_fp8_act``.  An unknown ``act`` raises."""
    if act not in GLU_ACTS:
        raise ValueError(f"{who}: unknown activation {act!r} (one of {', '.join(GLU_ACTS)})")
    return act == "gelu_tanh" and fc1b is not None


def _row_scales(who: str, x: torch.Tensor, fc1w: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor) -> bool:
    """The granularity of an fp8 GEMM1's reciprocal scales.  False: one number each (0-dim, or any one-element tensor) -- the operators
    GEMM1 always had.  True: ``scale_a`` one per token row of ``x`` (``[M]``, ``[B, M]`` for a batch) with ``scale_b`` one per row of
    ``fc1w`` (``[F]``) -- ``csp_mlp_mm1_fp8_act_rs``.  A mixed pair raises."""
    if scale_a is None or scale_b is None:
        raise ValueError(f"{who}: an fp8 GEMM1 needs scale_a and scale_b, the reciprocal quantisation scales")
    F = fc1w.shape[0] if fc1w.shape[-1] == x.shape[-1] else fc1w.shape[-1]
    rows = scale_a.dim() in (1, 2) and tuple(scale_a.shape) == tuple(x.shape[:-1])
    cols = scale_b.dim() == 1 and scale_b.shape[0] == F
    if rows and cols and (F > 1 or scale_a.numel() > 1):
        return True
    if scale_a.numel() == 1 and scale_b.numel() == 1:
        return False
    raise ValueError(f"{who}: scale_a {tuple(scale_a.shape)} with scale_b {tuple(scale_b.shape)} is a mixed pair: pass one number each "
                     f"(per-tensor scales), or scale_a {tuple(x.shape[:-1])} -- one per token row -- with scale_b ({F},) -- one per fc1 "
                     "column; a vector on one side only has no kernel")


def group_major(x: torch.Tensor, sparse_act_T: torch.Tensor) -> bool:
    """The operators' rule: a cache of one dimension more than ``x`` -- ``[G, F, 128]`` for ``x [M, K]``, ``[B, G, F, 128]`` for
    ``x [B, M, K]``, G = ceil(M / 128) -- is group-major (``mlp.cache_layout: group``), unless its shape is also a column-major one
    (``[1, F, M]``: M = 128, the same elements either way).  Only the operators this project added take it: on that route tanh-GELU
    with a bias goes through ``csp_mlp_mm1_act`` / ``csp_mlp_mm1_fp8_act`` as well, and the tail is GEMM1's own scatter-add or
    ``csp_scatter_add_gm``, then GEMM2 alone."""
    if sparse_act_T.ndim != x.ndim + 1:
        return False
    M = x.shape[-2]
    return not (sparse_act_T.shape[-1] == M and sparse_act_T.numel() == sparse_act_T.shape[-2] * M)


def scatter_add_gm(packed: torch.Tensor, unpacked_groups: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor) -> None:
    """``csp_scatter_add`` on the group-major cache: ``unpacked_groups[g, idx[g, j], r] += packed[g * 128 + r, j]``; 2-D ``packed`` with
    ``[G, F, 128]`` or a batch ``[B, M, F]`` with ``[B, G, F, 128]``."""
    if packed.ndim == 2:
        packed, unpacked_groups, indices, counts = packed.unsqueeze(0), unpacked_groups.unsqueeze(0), indices.unsqueeze(0), counts.unsqueeze(0)
    torch.ops.chipmunk.csp_scatter_add_gm(packed, unpacked_groups, indices, counts)


def _check_fc1_scale(who: str, x: torch.Tensor, fc1w: torch.Tensor, fc1_scale: torch.Tensor, scale_a, scale_b,
                     names=("scale_a", "scale_b")) -> None:
    """The rules of ``fc1_scale`` (weight-only fp8 ``fc1``): an e4m3 ``fc1w``, a bf16 ``x``, no activation / weight scale pair, and one
    number or one per row of ``fc1w``.  Every violation raises ``ValueError`` and names the argument."""
    if fc1w.dtype != torch.float8_e4m3fn:
        raise ValueError(f"{who}: fc1_scale is the reciprocal scale of a float8_e4m3fn fc1w (weight-only fp8); fc1w is {fc1w.dtype}")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"{who}: with fc1_scale (weight-only fp8) x must be bfloat16 (got {x.dtype}): the activations are not quantised")
    for name, t in zip(names, (scale_a, scale_b)):
        if t is not None:
            raise ValueError(f"{who}: {name} must be None with fc1_scale: a weight-only fc1 has no activation scale, and its weight scale "
                             "is fc1_scale")
    if fc1_scale.numel() != 1 and tuple(fc1_scale.shape) != (fc1w.shape[0],):
        raise ValueError(f"{who}: fc1_scale must hold one number, or one per row of fc1w ({fc1w.shape[0]},); got {tuple(fc1_scale.shape)}")


def _positional_act(fc1_scale, act):
    """``fc1_scale`` sits in front of ``act``, which stays the last parameter of ``mm1`` / ``mm1_scatter`` / ``run_e2e``: a caller that
    passed the activation's name by position still means the activation."""
    return (None, fc1_scale) if isinstance(fc1_scale, str) else (fc1_scale, act)


def mm1_w8(x: torch.Tensor, fc1w: torch.Tensor, fc1_scale: torch.Tensor, sparse_act_packed: torch.Tensor, fc1b: Optional[torch.Tensor],
           sparse_act_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, act: str = "gelu_tanh", update_cache: bool = False) -> None:
    """Weight-only fp8 GEMM1: ``packed = bf16(act((x f(fc1w)^T) * fc1_scale + fc1b) - cache)`` on the kept columns with bf16 ``x``, e4m3
    ``fc1w`` ``[F, K]`` and ``fc1_scale`` its RECIPROCAL scale (``W8Linear.scale_reciprocal``: one number, or ``[F]``); ``update_cache``
    also applies the scatter-add of the packed deltas to ``sparse_act_T``.  Every cache layout and batch form of ``csp_mlp_mm1_act``."""
    if act not in GLU_ACTS:
        raise ValueError(f"mm1_w8: unknown activation {act!r} (one of {', '.join(GLU_ACTS)})")
    _check_fc1_scale("mm1_w8", x, fc1w, fc1_scale, None, None)
    assert sparse_act_packed.dtype == torch.bfloat16 and sparse_act_T.dtype == torch.bfloat16
    scale = fc1_scale.float().reshape(1) if fc1_scale.numel() == 1 else fc1_scale.float().contiguous()
    torch.ops.chipmunk.csp_mlp_mm1_w8(x, fc1w.contiguous(), scale, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act,
                                      bool(update_cache))


def mm1(x: torch.Tensor, fc1w: torch.Tensor, sparse_act_packed: torch.Tensor, fc1b: Optional[torch.Tensor],
        sparse_act_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
        scale_a: Optional[torch.Tensor] = None, scale_b: Optional[torch.Tensor] = None, fc1_scale: Optional[torch.Tensor] = None,
        act: str = "gelu_tanh") -> None:
    fc1_scale, act = _positional_act(fc1_scale, act)
    if fc1_scale is not None:      # weight-only fp8 fc1: bf16 x, e4m3 fc1w (csp_mlp_mm1_w8); the cache is left to the scatter-add
        _check_fc1_scale("mm1", x, fc1w, fc1_scale, scale_a, scale_b)
        return mm1_w8(x, fc1w, fc1_scale, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act, update_cache=False)
    # (the reference asserts x is bf16 even on its fp8 branch, one of the reasons that branch cannot run as shipped)
    assert x.dtype == (torch.float8_e4m3fn if fc1w.dtype == torch.float8_e4m3fn else torch.bfloat16)
    assert sparse_act_packed.dtype == torch.bfloat16
    assert sparse_act_T.dtype == torch.bfloat16
    default = _default_form("mm1", act, fc1b) and not group_major(x, sparse_act_T)
    if fc1w.dtype == torch.bfloat16:
        if default:
            torch.ops.chipmunk.csp_mlp_mm1(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts)
        else:
            torch.ops.chipmunk.csp_mlp_mm1_act(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act, False)
    elif fc1w.dtype == torch.float8_e4m3fn:
        # reference: triton csp_mlp_mm1_fp8(x, fc1w.T, ...) (ops/mlp.py:22-23).  That kernel also stores the new
        # activation into the cache (triton/csp_mlp_mm1.py:140) and the scatter-add then adds the delta again; here
        # the cache is left to the scatter-add like on the bf16 path (set FP8_MM1_UPDATES_CACHE for the literal form).
        csp_mlp_mm1_fp8(x, fc1w, fc1b, indices, counts, sparse_act_T, sparse_act_packed, scale_a, scale_b, act)
    else:
        raise ValueError(f"Unsupported dtype: {fc1w.dtype}")


def mm1_scatter(x: torch.Tensor, fc1w: torch.Tensor, sparse_act_packed: torch.Tensor, fc1b: Optional[torch.Tensor],
                sparse_act_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, fc1_scale: Optional[torch.Tensor] = None,
                act: str = "gelu_tanh") -> None:
    """GEMM1 + ``csp_scatter_add`` of its output into ``sparse_act_T`` in one kernel (bf16, or -- with ``fc1_scale`` -- a weight-only
    e4m3 ``fc1w`` under a bf16 ``x``)."""
    fc1_scale, act = _positional_act(fc1_scale, act)
    if fc1_scale is not None:
        _check_fc1_scale("mm1_scatter", x, fc1w, fc1_scale, None, None)
        return mm1_w8(x, fc1w, fc1_scale, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act, update_cache=True)
    assert x.dtype == torch.bfloat16 and sparse_act_packed.dtype == torch.bfloat16 and sparse_act_T.dtype == torch.bfloat16
    if _default_form("mm1_scatter", act, fc1b) and not group_major(x, sparse_act_T):
        torch.ops.chipmunk.csp_mlp_mm1_scatter(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts)
    else:
        torch.ops.chipmunk.csp_mlp_mm1_act(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act, True)


def mm1_fp8_scatter(x: torch.Tensor, fc1w: torch.Tensor, sparse_act_packed: torch.Tensor, fc1b: Optional[torch.Tensor],
                    sparse_act_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, scale_a: torch.Tensor,
                    scale_b: torch.Tensor, act: str = "gelu_tanh") -> None:
    """fp8 GEMM1 + ``csp_scatter_add`` of its output into ``sparse_act_T`` in one kernel (the fp8 counterpart of ``mm1_scatter``;
    bit-identical in the packed deltas and in the cache to ``csp_mlp_mm1_fp8`` followed by the scatter-add)."""
    assert x.dtype == torch.float8_e4m3fn and fc1w.dtype == torch.float8_e4m3fn
    default = _default_form("mm1_fp8_scatter", act, fc1b) and not group_major(x, sparse_act_T)      # (the name is checked before anything else)
    if _row_scales("mm1_fp8_scatter", x, fc1w, scale_a, scale_b):   # update_cache 2: the scatter-add of the deltas
        torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs(x, fc1w.contiguous(), sparse_act_packed, fc1b, sparse_act_T, indices, counts,
                                                  scale_a.float().contiguous(), scale_b.float().contiguous(), act, 2)
    elif default:
        torch.ops.chipmunk.csp_mlp_mm1_fp8_scatter(x, fc1w.contiguous(), sparse_act_packed, fc1b, sparse_act_T, indices, counts,
                                                   scale_a.reshape(1).float(), scale_b.reshape(1).float())
    else:   # update_cache 2: the scatter-add of the deltas
        torch.ops.chipmunk.csp_mlp_mm1_fp8_act(x, fc1w.contiguous(), sparse_act_packed, fc1b, sparse_act_T, indices, counts,
                                               scale_a.reshape(1).float(), scale_b.reshape(1).float(), act, 2)


FP8_MM1_UPDATES_CACHE = False


def csp_mlp_mm1_fp8(a: torch.Tensor, b: torch.Tensor, fc1b: Optional[torch.Tensor], indices: torch.Tensor, counts: torch.Tensor,
                    sparse_act_unpacked_inout: torch.Tensor, sparse_act_packed_out: torch.Tensor,
                    scale_a: torch.Tensor, scale_b: torch.Tensor, act: str = "gelu_tanh") -> None:
    """Native counterpart of the reference's Triton ``csp_mlp_mm1_fp8`` (same argument order,
    triton/csp_mlp_mm1.py:143).  ``a`` fp8 ``[M,K]``; ``b`` fp8 ``[F,K]`` (the reference passes ``fc1w.T``, a view of
    the same storage); scales are the RECIPROCAL quantisation scales (modules/mlp.py:98-99)."""
    if b.shape[0] == a.shape[1] and b.shape[1] != a.shape[1]:
        b = b.T  # accept the reference's fc1w.T view
    default = _default_form("csp_mlp_mm1_fp8", act, fc1b) and not group_major(a, sparse_act_unpacked_inout)   # (the name is checked first)
    if _row_scales("csp_mlp_mm1_fp8", a, b, scale_a, scale_b):   # one scale per token row and per fc1 column: every activation / bias form
        torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs(a, b.contiguous(), sparse_act_packed_out, fc1b, sparse_act_unpacked_inout, indices,
                                                  counts, scale_a.float().contiguous(), scale_b.float().contiguous(), act,
                                                  1 if FP8_MM1_UPDATES_CACHE else 0)
    elif default:
        torch.ops.chipmunk.csp_mlp_mm1_fp8(a, b.contiguous(), sparse_act_packed_out, fc1b, sparse_act_unpacked_inout,
                                           indices, counts, scale_a.reshape(1).float(), scale_b.reshape(1).float(),
                                           FP8_MM1_UPDATES_CACHE)
    else:   # update_cache 1: the new activation is stored into the cache (FP8_MM1_UPDATES_CACHE), 0: the cache is left alone
        torch.ops.chipmunk.csp_mlp_mm1_fp8_act(a, b.contiguous(), sparse_act_packed_out, fc1b, sparse_act_unpacked_inout,
                                               indices, counts, scale_a.reshape(1).float(), scale_b.reshape(1).float(), act,
                                               1 if FP8_MM1_UPDATES_CACHE else 0)


def mm2_fused(packed: torch.Tensor, unpacked_colmajor: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
              sparse_act_packed: torch.Tensor, fc2wT: torch.Tensor, cached_out: torch.Tensor,
              num_sms_scatter_add: int) -> None:
    assert sparse_act_packed.dtype == torch.bfloat16
    assert fc2wT.dtype == torch.bfloat16
    assert cached_out.dtype == torch.bfloat16
    if packed.ndim == 3:   # a batch [B, M, F]: the operator's leading dimension is the batch; the weight stays [1, F, N]
        torch.ops.chipmunk.csp_mlp_mm2_and_scatter_add(packed, unpacked_colmajor, indices, counts, sparse_act_packed,
                                                       fc2wT.unsqueeze(0), cached_out, num_sms_scatter_add, csp_mlp_mm2_function_ptr)
        return
    torch.ops.chipmunk.csp_mlp_mm2_and_scatter_add(
        packed.unsqueeze(0), unpacked_colmajor.unsqueeze(0), indices.unsqueeze(0), counts.unsqueeze(0),
        sparse_act_packed.unsqueeze(0), fc2wT.unsqueeze(0), cached_out.unsqueeze(0), num_sms_scatter_add,
        csp_mlp_mm2_function_ptr)


def csp_mlp_mm2(sparse_act_packed: torch.Tensor, fc2wT: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
                cached_out: torch.Tensor, num_sms: int = 0, fc2_scale: Optional[torch.Tensor] = None) -> None:
    """Native counterpart of the reference's Triton ``csp_mlp_mm2`` (triton/csp_mlp_mm2.py:104-129).  An e4m3 ``fc2wT`` (``[F, N]``
    ``float8_e4m3fn``, plain row-major) takes the weight-only fp8 GEMM2 and needs ``fc2_scale``, the weight's RECIPROCAL quantisation scale
    (``F8Linear.scale_reciprocal``), which multiplies the fp32 sums before they are rounded to bf16.

    ``counts`` must be multiples of 8: both GEMM2 kernels mask the packed columns past a count in whole 16-byte pieces (the reference's
    Triton kernel reads whole k blocks), so a count of 154 would take columns 154 .. 159 of ``sparse_act_packed`` into the sum.
    ``topk_indices`` emits multiples of ``counts_multiple_of`` (256 / 128 as shipped).  GEMM1 and the scatter-add take any count."""
    if fc2wT.dtype == torch.float8_e4m3fn:
        if fc2_scale is None:
            raise ValueError("csp_mlp_mm2: an e4m3 fc2wT needs fc2_scale, the weight's reciprocal quantisation scale (F8Linear.scale_reciprocal)")
        torch.ops.chipmunk.csp_mlp_mm2_w8(sparse_act_packed, fc2wT, fc2_scale.reshape(1).float(), indices, counts, cached_out)
        return
    torch.ops.chipmunk.csp_mlp_mm2(sparse_act_packed, fc2wT, indices, counts, cached_out)


def _mm2_w8_after_gemm1(sparse_act_packed: torch.Tensor, fc2w_T: torch.Tensor, fc2_scale: Optional[torch.Tensor], indices: torch.Tensor,
                        counts: torch.Tensor, sparse_act_T: torch.Tensor, cached_out: torch.Tensor, num_sms_scatter_add: int) -> None:
    """The tail of a sparse step with an e4m3 ``fc2w_T`` whose GEMM1 left the cache alone: the scatter-add of the packed deltas, then the
    weight-only fp8 GEMM2 (``csp_mlp_mm2_and_scatter_add`` is bf16-only)."""
    scatter_add(sparse_act_packed, sparse_act_T, indices, counts, num_sms_scatter_add)
    csp_mlp_mm2(sparse_act_packed, fc2w_T, indices, counts, cached_out, fc2_scale=fc2_scale)


def mm2_unfused(sparse_act_packed: torch.Tensor, fc2wT: torch.Tensor, cached_out: torch.Tensor,
                unpacked_colmajor: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
                num_sms_scatter_add: int) -> None:
    assert sparse_act_packed.dtype == torch.bfloat16
    assert fc2wT.dtype == torch.bfloat16
    assert cached_out.dtype == torch.bfloat16
    scatter_add(sparse_act_packed, unpacked_colmajor, indices, counts, num_sms_scatter_add)
    csp_mlp_mm2(sparse_act_packed, fc2wT, indices, counts, cached_out, 132 - num_sms_scatter_add)


def _check_batch(x: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, sparse_act_T: torch.Tensor, cached_out: torch.Tensor) -> None:
    """``x`` is ``[M, K]`` or a batch ``[B, M, K]``, and a batch takes every other per-sequence tensor with the same leading ``B``."""
    assert x.ndim in (2, 3), "x must be [M, K] or [B, M, K]"
    if x.ndim == 3:
        B = x.shape[0]
        assert indices.ndim == 3 and counts.ndim == 2 and sparse_act_T.ndim in (3, 4) and cached_out.ndim == 3, \
            "a batched x [B, M, K] takes indices [B, G, F], counts [B, G], sparse_act_T [B, F, M] (group-major: [B, G, F, 128]) and " \
            "cached_out [B, M, N]"
        assert indices.shape[0] == B and counts.shape[0] == B and sparse_act_T.shape[0] == B and cached_out.shape[0] == B, \
            f"the batch size of indices / counts / sparse_act_T / cached_out must be that of x ({B})"


def _after_gemm1(cache_updated: bool, sparse_act_packed: torch.Tensor, fc2w_T: torch.Tensor, fc2_scale: Optional[torch.Tensor],
                 indices: torch.Tensor, counts: torch.Tensor, sparse_act_T: torch.Tensor, cached_out: torch.Tensor,
                 num_sms_scatter_add: int) -> None:
    """Everything behind GEMM1, whatever its form -- the packed deltas are bf16.  ``cache_updated``: GEMM1 applied the scatter-add of its
    own deltas (same bits as the two-kernel form), so GEMM2 runs alone; otherwise the scatter-add and GEMM2, in the form ``fc2w_T`` takes.
    (The operators are looked up in the module when they are called: a benchmark may have put timing wrappers in their place.)"""
    if cache_updated:
        csp_mlp_mm2(sparse_act_packed, fc2w_T, indices, counts, cached_out, fc2_scale=fc2_scale)
    elif group_major(sparse_act_packed, sparse_act_T):   # csp_mlp_mm2_and_scatter_add knows the column-major cache only
        scatter_add_gm(sparse_act_packed, sparse_act_T, indices, counts)
        csp_mlp_mm2(sparse_act_packed, fc2w_T, indices, counts, cached_out, fc2_scale=fc2_scale)
    elif fc2w_T.dtype == torch.float8_e4m3fn:
        _mm2_w8_after_gemm1(sparse_act_packed, fc2w_T, fc2_scale, indices, counts, sparse_act_T, cached_out, num_sms_scatter_add)
    elif USE_FUSED_MLP_MATMUL_2:
        mm2_fused(sparse_act_packed, sparse_act_T, indices, counts, sparse_act_packed, fc2w_T, cached_out, num_sms_scatter_add)
    else:
        mm2_unfused(sparse_act_packed, fc2w_T, cached_out, sparse_act_T, indices, counts, num_sms_scatter_add)


@torch.compiler.disable
def run_e2e(x: torch.Tensor, fc1w: torch.Tensor, fc1b: Optional[torch.Tensor], fc2w_T: torch.Tensor, indices: torch.Tensor,
            counts: torch.Tensor, sparse_act_T: torch.Tensor, cached_out: torch.Tensor, num_sms_scatter_add: int,
            mm1_scale_a: Optional[torch.Tensor] = None, mm1_scale_b: Optional[torch.Tensor] = None,
            fc2_scale: Optional[torch.Tensor] = None, fc1_scale: Optional[torch.Tensor] = None, act: str = "gelu_tanh") -> None:
    # fc1_scale (W8Linear.scale_reciprocal; the sibling of fc2_scale): fc1w is e4m3 under a bf16 x, weight-only -- GEMM1 is csp_mlp_mm1_w8, with
    # its own scatter-add or (mlp.fused_scatter off) the scatter-add behind it; mm1_scale_a / mm1_scale_b must then be None.
    # sparse_act_T of one dimension more than x ([G, F, 128] / [B, G, F, 128]) is the group-major cache: see group_major.  Otherwise:
    # M is any positive row count (ceil(M / 128) groups, the last one short); sparse_act_T is [F, M], contiguous or -- required when
    # M % 8 != 0 -- the [:, :M] view of a [F, ldc] buffer with ldc % 8 == 0; x and cached_out may be row views of larger buffers.
    # A batch: x [B, M, K1] with indices [B, G, F], counts [B, G], sparse_act_T [B, F, M] (or the [..., :M] view of [B, F, ldc]) and
    # cached_out [B, M, N] -- one launch per kernel for all B sequences, the bits of B calls on the slices.
    # fc2w_T float8_e4m3fn with fc2_scale (F8Linear.scale_reciprocal): the scatter-add is GEMM1's own (or csp_scatter_add with
    # mlp.fused_scatter off) and GEMM2 gathers e4m3 rows.
    # mm1_scale_a / mm1_scale_b (fp8 fc1): one number each, or mm1_scale_a [M] ([B, M]) -- one per token row -- with mm1_scale_b [F] -- one
    # per fc1 column (csp_mlp_mm1_fp8_act_rs in GEMM1's place); a mixed pair raises.
    # act (one of GLU_ACTS) names fc1's activation and fc1b may be None: anything but tanh-GELU with a bias takes csp_mlp_mm1_act /
    # csp_mlp_mm1_fp8_act in GEMM1's place, everything behind GEMM1 is unchanged.
    fc1_scale, act = _positional_act(fc1_scale, act)
    _check_batch(x, indices, counts, sparse_act_T, cached_out)
    M, K1 = x.shape[-2:]
    K2, K1_ = fc1w.shape
    assert K1 == K1_, "K1 must match"
    K2_, _N = fc2w_T.shape
    assert K2 == K2_, "K2 must match"
    sparse_act_packed = torch.empty(x.shape[:-1] + (K2,), device=x.device, dtype=sparse_act_T.dtype)  # bf16 also when x is fp8
    tail = (sparse_act_packed, fc2w_T, fc2_scale, indices, counts, sparse_act_T, cached_out, num_sms_scatter_add)
    if fc1_scale is not None:
        _check_fc1_scale("run_e2e", x, fc1w, fc1_scale, mm1_scale_a, mm1_scale_b, ("mm1_scale_a", "mm1_scale_b"))
        fused = bool(x.is_cuda and amd_key("mlp", "fused_scatter"))
        (mm1_scatter if fused else mm1)(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act=act, fc1_scale=fc1_scale)
        return _after_gemm1(fused, *tail)
    if (x.is_cuda and fc1w.dtype == torch.bfloat16
            and amd_key("mlp", "fused_scatter")):
        mm1_scatter(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts, act)
        return _after_gemm1(True, *tail)
    if (x.is_cuda and fc1w.dtype == torch.float8_e4m3fn and x.dtype == torch.float8_e4m3fn and amd_key("mlp", "fused_scatter")
            and not FP8_MM1_UPDATES_CACHE and K1 % 128 == 0):
        mm1_fp8_scatter(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts, mm1_scale_a, mm1_scale_b, act)
        return _after_gemm1(True, *tail)
    mm1(x, fc1w, sparse_act_packed, fc1b, sparse_act_T, indices, counts, mm1_scale_a, mm1_scale_b, act)
    if fc2w_T.dtype == torch.float8_e4m3fn and fc1w.dtype == torch.float8_e4m3fn and FP8_MM1_UPDATES_CACHE:
        raise ValueError("run_e2e: FP8_MM1_UPDATES_CACHE (GEMM1 stores the activation, the scatter-add adds the delta again) has no e4m3 fc2 form")
    _after_gemm1(False, *tail)


def _run_e2e_gated(gemm1, x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, fc2w_T: torch.Tensor, indices: torch.Tensor,
                   counts: torch.Tensor, sparse_act_T: torch.Tensor, cached_out: torch.Tensor, num_sms_scatter_add: int,
                   fc2_scale: Optional[torch.Tensor]) -> None:
    """``run_e2e_glu`` / ``run_e2e_glu_fp8`` around their GEMM1, ``gemm1(sparse_act_packed, update_cache)``."""
    _check_batch(x, indices, counts, sparse_act_T, cached_out)
    K1 = x.shape[-1]
    K2, K1_ = w_gate.shape
    assert K1 == K1_ and tuple(w_up.shape) == (K2, K1), "K1 must match, w_up must have the shape of w_gate"
    assert fc2w_T.shape[0] == K2, "K2 must match"
    sparse_act_packed = torch.empty(x.shape[:-1] + (K2,), device=x.device, dtype=sparse_act_T.dtype)   # bf16 also when x is fp8
    fused = bool(amd_key("mlp", "fused_scatter"))
    gemm1(sparse_act_packed, fused)
    _after_gemm1(fused, sparse_act_packed, fc2w_T, fc2_scale, indices, counts, sparse_act_T, cached_out, num_sms_scatter_add)


def mm1_glu(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, sparse_act_packed: torch.Tensor,
            b_gate: Optional[torch.Tensor], b_up: Optional[torch.Tensor], act: str, sparse_act_T: torch.Tensor,
            indices: torch.Tensor, counts: torch.Tensor, update_cache: bool = False) -> None:
    """Gated GEMM1: ``packed = bf16(act(x Wg^T + bg) * (x Wu^T + bu) - cache)`` on the kept columns; ``update_cache`` also applies the
    scatter-add of the packed deltas to ``sparse_act_T`` (the bits of ``csp_scatter_add`` afterwards).  ``w_gate`` / ``w_up`` are
    ``[F, K]`` bf16 with contiguous rows K apart -- two weights or the halves of one fused ``[2F, K]`` projection; either bias may be
    ``None``.  bf16 only: e4m3 operands go to ``mm1_glu_fp8``."""
    if act not in GLU_ACTS:
        raise ValueError(f"mm1_glu: unknown activation {act!r} (one of {', '.join(GLU_ACTS)})")
    if x.dtype != torch.bfloat16 or w_gate.dtype != torch.bfloat16 or w_up.dtype != torch.bfloat16:
        raise ValueError(f"mm1_glu: bf16 operands only (got x {x.dtype}, w_gate {w_gate.dtype}, w_up {w_up.dtype})")
    assert sparse_act_packed.dtype == torch.bfloat16 and sparse_act_T.dtype == torch.bfloat16
    torch.ops.chipmunk.csp_mlp_mm1_glu(x, w_gate, w_up, sparse_act_packed, b_gate, b_up, sparse_act_T, indices, counts, act,
                                       bool(update_cache))


@torch.compiler.disable
def run_e2e_glu(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, b_gate: Optional[torch.Tensor],
                b_up: Optional[torch.Tensor], act: str, fc2w_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
                sparse_act_T: torch.Tensor, cached_out: torch.Tensor, num_sms_scatter_add: int,
                fc2_scale: Optional[torch.Tensor] = None) -> None:
    """``run_e2e`` for a gated feed-forward ``fc2(act(x Wg^T + bg) * (x Wu^T + bu))``: only GEMM1 differs, GEMM2 and the scatter-add see
    the same packed deltas.  Shapes, pitched cache, batches and an e4m3 ``fc2w_T`` with ``fc2_scale`` as for ``run_e2e``."""
    _run_e2e_gated(lambda packed, upd: mm1_glu(x, w_gate, w_up, packed, b_gate, b_up, act, sparse_act_T, indices, counts, update_cache=upd),
                   x, w_gate, w_up, fc2w_T, indices, counts, sparse_act_T, cached_out, num_sms_scatter_add, fc2_scale)


def mm1_glu_fp8(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, sparse_act_packed: torch.Tensor,
                b_gate: Optional[torch.Tensor], b_up: Optional[torch.Tensor], act: str, sparse_act_T: torch.Tensor,
                indices: torch.Tensor, counts: torch.Tensor, scale_a: torch.Tensor, scale_b_gate: torch.Tensor,
                scale_b_up: torch.Tensor, update_cache: bool = False) -> None:
    """``mm1_glu`` over fp8 projections: ``x``, ``w_gate`` and ``w_up`` are ``float8_e4m3fn`` (K a multiple of 128) and each branch's sum is
    multiplied by ``scale_a`` and its own weight scale before its bias -- the RECIPROCAL quantisation scales, one float each, as
    ``csp_mlp_mm1_fp8`` takes them.  Biases, packed deltas and the cache are bf16."""
    if act not in GLU_ACTS:
        raise ValueError(f"mm1_glu_fp8: unknown activation {act!r} (one of {', '.join(GLU_ACTS)})")
    f8 = torch.float8_e4m3fn
    if x.dtype != f8 or w_gate.dtype != f8 or w_up.dtype != f8:
        raise ValueError(f"mm1_glu_fp8: float8_e4m3fn operands only (got x {x.dtype}, w_gate {w_gate.dtype}, w_up {w_up.dtype})")
    assert sparse_act_packed.dtype == torch.bfloat16 and sparse_act_T.dtype == torch.bfloat16
    torch.ops.chipmunk.csp_mlp_mm1_glu_fp8(x, w_gate, w_up, sparse_act_packed, b_gate, b_up, sparse_act_T, indices, counts,
                                           scale_a.reshape(1).float(), scale_b_gate.reshape(1).float(), scale_b_up.reshape(1).float(),
                                           act, bool(update_cache))


@torch.compiler.disable
def run_e2e_glu_fp8(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, b_gate: Optional[torch.Tensor],
                    b_up: Optional[torch.Tensor], act: str, fc2w_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
                    sparse_act_T: torch.Tensor, cached_out: torch.Tensor, num_sms_scatter_add: int, scale_a: torch.Tensor,
                    scale_b_gate: torch.Tensor, scale_b_up: torch.Tensor, fc2_scale: Optional[torch.Tensor] = None) -> None:
    """``run_e2e_glu`` with the gated fp8 GEMM1 (``x`` already quantised to e4m3): the packed deltas are bf16, so GEMM2 (``fc2w_T`` bf16, or
    e4m3 with ``fc2_scale``) and the scatter-add are the operators of the bf16 route."""
    _run_e2e_gated(lambda packed, upd: mm1_glu_fp8(x, w_gate, w_up, packed, b_gate, b_up, act, sparse_act_T, indices, counts, scale_a,
                                                   scale_b_gate, scale_b_up, update_cache=upd),
                   x, w_gate, w_up, fc2w_T, indices, counts, sparse_act_T, cached_out, num_sms_scatter_add, fc2_scale)


def mm1_glu_w8(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, scale_gate: torch.Tensor, scale_up: torch.Tensor,
               sparse_act_packed: torch.Tensor, b_gate: Optional[torch.Tensor], b_up: Optional[torch.Tensor], act: str,
               sparse_act_T: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, update_cache: bool = False) -> None:
    """``mm1_glu`` over weight-only fp8 projections: bf16 ``x``, e4m3 ``w_gate`` / ``w_up`` ``[F, K]`` (two weights or the halves of one
    fused ``[2F, K]`` tensor) and ``scale_gate`` / ``scale_up`` their RECIPROCAL scales (``W8Linear.scale_reciprocal``: one number, or
    ``[F]``).  ``packed = bf16(act((x f(Wg)^T) * scale_gate + bg) * ((x f(Wu)^T) * scale_up + bu) - cache)`` on the kept columns.  Every
    violation of these rules raises ``ValueError`` and names the argument."""
    if act not in GLU_ACTS:
        raise ValueError(f"mm1_glu_w8: unknown activation {act!r} (one of {', '.join(GLU_ACTS)})")
    for name, w in (("w_gate", w_gate), ("w_up", w_up)):
        if w.dtype != torch.float8_e4m3fn:
            raise ValueError(f"mm1_glu_w8: {name} must be float8_e4m3fn (weight-only fp8); got {w.dtype}")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"mm1_glu_w8: x must be bfloat16 (got {x.dtype}): the activations are not quantised")
    for name, s, w in (("scale_gate", scale_gate, w_gate), ("scale_up", scale_up, w_up)):
        if s.numel() != 1 and tuple(s.shape) != (w.shape[0],):
            raise ValueError(f"mm1_glu_w8: {name} must hold one number, or one per weight row ({w.shape[0]},); got {tuple(s.shape)}")
    assert sparse_act_packed.dtype == torch.bfloat16 and sparse_act_T.dtype == torch.bfloat16
    sg, su = (s.float().reshape(1) if s.numel() == 1 else s.float().contiguous() for s in (scale_gate, scale_up))
    torch.ops.chipmunk.csp_mlp_mm1_glu_w8(x, w_gate, w_up, sg, su, sparse_act_packed, b_gate, b_up, sparse_act_T, indices, counts, act,
                                          bool(update_cache))


@torch.compiler.disable
def run_e2e_glu_w8(x: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor, scale_gate: torch.Tensor, scale_up: torch.Tensor,
                   b_gate: Optional[torch.Tensor], b_up: Optional[torch.Tensor], act: str, fc2w_T: torch.Tensor, indices: torch.Tensor,
                   counts: torch.Tensor, sparse_act_T: torch.Tensor, cached_out: torch.Tensor, num_sms_scatter_add: int,
                   fc2_scale: Optional[torch.Tensor] = None) -> None:
    """``run_e2e_glu`` with the gated weight-only fp8 GEMM1 (bf16 ``x``, e4m3 gate / up weights): the packed deltas are bf16, so GEMM2
    (``fc2w_T`` bf16, or e4m3 with ``fc2_scale``) and the scatter-add are the operators of the bf16 route."""
    _run_e2e_gated(lambda packed, upd: mm1_glu_w8(x, w_gate, w_up, scale_gate, scale_up, packed, b_gate, b_up, act, sparse_act_T, indices,
                                                  counts, update_cache=upd),
                   x, w_gate, w_up, fc2w_T, indices, counts, sparse_act_T, cached_out, num_sms_scatter_add, fc2_scale)


__all__ = ["group_major", "scatter_add_gm", "mm1", "mm1_w8", "mm1_scatter", "mm1_fp8_scatter", "mm2_fused", "mm2_unfused", "run_e2e", "csp_mlp_mm2", "csp_mlp_mm1_fp8",
           "mm1_glu", "run_e2e_glu", "mm1_glu_fp8", "run_e2e_glu_fp8", "mm1_glu_w8", "run_e2e_glu_w8"]
