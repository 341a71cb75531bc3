"""Indexed-IO op wrappers (mirror of reference ``src/chipmunk/ops/indexed_io.py:1-37``)."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

# Longest row (last dimension of ``cs``, key count of the fused mask step) the top-k mask kernels take: CHIPMUNK_TOPK_MASK_MAX_N of
# ``csrc/common.h``.  Up to 122 880 columns a row's keys stay in registers; longer rows take the streaming form of the kernel.
TOPK_MASK_MAX_N = 1024 * 512


def copy_indices(bm_fc1: torch.Tensor, bm_mid_cache: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor) -> None:
    torch.ops.chipmunk.copy_indices(bm_fc1, bm_mid_cache, indices, counts)


def topk_indices(activations: torch.Tensor, indices_out: torch.Tensor, counts_out: torch.Tensor,
                 sparsity_amount: float, multiple_of: int, rk: float) -> None:
    torch.ops.chipmunk.topk_indices(activations, indices_out, counts_out, sparsity_amount, multiple_of, rk)


def _check_top_p(who: str, sparsity_amount: float, top_p: float, min_keys: float) -> None:
    if not (0.0 < top_p <= 1.0) or not (0.0 <= sparsity_amount <= 1.0) or not (0.0 <= min_keys <= 1.0 - sparsity_amount + 1e-9):
        raise ValueError(f"{who}: top_p must be in (0, 1], sparsity_amount in [0, 1] and min_keys in [0, 1 - sparsity_amount] "
                         f"(got top_p {top_p}, sparsity_amount {sparsity_amount}, min_keys {min_keys})")


def _f32(x: float) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32))


def _topk_indices_p_cpu(activations: torch.Tensor, indices_out: torch.Tensor, counts_out: torch.Tensor, sparsity_amount: float,
                        top_p: float, min_keys: float, multiple_of: int, rk: float) -> None:
    """The rule of ``topk_indices_p`` in plain torch: one sort per row, fp64 sums; output order and padding as the kernel's."""
    f = activations.shape[-1]
    if f < 1024:
        raise ValueError(f"topk_indices_p: rows of 1024 columns or more (the quantiles are taken over the first 1024); got {f}")
    rows = activations.reshape(-1, f).double()
    inds, counts = indices_out.view(-1, f), counts_out.view(-1)
    if _f32(sparsity_amount) == 1.0:       # keep nothing, as topk_indices
        inds.fill_(-1)
        counts.zero_()
        return
    mass = torch.where(rows > 0, rows, torch.zeros_like(rows))          # a zero, negative or NaN entry carries no mass
    desc, _ = mass.sort(dim=-1, descending=True)
    csum = desc.cumsum(-1)
    total = csum[:, -1:]
    first = (csum < top_p * total).sum(-1, keepdim=True).clamp(max=f - 1)       # the first prefix whose mass reaches the target
    inf = torch.full_like(total, float("inf"))
    thr_p = torch.where(total > 0, desc.gather(-1, first), inf)                 # its value: a class of equal values is taken whole
    sample = rows[:, :1024].sort(dim=-1).values
    iq = int(1024 * _f32(sparsity_amount))
    thr_q = -inf if sparsity_amount == 0 else sample[:, iq:iq + 1]
    im = 1024 if min_keys == 0 else max(int(1024 * _f32(1.0 - min_keys)), iq)
    thr_min = inf if im >= 1024 else sample[:, im:im + 1]
    thr = torch.minimum(torch.maximum(thr_p, thr_q), thr_min)
    keep = (rows > 0) & (rows >= thr)
    listed = keep | (~keep & (torch.rand(keep.shape) < rk)) if rk > 0 else keep
    cols = torch.arange(f, dtype=torch.int64)
    for r in range(rows.shape[0]):
        on = cols[listed[r]]
        off = cols[~listed[r]]
        last = torch.full((1024,), -1, dtype=torch.int64).scatter_reduce(0, off % 1024, off, "amax")     # last rejected column per residue
        pad = (-on.numel()) % multiple_of
        row = torch.cat([on, last[last >= 0][:pad]])
        inds[r, : row.numel()] = row.to(torch.int32)
        counts[r] = on.numel() + pad


def topk_indices_p(activations: torch.Tensor, indices_out: torch.Tensor, counts_out: torch.Tensor, sparsity_amount: float,
                   top_p: float, min_keys: float, multiple_of: int, rk: float) -> None:
    """``topk_indices`` with a column count per row (not in the reference; ``mlp.top_p``).  Per row of values ``v``: mass ``m_c = v_c``
    where positive (a zero, negative or NaN entry carries none), ``total`` over the whole row; ``thr_p`` the largest ``t`` whose columns
    ``v_c >= t`` carry ``top_p * total`` (a class of equal values is taken whole; +inf for an all-zero row); ``thr_q`` the threshold of
    ``topk_indices`` (element ``int(1024 * sparsity_amount)`` of the sorted first 1024 values; -inf for ``sparsity_amount == 0``);
    ``thr_min`` the same order statistic at ``1 - min_keys`` (+inf for ``min_keys == 0``); kept: ``m_c > 0 and v_c >= min(max(thr_p,
    thr_q), thr_min)``.  Random keys, padding, order and ``counts`` as ``topk_indices``.  The kept set is a subset of what
    ``topk_indices`` keeps (the cap is a threshold: no tie-break); an all-zero row keeps nothing (``topk_indices`` keeps all of it);
    ``sparsity_amount == 1`` keeps nothing; the floor is a sampled quantile like the cap, blind to columns past the first 1024.  The
    kernel sums in fp32 in a fixed order (same launch, same bits); CPU tensors take a sort with fp64 sums."""
    _check_top_p("topk_indices_p", sparsity_amount, top_p, min_keys)
    if not activations.is_cuda:
        return _topk_indices_p_cpu(activations, indices_out, counts_out, sparsity_amount, top_p, min_keys, multiple_of, rk)
    torch.ops.chipmunk.topk_indices_p(activations, indices_out, counts_out, sparsity_amount, top_p, min_keys, multiple_of, rk)


def topk_delta_indices_p(activations: torch.Tensor, cache: torch.Tensor, indices_out: torch.Tensor, counts_out: torch.Tensor,
                         sparsity_amount: float, top_p: float, min_keys: float, multiple_of: int, rk: float) -> None:
    """``|activations - cache|`` (rounded to the element type) -> ``topk_indices_p`` -> copy of every listed column of ``activations``
    into ``cache``, as one kernel: ``topk_delta_indices`` with the selection of ``topk_indices_p``.  GPU tensors only."""
    _check_top_p("topk_delta_indices_p", sparsity_amount, top_p, min_keys)
    torch.ops.chipmunk.topk_delta_indices_p(activations, cache, indices_out, counts_out, sparsity_amount, top_p, min_keys, multiple_of, rk)


def topk_group_delta_indices(activations: torch.Tensor, cache: torch.Tensor, indices_out: torch.Tensor, counts_out: torch.Tensor,
                             rows_per_group: int, sparsity_amount: float, multiple_of: int, rk: float) -> None:
    """``topk_delta_indices`` over ``R = rows_per_group`` block-mean rows per 128-row group (not in the reference; ``bm > mbm`` and the
    gate / up pairs of the gated MLP), as one kernel.  ``activations`` and ``cache`` are ``[B, rows, F]``; group ``g`` of
    ``G = ceil(rows / R)`` owns rows ``[g R, min((g + 1) R, rows))``; ``indices_out [B, G, F]``, ``counts_out [B, G]``.  The score of a
    column is ``T(sum_i float(T(|a_i - cache_i|)))``: rows ascending, summed in fp32, rounded to the element type once -- for ``R == 2``
    the bits of ``(a - cache).abs().reshape(B, G, 2, F).sum(2)``.  ``topk_indices`` on the scores; every listed column is copied from
    ``activations`` into ``cache`` in every row of the group, as ``copy_indices`` does.  GPU tensors only."""
    torch.ops.chipmunk.topk_group_delta_indices(activations, cache, indices_out, counts_out, rows_per_group, sparsity_amount, multiple_of, rk)


def topk_group_delta_indices_p(activations: torch.Tensor, cache: torch.Tensor, indices_out: torch.Tensor, counts_out: torch.Tensor,
                               rows_per_group: int, sparsity_amount: float, top_p: float, min_keys: float, multiple_of: int,
                               rk: float) -> None:
    """``topk_group_delta_indices`` with the selection of ``topk_indices_p`` on the scores.  GPU tensors only."""
    _check_top_p("topk_group_delta_indices_p", sparsity_amount, top_p, min_keys)
    torch.ops.chipmunk.topk_group_delta_indices_p(activations, cache, indices_out, counts_out, rows_per_group, sparsity_amount, top_p,
                                                  min_keys, multiple_of, rk)


def scatter_add(packed: torch.Tensor, unpacked: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor,
                num_sms: int) -> None:
    if packed.ndim == 3:   # a batch [B, M, F] with unpacked [B, F, M], indices [B, G, F], counts [B, G]: one launch
        torch.ops.chipmunk.csp_scatter_add(packed, unpacked, indices, counts, num_sms)
        return
    torch.ops.chipmunk.csp_scatter_add(packed.unsqueeze(0), unpacked.unsqueeze(0), indices.unsqueeze(0),
                                       counts.unsqueeze(0), num_sms)


def mask_to_indices(mask: torch.Tensor, multiple_of: int, pad_to_multiple_of: int) -> List[torch.Tensor]:
    return torch.ops.chipmunk.mask_to_indices(mask, multiple_of, pad_to_multiple_of)


def packed_mask_to_indices(packed: torch.Tensor, shape: Sequence[int], multiple_of: int,
                           pad_to_multiple_of: int) -> List[torch.Tensor]:
    """``mask_to_indices(bitunpack(packed, shape), ...)`` in one kernel (not in the reference)."""
    return torch.ops.chipmunk.packed_mask_to_indices(packed, list(shape), multiple_of, pad_to_multiple_of)


def mask_to_sorted_indices(mask: torch.Tensor, shape: Sequence[int], multiple_of: int,
                           pad_to_multiple_of: int) -> List[torch.Tensor]:
    """Same kept set / counts / padding as ``mask_to_indices`` (``mask`` bool) or ``packed_mask_to_indices`` (``mask``
    uint8 bit-packed, ``shape`` = original mask shape) with ASCENDING columns: sequential DRAM pages for the K/V gather."""
    return torch.ops.chipmunk.mask_to_sorted_indices(mask, list(shape), multiple_of, pad_to_multiple_of)


def mask_to_ragged_indices(mask: torch.Tensor, shape: Sequence[int], multiple_of: int, pad_to_multiple_of: int,
                           sorted: bool = True) -> List[torch.Tensor]:
    """The kept keys of every mask row as ragged rows, without the padded ``[b, h, m, pad_n]`` tensor: ``[flat, offsets, counts]``.
    ``mask`` bool ``[b, h, m, n]``, or uint8 bit-packed with ``shape`` (``n % 8 == 0``).  ``counts [b, h, m]`` int32: kept columns
    rounded up to ``multiple_of`` (it may exceed ``n``).  ``offsets [b*h*m + 1]`` int64: row ``r`` is ``flat[offsets[r]:offsets[r + 1]]``,
    ``min(counts[r], pad_n)`` rounded up to 32 entries wide.  ``flat`` int32, 64 spare zero entries at its end.  A row holds its True
    columns -- ascending (``sorted``), or the reference's order: classes ``c % 32`` one after the other, ascending inside a class --
    then the first False columns ascending up to ``counts[r]`` entries while there are any, then zeros.  What ``mask_to_sorted_indices``
    / ``(packed_)mask_to_indices`` followed by ``compact_indices`` give.  CPU tensors take the torch statement of that contract below."""
    if mask.is_cuda:
        return torch.ops.chipmunk.mask_to_ragged_indices(mask, list(shape), multiple_of, pad_to_multiple_of, sorted)
    if mask.dtype == torch.uint8:
        from .bitpack import bitunpack
        mask = bitunpack(mask, shape)
    b, h, m, n = mask.shape
    pad_n = (n + pad_to_multiple_of - 1) // pad_to_multiple_of * pad_to_multiple_of
    rows = mask.reshape(-1, n) != 0
    kept = rows.sum(dim=1)
    counts = (kept + multiple_of - 1) // multiple_of * multiple_of
    lengths = (counts.clamp(max=pad_n) + 31) // 32 * 32
    offsets = torch.zeros(rows.shape[0] + 1, dtype=torch.int64)
    offsets[1:] = lengths.cumsum(0)
    flat = torch.zeros(int(offsets[-1]) + 64, dtype=torch.int32)
    cols = torch.arange(n, dtype=torch.int32)
    for r in range(rows.shape[0]):
        true = cols[rows[r]]
        if not sorted:
            true = true[torch.argsort(true % 32, stable=True)]
        row = torch.cat([true, cols[~rows[r]][:int(counts[r] - kept[r])]])
        flat[int(offsets[r]):int(offsets[r]) + row.numel()] = row
    return [flat, offsets, counts.to(torch.int32).view(b, h, m)]


def topk_mask(cs: torch.Tensor, k: int, random_amount: float = 0.0, groups: Optional[torch.Tensor] = None,
              static_mask: Optional[torch.Tensor] = None, k_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``((top-k of cs | random) & groups) | static_mask`` as one kernel: the reference's ``random_and_topk``
    (``modules/attn.py:76-82``: randint + topk + scatter_ + two mask combines).  Exactly ``k`` columns per active row
    come from the top-k part (ties at the k-th value broken deterministically); the random part is a counter-based
    hash, so only ``random_amount = 0`` is comparable bit for bit with the torch chain.  Rows of up to
    ``TOPK_MASK_MAX_N`` columns; ties at the k-th value go to the columns lowest in ``((c % 4096) // 4, c)`` order.
    ``k_lens`` (an addition, int32 ``[B]`` on the GPU; padded batches): the rows of ``cs[b]`` select among their first
    ``k_lens[b]`` columns only -- ``k`` is capped there -- and are False past them whatever ``random_amount``, ``groups`` and
    ``static_mask`` say: ``mask[b, ..., :L]`` is the mask of ``cs[b, ..., :L]``."""
    from .attn import check_k_lens
    if check_k_lens(k_lens, cs, "topk_mask") is not None:
        return torch.ops.chipmunk.topk_mask_varlen(cs, k_lens, k, random_amount, groups, static_mask)
    return torch.ops.chipmunk.topk_mask(cs, k, random_amount, groups, static_mask)


def _bf16_keys(cs: torch.Tensor) -> torch.Tensor:
    """The order-preserving 16-bit image of bf16 bits as int64 (larger value = larger key; -0.0 below +0.0)."""
    bits = cs.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    return torch.where((bits & 0x8000) != 0, ~bits & 0xFFFF, bits | 0x8000)


def _topk_mask_p_cpu(cs: torch.Tensor, k: int, top_p: float, k_min: int, random_amount: float,
                     groups: Optional[torch.Tensor], static_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """The rule of ``topk_mask_p`` in plain torch: one sort per row in the kernels' total order, fp64 prefix sums."""
    if not (0.0 < top_p <= 1.0) or k_min < 0 or k < 0:
        raise ValueError(f"topk_mask_p: top_p must be in (0, 1], k and k_min >= 0 (got {top_p}, {k}, {k_min})")
    B, H, G, n = cs.shape
    k = min(int(k), n)
    cols = torch.arange(n, dtype=torch.int64)
    # one sortable integer per column: key descending, then ((c % 4096) // 4, c) ascending (n <= 2^19, tie rank < 2^30)
    rank = (0xFFFF - _bf16_keys(cs).view(-1, n)) * (1 << 30) + ((cols % 4096) // 4) * (1 << 20) + cols
    order = torch.argsort(rank, dim=-1)
    val = cs.reshape(-1, n).double()
    mass = torch.where(val > 0, val, torch.zeros_like(val)).gather(-1, order)      # negative and NaN entries carry no mass
    prefix = mass.cumsum(-1)
    total = prefix[:, -1:]
    k_p = (prefix < top_p * total).sum(-1) + 1                                     # the smallest count with prefix mass >= target
    k_p = torch.where(total[:, 0] > 0, k_p, torch.zeros_like(k_p))
    s = k_p.clamp(min=int(k_min)).clamp(max=k)
    keep = torch.zeros(cs.numel() // n, n, dtype=torch.bool)
    keep.scatter_(-1, order, cols[None, :] < s[:, None])
    keep = keep.view(B, H, G, n)
    if random_amount > 0:
        keep |= torch.rand(keep.shape) < random_amount
    if groups is not None:
        keep &= groups
    if static_mask is not None:
        keep = keep | static_mask
    return keep


def topk_mask_p(cs: torch.Tensor, k: int, top_p: float, k_min: int = 0, random_amount: float = 0.0,
                groups: Optional[torch.Tensor] = None, static_mask: Optional[torch.Tensor] = None,
                k_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``topk_mask`` with a count per row (not in the reference): an active row keeps the smallest top set of its columns that
    carries a share ``top_p`` of the row's column-sum mass -- at least ``k_min``, never more than ``k`` columns.  Order: value
    descending, ties by ``((c % 4096) // 4, c)``; mass of a column: its value where positive (negative and NaN entries carry none);
    ``s = min(k, max(k_p, k_min))`` with ``k_p`` the smallest prefix whose mass reaches ``top_p`` times the row's, 0 for an all-zero
    row.  The random, group and static parts are those of ``topk_mask``.  The kernel sums in fp32 in a fixed order (same launch,
    same bits); CPU tensors take a sort with fp64 sums.  ``k_lens`` as in ``topk_mask`` (the mass is that of the valid columns)."""
    from .attn import check_k_lens
    check_k_lens(k_lens, cs, "topk_mask_p")
    if not cs.is_cuda:
        return _topk_mask_p_cpu(cs, k, top_p, k_min, random_amount, groups, static_mask)
    if k_lens is not None:
        return torch.ops.chipmunk.topk_mask_p_varlen(cs, k_lens, k, top_p, k_min, random_amount, groups, static_mask)
    return torch.ops.chipmunk.topk_mask_p(cs, k, top_p, k_min, random_amount, groups, static_mask)


def manual_seed(seed: int) -> None:
    """Seed of the random-key hash used when ``random_amount`` / ``rk`` > 0 (see ``include/chipmunk_hip.h``:
    ``chipmunk_set_random_seed``).  Every launch draws a different set; the same seed and launch order reproduce a run."""
    from .._native import manual_seed as _seed
    _seed(seed)
