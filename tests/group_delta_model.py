"""The contract of ``topk_group_delta_indices[_p]`` (config ``mlp.fused_group_topk_delta``) in plain torch on the CPU.

``activation`` and ``cache`` are ``[B, rows, F]`` of one dtype T; group ``g`` of ``G = ceil(rows / R)`` owns rows ``[g R, min((g + 1) R, rows))``.

    score    s_c = T( sum_i float( T(|b_i[c] - cache_i[c]|) ) ): i ascending over the group's rows, an explicit fp32 loop that starts from
             the first term, rounded to T once
    list     ``oracle.topk_indices`` on the ``[B, G, F]`` scores (the ``_p`` form: ``mlp_top_p_model.selection`` row by row)
    copy     every listed column, padding included, from ``activation`` into ``cache`` in every row the group owns
"""
import torch

import mlp_top_p_model as tp
import oracle


def groups_of(rows: int, r: int) -> int:
    return (rows + r - 1) // r


def scores(b: torch.Tensor, cache: torch.Tensor, r: int) -> torch.Tensor:
    """[B, rows, F] x 2 -> [B, G, F] in the operands' dtype"""
    b, cache = b.cpu(), cache.cpu()
    assert b.shape == cache.shape and b.dtype == cache.dtype and b.ndim == 3
    bsz, rows, f = b.shape
    t = (b - cache).abs()                                 # T(|b - cache|): one rounding to T, the sign bit cleared
    out = torch.empty(bsz, groups_of(rows, r), f, dtype=b.dtype)
    for g in range(out.shape[1]):
        lo, hi = g * r, min((g + 1) * r, rows)
        s = t[:, lo].float()
        for i in range(lo + 1, hi):
            s = s + t[:, i].float()
        out[:, g] = s.to(b.dtype)
    return out


def copy_listed(b: torch.Tensor, cache: torch.Tensor, inds: torch.Tensor, counts: torch.Tensor, r: int) -> torch.Tensor:
    """the cache after the copy (a new tensor): rows of other groups and unlisted columns keep their bits"""
    out = cache.cpu().clone()
    b = b.cpu()
    bsz, rows, f = b.shape
    for s in range(bsz):
        for g in range(inds.shape[1]):
            cols = inds[s, g, : min(int(counts[s, g]), f)].long()
            cols = cols[(cols >= 0) & (cols < f)]          # (a count may run past the entries there are candidates for)
            lo, hi = g * r, min((g + 1) * r, rows)
            out[s, lo:hi, cols] = b[s, lo:hi, cols]
    return out


def run(b, cache, r, sparsity, multiple_of, fill=-9):
    """(indices [B, G, F] int32 with `fill` where nothing is listed, counts [B, G] int32, cache after the copy), random keys off"""
    sc = scores(b, cache, r)
    inds = torch.full(sc.shape, fill, dtype=torch.int32)
    counts = torch.zeros(sc.shape[:2], dtype=torch.int32)
    oracle.topk_indices(sc, inds, counts, sparsity, multiple_of, 0.0)
    return inds, counts, copy_listed(b, cache, inds, counts, r)


def run_p(b, cache, r, sparsity, top_p, min_keys, multiple_of):
    """the same for the ``_p`` form: indices carry -1 past the listed entries (compare ``[:count]``)"""
    sc = scores(b, cache, r)
    inds = torch.full(sc.shape, -1, dtype=torch.int32)
    counts = torch.zeros(sc.shape[:2], dtype=torch.int32)
    for s in range(sc.shape[0]):
        for g in range(sc.shape[1]):
            row, cnt = tp.selection(sc[s, g], sparsity, top_p, min_keys, multiple_of)
            inds[s, g], counts[s, g] = row, cnt
    return inds, counts, copy_listed(b, cache, inds, counts, r)
