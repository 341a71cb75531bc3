"""The rule of ``chipmunk_topk_mask`` written down as a small torch function: the yardstick for rows that contain
ties, where ``torch.topk`` leaves the choice among equal values open.  bf16 has fewer than 65 536 values, so every row longer than
that contains ties.

    mask[r, c] = (c in topk_k(cs[r, :n])) & groups[r]  |  static[r, c]          (random part off)

* keys: the order-preserving 16-bit image of the bf16 bits (``bf16_key``: larger value = larger key; -0.0 sorts below +0.0);
* ``k`` is clamped to ``n``; an inactive row or ``k = 0`` keeps only the static part;
* threshold T = the largest T with #{key >= T} >= k; every key above T is kept, and exactly ``k - #{key > T}`` of the keys equal
  to T, taken in ascending order of ``((c % 4096) // 4, c)``: the kernels' thread order under the mapping "thread t owns columns
  4t + 4096j + e", then ascending column inside a thread.
"""
import torch


def bf16_keys(cs: torch.Tensor) -> torch.Tensor:
    """int32 keys in [0, 65535] of a bf16 tensor."""
    bits = cs.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where((bits & 0x8000) != 0, ~bits & 0xFFFF, bits | 0x8000)


def topk_row(keys: torch.Tensor, k: int) -> torch.Tensor:
    """bool [n]: the top-k part of one row of keys (int32 [n])."""
    n = keys.numel()
    k = min(int(k), n)
    keep = torch.zeros(n, dtype=torch.bool)
    if k <= 0:
        return keep
    thr = int(torch.sort(keys, descending=True).values[k - 1])      # largest T with #{key >= T} >= k
    above = keys > thr
    keep |= above
    need = k - int(above.sum())
    assert need >= 1
    ties = torch.nonzero(keys == thr).flatten()
    order = torch.argsort(((ties % 4096) // 4) * (1 << 22) + ties)   # ((c % 4096) // 4, c), n < 2^22
    keep[ties[order[:need]]] = True
    return keep


def topk_mask_model(cs: torch.Tensor, k: int, groups=None, static=None) -> torch.Tensor:
    """``cs`` bf16 [B, H, G, n] (CPU); ``groups`` bool [1|B, H, G, 1] or None; ``static`` bool [1|B, H, G, n] or None."""
    cs = cs.cpu()
    B, H, G, n = cs.shape
    keys = bf16_keys(cs).view(-1, n)
    active = torch.ones(B * H * G, dtype=torch.bool) if groups is None else groups.cpu().expand(B, H, G, 1).reshape(-1)
    out = torch.zeros(B * H * G, n, dtype=torch.bool)
    for r in range(B * H * G):
        if bool(active[r]):
            out[r] = topk_row(keys[r], k)
    out = out.view(B, H, G, n)
    if static is not None:
        out = out | static.cpu()
    return out
