"""The rule of ``chipmunk_topk_mask_p`` written down as a small torch function, over the keys and the total order of
``topk_mask_model.py``, with fp64 sums:

    order   ``bf16_key`` descending, ties by ``((c % 4096) // 4, c)`` ascending
    mass    m_c = max(float(cs[c]), 0) (a NaN carries none), total = sum m_c, target = top_p * total
    k_p     the smallest count whose prefix of the order has mass >= target; 0 when total is 0
    s       min(k, max(k_p, k_min)), k clamped to n
    mask[r, c] = (c among the first s columns of the order) & groups[r]  |  static[r, c]          (random part off)

Also here: the exact-row generator of the GPU test (integer column sums whose every partial sum is exact in fp32) and a brute-force
statement of the rule for short rows.
"""
import torch

from topk_mask_model import bf16_keys


def row_order(keys: torch.Tensor) -> torch.Tensor:
    """int64 [n]: the columns of one row of keys (int32 [n]) in the total order."""
    n = keys.numel()
    cols = torch.arange(n, dtype=torch.int64)
    rank = (0xFFFF - keys.to(torch.int64)) * (1 << 32) + ((cols % 4096) // 4) * (1 << 22) + cols        # n < 2^22
    return torch.argsort(rank)


def topp_row(cs_row: torch.Tensor, k: int, top_p: float, k_min: int):
    """(keep bool [n], s, k_p) of one bf16 row."""
    n = cs_row.numel()
    k = min(int(k), n)
    order = row_order(bf16_keys(cs_row))
    val = cs_row.double()
    mass = torch.where(val > 0, val, torch.zeros_like(val))[order]
    total = float(mass.sum())
    k_p = 0
    if total > 0:
        prefix = torch.cumsum(mass, 0)
        k_p = int((prefix < top_p * total).sum()) + 1
    s = min(k, max(k_p, int(k_min)))
    keep = torch.zeros(n, dtype=torch.bool)
    keep[order[:s]] = True
    return keep, s, k_p


def topk_mask_p_model(cs: torch.Tensor, k: int, top_p: float, k_min: int, groups=None, static=None):
    """``cs`` bf16 [B, H, G, n] (CPU); ``groups`` bool [1|B, H, G, 1] or None; ``static`` bool [1|B, H, G, n] or None.
    Returns (mask [B, H, G, n], counts int64 [B*H*G, 2]: per row (s, k_p); (0, 0) for an inactive row)."""
    cs = cs.cpu()
    B, H, G, n = cs.shape
    rows = cs.reshape(-1, n)
    active = torch.ones(B * H * G, dtype=torch.bool) if groups is None else groups.cpu().expand(B, H, G, 1).reshape(-1)
    out = torch.zeros(B * H * G, n, dtype=torch.bool)
    counts = torch.zeros(B * H * G, 2, dtype=torch.int64)
    for r in range(B * H * G):
        if bool(active[r]):
            out[r], s, k_p = topp_row(rows[r], k, top_p, k_min)
            counts[r, 0], counts[r, 1] = s, k_p
    out = out.view(B, H, G, n)
    if static is not None:
        out = out | static.cpu()
    return out, counts


def brute_force_row(cs_row: torch.Tensor, k: int, top_p: float, k_min: int):
    """The rule for a short row with Python lists and a Python sort, the sums in Python floats (fp64; the callers' values are small
    multiples of 1/8, whose sums are exact): (kept columns as a set, s, k_p)."""
    n = cs_row.numel()
    keys = bf16_keys(cs_row).tolist()
    vals = [x if x > 0 else 0.0 for x in cs_row.double().tolist()]     # (NaN > 0 is False)
    order = sorted(range(n), key=lambda c: (-keys[c], (c % 4096) // 4, c))
    total = sum(vals)
    target = top_p * total
    k_p = 0
    if total > 0:
        acc = 0.0
        for i, c in enumerate(order):
            acc += vals[c]
            if acc >= target:
                k_p = i + 1
                break
    s = min(min(k, n), max(k_p, k_min))
    return set(order[:s]), s, k_p


def exact_rows(rows: int, n: int, hot: int, seed: int) -> torch.Tensor:
    """bf16 [1, 1, rows, n]: integer column sums -- a background uniform in {0, 1, 2} and ``hot`` random columns set to 2^e, e uniform
    in 3..7.  Every value and every partial sum in any order is an integer below 2^20 (n <= 131 072: at most 2 * 131 072 + 128 * hot),
    so fp32 sums are exact, and so is ``top_p * total`` for top_p in {0.5, 0.75}."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 3, (rows, n), generator=g).float()
    for r in range(rows):
        cols = torch.randperm(n, generator=g)[:hot]
        x[r, cols] = 2.0 ** torch.randint(3, 8, (hot,), generator=g).float()
    assert float(x.sum(-1).max()) < 2 ** 20
    return x.to(torch.bfloat16).view(1, 1, rows, n)


def regime(s_kp, k: int, k_min: int) -> str:
    """Which of the three regimes a row's (s, k_p) is in."""
    k_p = int(s_kp[1])
    return "k_min" if k_p < k_min else ("top_p" if k_p < k else "cap")


def threshold_inside_tie_class(cs_row: torch.Tensor, s: int) -> bool:
    """True when the s-th column of the order has the same key as the (s+1)-th: the kept set ends inside a class of equal values."""
    keys = bf16_keys(cs_row)
    order = row_order(keys)
    return 0 < s < cs_row.numel() and int(keys[order[s - 1]]) == int(keys[order[s]])
