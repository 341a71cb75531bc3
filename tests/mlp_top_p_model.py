"""The rule of ``chipmunk_topk_indices_p`` / ``chipmunk_topk_delta_indices_p`` (config ``mlp.top_p``) written down as small
torch functions with fp64 sums, the checker the tests hold a stored selection to, the exact-row generator of the GPU test and a
brute-force statement of the rule for short rows.

One row of values ``v_c``, c in [0, F) -- the plain operator takes the activations as given, the fused delta form ``|T(b_c - cache_c)|``
rounded to the element type T:

    mass     m_c = v_c where v_c > 0 (a zero, negative or NaN entry carries none)
    total    sum of m_c over the WHOLE row (not over the sample), target = top_p * total
    thr_p    the largest t with sum of m_c over {v_c >= t} >= target (a class of equal values is taken whole); +inf when total == 0
    thr_q    today's threshold: element int(1024 q) of the ascending-sorted first 1024 values, q = sparsity_amount = 1 - top_keys;
             -inf for q == 0 (no cap); q == 1 keeps nothing, as today
    thr_min  the same order statistic at q = 1 - min_keys (its index never below thr_q's); +inf when min_keys == 0
    thr      min(max(thr_p, thr_q), thr_min)
    kept     m_c > 0 and v_c >= thr, in ascending column order

Then, as ``topk_indices``: the count is rounded up to ``multiple_of`` with rejected columns -- the last rejected column of every residue
mod 1024, residues ascending, as far as there are any -- and ``counts`` is kept + padding.

Consequences: the kept set is a subset of what the ``top_keys`` rule keeps (the cap is a threshold: no tie-break); an all-zero row
keeps nothing (today's rule keeps the whole row); the floor is a sampled quantile like the cap, blind to columns past the first 1024.
``defect=`` turns `thresholds` / `kept_columns` / `selection` into one of the mutants of tests/test_mlp_top_p_host.py.
"""
import math

import torch

DEFECTS = ("total_over_sample", "strict_target", "cap_ignored", "floor_ignored", "tie_class_high", "tie_class_low", "zero_mass_kept",
           "padding_repeats_kept")
SAMPLE = 1024
INF = float("inf")


def quantile_index(q: float) -> int:
    """``int(1024 * q)`` with q rounded to fp32 first, as the kernels hold it"""
    return int(SAMPLE * float(torch.tensor(float(q), dtype=torch.float32)))


def sample_value(v64: torch.Tensor, idx: int) -> float:
    """element `idx` of the ascending-sorted first 1024 values; +inf past the sample's end"""
    return INF if idx >= SAMPLE else float(v64[:SAMPLE].sort().values[idx])


def thresholds(v: torch.Tensor, sparsity_amount: float, top_p: float, min_keys: float, defect=None):
    """dict(thr_p, thr_q, thr_min, thr, total) of one row (any float dtype; taken to fp64, which holds bf16 / fp16 / fp32 exactly)."""
    assert defect is None or defect in DEFECTS, defect
    v64 = v.detach().cpu().double().flatten()
    mass = torch.where(v64 > 0, v64, torch.zeros_like(v64))
    total = float(mass[:SAMPLE].sum() if defect == "total_over_sample" else mass.sum())
    target = float(top_p) * total
    thr_p = INF
    if total > 0:
        pos = mass[mass > 0].sort(descending=True).values
        csum = torch.cumsum(pos, 0)
        reached = (csum > target) if defect == "strict_target" else (csum >= target)
        # (only the mutants can miss the target: they then keep every positive column)
        thr_p = float(pos[int(torch.nonzero(reached)[0])]) if bool(reached.any()) else float(pos[-1])
        classes = torch.unique(pos)             # ascending
        at = int(torch.searchsorted(classes, torch.tensor(thr_p, dtype=torch.float64)))
        if defect == "tie_class_high":
            thr_p = float(classes[at + 1]) if at + 1 < classes.numel() else INF
        if defect == "tie_class_low" and at > 0:
            thr_p = float(classes[at - 1])
    iq = quantile_index(sparsity_amount)
    thr_q = -INF if float(sparsity_amount) == 0.0 else sample_value(v64, iq)
    thr_min = INF if float(min_keys) == 0.0 else sample_value(v64, max(quantile_index(1.0 - float(min_keys)), iq))
    if defect == "cap_ignored":
        thr_q = -INF
    if defect == "floor_ignored":
        thr_min = INF
    return dict(thr_p=thr_p, thr_q=thr_q, thr_min=thr_min, thr=min(max(thr_p, thr_q), thr_min), total=total)


def kept_columns(v: torch.Tensor, sparsity_amount: float, top_p: float, min_keys: float, defect=None) -> torch.Tensor:
    """int64, ascending: the columns the threshold part keeps"""
    v64 = v.detach().cpu().double().flatten()
    if float(torch.tensor(float(sparsity_amount), dtype=torch.float32)) == 1.0:
        return torch.zeros(0, dtype=torch.int64)
    thr = thresholds(v64, sparsity_amount, top_p, min_keys, defect)["thr"]
    keep = v64 >= thr
    if defect != "zero_mass_kept":
        keep &= v64 > 0
    return torch.nonzero(keep).flatten()


def padding_columns(kept: torch.Tensor, f: int, multiple_of: int) -> torch.Tensor:
    """the padding of a row without random keys: the last rejected column of every residue mod 1024, residues ascending, at most
    ``-len(kept) % multiple_of`` of them"""
    pad = (-kept.numel()) % multiple_of
    rejected = torch.ones(f, dtype=torch.bool)
    rejected[kept] = False
    last = {}
    for c in torch.nonzero(rejected).flatten().tolist():
        last[c % SAMPLE] = c
    return torch.tensor([last[t] for t in sorted(last)][:pad], dtype=torch.int64)


def selection(v: torch.Tensor, sparsity_amount: float, top_p: float, min_keys: float, multiple_of: int, defect=None):
    """(indices int32 [F] with -1 past the listed entries, count) of one row, random keys off"""
    f = v.numel()
    kept = kept_columns(v, sparsity_amount, top_p, min_keys, defect)
    padding = padding_columns(kept, f, multiple_of)
    if defect == "padding_repeats_kept" and padding.numel() and kept.numel():
        padding[0] = kept[0]
    out = torch.full((f,), -1, dtype=torch.int32)
    out[: kept.numel()] = kept.to(torch.int32)
    out[kept.numel(): kept.numel() + padding.numel()] = padding.to(torch.int32)
    return out, (kept.numel() + multiple_of - 1) // multiple_of * multiple_of


def regime(t) -> str:
    """which part of ``thr = min(max(thr_p, thr_q), thr_min)`` decides a row (`t` from `thresholds`)"""
    if t["thr_p"] > t["thr_min"]:
        return "floor"
    return "cap" if t["thr_p"] < t["thr_q"] else "top_p"


# ------------------------------------------------------------------------------------------------------------------ checker
def check_row(indices_row: torch.Tensor, count: int, kept: torch.Tensor, f: int, multiple_of: int, where: str = "") -> None:
    """A stored row (indices [F], count) against the model's kept set S (``kept``, ascending), random keys off:
    ``count == ceil(|S| / multiple_of) * multiple_of``; ``indices[:|S|] == sorted(S)``; the padding entries ``indices[|S|:count]`` are
    distinct, in range and not in S (there are as many as there are residues mod 1024 with a rejected column, when that is fewer)."""
    s = kept.numel()
    want = (s + multiple_of - 1) // multiple_of * multiple_of
    assert int(count) == want, f"{where}: count {int(count)}, the model keeps {s} -> {want}"
    row = indices_row.detach().cpu().to(torch.int64)
    assert torch.equal(row[:s], kept), f"{where}: the first {s} entries are not the model's kept columns in ascending order"
    in_s = torch.zeros(f, dtype=torch.bool)
    in_s[kept] = True
    residues = torch.unique(torch.nonzero(~in_s).flatten() % SAMPLE).numel()
    pad = row[s: s + min(want - s, residues)]
    assert pad.numel() == min(want - s, residues)
    assert bool(((pad >= 0) & (pad < f)).all()), f"{where}: padding entries out of range"
    assert torch.unique(pad).numel() == pad.numel(), f"{where}: padding entries repeat"
    assert not bool(in_s[pad].any()), f"{where}: a padding entry repeats a kept column"


def check_rows(indices: torch.Tensor, counts: torch.Tensor, values: torch.Tensor, sparsity_amount: float, top_p: float, min_keys: float,
               multiple_of: int, where: str = ""):
    """`check_row` over [R, F] rows of values; returns the model's kept counts"""
    f = values.shape[-1]
    values, indices, counts = values.reshape(-1, f).cpu(), indices.reshape(-1, f).cpu(), counts.reshape(-1).cpu()
    sizes = []
    for r in range(values.shape[0]):
        kept = kept_columns(values[r], sparsity_amount, top_p, min_keys)
        check_row(indices[r], int(counts[r]), kept, f, multiple_of, f"{where} row {r}")
        sizes.append(kept.numel())
    return sizes


def check_mlp_trace(trace, mods, cfg):
    """Every selection a SparseDiffMlp route stored (``trace`` of method_model.run_mlp_route, ``mods`` its modules, ``cfg`` the mlp
    section still as the run left it) against the model, over block means recomputed here with the module's own functions: the cache is
    the block means of the last full step with the listed columns of every later selection copied in.  Returns (calls that made a
    selection, those among them in which some group stored a smaller count than ``ops.topk_indices`` gives for the same values)."""
    from chipmunk_amd import ops
    from chipmunk_amd.modules.mlp import block_mean
    assert cfg["bm"] == cfg["mbm"] and cfg["random_keys"] == 0.0
    sparsity, top_p, min_keys, mult = 1 - cfg["top_keys"], cfg["top_p"], cfg["top_p_min_keys"], cfg["counts_multiple_of"]
    cache, selected, made, smaller = {}, set(), 0, 0
    with torch.no_grad():
        for e in trace:
            key, fc1, x, step = (e["layer"], e["inv"]), mods[e["layer"]].fc1[0], e["x"], e["step"]
            if step % cfg["full_step_every"] == 0:
                cache[key] = block_mean(fc1(x), cfg["mbm"]).clone()
                continue
            if step % cfg["block_mask_cache"] != 0 and step >= 10 and key in selected:
                continue                                    # the cached-selection branch: nothing selected, block means left alone
            selected.add(key)
            bmfc1 = fc1(block_mean(x, cfg["mbm"]))
            v = (bmfc1 - cache[key]).abs()
            inds, counts = e["sel"]
            check_rows(inds, counts, v[0], sparsity, top_p, min_keys, mult, f"step {step} invocation {e['inv']} layer {e['layer']}")
            ti, tc = torch.empty_like(v, dtype=torch.int32), torch.empty(v.shape[:2], dtype=torch.int32, device=v.device)
            ops.topk_indices(v, ti, tc, sparsity, mult, 0.0)
            made += 1
            smaller += bool((counts.cpu() < tc[0].cpu()).any())
            assert bool((counts.cpu() <= tc[0].cpu()).all()), "a group stores more columns than the top_keys rule gives"
            for g in range(inds.shape[0]):
                cols = inds[g, : int(counts[g])].long()
                cache[key][0, g, cols] = bmfc1[0, g, cols]
    return made, smaller


# ------------------------------------------------------------------------------------------------------------------ exact rows
EXACT_ROWS = 24
EXACT_F = (1024, 1500, 12288, 17024)
EXACT_TOP_KEYS = 0.3
EXACT_PARAMS = ((0.5, 0.1), (0.75, 0.05))       # (top_p, min_keys)


def exact_rows(f: int) -> torch.Tensor:
    """fp32 [24, f]: row r is floor(255.999 u^conc), u uniform, conc = (1, 2, 4, 8)[r % 4].  Every value is a bf16-exact integer <= 255
    and every sum is below 2^24 / 3 (f <= 21 000), so every partial sum in any order -- and ``top_p * total`` for top_p in {0.5, 0.75} -- is
    exact in fp32: a kernel that sums in fp32 must give the fp64 rule bit for bit."""
    assert 255 * f < 2 ** 24 // 3
    g = torch.Generator().manual_seed(7)
    u = torch.rand(EXACT_ROWS, f, generator=g, dtype=torch.float64)
    conc = torch.tensor([(1.0, 2.0, 4.0, 8.0)[r % 4] for r in range(EXACT_ROWS)], dtype=torch.float64)[:, None]
    return torch.floor(255.999 * u ** conc).float()


def regimes_of(rows: torch.Tensor, top_keys: float, top_p: float, min_keys: float):
    return [regime(thresholds(rows[r], 1 - top_keys, top_p, min_keys)) for r in range(rows.shape[0])]


def assert_exact_rows_cover_the_regimes():
    """each of cap / top_p / floor decides at least 6 rows over the GPU test's parameter set, and no row keeps everything"""
    seen = {"cap": 0, "top_p": 0, "floor": 0}
    for f in EXACT_F:
        rows = exact_rows(f)
        for top_p, min_keys in EXACT_PARAMS:
            for name in regimes_of(rows, EXACT_TOP_KEYS, top_p, min_keys):
                seen[name] += 1
            for r in range(EXACT_ROWS):
                assert kept_columns(rows[r], 1 - EXACT_TOP_KEYS, top_p, min_keys).numel() < f
    assert min(seen.values()) >= 6, seen
    return seen


# ------------------------------------------------------------------------------------------------------------------ brute force
def brute_force_row(values, sparsity_amount: float, top_p: float, min_keys: float):
    """The rule for a short row with Python lists, a Python sort and Python floats (the callers' values are multiples of 1/8, whose
    sums are exact): the kept columns as a sorted list."""
    vals = [float(x) for x in values]
    if sparsity_amount == 1.0:
        return []
    total = sum(x for x in vals if x > 0)
    target = top_p * total
    thr_p = INF
    if total > 0:
        for t in sorted(set(x for x in vals if x > 0), reverse=True):        # candidates from the largest down: the first that reaches
            if sum(x for x in vals if x > 0 and x >= t) >= target:
                thr_p = t
                break
    sample = sorted(vals[:SAMPLE])
    iq = int(SAMPLE * sparsity_amount)
    thr_q = -INF if sparsity_amount == 0 else sample[iq]
    thr_min = INF
    if min_keys != 0:
        im = max(int(SAMPLE * (1.0 - min_keys)), iq)
        thr_min = sample[im] if im < SAMPLE else INF
    thr = min(max(thr_p, thr_q), thr_min)
    return [c for c, x in enumerate(vals) if x > 0 and x >= thr]


def ceil_to(n: int, multiple_of: int) -> int:
    return int(math.ceil(n / multiple_of)) * multiple_of
