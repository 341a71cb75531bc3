"""``topk_indices_p`` / ``topk_delta_indices_p`` on the device against the rule's model (tests/mlp_top_p_model.py).

* exact rows (integers whose every partial sum is exact in fp32): indices, counts and the fused form's cache bit for bit against the fp64
  rule, over row lengths with a tail that is no multiple of 1024 (1500) and with columns past the registers and a second compaction pass
  (17 024 = 16 384 + 640), plain and delta forms, three dtypes;
* hand-made rows: all-zero, one-hot, constant, mass where the sample is blind, top_p = 1, sparsity 0 and 1;
* general bf16 rows, where the fp32 summation order matters: the kept set lies between the model's sets at top_p (1 -+ eps),
  eps = 4 F 2^-24 (an fp32 sum of F non-negative terms in any order is off by at most (F - 1) 2^-24 relative; both sums and the product);
* random keys: the listed set contains the model's, the number of extras is binomial, launches differ, a seed repeats them.
"""
import functools
import math

import pytest
import torch

import mlp_top_p_model as tp

pytestmark = pytest.mark.gpu
SPARSITY = 1 - tp.EXACT_TOP_KEYS
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    tp.assert_exact_rows_cover_the_regimes()        # from the model, before the device is touched
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def exact_kept(f, top_p, min_keys):
    """the model's kept columns of the exact rows, computed once per (F, parameters) and shared by the forms and dtypes"""
    rows = tp.exact_rows(f)
    return tuple(tp.kept_columns(rows[r], SPARSITY, top_p, min_keys) for r in range(rows.shape[0]))


def delta_operands(vals, dtype, seed=11):
    """(b, cache) with |T(b - cache)| == vals exactly: cache in {0, 1}, b = cache +- vals (vals <= 255: every operand an integer of at
    most 256 in magnitude, exact in bf16)"""
    g = torch.Generator().manual_seed(seed)
    cache = torch.randint(0, 2, vals.shape, generator=g).float()
    sign = torch.where((torch.rand(vals.shape, generator=g) < 0.5) & (vals < 255), -1.0, 1.0)
    b = cache + sign * vals
    assert float(b.abs().max()) <= 256 and torch.equal((b - cache).abs(), vals)
    return b.to(dtype), cache.to(dtype)


def launch(dev, vals, form, sparsity, top_p, min_keys, multiple_of, rk, dtype=torch.bfloat16):
    """vals [R, F] fp32 -> (indices [R, F] cpu, counts [R] cpu); the fused form's cache contract is asserted here"""
    from chipmunk_amd import ops
    r, f = vals.shape
    inds = torch.full((1, r, f), -9, dtype=torch.int32, device=dev)
    counts = torch.full((1, r), -9, dtype=torch.int32, device=dev)
    if form == "plain":
        assert torch.equal(vals.to(dtype).float(), vals)
        ops.topk_indices_p(vals.to(dtype)[None].to(dev), inds, counts, sparsity, top_p, min_keys, multiple_of, rk)
    else:
        b, cache0 = delta_operands(vals, dtype)
        b, cache = b[None].to(dev), cache0[None].to(dev)
        ops.topk_delta_indices_p(b, cache, inds, counts, sparsity, top_p, min_keys, multiple_of, rk)
        # the cache equals the activation on every listed column and keeps its bits everywhere else
        listed = torch.zeros(r, f, dtype=torch.bool)
        ci, cc = inds[0].cpu(), counts[0].cpu()
        for i in range(r):
            cols = ci[i, : int(cc[i])].long()
            listed[i, cols[(cols >= 0) & (cols < f)]] = True
        want = torch.where(listed, b[0].cpu().float(), cache0.float())
        assert torch.equal(cache[0].cpu().float(), want), f"{form}: cache contract"
    torch.cuda.synchronize()
    return inds[0].cpu(), counts[0].cpu()


# ------------------------------------------------------------------------------------------------------------------ exact rows
@pytest.mark.parametrize("form", ["plain", "delta"])
@pytest.mark.parametrize("top_p,min_keys", tp.EXACT_PARAMS)
@pytest.mark.parametrize("f", tp.EXACT_F)
def test_exact_rows_bit_for_bit(dev, f, top_p, min_keys, form):
    vals = tp.exact_rows(f)
    inds, counts = launch(dev, vals, form, SPARSITY, top_p, min_keys, 256, 0.0)
    kept = exact_kept(f, top_p, min_keys)
    for r in range(vals.shape[0]):
        tp.check_row(inds[r], int(counts[r]), kept[r], f, 256, f"F {f} top_p {top_p} {form} row {r}")
    print(f"F {f} top_p {top_p} min_keys {min_keys} {form}: kept per row", [k.numel() for k in kept])


@pytest.mark.parametrize("form", ["plain", "delta"])
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_exact_rows_other_dtypes(dev, dtype, form):
    top_p, min_keys = tp.EXACT_PARAMS[0]
    vals = tp.exact_rows(1500)
    inds, counts = launch(dev, vals, form, SPARSITY, top_p, min_keys, 256, 0.0, DTYPES[dtype])
    kept = exact_kept(1500, top_p, min_keys)
    for r in range(vals.shape[0]):
        tp.check_row(inds[r], int(counts[r]), kept[r], 1500, 256, f"{dtype} {form} row {r}")


# ------------------------------------------------------------------------------------------------------------------ hand-made rows
@pytest.mark.parametrize("form", ["plain", "delta"])
@pytest.mark.parametrize("f", [1024, 1500])
def test_hand_made_rows(dev, f, form):
    from chipmunk_amd import ops
    zero = torch.zeros(f)
    one_hot = zero.clone()
    one_hot[f - 7] = 5.0
    const = torch.full((f,), 3.0)
    exact = tp.exact_rows(f)[1]
    rows = {"zero": zero, "one_hot": one_hot, "const": const, "exact": exact}
    if f > 1024:
        blind = zero.clone()
        blind[1024:] = tp.exact_rows(f)[2, 1024:].clamp(min=1.0)       # mass only where the 1024-column sample cannot see it
        rows["blind"] = blind
    vals = torch.stack(list(rows.values()))
    name = list(rows)
    seen = {}
    for sparsity, top_p, min_keys in ((SPARSITY, 0.5, 0.0), (SPARSITY, 0.5, 0.1), (SPARSITY, 1.0, 0.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.25),
                                      (1.0, 0.5, 0.0)):
        inds, counts = launch(dev, vals, form, sparsity, top_p, min_keys, 256, 0.0)
        sizes = tp.check_rows(inds, counts, vals, sparsity, top_p, min_keys, 256, f"{form} F {f} sparsity {sparsity} top_p {top_p} min_keys {min_keys}")
        seen[(sparsity, top_p, min_keys)] = dict(zip(name, sizes))
        assert int(counts[name.index("zero")]) == 0                             # an all-zero row keeps nothing, with a floor and without
        if sparsity == 1.0:
            assert (counts == 0).all() and (inds == -1).all()                   # keeps nothing, as topk_indices
            continue
        assert sizes[name.index("one_hot")] == 1 and int(inds[name.index("one_hot"), 0]) == f - 7
        assert sizes[name.index("const")] == f                                  # one class of equal values: taken whole
        if f > 1024:
            # thr_q = thr_min = 0 from an all-zero sample: top-p alone decides among the columns the sample cannot see
            assert 0 < sizes[name.index("blind")] <= f - 1024
        if top_p == 1.0:        # every positive column that passes the cap
            thr_q = tp.thresholds(exact, sparsity, 1.0, min_keys)["thr_q"]
            assert sizes[name.index("exact")] == int(((exact > 0) & (exact >= thr_q)).sum())
    assert seen[(0.0, 1.0, 0.25)]["exact"] == int((exact > 0).sum()) > seen[(SPARSITY, 1.0, 0.0)]["exact"]     # sparsity 0: no cap
    # the constant row: the cap's own set, entry for entry
    act = const.to(torch.bfloat16)[None, None].to(dev)
    ti, tc = torch.full((1, 1, f), -9, dtype=torch.int32, device=dev), torch.zeros(1, 1, dtype=torch.int32, device=dev)
    ops.topk_indices(act, ti, tc, SPARSITY, 256, 0.0)
    pi, pc = torch.full_like(ti, -9), torch.zeros_like(tc)
    ops.topk_indices_p(act, pi, pc, SPARSITY, 0.5, 0.0, 256, 0.0)
    assert torch.equal(tc, pc) and torch.equal(ti, pi)


# ------------------------------------------------------------------------------------------------------------------ general rows
def general_rows(rows, f, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, f, generator=g).abs() * torch.exp(torch.randn(1, f, generator=g))).to(torch.bfloat16).float()


@pytest.mark.parametrize("form", ["plain", "delta"])
@pytest.mark.parametrize("f,top_p,min_keys", [(1500, 0.5, 0.1), (12288, 0.75, 0.05), (17024, 0.9, 0.0)])
def test_general_rows_within_the_fp32_bound(dev, f, top_p, min_keys, form):
    from chipmunk_amd import ops
    vals = general_rows(8, f, 5)
    if form == "plain":
        inds, counts = launch(dev, vals, "plain", SPARSITY, top_p, min_keys, 256, 0.0)
        again = launch(dev, vals, "plain", SPARSITY, top_p, min_keys, 256, 0.0)
    else:           # the delta of general values: cache 0, so that |bf16(b - 0)| is the value itself
        def fused():
            b, cache = vals.to(torch.bfloat16)[None].to(dev), torch.zeros(1, *vals.shape, dtype=torch.bfloat16, device=dev)
            i, c = torch.full((1, *vals.shape), -9, dtype=torch.int32, device=dev), torch.zeros(1, vals.shape[0], dtype=torch.int32, device=dev)
            ops.topk_delta_indices_p(b, cache, i, c, SPARSITY, top_p, min_keys, 256, 0.0)
            return i[0].cpu(), c[0].cpu()
        (inds, counts), again = fused(), fused()
    assert torch.equal(counts, again[1])            # two launches: identical bits
    eps = 4 * f * 2.0 ** -24
    for r in range(vals.shape[0]):
        c = int(counts[r])
        assert torch.equal(inds[r, :c], again[0][r, :c])
        lo = tp.kept_columns(vals[r], SPARSITY, top_p * (1 - eps), min_keys)
        hi = tp.kept_columns(vals[r], SPARSITY, min(1.0, top_p * (1 + eps)), min_keys)
        assert set(lo.tolist()) <= set(hi.tolist())
        # the kept sets are nested threshold sets: the device's is one of those between lo and hi (each with its own padding)
        between = torch.unique(vals[r][hi]).tolist()
        cands = [hi[vals[r][hi] >= t] for t in between if t <= (float(vals[r][lo].min()) if lo.numel() else float("inf"))] or [lo]
        ok = False
        for kept in cands:
            try:
                tp.check_row(inds[r], c, kept, f, 256)
                ok = True
                break
            except AssertionError:
                pass
        assert ok, f"{form} F {f} row {r}: the kept set is not between the model's at top_p (1 -+ {eps:.2e}) ({lo.numel()} .. {hi.numel()} columns)"


# ------------------------------------------------------------------------------------------------------------------ random keys
@pytest.mark.parametrize("form", ["plain", "delta"])
def test_random_keys(dev, form):
    from chipmunk_amd import ops
    f, (top_p, min_keys), rk = 12288, tp.EXACT_PARAMS[0], 0.05
    vals = tp.exact_rows(f)
    kept = exact_kept(f, top_p, min_keys)
    ops.manual_seed(1234)
    i1, c1 = launch(dev, vals, form, SPARSITY, top_p, min_keys, 1, rk)       # multiple_of 1: no padding, the count is kept + random
    i2, c2 = launch(dev, vals, form, SPARSITY, top_p, min_keys, 1, rk)
    ops.manual_seed(1234)
    i3, c3 = launch(dev, vals, form, SPARSITY, top_p, min_keys, 1, rk)
    differ = False
    for r in range(vals.shape[0]):
        s, c = kept[r].numel(), int(c1[r])
        listed = i1[r, :c].long()
        assert bool((listed[1:] > listed[:-1]).all()) and 0 <= int(listed[0]) and int(listed[-1]) < f       # ascending, in range
        assert set(kept[r].tolist()) <= set(listed.tolist())
        extras, n = c - s, f - s
        sd = math.sqrt(n * rk * (1 - rk))
        assert abs(extras - n * rk) <= 6 * sd, f"row {r}: {extras} random keys among {n} columns not kept (expected {n * rk:.0f} +- {sd:.1f})"
        differ |= not torch.equal(i1[r, :c], i2[r, : int(c2[r])])
        assert int(c3[r]) == c and torch.equal(i3[r, :c], i1[r, :c])                                        # the seed repeats the launch
    assert differ
    # with padding: counts are multiples, the padding repeats nothing
    i4, c4 = launch(dev, vals, form, SPARSITY, top_p, min_keys, 256, rk)
    for r in range(vals.shape[0]):
        listed = i4[r, : int(c4[r])].tolist()
        assert int(c4[r]) % 256 == 0 and len(set(listed)) == len(listed) and set(kept[r].tolist()) <= set(listed)
