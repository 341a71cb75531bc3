"""Attention kernels against exact fp64 attention (helpers.attn_exact, plain torch on the device) under the row-relative
bound ROW_ERR_MARGIN * ORACLE_ROW_ERR, at the sizes and edges the oracle-based files do not reach:

* a path matrix at 4 160 - 8 448 keys (where an absolute tolerance of 2e-2 no longer sees a dropped tile): every dense and
  gathered kernel selection, ragged query rows, ragged counts (0, 7, a full list, tails that are no multiple of 16 / 32 /
  64), index rows that are not 16-byte aligned, plain / in-place / out-of-place / o_scale = -1 forms;
* indicator V through every path: o[i, d] is the softmax mass of key class d, so a tile that is skipped, read twice or
  taken from another group is one column wrong by its whole value, and every row sums to 1;
* inputs that sit ON the data-dependent loop choices: the fixed reference point of attn64.hip (2 |q_i| max|k| c <= 64), the
  unit-weight column sums (<= 80), the folded scale of attn96.hip (|q_i| max|k| c <= 55), the lagging reference point of
  attn.hip (MAX_LAG = 4), with queries along / against the keys so that the scores sit at the ends of the proven range.

No oracle call: the floor ORACLE_ROW_ERR is a constant that tests/test_attn_metric_cpu.py pins.  docs/TEST_SENSITIVITY.md
has the measured error of every path."""
import contextlib
import math

import pytest
import torch

from helpers import (ORACLE_ROWSUM_ERR, ROW_ERR_MARGIN, assert_close_bf16, assert_delta_rows_close,
                     assert_rows_close, attn_exact, attn_exact_csp96, attn_exact_dense64, colsum_exact, gathered_matrix_inputs, indicator_v, randn_bf16,
                     straddle_inputs, STRADDLE_PATTERNS)

pytestmark = pytest.mark.gpu

C = math.log2(math.e) / math.sqrt(128)        # the kernels' SCALE_LOG2E: scores in exp2 units are q.k * C


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def options(**kw):
    from chipmunk_amd import _native
    try:
        for name, value in kw.items():
            _native.set_option(name, value)
        yield
    finally:
        for name in kw:
            _native.set_option(name, 0)


def assert_indicator_rows(o, exact, what, kind):
    """rows close as everywhere, the message naming the key class whose mass is off; every row of a non-empty group sums to 1
    within the margin over what the oracle's roundings do to that sum (helpers.ORACLE_ROWSUM_ERR)"""
    pair = exact
    if isinstance(exact, tuple):
        exact = exact[0]
    try:
        assert_rows_close(o, pair, what=what)
    except AssertionError as e:
        d = torch.nan_to_num((o.double() - exact).abs(), nan=float("inf"))
        b, h, r, c = [int(x) for x in (d == d.max()).nonzero()[0]]
        unit = {"key": "keys j = {c} mod 128", "tile": "32-key tiles t = {c} mod 128",
                "position": "32-key tiles t = {c} mod 128 of the index list"}[kind].format(c=c)
        raise AssertionError(f"{e}; worst column: head {h} row {r} class {c} ({unit}): mass {float(o[b, h, r, c]):.5f}, "
                             f"exact {float(exact[b, h, r, c]):.5f}") from None
    live = exact.sum(-1) > 0.5
    dev_ = (o.double().sum(-1) - 1).abs()[live].max().item()
    print(f"row sum {what}: worst |sum - 1| {dev_:.6f}")
    assert dev_ <= ROW_ERR_MARGIN * ORACLE_ROWSUM_ERR, f"{what}: a row's class masses sum to 1 +- {dev_:.5f}"


# ------------------------------------------------------------------------------------------------ path matrix, dense
DENSE_PATHS = {"general dense kernel": dict(attn_dense64=2), "dense64": dict(attn_dense64=1)}


@pytest.fixture(scope="module")
def dense_case(dev):
    """3 heads, 4 420 query rows (ragged last group and last 256-row workgroup), 4 160 keys (65 tiles of 64, 130 of 32)"""
    H, nq, nk = 3, 4420, 4160
    q, k, v = [randn_bf16(1, H, n, 128, seed=s).to(dev) for n, s in ((nq, 201), (nk, 202), (nk, 203))]
    case = {"q": q, "k": k, "v": v, "exact": attn_exact(q, k, v)}
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(128)
    case["l"] = 1.0 / torch.exp(s).sum(-1, keepdim=True)
    case["cs"] = colsum_exact(q, k, case["l"])            # softmax column sums per 192-row group, fp64
    for kind in ("key", "tile"):
        vi = indicator_v(nk, kind, dev).expand(1, H, nk, 128).contiguous()
        case[kind] = (vi, attn_exact(q, k, vi))
    return case


@pytest.mark.parametrize("path", list(DENSE_PATHS))
def test_dense_paths(dev, dense_case, path):
    c = dense_case
    with options(**DENSE_PATHS[path]):
        o, l = torch.ops.chipmunk.dense_attn(c["q"], c["k"], c["v"])
        ind = {kind: torch.ops.chipmunk.dense_attn(c["q"], c["k"], c[kind][0])[0] for kind in ("key", "tile")}
    # (dense64 takes its fixed reference point here: the bound carries that path's per-row term, helpers.attn_exact_dense64)
    d64 = path == "dense64"
    assert_rows_close(o, attn_exact_dense64(c["q"], c["k"], c["v"]) if d64 else c["exact"], what=f"{path}, 4160 keys")
    torch.testing.assert_close(l.double(), c["l"], rtol=1e-3, atol=0)
    for kind, oi in ind.items():
        x = attn_exact_dense64(c["q"], c["k"], c[kind][0]) if d64 else c[kind][1]
        assert_indicator_rows(oi, x, f"{path}, indicator V by {kind}", kind)


@pytest.mark.parametrize("route", ["fused", "fused_weighted", "fused_runmax", "two_pass"])
def test_column_sum_paths(dev, dense_case, route):
    """dense_colsum_attn with p = the exact normaliser: o, l, and the column sums against fp64 softmax column sums under the
    tolerance test_gpu_attn.py states for them (rtol 3e-2 + atol 2e-3)"""
    c = dense_case
    nk = c["k"].shape[2]
    opts = dict(attn_dense64=1, attn_colsum64=1, attn_fused_colsum={"two_pass": 2, "fused_weighted": 3}.get(route, 0),
                attn_nomax=2 if route == "fused_runmax" else 0)
    with options(**opts):
        o, cs, l = torch.ops.chipmunk.dense_colsum_attn(c["q"], c["k"], c["v"], c["l"].float())
        ind = {kind: torch.ops.chipmunk.dense_colsum_attn(c["q"], c["k"], c[kind][0], c["l"].float())[0] for kind in ("key", "tile")}
    fixed = route != "fused_runmax"          # a reference point that is not the row maximum: the fixed one, or -log2 p_i (unit weights)
    assert_rows_close(o, attn_exact_dense64(c["q"], c["k"], c["v"]) if fixed else c["exact"], what=f"column-sum pass o, {route}, 4160 keys")
    torch.testing.assert_close(l.double(), c["l"], rtol=1e-3, atol=0)
    assert_close_bf16(cs[..., :nk], c["cs"], atol=2e-3, rtol=3e-2, what=f"column sums, {route}, vs fp64")
    for kind, oi in ind.items():
        assert_indicator_rows(oi, attn_exact_dense64(c["q"], c["k"], c[kind][0]) if fixed else c[kind][1],
                              f"column-sum pass o, {route}, indicator V by {kind}", kind)


# ------------------------------------------------------------------------------------------------ path matrix, gathered
GATHERED_PATHS = {          # name -> (options, index rows of an odd width: not 16-byte aligned; not for csp96, which hands rows whose
                            # width is no multiple of 4 to the general kernel: attn.hip `fits96`)
    "general gathered kernel": (dict(attn_csp96=2, attn_row_split=2), True),
    "key-split tail": (dict(attn_csp96=2, attn_split_gather=1, attn_row_split=2), False),
    "row-split tail": (dict(attn_csp96=2, attn_row_split=1), False),
    "csp64": (dict(attn_csp64=1), True),
    "csp96": (dict(attn_csp96=1), False),
    "csp96 running maximum": (dict(attn_csp96=1, attn_nomax=2), False),
}


@pytest.fixture(scope="module")
def gathered_case(dev):
    """helpers.gathered_matrix_inputs on the device, with the exact outputs for the random and the three indicator V"""
    m = gathered_matrix_inputs()
    q, k, v, inds, counts, shared, v_pos = [m[n].to(dev) for n in ("q", "k", "v", "inds", "counts", "shared", "v_pos")]
    H, nq, nk = q.shape[1], q.shape[2], k.shape[2]
    odd = torch.zeros(1, H, inds.shape[2], nk + 1, dtype=torch.int32, device=dev)
    odd[..., :nk] = inds
    case = {"q": q, "k": k, "v": v, "inds": inds, "odd": odd, "shared": shared, "counts": counts,
            "exact": attn_exact(q, k, v, inds, counts), "position": (v_pos, attn_exact(q, k, v_pos, shared, counts))}
    for kind in ("key", "tile"):
        vi = indicator_v(nk, kind, dev).expand(1, H, nk, 128).contiguous()
        case[kind] = (vi, attn_exact(q, k, vi, inds, counts))
    rms = float(case["exact"].pow(2).mean().sqrt())
    case["base"] = randn_bf16(1, H, nq, 128, seed=215, scale=rms).to(dev)     # a base of the delta's magnitude
    return case


@pytest.mark.parametrize("path", list(GATHERED_PATHS))
def test_gathered_paths(dev, gathered_case, path):
    c = gathered_case
    opts, odd = GATHERED_PATHS[path]
    q, k, v, counts, base = c["q"], c["k"], c["v"], c["counts"], c["base"]
    inds = c["odd"] if odd else c["inds"]
    with options(**opts):
        o = torch.ops.chipmunk.csp_128_attn(q, k, v, inds, counts)
        ind = {kind: torch.ops.chipmunk.csp_128_attn(q, k, c[kind][0], c["shared"] if kind == "position" else inds, counts)
               for kind in ("key", "tile", "position")}
        out = torch.ops.chipmunk.csp_attn_out(q, k, v, base, inds, counts, -1)
        acc = base.clone()
        torch.ops.chipmunk.csp_attn(q, k, v, acc, inds, counts, 1)
        torch.cuda.synchronize()
    exact = {"random": c["exact"], **{kind: c[kind][1] for kind in ind}}
    if path == "csp96":
        # attn96.hip folds c into the bf16 Q fragments here (|q_i| max|k| c is about 20 of the 55 it allows) and takes the
        # exponentials without a reference point: held against attention over bf16(q c) with that path's per-row term
        # (helpers.attn_exact_csp96),
        # the error against plain exact attention recorded
        for name, (vv, ii) in {"random": (v, inds), **{kind: (c[kind][0], c["shared"] if kind == "position" else inds) for kind in ind}}.items():
            got = o if name == "random" else ind[name]
            assert_rows_close(got, exact[name], bound=float("inf"), what=f"{path}, {name} V (vs plain exact attention, recorded)")
            exact[name] = attn_exact_csp96(q, k, vv, ii, counts)
    assert_rows_close(o, exact["random"], what=f"{path}, ragged counts of 8448 keys")
    assert not o[0, 0, 192:384].any(), "a group without keys gives zeros"
    for kind, oi in ind.items():
        assert_indicator_rows(oi, exact[kind], f"{path}, indicator V by {kind}", kind)
    assert_delta_rows_close(out, base, exact["random"], -1, what=f"{path}, csp_attn_out, o_scale -1, small base")
    assert_delta_rows_close(acc, base, exact["random"], 1, what=f"{path}, csp_attn in place, small base")
    assert torch.equal(out[0, 0, 192:384], base[0, 0, 192:384]) and torch.equal(acc[0, 0, 192:384], base[0, 0, 192:384])


def test_ragged_index_rows_path(dev, gathered_case):
    """the compacted index rows (compact_indices -> csp_attn_out_ragged), as the shipped sparse step passes them"""
    import chipmunk_amd.ops as ops
    c = gathered_case
    flat, offsets = ops.compact_indices(c["inds"], c["counts"])
    for o_scale in (1, -1):
        out = ops.csp_attn_out_ragged(c["q"], c["k"], c["v"], c["base"], flat, offsets, c["counts"], o_scale)
        assert_delta_rows_close(out, c["base"], c["exact"], o_scale, what=f"ragged index rows, o_scale {o_scale}, small base")
    zero = torch.zeros_like(c["base"])
    for kind in ("key", "tile"):
        oi = ops.csp_attn_out_ragged(c["q"], c["k"], c[kind][0], zero, flat, offsets, c["counts"], 1)
        assert_indicator_rows(oi, c[kind][1], f"ragged index rows, indicator V by {kind}", kind)


# ------------------------------------------------------------------------------------------------ threshold straddles
PATTERNS = STRADDLE_PATTERNS


def _straddle_inputs(dev, *args, **kw):
    q, k, v, bound = straddle_inputs(*args, **kw)
    return q.to(dev), k.to(dev), v.to(dev), bound.to(dev)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("align", ["random", "along", "against"])
def test_dense64_fixed_reference_point_threshold(dev, align, pattern):
    """attn64.hip takes the fixed reference point when 2 |q_i| max|k| c <= 64 for every query of a 64-row wave"""
    q, k, v, _ = _straddle_inputs(dev, align, pattern, 64.0, 2.0, 128, 1100, 4160, seed=301)
    lx = 1.0 / torch.exp((q.double() @ k.double().transpose(-1, -2)) / math.sqrt(128)).sum(-1, keepdim=True)
    with options(attn_dense64=1):
        o, l = torch.ops.chipmunk.dense_attn(q, k, v)
    what = f"dense64 at its threshold, {align} queries, {pattern}"
    assert_rows_close(o, attn_exact(q, k, v), bound=float("inf"), what=what + " (vs plain exact attention, recorded)")
    assert_rows_close(o, attn_exact_dense64(q, k, v), what=what)
    torch.testing.assert_close(l.double(), lx, rtol=2e-3, atol=0)      # (the files' tolerance for l where the reference point is data-dependent)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("align", ["random", "along", "against"])
def test_fused_column_sum_fixed_reference_point_threshold(dev, align, pattern):
    """the same choice inside the fused column-sum body (attn64.hip MODE 3), with p = the exact normaliser: o, l and the
    column sums against fp64 softmax column sums (rtol 3e-2 + atol 2e-3, as test_gpu_attn.py states for them)"""
    q, k, v, _ = _straddle_inputs(dev, align, pattern, 64.0, 2.0, 128, 1100, 768, seed=306)
    nq, nk = q.shape[2], k.shape[2]
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(128)
    lx = 1.0 / torch.exp(s).sum(-1, keepdim=True)
    cs_x = colsum_exact(q, k, lx)
    with options(attn_dense64=1, attn_colsum64=1):
        o, cs, l = torch.ops.chipmunk.dense_colsum_attn(q, k, v, lx.float())
    assert_rows_close(o, attn_exact_dense64(q, k, v), what=f"column-sum pass o at the fixed-reference threshold, {align} queries, {pattern}")
    torch.testing.assert_close(l.double(), lx, rtol=2e-3, atol=0)
    torch.testing.assert_close(cs[..., :nk].double(), cs_x, rtol=3e-2, atol=2e-3)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_column_sum_unit_weight_threshold(dev, pattern):
    """the fused column sums take unit weights while |q_i| max|k| c + |log2 p_i| <= 80 for every query of the wave: with
    |q_i| max|k| c at 28, p_i = 2^(f_i 80 - 28) puts that sum at f_i x 80 (p is an input; the sums scale with it)"""
    q, k, v, _ = _straddle_inputs(dev, "random", "all rows at 0.9", 64.0, 2.0, 128, 960, 768, seed=302)
    nq, nk = q.shape[2], k.shape[2]
    kmax = k.double().norm(dim=-1).max(-1).values[..., None]
    m = q.double().norm(dim=-1) * kmax * C                             # 28.8
    f_lo, f_hi = PATTERNS[pattern]
    f = torch.full((nq,), f_lo, dtype=torch.float64, device=dev)
    if f_hi is not None:
        f[5::128] = f_hi
    p = torch.exp2(f * 80.0 - m)[..., None].float()                    # [1, H, nq, 1]
    assert (((m + p[..., 0].double().log2().abs()) / 80.0 - f).abs() < 1e-3).all()
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(128)
    cs_x = colsum_exact(q, k, p)
    with options(attn_dense64=1, attn_colsum64=1):
        o, cs, l = torch.ops.chipmunk.dense_colsum_attn(q, k, v, p)
    assert_rows_close(o, attn_exact_dense64(q, k, v), what=f"column-sum pass o at the unit-weight threshold, {pattern}")
    torch.testing.assert_close(l.double(), 1.0 / torch.exp(s).sum(-1, keepdim=True), rtol=1e-3, atol=0)
    torch.testing.assert_close(cs[..., :nk].double(), cs_x, rtol=3e-2, atol=2e-3)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("align", ["random", "along", "against", "along a key outside every list"])
def test_csp96_folded_scale_threshold(dev, align, pattern):
    """attn96.hip drops the reference point and folds c into the bf16 Q fragments when |q_i| max|k| c <= 55 for every query of
    a 96-row wave (max|k| over ALL keys of the head, listed or not).  Rounding q c to bf16 is a documented design rounding
    (attn96.hip, load_q: `pack_bf16x2(lo * SCALE_LOG2E, hi * SCALE_LOG2E)`) whose exact effect on these inputs is attention
    over bf16(q c) with the rest of the scale in fp64: waves that fold are held to the ordinary bound against THAT, the
    others against plain exact attention; the error of the whole output against plain exact attention is recorded."""
    planted = align == "along a key outside every list"
    nq, nk = 1100, 4160
    q, k, v, bound = _straddle_inputs(dev, "along" if planted else align, pattern, 55.0, 1.0, 192, nq, nk, seed=303, planted=planted)
    G = math.ceil(nq / 192)
    gen = torch.Generator().manual_seed(304)
    inds = torch.stack([1 + torch.randperm(nk - 1, generator=gen) for _ in range(2 * G)]).view(1, 2, G, nk - 1)
    inds = torch.nn.functional.pad(inds, (0, 1)).to(torch.int32)       # key 0 is in no list; width 4160
    counts = torch.full((1, 2, G), 1100, dtype=torch.int32)
    counts[0, 0, 2], counts[0, 1, 3] = 37, 3000
    with options(attn_csp96=1):
        o = torch.ops.chipmunk.csp_128_attn(q, k, v, inds.to(dev), counts.to(dev))
    what = f"csp96 at its threshold, {align} queries, {pattern}"
    assert_rows_close(o, attn_exact(q, k, v, inds, counts), bound=float("inf"), what=what + " (vs plain exact attention, recorded)")
    assert_rows_close(o, attn_exact_csp96(q, k, v, inds, counts), what=what)


@pytest.mark.parametrize("f", [0.9, 1.0, 1.1])
def test_general_kernel_lagging_reference_point(dev, f):
    """attn.hip moves the reference point of the exponentials only when a tile's maximum outgrows it by MAX_LAG = 4 (exp2
    units), per wave.  Three keys (tiles 20, 60, 100) each lift the row maximum by f x 4 over what came before, the noise of
    the other keys spreading the rows of a wave to both sides of the lag.  Dense, and gathered without / by shape / with
    the row-split tail (whose waves hold 16 rows instead of 48, so the choice falls differently; at these 44 items "by shape"
    is the unsplit launch, it is run to pin that)."""
    H, n = 2, 4160
    g = torch.Generator().manual_seed(305)
    q, k, v = [torch.randn(1, H, n, 128, generator=g) for _ in range(3)]
    u = torch.randn(128, generator=g)
    u = u / u.norm()
    q = 0.05 * q + math.sqrt(128) * u
    k = 0.3 * k
    noise_top = 2.5 * 0.3 * math.sqrt(128) * C                         # about the largest of a tile's noise scores, exp2 units
    for step, tile in enumerate((20, 60, 100)):
        k[0, :, 32 * tile + 7] = (noise_top + (step + 1) * f * 4.0) / (math.sqrt(128) * C) * u
    q, k, v = [t.to(torch.bfloat16).to(dev) for t in (q, k, v)]
    exact = attn_exact(q, k, v)
    with options(attn_dense64=2):
        o, _ = torch.ops.chipmunk.dense_attn(q, k, v)
    assert_rows_close(o, exact, what=f"general dense kernel, maxima rising by {f} x MAX_LAG")
    G = math.ceil(n / 192)
    inds = torch.arange(n, dtype=torch.int32, device=dev).expand(1, H, G, n).contiguous()
    counts = torch.full((1, H, G), n, dtype=torch.int32, device=dev)
    for split in (2, 0, 1):
        with options(attn_csp96=2, attn_row_split=split):
            o = torch.ops.chipmunk.csp_128_attn(q, k, v, inds, counts)
        assert_rows_close(o, exact, what=f"general gathered kernel, attn_row_split={split}, maxima rising by {f} x MAX_LAG")
