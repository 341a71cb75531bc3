"""The sparse-MLP kernels of mlp.hip against exact fp64 under the segment-relative bound of tests/test_mlp_metric_cpu.py
(docs/TEST_SENSITIVITY.md, "Sparse MLP kernels"): per token row and per segment of 64 packed columns (GEMM1, cache) or 256 output
columns (GEMM2), ||got - exact|| / ||exact|| <= MLP_SEG_MARGIN * ORACLE_MLP_SEG_ERR, plus a term computed from the inputs where the
operator documents one more rounding.  Shipped forms only (mm1_variant = mm2_variant = 0).  Every live segment of every live group is
asserted; only empty groups and the columns at and past a count are left out (and those must keep their sentinel).

Inputs and case list are helpers.mlp1_cases / mlp2_cases, the ones the CPU file measures the references on: M = 333 (pitch 336, last
group 77 rows) and 1000 (eight groups, one empty), counts with partial 64-column tiles (208, 16, 40, 272) and one that ends inside an
8-column store (40); K = 320 / 256 bf16 and 384 e4m3; N2 = 384 / 512; both cache regimes.  NaN slack rows behind a, NaN cache padding,
a canary row behind the cache and sentinel rows behind the outputs as in tests/test_gpu_mlp_glu.py; the packed columns past each
count hold NaN for GEMM2.  The exact references run on the device in plain torch and are computed once per case."""
import functools

import pytest
import torch

from helpers import (MLP_BM, MLP_SEG_BOUND, MLP_SEG_W1, MLP_SEG_W2, assert_segs_close, gathered_cache, mlp1_cases, mlp2_base, mlp2_cases,
                     mlp2_problem, mlp_exact_args, mlp_group_cols, mlp_problem, mm1_exact, mm2_exact, refreshed_cache_term, seg_term)

pytestmark = pytest.mark.gpu

SENT = 7.0
CASES1, CASES2 = mlp1_cases(), mlp2_cases()
BASES = ("zero", "product", "unit")


def _names(kind):
    return [n for n in CASES1 if n.startswith(kind + " ") and (kind != "glu" or not n.startswith("glu fp8 "))]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    from chipmunk_amd import _native
    _native.set_option("mm1_variant", 0)         # shipped forms only
    _native.set_option("mm2_variant", 0)
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def with_slack(rows, fill):
    """[M, C] tensor -> its copy as the [:M] view of a [M + 128, C] buffer whose slack rows hold `fill` (returns buffer, view)."""
    buf = torch.full((rows.shape[0] + MLP_BM, rows.shape[1]), fill, dtype=torch.float32, device=rows.device).to(rows.dtype)
    buf[: rows.shape[0]] = rows
    return buf, buf[: rows.shape[0]]


def to_dev(p, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def problem1(name):
    """the case's problem on the device (a as the view of a buffer with NaN slack rows) and its exact deltas / activations"""
    dev = torch.device("cuda:0")
    p = to_dev(mlp_problem(**CASES1[name]), dev)
    p["a_buf"], p["a"] = with_slack(p["a"], float("nan"))
    p["ldc"] = (p["M"] + 7) // 8 * 8
    p["exact"], p["fresh"] = mm1_exact(p["a"], p["w"], p["bias"], p["cache0"], p["inds"], p["cnt"], **mlp_exact_args(p))
    p["cols"] = mlp_group_cols(p["cnt"], p["M"])
    return p


def fresh_state(p):
    """Mutable tensors of one launch: c (packed deltas out) and the cache, as views of buffers with canaries."""
    dev, M, f, ldc = p["cache0"].device, p["M"], p["F"], p["ldc"]
    cache_buf = torch.full((f + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)      # padding [M, ldc) = NaN
    cache_buf[f] = SENT                                                                           # the canary row
    cache_buf[:f, :M] = p["cache0"]
    c_buf, c = with_slack(torch.full((M, f), SENT, dtype=torch.bfloat16, device=dev), SENT)
    return dict(c=c, c_buf=c_buf, cache=cache_buf[:f, :M], cache_buf=cache_buf)


def check_untouched(p, s, what, cache_written):
    M, f = p["M"], p["F"]
    assert (s["c_buf"][M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    assert (s["cache_buf"][f] == SENT).all(), f"{what}: the row behind the cache's F * ldc elements was written"
    assert torch.isnan(p["a_buf"][M:].float()).all(), f"{what}: the input's slack rows changed"
    past = torch.arange(f, device=s["c"].device) >= p["cols"][:, None]
    assert (s["c"][past] == SENT).all(), f"{what}: packed columns at or past a count were written"
    if not cache_written:
        assert torch.equal(bits(s["cache"]), bits(p["cache0"])), f"{what}: the cache was written"


def assert_deltas(p, s, what, term=None):
    return assert_segs_close(s["c"], p["exact"], MLP_SEG_BOUND, f"{what}: packed deltas", extra=term, cols=p["cols"])


def assert_cache(p, s, what, accumulate=True, act_rounded=False):
    """the refreshed cache columns against the fresh fp64 activation.  accumulate: the column is bf16(cache + delta), which inherits
    the packed delta's error and rounds the stored sum once more (helpers.refreshed_cache_term; in the previous-step regime the
    method's claim that a refreshed column is one rounding from fresh); act_rounded: the route rounded the activation to bf16 first
    (ungated fp8).  Not accumulate: the cache is the activation itself, rounded once."""
    got = gathered_cache(s["cache"], p["inds"], p["cnt"])
    term = refreshed_cache_term(got, p["fresh"], p["exact"], MLP_SEG_BOUND, MLP_SEG_W1, p["cols"], act_rounded) if accumulate else None
    return assert_segs_close(got, p["fresh"], MLP_SEG_BOUND, f"{what}: refreshed cache columns", extra=term, cols=p["cols"])


# ------------------------------------------------------------------------------------------------ GEMM1
@pytest.mark.parametrize("name", _names("bf16"))
def test_ungated_gemm1_and_its_scatter(dev, name):
    p = problem1(name)
    ops = torch.ops.chipmunk
    s = fresh_state(p)
    ops.csp_mlp_mm1(p["a"], p["w"], s["c"], p["bias"], s["cache"], p["inds"], p["cnt"])
    check_untouched(p, s, "csp_mlp_mm1", cache_written=False)
    assert_deltas(p, s, f"csp_mlp_mm1 | {name}")
    s = fresh_state(p)
    ops.csp_mlp_mm1_scatter(p["a"], p["w"], s["c"], p["bias"], s["cache"], p["inds"], p["cnt"])
    check_untouched(p, s, "csp_mlp_mm1_scatter", cache_written=True)
    assert_deltas(p, s, f"csp_mlp_mm1_scatter | {name}")
    assert_cache(p, s, f"csp_mlp_mm1_scatter | {name}")


@pytest.mark.parametrize("name", _names("fp8"))
def test_ungated_fp8_gemm1(dev, name):
    """mlp.hip rounds the activation to bf16 and subtracts in bf16 ("gelu -> bf16, then a bf16 subtract", the reference's order): the
    term 2^-8 ||act_seg|| / ||delta_seg||.  With the previous step's activations in the cache that term is several times the bound
    (the deltas are a tenth of the activations); the route is asserted in both regimes, and the random-cache regime is the one
    where its assertion is sharp.  The scales are 448 / amax reciprocals: no powers of two."""
    p = problem1(name)
    ops = torch.ops.chipmunk
    term = seg_term(p["fresh"], p["exact"], MLP_SEG_W1, p["cols"])
    for update in (False, True):
        s = fresh_state(p)
        ops.csp_mlp_mm1_fp8(p["a"], p["w"], s["c"], p["bias"], s["cache"], p["inds"], p["cnt"], p["ra"], p["rb"], update)
        what = f"csp_mlp_mm1_fp8 update {'on' if update else 'off'}"
        check_untouched(p, s, what, cache_written=update)
        assert_deltas(p, s, f"{what} | {name}", term)
        if update:                       # the cache is the activation itself, rounded once
            assert_cache(p, s, f"{what} | {name}", accumulate=False)
    s = fresh_state(p)
    ops.csp_mlp_mm1_fp8_scatter(p["a"], p["w"], s["c"], p["bias"], s["cache"], p["inds"], p["cnt"], p["ra"], p["rb"])
    check_untouched(p, s, "csp_mlp_mm1_fp8_scatter", cache_written=True)
    assert_deltas(p, s, f"csp_mlp_mm1_fp8_scatter | {name}", term)
    assert_cache(p, s, f"csp_mlp_mm1_fp8_scatter | {name}", act_rounded=True)


@pytest.mark.parametrize("name", _names("glu"))
def test_gated_gemm1(dev, name):
    p = problem1(name)
    for update in (False, True):
        s = fresh_state(p)
        torch.ops.chipmunk.csp_mlp_mm1_glu(p["a"], p["w"], p["wu"], s["c"], p["bias"], p["bu"], s["cache"], p["inds"], p["cnt"], p["act"], update)
        what = f"csp_mlp_mm1_glu update {'on' if update else 'off'}"
        check_untouched(p, s, what, cache_written=update)
        assert_deltas(p, s, f"{what} | {name}")
        if update:
            assert_cache(p, s, f"{what} | {name}")


@pytest.mark.parametrize("name", _names("glu fp8"))
def test_gated_fp8_gemm1(dev, name):
    """one rounding, as the bf16 gated form (fma(act(gate), up, -cache)): no term.  The gate's and the up projection's weight scales
    differ by about 2 x."""
    p = problem1(name)
    assert 1.5 < float(p["rbu"] / p["rb"]) < 3.0
    for update in (False, True):
        s = fresh_state(p)
        torch.ops.chipmunk.csp_mlp_mm1_glu_fp8(p["a"], p["w"], p["wu"], s["c"], p["bias"], p["bu"], s["cache"], p["inds"], p["cnt"],
                                               p["ra"], p["rb"], p["rbu"], p["act"], update)
        what = f"csp_mlp_mm1_glu_fp8 update {'on' if update else 'off'}"
        check_untouched(p, s, what, cache_written=update)
        assert_deltas(p, s, f"{what} | {name}")
        if update:
            assert_cache(p, s, f"{what} | {name}")


def test_batch_of_two_ungated_gemm1(dev):
    """batch = slices is a bit test elsewhere; this puts the batched launch itself under the fp64 bound"""
    name = "bf16 gelu_tanh M333 K320, random cache"
    ps = [problem1(name), to_dev(mlp_problem(**dict(CASES1[name], seed=901, counts=[40, 512, 0])), dev)]
    p, q = ps
    M, F, ldc = p["M"], p["F"], p["ldc"]
    q["exact"], _ = mm1_exact(q["a"], p["w"], p["bias"], q["cache0"], q["inds"], q["cnt"])
    cache_buf = torch.full((2, F + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
    cache_buf[:, F] = SENT
    c_buf = torch.full((2 * M + MLP_BM, F), SENT, dtype=torch.bfloat16, device=dev)
    c, cache = c_buf[: 2 * M].view(2, M, F), cache_buf[:, :F, :M]
    for b in range(2):
        cache[b] = ps[b]["cache0"]
    a, inds, cnt = (torch.stack([x[k] for x in ps]) for k in ("a", "inds", "cnt"))
    torch.ops.chipmunk.csp_mlp_mm1(a, p["w"], c, p["bias"], cache, inds, cnt)
    assert (c_buf[2 * M:] == SENT).all() and (cache_buf[:, F] == SENT).all()
    cols = torch.stack([mlp_group_cols(x["cnt"], M) for x in ps])
    assert (c[torch.arange(F, device=dev) >= cols[..., None]] == SENT).all()
    assert_segs_close(c, torch.stack([p["exact"], q["exact"]]), MLP_SEG_BOUND, "csp_mlp_mm1, batch of two | packed deltas", cols=cols)


# ------------------------------------------------------------------------------------------------ GEMM2
@functools.lru_cache(maxsize=None)
def problem2(name):
    dev = torch.device("cuda:0")
    p = to_dev(mlp2_problem(**CASES2[name]), dev)
    p["packed_buf"], p["packed"] = with_slack(p["packed"], float("nan"))
    p["exact"] = {"mm2": mm2_exact(p["packed"], p["w2T"], p["inds"], p["cnt"]),
                  "w8": mm2_exact(p["packed"], p["w8"], p["inds"], p["cnt"], p["r8"])}
    g = torch.Generator().manual_seed(p["seed"] + 1)
    p["cache0"] = (torch.randn(p["F"], p["M"], generator=g) * 0.3).to(torch.bfloat16).to(dev)
    p["ldc"] = (p["M"] + 7) // 8 * 8
    return p


def launch2(op, p, out, cache):
    ops = torch.ops.chipmunk
    if op == "csp_mlp_mm2":
        ops.csp_mlp_mm2(p["packed"], p["w2T"], p["inds"], p["cnt"], out)
    elif op == "csp_mlp_mm2_w8":
        ops.csp_mlp_mm2_w8(p["packed"], p["w8"], p["r8"], p["inds"], p["cnt"], out)
    else:
        ops.csp_mlp_mm2_and_scatter_add(p["packed"].unsqueeze(0), cache.unsqueeze(0), p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0),
                                        p["packed"].unsqueeze(0), p["w2T"].unsqueeze(0), out.unsqueeze(0), 6, 0)


@pytest.mark.parametrize("op", ["csp_mlp_mm2", "csp_mlp_mm2_and_scatter_add", "csp_mlp_mm2_w8"])
@pytest.mark.parametrize("name", list(CASES2))
def test_gemm2_on_a_zero_a_product_sized_and_a_unit_base(dev, name, op):
    """bf16(bf16(sum) + base): on the zero base a plain output, one rounding, no term -- the sharp assertion (a 1 % error of the sum
    is 0.011 against the bound).  On a base of the product's size the accumulate term 2^-8 ||result_seg|| / ||exact_seg|| is about the
    bound; on the unit base it is several times the bound and hides a 1 % error: that base only shows that the base survives and
    the product is added once.  csp_mlp_mm2_w8's scale is an amax reciprocal, no power of two."""
    p = problem2(name)
    exact = p["exact"]["w8" if op.endswith("w8") else "mm2"]
    M, F = p["M"], p["F"]
    for kind in BASES:
        base = mlp2_base(p, kind, exact.cpu()).to(dev)
        out_buf, out = with_slack(base, SENT)
        cache_buf = torch.full((F + 1, p["ldc"]), float("nan"), dtype=torch.bfloat16, device=dev)
        cache_buf[F] = SENT
        cache_buf[:F, :M] = p["cache0"]
        cache = cache_buf[:F, :M]
        launch2(op, p, out, cache)
        what = f"{op}, {kind} base | {name}"
        assert (out_buf[M:] == SENT).all(), f"{what}: rows at or past M were written"
        assert torch.isnan(p["packed_buf"][M:].float()).all() and (cache_buf[F] == SENT).all()
        res = out.double()
        delta = torch.where(torch.isfinite(res), res - base.double(), res)
        term = None if kind == "zero" else seg_term(out, exact, MLP_SEG_W2)
        assert_segs_close(delta, exact, MLP_SEG_BOUND, what, extra=term, width=MLP_SEG_W2)
        if op != "csp_mlp_mm2_and_scatter_add":
            assert torch.equal(bits(cache), bits(p["cache0"]))
        elif kind == "zero":               # the scatter-add half: bf16(cache + packed) on the kept columns, against the fp64 sum
            cols = mlp_group_cols(p["cnt"], M)
            live = torch.arange(F, device=dev) < cols[:, None]
            want = gathered_cache(p["cache0"], p["inds"], p["cnt"]).double() + torch.where(live, p["packed"].double(), 0.0)
            got = gathered_cache(cache, p["inds"], p["cnt"])
            assert_segs_close(got, want, MLP_SEG_BOUND, f"{op} | {name}: cache after the scatter-add", cols=cols)


@pytest.mark.parametrize("op", ["csp_mlp_mm2", "csp_mlp_mm2_w8"])
def test_batch_of_two_gemm2(dev, op):
    name = "M333 N384"
    p = problem2(name)
    q = to_dev(mlp2_problem(**dict(CASES2[name], seed=902, counts=[40, 512, 0])), dev)
    w8 = op.endswith("w8")
    w, scale = (p["w8"], p["r8"]) if w8 else (p["w2T"], None)
    exact = torch.stack([p["exact"]["w8" if w8 else "mm2"], mm2_exact(q["packed"], w, q["inds"], q["cnt"], scale)])
    M, N2 = p["M"], p["N2"]
    buf = torch.full((2 * M + MLP_BM, N2), SENT, dtype=torch.bfloat16, device=dev)
    out = buf[: 2 * M].view(2, M, N2)
    out.zero_()
    packed, inds, cnt = (torch.stack([x[k] for x in (p, q)]) for k in ("packed", "inds", "cnt"))
    if w8:
        torch.ops.chipmunk.csp_mlp_mm2_w8(packed, w, scale, inds, cnt, out)
    else:
        torch.ops.chipmunk.csp_mlp_mm2(packed, w, inds, cnt, out)
    assert (buf[2 * M:] == SENT).all()
    assert_segs_close(out, exact, MLP_SEG_BOUND, f"{op}, batch of two, zero base", width=MLP_SEG_W2)


# ------------------------------------------------------------------------------------------------ both stages
@pytest.mark.parametrize("kept", [512, 152], ids=["all columns kept", "30 % kept"])
@pytest.mark.parametrize("gated", [False, True], ids=["run_e2e", "run_e2e_glu"])
def test_both_stages_previous_step_regime(dev, fresh_config, gated, kept):
    """out_cache - out_cache0 against fp64 (act(h(x)) - cache^T)[:, kept] . W2^T[kept].  The bound is the two stages', not tuned:

    GEMM1 leaves packed deltas d^ = d + e1 with ||e1_seg|| <= B ||d_seg|| in every 64-column segment (B = MLP_SEG_BOUND, what the tests
    above assert), so ||e1_i|| <= B ||d_i|| over the row.  Through GEMM2 that error reaches a 256-column segment S of the output as
    e1_i W_S with ||e1_i W_S|| <= ||e1_i|| sigma_S, sigma_S the largest singular value of W2^T[kept_g][:, S]: the GEMM1 bound times the
    norm entering GEMM2.  GEMM2 itself is within B of ITS exact product d^_i W_S, of norm at most ||x_S|| + B ||d_i|| sigma_S (x the
    exact output), plus the accumulate term 2^-8 ||result_S||.  Divided by ||x_S||, with kappa = ||d_i|| sigma_S / ||x_S||:
        error <= B + (1 + B) B kappa + 2^-8 ||result_S|| / ||x_S||.
    kappa is 2 - 3 for these weights (sigma_S ~ 0.05 (sqrt(n) + 16) against ||x_S|| ~ 0.05 * 16 ||d_i||).  The base has the
    product's own magnitude (as in the GEMM2 test: under a unit base the last term would swallow the rest).  30 % of 512 columns is
    152 here: GEMM2 masks the packed columns past a count in units of 8 (mlp.hip, "counts are multiples of 8"), see ops.csp_mlp_mm2."""
    from chipmunk_amd.ops.mlp import run_e2e, run_e2e_glu
    M, K, F, N2 = 333, 320, 512, 384
    p = to_dev(mlp_problem(M=M, K=K, F=F, seed=950 + gated, regime="previous step", act="silu" if gated else "gelu_tanh", gated=gated,
                           counts=[kept] * 3), dev)
    p["ldc"] = 336
    p["cols"] = mlp_group_cols(p["cnt"], M)
    p["a_buf"], p["a"] = with_slack(p["a"], float("nan"))
    g = torch.Generator().manual_seed(960)
    w2T = (torch.randn(F, N2, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    d, p["fresh"] = mm1_exact(p["a"], p["w"], p["bias"], p["cache0"], p["inds"], p["cnt"], **mlp_exact_args(p))
    p["exact"] = d
    exact = mm2_exact(d, w2T, p["inds"], p["cnt"])
    out0 = (torch.randn(M, N2, generator=g) * float(exact.pow(2).mean().sqrt())).to(torch.bfloat16).to(dev)
    out_buf, out = with_slack(out0, SENT)
    s = fresh_state(p)
    if gated:
        run_e2e_glu(p["a"], p["w"], p["wu"], p["bias"], p["bu"], p["act"], w2T, p["inds"], p["cnt"], s["cache"], out, 6)
    else:
        run_e2e(p["a"], p["w"], p["bias"], w2T, p["inds"], p["cnt"], s["cache"], out, 6)
    torch.cuda.synchronize()
    assert (out_buf[M:] == SENT).all() and (s["cache_buf"][F] == SENT).all() and torch.isnan(p["a_buf"][M:].float()).all()
    segs = (N2 + MLP_SEG_W2 - 1) // MLP_SEG_W2
    sigma = torch.zeros(M, segs, dtype=torch.float64)
    for gi in range(p["G"]):
        wg = w2T[p["inds"][gi, :kept].long()].double().cpu()
        for si in range(segs):
            sigma[gi * MLP_BM:(gi + 1) * MLP_BM, si] = torch.linalg.matrix_norm(wg[:, si * MLP_SEG_W2:(si + 1) * MLP_SEG_W2], ord=2)
    B = MLP_SEG_BOUND
    xnorm = torch.nn.functional.pad(exact, (0, (-N2) % MLP_SEG_W2)).unflatten(-1, (segs, MLP_SEG_W2)).norm(dim=-1)
    kappa = d.norm(dim=-1)[:, None] * sigma.to(dev) / xnorm
    print(f"kappa {float(kappa.min()):.2f} .. {float(kappa.max()):.2f}")
    extra = (1 + B) * B * kappa + seg_term(out, exact, MLP_SEG_W2)
    what = f"{'run_e2e_glu' if gated else 'run_e2e'}, previous step, {kept} of {F} kept"
    assert_segs_close(out.double() - out0.double(), exact, B, f"{what}: out_cache - out_cache0", extra=extra, width=MLP_SEG_W2)
    assert_cache(p, s, what)
