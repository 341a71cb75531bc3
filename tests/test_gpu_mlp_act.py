"""csp_mlp_mm1_act / csp_mlp_mm1_fp8_act (the ungated GEMM1 with SiLU, exact GELU or tanh-GELU and an optional bias) on the device.

Shapes of tests/mlp_act_model.act_cases: M = 333 (three groups, the last of 77 rows, cache pitch 336) and 1000 (eight groups, one
empty), F = 512, K = 320 / 256 bf16 and 384 e4m3, counts helpers.MLP_COUNTS (partial 64-column tiles, one count that ends inside an
8-column store).  NaN slack rows behind a, NaN cache padding, a canary row behind the cache, sentinel rows behind the outputs, NaN in
the packed columns at and past the counts.

1. tanh-GELU with a bias through the new operators: the bits of csp_mlp_mm1 / _scatter / csp_mlp_mm1_fp8 / _fp8_scatter;
2. a null bias: the bits of a zero bias vector;
3. every activation x bias x operand type x cache regime against fp64 under the bound proven in tests/test_mlp_act_host.py, every
   update mode, the refreshed cache columns included; exact and tanh GELU told apart by projection;
4. the scatter form = the plain form + csp_scatter_add;  5. B = 2 = two calls on the slices;  6. two launches, the same bits;
7. / 8. nothing outside the live outputs is written (asserted after every launch of 3.);
9. run_e2e(..., act="silu", fc1b=None) with mlp.fused_scatter on and off."""
import functools

import pytest
import torch

import mlp_act_model as am
from helpers import MLP_ACTS, MLP_BM, mlp_group_cols, mlp_problem, mm1_exact, mlp_exact_args

pytestmark = pytest.mark.gpu

SENT = am.SENT
CASES = am.act_cases()
MODES = {False: ("none", "scatter"), True: ("none", "store", "scatter")}


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    from chipmunk_amd import _native
    _native.set_option("mm1_variant", 0)         # shipped forms only
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


def prepared(p, dev):
    p = to_dev(p, dev)
    p["a_buf"], p["a"] = with_slack(p["a"], float("nan"))
    p["ldc"] = (p["M"] + 7) // 8 * 8
    p["exact"], p["fresh"] = mm1_exact(p["a"], p["w"], p["bias"], p["cache0"], p["inds"], p["cnt"], **mlp_exact_args(p))
    p["cols"] = mlp_group_cols(p["cnt"], p["M"])
    p["live"] = torch.arange(p["F"], device=dev) < p["cols"][:, None]
    return p


@functools.lru_cache(maxsize=None)
def problem(name):
    """the case's problem on the device (a as the view of a buffer with NaN slack rows) and its exact deltas / activations"""
    return prepared(mlp_problem(**CASES[name]), torch.device("cuda:0"))


def fresh_state(p):
    """Mutable tensors of one launch: c (packed deltas out, NaN everywhere) and the cache, as views of buffers with canaries."""
    dev, M, f, ldc = p["cache0"].device, p["M"], p["F"], p["ldc"]
    cache_buf = torch.full((f + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)      # padding [M, ldc) = NaN
    cache_buf[f] = SENT                                                                           # the canary row
    cache_buf[:f, :M] = p["cache0"]
    c_buf, c = with_slack(torch.full((M, f), float("nan"), dtype=torch.bfloat16, device=dev), SENT)
    return dict(c=c, c_buf=c_buf, cache=cache_buf[:f, :M], cache_buf=cache_buf)


def launch(p, s, mode, act=None, bias="own"):
    """the new operator of p's operand type; mode "none" | "scatter" | "store" (fp8: the cache takes the bf16 activation)"""
    ops = torch.ops.chipmunk
    act = p["act"] if act is None else act
    bias = p["bias"] if isinstance(bias, str) else bias
    if p["fp8"]:
        ops.csp_mlp_mm1_fp8_act(p["a"], p["w"], s["c"], bias, s["cache"], p["inds"], p["cnt"], p["ra"], p["rb"], act,
                                {"none": 0, "store": 1, "scatter": 2}[mode])
    else:
        ops.csp_mlp_mm1_act(p["a"], p["w"], s["c"], bias, s["cache"], p["inds"], p["cnt"], act, {"none": False, "scatter": True}[mode])
    return s


def check_untouched(p, s, what, cache_written):
    M, f = p["M"], p["F"]
    assert (s["c_buf"][M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    assert (s["cache_buf"][f] == SENT).all(), f"{what}: the row behind the cache's F * ldc elements was written"
    assert torch.isnan(s["cache_buf"][:f, M:].float()).all(), f"{what}: the cache's padding columns were written"
    assert torch.isnan(p["a_buf"][M:].float()).all(), f"{what}: the input's slack rows changed"
    assert torch.isnan(s["c"][~p["live"]].float()).all(), f"{what}: packed columns at or past a count were written"
    assert not torch.isnan(s["c"][p["live"]].float()).any(), f"{what}: a live packed column was not written"
    if not cache_written:
        assert torch.equal(bits(s["cache"]), bits(p["cache0"])), f"{what}: the cache was written"


def same_bits(p, s, t, what):
    assert torch.equal(bits(s["c"])[p["live"]], bits(t["c"])[p["live"]]), f"{what}: packed deltas differ"
    assert torch.equal(bits(s["cache"]), bits(t["cache"])), f"{what}: caches differ"


def names(**want):
    return [n for n, c in CASES.items() if all(c[k] == v for k, v in want.items())]


# ------------------------------------------------------------------------------------------------ 1.
@pytest.mark.parametrize("name", names(act="gelu_tanh", biases=True, regime="random"))
def test_tanh_gelu_with_a_bias_gives_the_bits_of_the_existing_operators(dev, name):
    p = problem(name)
    ops = torch.ops.chipmunk
    args = lambda s: (p["a"], p["w"], s["c"], p["bias"], s["cache"], p["inds"], p["cnt"])      # noqa: E731
    if p["fp8"]:
        old = {"none": lambda s: ops.csp_mlp_mm1_fp8(*args(s), p["ra"], p["rb"], False),
               "store": lambda s: ops.csp_mlp_mm1_fp8(*args(s), p["ra"], p["rb"], True),
               "scatter": lambda s: ops.csp_mlp_mm1_fp8_scatter(*args(s), p["ra"], p["rb"])}
    else:
        old = {"none": lambda s: ops.csp_mlp_mm1(*args(s)), "scatter": lambda s: ops.csp_mlp_mm1_scatter(*args(s))}
    for mode in MODES[p["fp8"]]:
        s, t = launch(p, fresh_state(p), mode), fresh_state(p)
        old[mode](t)
        same_bits(p, s, t, f"{name}, update {mode}")
        check_untouched(p, s, f"{name}, update {mode}", cache_written=mode != "none")


# ------------------------------------------------------------------------------------------------ 2.
@pytest.mark.parametrize("act", MLP_ACTS)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_a_null_bias_gives_the_bits_of_a_zero_bias(dev, fp8, act):
    p = problem(names(act=act, fp8=fp8, biases=False, regime="random", M=333)[0])
    assert p["bias"] is None
    zero = torch.zeros(p["F"], dtype=torch.bfloat16, device=dev)
    for mode in MODES[fp8]:
        s, t = launch(p, fresh_state(p), mode, bias=None), launch(p, fresh_state(p), mode, bias=zero)
        same_bits(p, s, t, f"{act}, update {mode}")
    # ... and not those of a bias that is there
    u = launch(p, fresh_state(p), "none", bias=am.other_bias(p).to(dev))
    assert not torch.equal(bits(s["c"])[p["live"]], bits(u["c"])[p["live"]])


# ------------------------------------------------------------------------------------------------ 3., 7., 8.
@pytest.mark.parametrize("name", list(CASES))
def test_against_fp64_under_the_proven_bound(dev, name):
    """packed deltas and refreshed cache columns of every update mode; fp8: the documented bf16 rounding of the activation is the
    derived term of mlp_act_model.delta_term / helpers.refreshed_cache_term(act_rounded=True)"""
    p = problem(name)
    for mode in MODES[p["fp8"]]:
        s = launch(p, fresh_state(p), mode)
        what = f"update {mode} | {name}"
        check_untouched(p, s, what, cache_written=mode != "none")
        am.assert_act_deltas(p, s["c"], p["exact"], p["fresh"], what)
        if mode != "none":
            am.assert_act_cache(p, s["cache"], p["exact"], p["fresh"], what, accumulate=mode == "scatter")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_exact_gelu_and_tanh_gelu_are_told_apart(dev, fp8):
    """The two differ by 5e-4 at most, inside the bound above in the shipped regimes (and, on the fp8 route, inside its derived term in
    every regime): projected on the difference of the two fp64 references, each kernel's output lies at its own end.  Zero cache: the
    result is the activation itself; every column kept: 170 000 elements."""
    base = CASES[names(act="gelu", fp8=fp8, biases=True, regime="random", M=333)[0]]
    p = mlp_problem(**dict(base, counts=[base["F"]] * 3))
    p["cache0"] = torch.zeros_like(p["cache0"])
    p = prepared(p, dev)
    want = {act: mm1_exact(p["a"], p["w"], p["bias"], p["cache0"], p["inds"], p["cnt"], **dict(mlp_exact_args(p), act=act))[0] for act in ("gelu_tanh", "gelu")}
    got = {act: launch(p, fresh_state(p), "none", act=act)["c"] for act in ("gelu_tanh", "gelu")}
    assert not torch.equal(bits(got["gelu"]), bits(got["gelu_tanh"])), "exact GELU and tanh-GELU gave the same bits"
    at_tanh, at_erf = (am.gelu_projection(got[act], want["gelu_tanh"], want["gelu"]) for act in ("gelu_tanh", "gelu"))
    print(f"projection on (exact - tanh), {'fp8' if fp8 else 'bf16'}: tanh-GELU kernel {at_tanh:.3f}, exact-GELU kernel {at_erf:.3f}")
    assert abs(at_tanh) < 0.25 and abs(at_erf - 1.0) < 0.25


# ------------------------------------------------------------------------------------------------ 4.
@pytest.mark.parametrize("name", names(biases=False, regime="previous step", M=333) + names(act="silu", biases=True, regime="random", M=1000))
def test_the_scatter_form_equals_the_plain_form_and_csp_scatter_add(dev, name):
    from chipmunk_amd.ops import scatter_add
    p = problem(name)
    s, t = launch(p, fresh_state(p), "scatter"), launch(p, fresh_state(p), "none")
    scatter_add(t["c"], t["cache"], p["inds"], p["cnt"], 6)
    same_bits(p, s, t, name)
    assert not torch.equal(bits(s["cache"]), bits(p["cache0"]))


# ------------------------------------------------------------------------------------------------ 5.
@pytest.mark.parametrize("mode", ["none", "scatter"])
@pytest.mark.parametrize("name", names(act="silu", biases=False, regime="random", M=333) + names(act="gelu", biases=True, regime="random", M=333))
def test_a_batch_of_two_equals_two_calls_on_the_slices(dev, name, mode):
    p = problem(name)
    q = prepared(dict(mlp_problem(**dict(CASES[name], seed=901, counts=[40, 512, 0])), w=p["w"].cpu(), bias=None if p["bias"] is None else p["bias"].cpu()), dev)
    if p["fp8"]:        # one weight, one pair of scales: the second sequence is quantised with the first one's input scale
        q["ra"], q["rb"] = p["ra"], p["rb"]
    M, F, ldc = p["M"], p["F"], p["ldc"]
    cache_buf = torch.full((2, F + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
    cache_buf[:, F] = SENT
    c_buf = torch.full((2 * M + MLP_BM, F), SENT, dtype=torch.bfloat16, device=dev)
    c_buf[: 2 * M] = float("nan")
    c, cache = c_buf[: 2 * M].view(2, M, F), cache_buf[:, :F, :M]
    ps = (p, q)
    for b in range(2):
        cache[b] = ps[b]["cache0"]
    a, inds, cnt = (torch.stack([x[k] for x in ps]) for k in ("a", "inds", "cnt"))
    launch(dict(p, a=a, inds=inds, cnt=cnt), dict(c=c, cache=cache), mode)
    assert (c_buf[2 * M:] == SENT).all() and (cache_buf[:, F] == SENT).all() and torch.isnan(cache_buf[:, :F, M:].float()).all()
    for b in range(2):
        s = launch(ps[b], fresh_state(ps[b]), mode)
        live = ps[b]["live"]
        assert torch.equal(bits(c[b])[live], bits(s["c"])[live]) and torch.isnan(c[b][~live].float()).all(), f"sequence {b}: packed deltas"
        assert torch.equal(bits(cache[b]), bits(s["cache"])), f"sequence {b}: cache"


# ------------------------------------------------------------------------------------------------ 6.
@pytest.mark.parametrize("name", names(act="gelu", biases=False, regime="previous step", M=1000) + names(act="silu", biases=True, regime="random", M=333))
def test_two_launches_from_the_same_state_give_the_same_bits(dev, name):
    p = problem(name)
    for mode in MODES[p["fp8"]]:
        same_bits(p, launch(p, fresh_state(p), mode), launch(p, fresh_state(p), mode), f"{name}, update {mode}")


# ------------------------------------------------------------------------------------------------ 9.
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_run_e2e_without_a_bias_is_the_same_with_fused_scatter_on_and_off(dev, fresh_config, fp8):
    from chipmunk_amd.ops.mlp import run_e2e
    p = problem(names(act="silu", fp8=fp8, biases=False, regime="previous step", M=333)[0])
    M, F, N2 = p["M"], p["F"], 384
    g = torch.Generator().manual_seed(960)
    w2T = (torch.randn(F, N2, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    out0 = (torch.randn(M, N2, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    assert all(n % 8 == 0 for n in p["counts"])      # (GEMM2 takes counts that are multiples of 8)
    res = {}
    for fused in (True, False):
        fresh_config["mlp"]["fused_scatter"] = fused
        s = fresh_state(p)
        out_buf, out = with_slack(out0, SENT)
        run_e2e(p["a"], p["w"], None, w2T, p["inds"], p["cnt"], s["cache"], out, 6, p.get("ra"), p.get("rb"), act="silu")
        torch.cuda.synchronize()
        assert (out_buf[M:] == SENT).all() and (s["cache_buf"][F] == SENT).all()
        res[fused] = (out.clone(), s["cache"].clone())
    assert torch.equal(bits(res[True][0]), bits(res[False][0])) and torch.equal(bits(res[True][1]), bits(res[False][1]))
    assert not torch.equal(bits(res[True][0]), bits(out0)) and not torch.equal(bits(res[True][1]), bits(p["cache0"]))
    # ... and it is SiLU without a bias that ran: the refreshed cache columns against fp64
    d, f = mm1_exact(p["a"], p["w"], None, p["cache0"], p["inds"], p["cnt"], **mlp_exact_args(p))
    am.assert_act_cache(p, res[True][1], d, f, f"run_e2e silu without a bias, {'fp8' if fp8 else 'bf16'}")
