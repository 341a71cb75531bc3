"""csp_mlp_mm1_fp8_act_rs (the fp8 GEMM1 with one scale per token row and one per fc1 column) on the device.

Problems of tests/mlp_rowscale_model.rs_cases: K = 128, M = 128 (one group), 200 (a ragged last group; the 16-byte row-scale reads) and
203 (M % 4 != 0, cache pitch 208: the clamped single reads), F = 64 / 256 / 128, counts that end inside a 64-column tile; every
activation, with and without a bias.  The [M] scale vector is the head of a buffer whose slack is NaN, so a row at or past M that leaked
into a stored value would show; NaN slack rows behind a, NaN cache padding, sentinels behind the outputs.

1. constant vectors: the bits of csp_mlp_mm1_fp8_act with 0-dim scales, every update mode, unbatched and batched;
2. varying scales against fp64 under MLP_SEG_BOUND, on the inputs whose mutants tests/test_mlp_rowscale_host.py proved visible;
3. the scatter form = the plain form + csp_scatter_add;  4. B = 2 = two calls on the slices;  5. nothing outside the live outputs is
written (asserted after every launch of 1. and 2.);  6. a scale vector at an address that is no multiple of 16;
7. wrong dtype / shape / device of the scales raises before anything runs;  8. ops.mlp.run_e2e dispatches on the scales' rank."""
import functools

import pytest
import torch

import mlp_act_model as am
import mlp_rowscale_model as rm
from helpers import MLP_BM, MLP_SEG_BOUND, mlp_group_cols

pytestmark = pytest.mark.gpu

SENT = am.SENT
CASES = rm.rs_cases()
MODES = {"none": 0, "store": 1, "scatter": 2}


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
    buf = torch.full((rows.shape[0] + MLP_BM,) + tuple(rows.shape[1:]), fill, dtype=torch.float32, device=rows.device).to(rows.dtype)
    buf[: rows.shape[0]] = rows
    return buf, buf[: rows.shape[0]]


@functools.lru_cache(maxsize=None)
def problem(name):
    """the case's problem on the device, its exact deltas / activations (fp64, computed once), a and sa as heads of NaN-slack buffers"""
    dev = torch.device("cuda:0")
    p = {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in rm.rs_problem(**CASES[name]).items()}
    p["a_buf"], p["a"] = with_slack(p["a"], float("nan"))
    p["sa_buf"], p["sa"] = with_slack(p["sa"], float("nan"))
    p["ldc"] = (p["M"] + 7) // 8 * 8
    p["exact"], p["fresh"] = rm.rs_exact(p)
    p["cols"] = mlp_group_cols(p["cnt"], p["M"])
    p["live"] = torch.arange(p["F"], device=dev) < p["cols"][:, None]
    p["fp8"] = True
    return p


def fresh_state(p):
    dev, M, f, ldc = p["cache0"].device, p["M"], p["F"], p["ldc"]
    cache_buf = torch.full((f + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)      # padding [M, ldc) = NaN
    cache_buf[f] = SENT                                                                           # the canary row
    cache_buf[:f, :M] = p["cache0"]
    c_buf, c = with_slack(torch.full((M, f), float("nan"), dtype=torch.bfloat16, device=dev), SENT)
    return dict(c=c, c_buf=c_buf, cache=cache_buf[:f, :M], cache_buf=cache_buf)


def launch(p, s, mode, sa=None, sb=None, bias="own"):
    bias = p["bias"] if isinstance(bias, str) else bias
    torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs(p["a"], p["w"], s["c"], bias, s["cache"], p["inds"], p["cnt"], p["sa"] if sa is None else sa,
                                              p["sb"] if sb is None else sb, p["act"], MODES[mode])
    return s


def launch_scalar(p, s, mode):
    torch.ops.chipmunk.csp_mlp_mm1_fp8_act(p["a"], p["w"], s["c"], p["bias"], s["cache"], p["inds"], p["cnt"], p["ra"].reshape(()), p["rb"].reshape(()),
                                           p["act"], MODES[mode])
    return s


def check_untouched(p, s, what, cache_written):
    M, f = p["M"], p["F"]
    assert (s["c_buf"][M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    assert (s["cache_buf"][f] == SENT).all(), f"{what}: the row behind the cache's F * ldc elements was written"
    assert torch.isnan(s["cache_buf"][:f, M:].float()).all(), f"{what}: the cache's padding columns were written"
    assert torch.isnan(p["a_buf"][M:].float()).all() and torch.isnan(p["sa_buf"][M:]).all(), f"{what}: the slack of a / scale_a changed"
    assert torch.isnan(s["c"][~p["live"]].float()).all(), f"{what}: packed columns at or past a count were written"
    assert not torch.isnan(s["c"][p["live"]].float()).any(), f"{what}: a live packed column is NaN or was not written"
    if not cache_written:
        assert torch.equal(bits(s["cache"]), bits(p["cache0"])), f"{what}: the cache was written"
    else:
        assert not torch.isnan(s["cache"].float()).any(), f"{what}: NaN in the cache"


def same_bits(p, s, t, what):
    assert torch.equal(bits(s["c"])[p["live"]], bits(t["c"])[p["live"]]), f"{what}: packed deltas differ"
    assert torch.equal(bits(s["cache"]), bits(t["cache"])), f"{what}: caches differ"


# ------------------------------------------------------------------------------------------------ 1., 5.
@pytest.mark.parametrize("name", list(CASES))
def test_constant_vectors_give_the_bits_of_the_scalar_operator(dev, name):
    p = problem(name)
    sa_buf, sa = with_slack(p["ra"].expand(p["M"]).contiguous(), float("nan"))
    sb = p["rb"].expand(p["F"]).contiguous()
    for mode in MODES:
        s, t = launch(p, fresh_state(p), mode, sa, sb), launch_scalar(p, fresh_state(p), mode)
        same_bits(p, s, t, f"{name}, update {mode}")
        check_untouched(p, s, f"{name}, update {mode}", cache_written=mode != "none")
        assert (mode == "none") == torch.equal(bits(s["cache"]), bits(p["cache0"]))


@pytest.mark.parametrize("mode", list(MODES))
def test_constant_vectors_give_the_bits_of_the_scalar_operator_batched(dev, mode):
    ps = (problem("M200 F256 silu"), problem("M200 F256 gelu"))
    p = ps[0]
    M, F, ldc = p["M"], p["F"], p["ldc"]

    def state():
        cache_buf = torch.full((2, F + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
        cache_buf[:, F] = SENT
        c_buf = torch.full((2 * M + MLP_BM, F), SENT, dtype=torch.bfloat16, device=dev)
        c_buf[: 2 * M] = float("nan")
        c, cache = c_buf[: 2 * M].view(2, M, F), cache_buf[:, :F, :M]
        for b in range(2):
            cache[b] = ps[b]["cache0"]
        return c, cache, c_buf, cache_buf

    a, inds, cnt = (torch.stack([x[k] for x in ps]) for k in ("a", "inds", "cnt"))
    sa_buf, sa = with_slack(p["ra"].expand(2 * M).contiguous(), float("nan"))
    c, cache, c_buf, cache_buf = state()
    torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs(a, p["w"], c, p["bias"], cache, inds, cnt, sa.view(2, M), p["rb"].expand(F).contiguous(), "silu", MODES[mode])
    c0, cache0, _, _ = state()
    torch.ops.chipmunk.csp_mlp_mm1_fp8_act(a, p["w"], c0, p["bias"], cache0, inds, cnt, p["ra"].reshape(()), p["rb"].reshape(()), "silu", MODES[mode])
    live = torch.stack([x["live"] for x in ps])
    assert torch.equal(bits(c)[live], bits(c0)[live]) and torch.isnan(c[~live].float()).all() and torch.equal(bits(cache), bits(cache0))
    assert (c_buf[2 * M:] == SENT).all() and (cache_buf[:, F] == SENT).all() and torch.isnan(cache_buf[:, :F, M:].float()).all()


# ------------------------------------------------------------------------------------------------ 2., 5.
@pytest.mark.parametrize("name", list(CASES))
def test_varying_scales_against_fp64_under_the_proven_bound(dev, name):
    p = problem(name)
    assert am.ACT_SEG_BOUND == MLP_SEG_BOUND
    for mode in MODES:
        s = launch(p, fresh_state(p), mode)
        what = f"update {mode} | {name}"
        check_untouched(p, s, what, cache_written=mode != "none")
        worst = am.assert_act_deltas(p, s["c"], p["exact"], p["fresh"], what)
        print(f"{what}: packed deltas, worst segment {worst:.4f}")
        if mode != "none":
            am.assert_act_cache(p, s["cache"], p["exact"], p["fresh"], what, accumulate=mode == "scatter")
        # ... and the bits of the fp32 mirror's arithmetic are close by: the same roundings, another summation order
        t = launch(p, fresh_state(p), mode)
        same_bits(p, s, t, f"{what}: two launches")


# ------------------------------------------------------------------------------------------------ 3.
@pytest.mark.parametrize("name", ["M200 F256 gelu_tanh", "M203 F128 silu no bias"])
def test_the_scatter_form_equals_the_plain_form_and_csp_scatter_add(dev, name):
    from chipmunk_amd.ops import scatter_add
    p = problem(name)
    s, t = launch(p, fresh_state(p), "scatter"), launch(p, fresh_state(p), "none")
    scatter_add(t["c"], t["cache"], p["inds"], p["cnt"], 6)
    same_bits(p, s, t, name)
    assert not torch.equal(bits(s["cache"]), bits(p["cache0"]))


# ------------------------------------------------------------------------------------------------ 4.
@pytest.mark.parametrize("mode", ["none", "scatter"])
@pytest.mark.parametrize("shape", ["M200 F256", "M203 F128"])
def test_a_batch_of_two_equals_two_calls_on_the_slices(dev, shape, mode):
    ps = (problem(f"{shape} gelu"), problem(f"{shape} silu"))       # one weight, one bias, one activation for the batch: the first one's
    p = ps[0]
    qs = (p, dict(ps[1], w=p["w"], bias=p["bias"], sb=p["sb"], act=p["act"]))
    M, F, ldc = p["M"], p["F"], p["ldc"]
    cache_buf = torch.full((2, F + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
    cache_buf[:, F] = SENT
    c_buf = torch.full((2 * M + MLP_BM, F), SENT, dtype=torch.bfloat16, device=dev)
    c_buf[: 2 * M] = float("nan")
    c, cache = c_buf[: 2 * M].view(2, M, F), cache_buf[:, :F, :M]
    for b in range(2):
        cache[b] = qs[b]["cache0"]
    a, inds, cnt = (torch.stack([x[k] for x in qs]) for k in ("a", "inds", "cnt"))
    sa_buf, sa = with_slack(torch.cat([x["sa"] for x in qs]), float("nan"))
    launch(dict(p, a=a, inds=inds, cnt=cnt), dict(c=c, cache=cache), mode, sa=sa.view(2, M))
    assert (c_buf[2 * M:] == SENT).all() and (cache_buf[:, F] == SENT).all() and torch.isnan(cache_buf[:, :F, M:].float()).all()
    for b in range(2):
        s = launch(qs[b], fresh_state(qs[b]), mode)
        live = qs[b]["live"]
        assert torch.equal(bits(c[b])[live], bits(s["c"])[live]) and torch.isnan(c[b][~live].float()).all(), f"sequence {b}: packed deltas"
        assert torch.equal(bits(cache[b]), bits(s["cache"])), f"sequence {b}: cache"


# ------------------------------------------------------------------------------------------------ 6.
def test_a_scale_vector_off_a_16_byte_boundary_gives_the_same_bits(dev):
    p = problem("M200 F256 silu")
    buf = torch.full((p["M"] + 9,), float("nan"), device=dev)
    buf[1: p["M"] + 1] = p["sa"]
    sa = buf[1: p["M"] + 1]
    assert sa.data_ptr() % 16 == 4 and sa.is_contiguous()
    for mode in MODES:
        same_bits(p, launch(p, fresh_state(p), mode, sa=sa), launch(p, fresh_state(p), mode), f"update {mode}")


# ------------------------------------------------------------------------------------------------ 7.
def test_wrong_scale_tensors_raise_before_anything_is_enqueued(dev):
    p = problem("M200 F256 silu")
    M, F = p["M"], p["F"]
    s = fresh_state(p)
    bad = {"scale_a float64": dict(sa=p["sa"].double()), "scale_b bfloat16": dict(sb=p["sb"].bfloat16()),
           "scale_a one element": dict(sa=p["sa"][:1]), "scale_b one element": dict(sb=p["sb"][:1]),
           "scale_a [M + 1]": dict(sa=torch.ones(M + 1, device=dev)), "scale_a [1, M]": dict(sa=p["sa"].reshape(1, M)),
           "scale_b [F, 1]": dict(sb=p["sb"].reshape(F, 1)), "scale_b [F - 1]": dict(sb=p["sb"][: F - 1]),
           "scale_a strided": dict(sa=torch.ones(2 * M, device=dev)[::2]), "scale_b strided": dict(sb=torch.ones(2 * F, device=dev)[::2]),
           "scale_a on the host": dict(sa=p["sa"].cpu()), "scale_b on the host": dict(sb=p["sb"].cpu())}
    for what, kw in bad.items():
        with pytest.raises(RuntimeError, match="scale_a|scale_b"):
            launch(p, s, "scatter", **kw)
    torch.cuda.synchronize()
    assert torch.isnan(s["c"].float()).all() and torch.equal(bits(s["cache"]), bits(p["cache0"])), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ 8.
def test_run_e2e_dispatches_on_the_rank_of_the_scales(dev, fresh_config):
    from chipmunk_amd.ops.mlp import run_e2e
    p = problem("M200 F256 silu")
    M, F, N2 = p["M"], p["F"], 384
    g = torch.Generator().manual_seed(961)
    w2T = (torch.randn(F, N2, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    out0 = (torch.randn(M, N2, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    res = {}
    for fused in (True, False):
        fresh_config["mlp"]["fused_scatter"] = fused
        s = fresh_state(p)
        out_buf, out = with_slack(out0, SENT)
        run_e2e(p["a"], p["w"], p["bias"], w2T, p["inds"], p["cnt"], s["cache"], out, 6, p["sa"], p["sb"], act="silu")
        torch.cuda.synchronize()
        assert (out_buf[M:] == SENT).all() and (s["cache_buf"][F] == SENT).all()
        res[fused] = (out.clone(), s["cache"].clone())
    assert torch.equal(bits(res[True][0]), bits(res[False][0])) and torch.equal(bits(res[True][1]), bits(res[False][1]))
    am.assert_act_cache(p, res[True][1], p["exact"], p["fresh"], "run_e2e with scale vectors")      # the vectors reached GEMM1
    # 0-dim scales: the operators of today (the cache differs: other scales, other activations)
    fresh_config["mlp"]["fused_scatter"] = True
    s = fresh_state(p)
    run_e2e(p["a"], p["w"], p["bias"], w2T, p["inds"], p["cnt"], s["cache"], out0.clone(), 6, p["ra"].reshape(()), p["rb"].reshape(()), act="silu")
    t = launch_scalar(p, fresh_state(p), "scatter")
    assert torch.equal(bits(s["cache"]), bits(t["cache"]))
    with pytest.raises(ValueError, match="mixed pair"):
        run_e2e(p["a"], p["w"], p["bias"], w2T, p["inds"], p["cnt"], s["cache"], out0.clone(), 6, p["sa"], p["rb"], act="silu")
