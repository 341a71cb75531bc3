"""The segment-relative error metric of the sparse-MLP kernel tests (helpers.mm1_exact / mm2_exact / seg_rel_err /
assert_segs_close), proven on the CPU: over the case list of helpers.mlp1_cases / mlp2_cases

1. the CPU references pass at the shipped bound and their worst segment sits at or under ORACLE_MLP_SEG_ERR.  References: the
   oracle for csp_mlp_mm1, csp_mlp_mm1_fp8, csp_mlp_mm2 and csp_mlp_mm2_and_scatter_add; for the gated operators the plain-torch
   mirrors of tests/glu_method_model.py and tests/glu_fp8_method_model.py; for csp_mlp_mm2_w8 the fp32 statement `_mm2_w8_fp32`;
2. every mutant -- the exact fp64 result with ONE defect, rounded to bf16 where the operator rounds -- fails, unless the defect is
   inert on the input (proven by test_inert_pairs_are_inert) or hidden by a derived term (`_term_limited`: one pair, stated there);
3. MLP_SEG_MARGIN * ORACLE_MLP_SEG_ERR is at most half the weakest counted mutant's error (a condition, not a measurement).

No kernel is involved.  `python tests/test_mlp_metric_cpu.py` prints the tables of docs/TEST_SENSITIVITY.md, "Sparse MLP
kernels" (floor per case, error per mutant, and whether assert_close_bf16's defaults against the reference accept the mutant)."""
import functools
import os
import sys

import pytest
import torch

for _p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
    if _p not in sys.path:
        sys.path.insert(0, _p)             # (run as a script: helpers and the oracle package)

import oracle  # noqa: E402
from glu_fp8_method_model import mm1_glu_fp8_mirror  # noqa: E402
from glu_method_model import mm1_glu_mirror  # noqa: E402
from helpers import (BF16_EPS, MLP_BM, MLP_SEG_BOUND, MLP_SEG_MARGIN, MLP_SEG_W1, MLP_SEG_W2, ORACLE_MLP_SEG_ERR, assert_close_bf16,  # noqa: E402
                     assert_segs_close, gathered_cache, mlp1_cases, mlp2_base, mlp2_cases, mlp2_problem, mlp_exact_args,
                     mlp_group_cols, mlp_problem, mm1_exact, mm2_exact, seg_rel_err, seg_term)

SENT = 7.0
CASES1, CASES2 = mlp1_cases(), mlp2_cases()
BASES = ("zero", "product", "unit")
RECORDED_ONLY = {"pre-activation x 1.01", "result x 1.01", "sum x 1.01"}     # 0.01 plus rounding by construction: rejected, not counted
NOT_SEPARABLE = {"the other GELU (tanh / exact)"}       # at the floor: test_gpu_mlp_glu.py's projection test tells the two apart


def _bf16(x):
    return x.to(torch.bfloat16)


def _padded(t, dim, n, fill=0.0):
    """t with dimension `dim` grown to n entries (the oracle's GEMM1 and scatter-add take whole 128-row groups)"""
    shape = list(t.shape)
    shape[dim] = n
    out = torch.full(shape, fill, dtype=torch.float32).to(t.dtype)
    idx = [slice(None)] * t.dim()
    idx[dim] = slice(0, t.shape[dim])
    if t.dtype == torch.float8_e4m3fn:
        out.view(torch.uint8)[tuple(idx)] = t.view(torch.uint8)
    else:
        out[tuple(idx)] = t
    return out


def _reference1(p):
    """the packed deltas [M, F] bf16 of problem p by the CPU reference of its operator (sentinel at and past the counts); for the
    ungated operators also the cache after the operator's scatter-add / update"""
    M, F, Mp = p["M"], p["F"], p["G"] * MLP_BM
    if p["gated"]:
        args = (p["a"], p["w"], p["wu"], p["bias"], p["bu"], p["act"], p["cache0"], p["inds"], p["cnt"])
        c = mm1_glu_fp8_mirror(*args, p["ra"], p["rb"], p["rbu"]) if p["fp8"] else mm1_glu_mirror(*args)
        return dict(c=c)
    c = torch.full((Mp, F), SENT, dtype=torch.bfloat16)
    cache = _padded(p["cache0"], 1, Mp)
    out = {}
    if p["fp8"]:
        oracle.csp_mlp_mm1_fp8(_padded(p["a"], 0, Mp), p["w"], c, p["bias"], cache, p["inds"], p["cnt"], p["ra"], p["rb"], True)
        out["cache updated"] = cache[:, :M]        # the activation itself, stored by GEMM1
        cache = _padded(p["cache0"], 1, Mp)
    else:
        oracle.csp_mlp_mm1(_padded(p["a"], 0, Mp), p["w"], c, p["bias"], cache, p["inds"], p["cnt"])
    oracle.csp_scatter_add(c, cache, p["inds"], p["cnt"])
    return dict(out, c=c[:M], cache=cache[:, :M])


def _mm1(p, pre_mul=1.0, **over):
    q = dict(p, **over)
    return mm1_exact(q["a"], q["w"], q["bias"], q["cache0"], q["inds"], q["cnt"], pre_mul=pre_mul, **mlp_exact_args(q))


def _k_cut(p, n):
    over = dict(a=p["a"][:, :-n], w=p["w"][:, :-n])
    if p["gated"]:
        over["wu"] = p["wu"][:, :-n]
    return over


@functools.lru_cache(maxsize=None)
def _evaluate1(name):
    """exact deltas, reference output and the mutants (bf16) of one GEMM1 case"""
    p = mlp_problem(**CASES1[name])
    M, F, G, counts = p["M"], p["F"], p["G"], p["counts"]
    delta, fresh = _mm1(p)
    cols = mlp_group_cols(p["cnt"], M)
    ungated_fp8 = p["fp8"] and not p["gated"]
    # sec. 2 of the issue: the ungated fp8 operator rounds the activation to bf16, then subtracts in bf16
    term = seg_term(fresh, delta, MLP_SEG_W1, cols) if ungated_fp8 else None

    def stored(res):                       # (delta, fresh) of a mutant -> what the operator would store
        d, f = res
        return _bf16(_bf16(f).double() - (f - d)) if ungated_fp8 else _bf16(d)          # (f - d: the cache the mutant read)
    mut = {}
    mut["last k element dropped"] = stored(_mm1(p, **_k_cut(p, 1)))
    mut["last 32 k dropped"] = stored(_mm1(p, **_k_cut(p, 32)))
    mut["last 64 k dropped"] = stored(_mm1(p, **_k_cut(p, 64)))
    if p["bias"] is not None:
        mut["bias absent"] = stored(_mm1(p, bias=None))
        mut["bias of column idx+1"] = stored(_mm1(p, bias=p["bias"].roll(-1)))
    mut["cache column idx+1"] = stored(_mm1(p, cache0=p["cache0"].roll(-1, 0)))
    mut["cache of token i+1"] = stored(_mm1(p, cache0=p["cache0"].roll(-1, 1)))
    swapped = stored((delta, fresh)).clone()
    for g in range(G):
        half = min(64, M - g * MLP_BM - 64)          # the rows present in the second half
        if half > 0:
            a, b = g * MLP_BM, g * MLP_BM + 64
            swapped[a:a + half], swapped[b:b + half] = swapped[b:b + half].clone(), swapped[a:a + half].clone()
    mut["rows 0..63 and 64..127 of a group swapped"] = swapped
    far = p["inds"].clone()
    for g, n in enumerate(counts):
        if 0 < n < F:
            far[g, n - 1] = p["inds"][g, n]
    mut["last kept column from the first padding index"] = stored(_mm1(p, inds=far))
    mut["pre-activation x 1.02"] = stored(_mm1(p, pre_mul=1.02))
    mut["pre-activation x 1.01"] = stored(_mm1(p, pre_mul=1.01))
    mut["result x 1.01"] = _bf16(1.01 * stored((delta, fresh)).double()) if ungated_fp8 else _bf16(1.01 * delta)
    if p["gated"]:
        if p["bu"] is not None:
            mut["up bias absent"] = stored(_mm1(p, bu=None))
        over = dict(w=p["wu"], wu=p["w"])
        if p["fp8"]:
            over.update(rb=p["rbu"], rbu=p["rb"])
            mut["gate scale used for the up branch"] = stored(_mm1(p, rbu=p["rb"]))
        mut["gate and up weights swapped"] = stored(_mm1(p, **over))
        mut["activation of another kind"] = stored(_mm1(p, act="gelu_tanh" if p["act"] == "silu" else "silu"))
        if p["act"] != "silu":
            mut["the other GELU (tanh / exact)"] = stored(_mm1(p, act="gelu" if p["act"] == "gelu_tanh" else "gelu_tanh"))
    return dict(p=p, exact=delta, fresh=fresh, cols=cols, term=term, ref=_reference1(p), mut=mut)


def _mm2_w8_fp32(p, base):
    """csp_mlp_mm2_w8 as documented (ops/mlp.py): c = bf16(bf16(fp32 sum * scale) + c), in fp32 torch"""
    out = base.clone()
    for g, n in enumerate(p["counts"]):
        rows = slice(g * MLP_BM, min(p["M"], (g + 1) * MLP_BM))
        if n:
            acc = (p["packed"][rows, :n].float() @ p["w8"].float()[p["inds"][g, :n].long()]) * p["r8"]
            out[rows] = _bf16(_bf16(acc).float() + base[rows].float())
    return out


@functools.lru_cache(maxsize=None)
def _evaluate2(name, op):
    """exact product and, per base, the reference result and the mutant results of one GEMM2 case; op "mm2" | "w8" """
    p = mlp2_problem(**CASES2[name])
    M, F, counts = p["M"], p["F"], p["counts"]
    w, scale = (p["w8"], p["r8"]) if op == "w8" else (p["w2T"], None)
    exact = mm2_exact(p["packed"], w, p["inds"], p["cnt"], scale)
    lower = torch.tensor([max(0, n - 1) for n in counts])
    cut32 = torch.tensor([(n - 1) // 32 * 32 if n else 0 for n in counts])
    other = p["inds"].clone()
    for g, n in enumerate(counts):
        if n:
            other[g, n // 2] = (other[g, n // 2] + 1) % F
    prod = {"last kept column dropped": mm2_exact(p["packed"], w, p["inds"], lower, scale),
            "count cut to the next lower multiple of 32": mm2_exact(p["packed"], w, p["inds"], cut32, scale),
            "weight row idx+1 for one kept column": mm2_exact(p["packed"], w, other, p["cnt"], scale),
            "sum x 1.02": 1.02 * exact, "sum x 1.01": 1.01 * exact}
    out = {}
    for kind in BASES:
        base = mlp2_base(p, kind, exact)

        def stored(x, b=None):         # bf16 of the fp32 sum, then the bf16 add (the reference's accumulate)
            return _bf16(_bf16(x).double() + (base if b is None else b).double())
        if op == "w8":
            ref = _mm2_w8_fp32(p, base)
        else:
            ref = base.clone()
            oracle.csp_mlp_mm2(p["packed"], p["w2T"], ref, p["inds"], p["cnt"])
        mut = {m: stored(x) for m, x in prod.items()} if kind != "unit" else {}
        mut["product added twice"] = stored(exact, stored(exact))
        mut["base lost"] = _bf16(exact)
        if op == "w8":
            mut["scale applied to the base as well"] = stored(exact, _bf16(base.double() * float(p["r8"])))
        out[kind] = dict(base=base, ref=ref, mut=mut)
    return dict(p=p, exact=exact, bases=out)


def _delta(result, base):
    r = result.double()
    return torch.where(torch.isfinite(r), r - base.double(), r)


def _term2(result, base_kind, exact):
    """the accumulate term of a GEMM2 result: none on a zero base (a plain output: bf16(bf16(sum) + 0) is one rounding)"""
    return None if base_kind == "zero" else seg_term(result, exact, MLP_SEG_W2)


def _err1(e, o):
    err = seg_rel_err(o, e["exact"], MLP_SEG_W1, e["cols"])
    return float((err if e["term"] is None else err - e["term"]).max())


def _err2(e, kind, o):
    err = seg_rel_err(_delta(o, e["bases"][kind]["base"]), e["exact"], MLP_SEG_W2)
    term = _term2(o, kind, e["exact"])
    return float((err if term is None else err - term).max())


# Ungated fp8 GEMM1 with the previous step's activations in the cache: the term 2^-8 ||act_seg|| / ||delta_seg|| of the operator's
# documented bf16 activation is several times the bound there (the deltas are a tenth of the activations), and what it has to allow
# hides a 1 % error of the stored result, which is all of that rounding's size.  Every other mutant is rejected there too.  The route
# is asserted in both regimes; the random-cache regime is the one where its assertion is sharp, and every mutant is rejected there.
def _term_limited(name, m="result x 1.01"):
    c = CASES1[name]
    return c["fp8"] and not c["gated"] and c["regime"] == "previous step" and m == "result x 1.01"


def _inert2(kind, m):
    """on a zero base `base lost` and `scale applied to the base as well` change nothing: test_inert_pairs_are_inert"""
    return kind == "zero" and m in ("base lost", "scale applied to the base as well")


# ------------------------------------------------------------------------------------------------ floors
def _floors():
    floors = {}
    for name in CASES1:
        e = _evaluate1(name)
        floors[f"{name}: packed deltas"] = _err1(e, e["ref"]["c"])
        if "cache" in e["ref"]:
            # bf16(cache + delta): the delta's error, in units of ||delta_seg|| (what the bound is taken in), after the rounding of the stored
            # sum -- and on the fp8 route of the activation -- is taken off: helpers.refreshed_cache_term
            got = gathered_cache(e["ref"]["cache"], e["p"]["inds"], e["p"]["cnt"])
            rho = seg_term(e["exact"], e["fresh"], MLP_SEG_W1, e["cols"]) / BF16_EPS
            off = seg_term(got, e["fresh"], MLP_SEG_W1, e["cols"]) + (BF16_EPS if "cache updated" in e["ref"] else 0.0)
            err = seg_rel_err(got, e["fresh"], MLP_SEG_W1, e["cols"])
            floors[f"{name}: cache after the scatter-add"] = float(((err - off)[rho > 0] / rho[rho > 0]).max())
            if "cache updated" in e["ref"]:
                upd = gathered_cache(e["ref"]["cache updated"], e["p"]["inds"], e["p"]["cnt"])
                floors[f"{name}: cache = activation"] = float(seg_rel_err(upd, e["fresh"], MLP_SEG_W1, e["cols"]).max())
    for name in CASES2:
        for op in ("mm2", "w8"):
            e = _evaluate2(name, op)
            for kind in BASES:
                floors[f"{op} {name}, {kind} base"] = _err2(e, kind, e["bases"][kind]["ref"])
    return floors


@pytest.mark.parametrize("name", list(CASES1))
def test_gemm1_reference_passes_and_pins_the_floor(name):
    e = _evaluate1(name)
    worst = assert_segs_close(e["ref"]["c"], e["exact"], MLP_SEG_BOUND, f"reference, {name}", extra=e["term"], cols=e["cols"])
    assert worst <= ORACLE_MLP_SEG_ERR, f"{name}: the reference's worst segment {worst:.5f} is above ORACLE_MLP_SEG_ERR = {ORACLE_MLP_SEG_ERR}"
    p = e["p"]
    for g, n in enumerate(p["counts"]):
        assert (e["ref"]["c"][g * MLP_BM:(g + 1) * MLP_BM, n:] == SENT).all()


@pytest.mark.parametrize("op", ["mm2", "w8"])
@pytest.mark.parametrize("name", list(CASES2))
def test_gemm2_reference_passes_and_pins_the_floor(name, op):
    e = _evaluate2(name, op)
    for kind in BASES:
        b = e["bases"][kind]
        worst = assert_segs_close(_delta(b["ref"], b["base"]), e["exact"], MLP_SEG_BOUND, f"reference, {op} {name}, {kind} base",
                                  extra=_term2(b["ref"], kind, e["exact"]), width=MLP_SEG_W2)
        assert worst <= ORACLE_MLP_SEG_ERR, f"{op} {name}, {kind} base: {worst:.5f} is above ORACLE_MLP_SEG_ERR = {ORACLE_MLP_SEG_ERR}"


def test_floor_constant_is_tight():
    """ORACLE_MLP_SEG_ERR is the measured maximum over every operator, regime and base (terms taken off), rounded up to two digits"""
    floors = _floors()
    top = max(floors, key=floors.get)
    assert floors[top] <= ORACLE_MLP_SEG_ERR <= floors[top] + 1e-4, (top, floors[top])


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("name", list(CASES1))
def test_every_gemm1_mutant_is_rejected(name):
    e = _evaluate1(name)
    for m, o in e["mut"].items():
        if m in NOT_SEPARABLE or _term_limited(name, m):
            continue
        with pytest.raises(AssertionError, match=r"group \d+ row \d+ \(row \d+ of its group\) segment \d+ .*segments over the bound"):
            assert_segs_close(o, e["exact"], MLP_SEG_BOUND, f"{name}, {m}", extra=e["term"], cols=e["cols"])


@pytest.mark.parametrize("op", ["mm2", "w8"])
@pytest.mark.parametrize("name", list(CASES2))
def test_every_gemm2_mutant_is_rejected(name, op):
    e = _evaluate2(name, op)
    for kind in BASES:
        b = e["bases"][kind]
        for m, o in b["mut"].items():
            if _inert2(kind, m) or (m in RECORDED_ONLY and kind != "zero"):     # (sum x 1.01 under the accumulate term: see below)
                continue
            with pytest.raises(AssertionError, match=r"group \d+ row \d+ \(row \d+ of its group\) segment \d+"):
                assert_segs_close(_delta(o, b["base"]), e["exact"], MLP_SEG_BOUND, f"{op} {name}, {kind} base, {m}",
                                  extra=_term2(o, kind, e["exact"]), width=MLP_SEG_W2)


def test_inert_pairs_are_inert():
    """the pairs left out above change nothing, for the reason stated: with a base of zeros the result IS the product's bf16"""
    for name in CASES2:
        e = _evaluate2(name, "w8")
        z = e["bases"]["zero"]
        assert not z["base"].any()
        want = _bf16(_bf16(e["exact"]).double() + z["base"].double())
        for m in ("base lost", "scale applied to the base as well"):
            assert torch.equal(z["mut"][m], want), (name, m)
        assert not torch.equal(e["bases"]["product"]["mut"]["base lost"], _bf16(_bf16(e["exact"]).double() + e["bases"]["product"]["base"].double()))


def test_the_term_limited_pair_is_hidden_by_the_term_alone():
    """ungated fp8, previous-step cache, result x 1.01: the term exceeds the bound in every live segment, and without it the mutant is
    far over the bound -- the operator's documented rounding hides it, not the metric"""
    seen = 0
    for name in CASES1:
        if not _term_limited(name):
            continue
        e = _evaluate1(name)
        live = e["term"] > 0
        assert float(e["term"][live].min()) > MLP_SEG_BOUND
        raw = seg_rel_err(e["mut"]["result x 1.01"], e["exact"], MLP_SEG_W1, e["cols"])
        assert float(raw.max()) > 2 * MLP_SEG_BOUND and _err1(e, e["mut"]["result x 1.01"]) <= MLP_SEG_BOUND
        seen += 1
    assert seen == 2


def _mutant_errors(counted_only=True):
    errs = {}
    for name in CASES1:
        e = _evaluate1(name)
        for m, o in e["mut"].items():
            if counted_only and (m in RECORDED_ONLY | NOT_SEPARABLE or _term_limited(name, m)):
                continue
            errs[(name, m)] = _err1(e, o)
    for name in CASES2:
        for op in ("mm2", "w8"):
            e = _evaluate2(name, op)
            for kind in BASES:
                for m, o in e["bases"][kind]["mut"].items():
                    if counted_only and (m in RECORDED_ONLY or _inert2(kind, m)):
                        continue
                    errs[(f"{op} {name}, {kind} base", m)] = _err2(e, kind, o)
    return errs


def test_separation_of_bound_and_weakest_mutant():
    assert MLP_SEG_MARGIN in (1.5, 1.75, 2.0)
    errs = _mutant_errors()
    weakest = min(errs, key=errs.get)
    assert MLP_SEG_MARGIN * ORACLE_MLP_SEG_ERR <= 0.5 * errs[weakest], (
        f"bound {MLP_SEG_BOUND:.5f} is more than half of the weakest counted mutant's error {errs[weakest]:.5f} {weakest}")
    for step in (2.0, 1.75):      # the margin is the largest of 2 / 1.75 / 1.5 that keeps the condition
        if step > MLP_SEG_MARGIN:
            assert step * ORACLE_MLP_SEG_ERR > 0.5 * errs[weakest], f"margin {step} holds as well: ship it"


def test_the_recorded_one_percent_mutants_exceed_the_bound():
    """x 1.01 is 0.01 plus rounding by construction: over the bound, though not by a factor of two (so not in the minimum).  GEMM2's is
    judged on the zero base: on a base of the product's size the accumulate term (0.0055 there) takes it to 0.006 - 0.007, under the
    bound -- which is why the GPU test asserts GEMM2 on a zero base first."""
    errs = _mutant_errors(counted_only=False)
    seen = 0
    for (name, m), v in errs.items():
        if m in RECORDED_ONLY and not (name in CASES1 and _term_limited(name, m)) and (name in CASES1 or name.endswith("zero base")):
            assert v > MLP_SEG_BOUND, (name, m, v)
            seen += 1
    assert seen == 2 * len(CASES1) - 2 + 2 * len(CASES2)


def _old_tolerance_accepts(o, ref, live=None):
    try:
        assert_close_bf16(o if live is None else torch.where(live, o, ref), ref)
    except AssertionError:
        return False
    return True


if __name__ == "__main__":
    oracle.build()
    floors = _floors()
    print("| reference | worst segment (term taken off) |\n|---|---|")
    for n, f in floors.items():
        print(f"| {n} | {f:.4f} |")
    print(f"\nmaximum {max(floors.values()):.5f}\n")
    rows = {}
    for name in CASES1:
        e = _evaluate1(name)
        live = torch.arange(e["p"]["F"]) < e["cols"][:, None]
        kind, regime = name.split(" M")[0].replace(" no bias", ""), name.split(", ")[1]
        for m, o in e["mut"].items():
            v, acc = _err1(e, o), _old_tolerance_accepts(o, e["ref"]["c"], live)
            r = rows.setdefault((f"GEMM1 {kind}, {regime}", m), [v, v, False])
            r[0], r[1], r[2] = min(r[0], v), max(r[1], v), r[2] or acc
    for name in CASES2:
        for op in ("mm2", "w8"):
            e = _evaluate2(name, op)
            for kind in BASES:
                b = e["bases"][kind]
                for m, o in b["mut"].items():
                    v, acc = _err2(e, kind, o), _old_tolerance_accepts(o, b["ref"])
                    r = rows.setdefault((f"GEMM2 {op}, {kind} base", m + (" (inert)" if _inert2(kind, m) else "")), [v, v, False])
                    r[0], r[1], r[2] = min(r[0], v), max(r[1], v), r[2] or acc
    print("| operator, regime | mutant | weakest case | strongest case | old tolerance |\n|---|---|---|---|---|")
    for (what, m), (lo, hi, acc) in rows.items():
        print(f"| {what} | {m} | {lo:.4f} | {hi:.4f} | {'accepts *' if acc else 'rejects'} |")
    errs = _mutant_errors()
    weakest = min(errs, key=errs.get)
    print(f"\nweakest counted mutant {weakest}: {errs[weakest]:.4f}; bound {MLP_SEG_BOUND:.4f}; separation {errs[weakest] / MLP_SEG_BOUND:.2f}")
