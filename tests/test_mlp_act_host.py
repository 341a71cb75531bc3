"""Ungated activations in the sparse MLP without a GPU ("Ungated activations"):

1. the C ABI lists ``chipmunk_csp_mlp_mm1_act[_batched]`` / ``chipmunk_csp_mlp_mm1_fp8_act[_batched]`` and refuses bad arguments with
   code 1 and a message; the fake kernels trace; the wrappers refuse an unknown activation by name;
2. ``activation_code`` and ``SparseDiffMlp``'s construction: the three modules, a named callable, a bias-free fc1, what is refused;
3. (the compile audit of the kernels is tests/test_mlp_mm1_form_audit.py;)
4. the segment-relative checker of the GPU test (tests/mlp_act_model.py), proven on the CPU: the plain-torch mirror of the new epilogue
   arithmetic passes and pins the floor, the bound follows from the floor by the rule of docs/TEST_SENSITIVITY.md, every mutant is
   rejected, and margin x floor is at most half the weakest counted mutant's error.

`python tests/test_mlp_act_host.py` prints the floor and mutant tables of docs/TEST_SENSITIVITY.md, "Ungated activations"."""
import ctypes
import functools
import os
import re
import sys

import pytest
import torch

for _p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
    if _p not in sys.path:
        sys.path.insert(0, _p)             # (run as a script)

import mlp_act_model as am  # noqa: E402
from cpu_ops import ExactGELU  # noqa: E402
from helpers import (BF16_EPS, MLP_ACTS, MLP_SEG_BOUND, MLP_SEG_MARGIN, MLP_SEG_W1, ORACLE_MLP_SEG_ERR, assert_segs_close, gathered_cache,  # noqa: E402
                     mlp_group_cols, mlp_problem, seg_rel_err, seg_term)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3 = torch.float8_e4m3fn
CASES = am.act_cases()
NAMES = ("chipmunk_csp_mlp_mm1_act", "chipmunk_csp_mlp_mm1_act_batched", "chipmunk_csp_mlp_mm1_fp8_act", "chipmunk_csp_mlp_mm1_fp8_act_batched")


# ------------------------------------------------------------------------------------------------------------------ 1. C ABI, operators
def test_abi_lists_the_four_entries_and_refuses_bad_arguments():
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    for name in NAMES:
        assert name in _native.SYMBOLS and re.search(rf"\b{name}\s*\(", header)
        assert hasattr(_native.lib(), name), f"{name} is not exported"
    assert _native.lib().chipmunk_abi_version() == 1
    lib, p, null = _native.lib(), ctypes.c_void_p(16), ctypes.c_void_p(0)      # (no launch happens: every call below is refused)

    def bf16(a=p, b=p, c=p, bias=null, cache=p, inds=p, cnt=p, M=100, K=128, F=256, ldc=104, act=1, upd=0, B=None, bs=None):
        bs = F * ldc if bs is None else bs
        if B is None:
            return lib.chipmunk_csp_mlp_mm1_act(a, b, c, bias, cache, inds, cnt, M, K, F, ldc, act, upd, null), _native.last_error()
        return lib.chipmunk_csp_mlp_mm1_act_batched(a, b, c, bias, cache, inds, cnt, M, K, F, ldc, act, upd, B, ctypes.c_int64(bs), null), _native.last_error()

    def fp8(a=p, b=p, c=p, bias=null, cache=p, inds=p, cnt=p, sa=p, sb=p, M=100, K=128, F=256, ldc=104, act=2, upd=0, B=None, bs=None):
        bs = F * ldc if bs is None else bs
        if B is None:
            return lib.chipmunk_csp_mlp_mm1_fp8_act(a, b, c, bias, cache, inds, cnt, sa, sb, M, K, F, ldc, act, upd, null), _native.last_error()
        return lib.chipmunk_csp_mlp_mm1_fp8_act_batched(a, b, c, bias, cache, inds, cnt, sa, sb, M, K, F, ldc, act, upd, B, ctypes.c_int64(bs),
                                                        null), _native.last_error()
    common = [(dict(a=null), "null"), (dict(b=null), "null"), (dict(c=null), "null"), (dict(cache=null), "null"),
              (dict(inds=null), "indices / counts"), (dict(cnt=null), "indices / counts"), (dict(M=0), "M must be positive"),
              (dict(F=96), "multiple of 64"), (dict(ldc=96), "cache pitch"), (dict(ldc=100), "cache pitch"),
              (dict(act=3), "unknown activation 3"), (dict(act=-1), "unknown activation -1"), (dict(upd=-1), "update_cache"), (dict(K=0), "K must be"),
              (dict(M=1 << 20, ldc=1 << 20, K=2048), "32-bit offsets"), (dict(F=1 << 20, K=2048), "32-bit offsets")]
    for fn, who, extra in ((bf16, "csp_mlp_mm1_act", [(dict(upd=2), "update_cache must be 0 or 1"), (dict(K=96), "multiple of 64"), (dict(K=32), "multiple of 64")]),
                           (fp8, "csp_mlp_mm1_fp8_act", [(dict(upd=3), "update_cache must be 0, 1 or 2"), (dict(K=192), "multiple of 128"),
                                                         (dict(K=64), "multiple of 128"), (dict(sa=null), "null"), (dict(sb=null), "null")])):
        for kw, text in common + extra:
            for batch in (dict(), dict(B=2)):
                rc, msg = fn(**kw, **batch)
                assert rc == 1 and text in msg, (who, kw, batch, rc, msg)
            if set(kw) & {"act", "upd", "K"}:        # the entry's own checks name it
                assert fn(**kw)[1].startswith(who + ":"), (who, kw, fn(**kw)[1])
        for kw, text in ((dict(B=0), "batch size"), (dict(B=-1), "batch size"), (dict(B=65536), "65535"), (dict(B=2, bs=256 * 104 - 8), "batch stride"),
                         (dict(B=2, bs=256 * 104 + 4), "batch stride")):
            rc, msg = fn(**kw)
            assert rc == 1 and text in msg, (who, kw, rc, msg)


def test_fake_kernels_trace_without_a_gpu_and_check_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16 = torch.bfloat16
        a, w, c = torch.empty(2, 333, 256, dtype=bf16), torch.empty(512, 256, dtype=bf16), torch.empty(2, 333, 512, dtype=bf16)
        cache, bias = torch.empty(2, 512, 336, dtype=bf16)[..., :333], torch.empty(512, dtype=bf16)
        inds, counts, s = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32), torch.empty(1)
        op, op8 = torch.ops.chipmunk.csp_mlp_mm1_act, torch.ops.chipmunk.csp_mlp_mm1_fp8_act
        assert op(a, w, c, bias, cache, inds, counts, "silu", True) is None
        assert op(a[0], w, c[0], None, cache[0], inds[0], counts[0], "gelu", False) is None
        assert op8(a.to(E4M3), w.to(E4M3), c, None, cache, inds, counts, s, s, "gelu_tanh", 2) is None
        with pytest.raises(RuntimeError, match="unknown activation"):
            op(a, w, c, bias, cache, inds, counts, "relu", True)
        with pytest.raises(RuntimeError, match=r"c must be \[M, F\]"):
            op(a, w, c[0], bias, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            op8(a, w, c, None, cache, inds, counts, s, s, "silu", 0)
        with pytest.raises(RuntimeError, match="0, 1 or 2"):
            op8(a.to(E4M3), w.to(E4M3), c, None, cache, inds, counts, s, s, "silu", 3)


def test_the_wrappers_refuse_an_unknown_activation_by_name():
    import chipmunk_amd.ops  # noqa: F401
    om = sys.modules["chipmunk_amd.ops.mlp"]             # (the package exports run_e2e under the module's name)
    z = torch.zeros(2, 2, dtype=torch.bfloat16)          # (the name is checked before any operator is reached)
    for fn, args in ((om.mm1, (z,) * 7), (om.mm1_scatter, (z,) * 7), (om.csp_mlp_mm1_fp8, (z,) * 9)):
        with pytest.raises(ValueError, match="gelu_tanh, silu, gelu"):
            fn(*args, act="relu")
    assert om.GLU_ACTS == MLP_ACTS
    import inspect
    for fn in (om.mm1, om.mm1_scatter, om.mm1_fp8_scatter, om.csp_mlp_mm1_fp8, om.run_e2e):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "act" and last.default == "gelu_tanh", fn.__name__


# ------------------------------------------------------------------------------------------------------------------ 2. module
def lin(i, o, bias=True):
    return torch.nn.Linear(i, o, bias=bias).bfloat16()


def test_activation_code_and_what_sparse_diff_mlp_accepts(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.modules import F8Linear, SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.modules.mlp import activation_code
    from chipmunk_amd.modules import mlp_glu
    from chipmunk_amd.util.layer_counter import LayerCounter
    assert mlp_glu.activation_code is activation_code
    assert activation_code(torch.nn.GELU(approximate="tanh")) == "gelu_tanh" and activation_code(ExactGELU(approximate="tanh")) == "gelu_tanh"
    assert activation_code(torch.nn.GELU()) == "gelu" and activation_code(ExactGELU()) == "gelu" and activation_code(torch.nn.SiLU()) == "silu"
    counter = LayerCounter(1, 1)
    for module, code in ((torch.nn.GELU(approximate="tanh"), "gelu_tanh"), (ExactGELU(approximate="tanh"), "gelu_tanh"), (torch.nn.GELU(), "gelu"),
                         (torch.nn.SiLU(), "silu")):
        assert SparseDiffMlp(0, counter, lin(128, 256), module, lin(256, 128)).act_code == code
    with pytest.raises(ValueError, match="SparseDiffMlp: unsupported activation") as e:
        SparseDiffMlp(0, counter, lin(128, 256), torch.nn.ReLU(), lin(256, 128))
    for text in ("nn.SiLU()", "nn.GELU(approximate='tanh')", "nn.GELU()", "act="):
        assert text in str(e.value)
    with pytest.raises(ValueError, match="unsupported activation"):
        SparseDiffMlp(0, counter, lin(128, 256), lambda x: x * torch.sigmoid(x), lin(256, 128))
    assert SparseDiffMlp(0, counter, lin(128, 256), lambda x: x * torch.sigmoid(x), lin(256, 128), act="silu").act_code == "silu"
    assert SparseDiffMlp(0, counter, lin(128, 256), torch.nn.ReLU(), lin(256, 128), 6, "gelu").act_code == "gelu"      # (the name wins)
    with pytest.raises(ValueError, match="unknown act 'relu'"):
        SparseDiffMlp(0, counter, lin(128, 256), torch.nn.ReLU(), lin(256, 128), act="relu")
    # a bias-free fc1: nn.Linear and an e4m3 F8Linear (from_linear carries bias=None over)
    assert SparseDiffMlp(0, counter, lin(128, 256, bias=False), torch.nn.SiLU(), lin(256, 128)).fc1[0].bias is None
    f8 = F8Linear.from_linear(lin(128, 256, bias=False), input_float8_dtype=E4M3)
    assert f8.bias is None and f8.weight.dtype == E4M3
    assert SparseDiffMlp(0, counter, f8, torch.nn.GELU(), lin(256, 128)).act_code == "gelu"
    # the gated module's refusal is word for word what it was
    with pytest.raises(ValueError) as e:
        SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), torch.nn.ReLU(), lin(256, 128))
    assert str(e.value) == ("SparseDiffGatedMlp: unsupported activation ReLU(): the gated GEMM1 computes nn.SiLU(), "
                            "nn.GELU(approximate='tanh') and nn.GELU() only")


# ------------------------------------------------------------------------------------------------------------------ 4. the checker
UPDATES = {False: ("none", "scatter"), True: ("none", "scatter", "store")}


@functools.lru_cache(maxsize=None)
def _evaluate(name):
    """problem, exact fp64 deltas / activations, the mirror's outputs per update mode and the mutants of one case"""
    p = mlp_problem(**CASES[name])
    delta, fresh = am.exact(p)
    return dict(p=p, delta=delta, fresh=fresh, cols=mlp_group_cols(p["cnt"], p["M"]), mirror={u: am.mm1_act_mirror(p, u) for u in UPDATES[p["fp8"]]},
                mut=am.act_mutants(p))


@functools.lru_cache(maxsize=None)
def _evaluate_small_step(name):
    """the exact-GELU cases in the previous-step regime with step ERF_MUTANT_STEP"""
    p = am.small_step_problem(CASES[name], am.ERF_MUTANT_STEP)
    delta, fresh = am.exact(p)
    return dict(p=p, delta=delta, fresh=fresh, cols=mlp_group_cols(p["cnt"], p["M"]), mirror={"none": am.mm1_act_mirror(p)}, mut=am.act_mutants(p))


SMALL_STEP = [n for n, c in CASES.items() if c["act"] == "gelu" and c["regime"] == "random"]       # (the regime is replaced: see small_step_problem)


def _floors(e):
    """what the GPU test asserts of one case, on the mirror: packed deltas per update mode, the cache after the scatter-add in units of
    ||delta_seg|| with its derived terms off (tests/test_mlp_metric_cpu.py, _floors), the cache that holds the activation itself"""
    p, out = e["p"], {}
    for upd, (c, cache) in e["mirror"].items():
        out[f"packed deltas, update {upd}"] = am.delta_err(p, c, e["delta"], e["fresh"])
        got = gathered_cache(cache, p["inds"], p["cnt"])
        if upd == "scatter":
            rho = seg_term(e["delta"], e["fresh"], MLP_SEG_W1, e["cols"]) / BF16_EPS
            off = seg_term(got, e["fresh"], MLP_SEG_W1, e["cols"]) + (BF16_EPS if p["fp8"] else 0.0)
            err = seg_rel_err(got, e["fresh"], MLP_SEG_W1, e["cols"])
            out["cache after the scatter-add"] = float(((err - off)[rho > 0] / rho[rho > 0]).max())
        elif upd == "store":
            out["cache = activation"] = float(seg_rel_err(got, e["fresh"], MLP_SEG_W1, e["cols"]).max())
    return out


def _floor():
    return max(v for n in CASES for v in _floors(_evaluate(n)).values())


def _counted(e, m):
    """exact against tanh GELU is counted where it can show: bf16 operands, the small-step regime (module docstring of mlp_act_model)"""
    return m != am.TANH_FOR_ERF or (not e["p"]["fp8"] and e["p"]["regime"].startswith("previous step, step"))


@pytest.mark.parametrize("name", list(CASES))
def test_mirror_passes_at_the_gpu_bound(name):
    e = _evaluate(name)
    p = e["p"]
    for upd, (c, cache) in e["mirror"].items():
        what = f"mirror, update {upd} | {name}"
        am.assert_act_deltas(p, c, e["delta"], e["fresh"], what)
        past = torch.arange(p["F"]) >= e["cols"][:, None]
        assert (c[past] == am.SENT).all()
        if upd == "none":
            assert torch.equal(cache.view(torch.int16), p["cache0"].view(torch.int16))
        else:
            am.assert_act_cache(p, cache, e["delta"], e["fresh"], what, accumulate=upd == "scatter")


def test_the_bound_follows_from_the_mirrors_floor():
    floor = _floor()
    small = max(_floors(_evaluate_small_step(n))["packed deltas, update none"] for n in SMALL_STEP)
    print(f"mirror floor {floor:.5f} (small-step cases {small:.5f}); ORACLE_MLP_SEG_ERR {ORACLE_MLP_SEG_ERR}; bound {am.ACT_SEG_BOUND}")
    assert am.ACT_SEG_BOUND == am.act_bound(max(floor, small))
    assert floor <= ORACLE_MLP_SEG_ERR and am.ACT_SEG_BOUND == MLP_SEG_BOUND      # (what mlp_act_model records)


@pytest.mark.parametrize("name", list(CASES))
def test_every_mutant_is_rejected(name):
    e = _evaluate(name)
    assert e["mut"]
    for m, o in e["mut"].items():
        if m == am.TANH_FOR_ERF:
            continue            # (counted in the small-step regime below)
        with pytest.raises(AssertionError, match=r"group \d+ row \d+ \(row \d+ of its group\) segment \d+ .*segments over the bound"):
            am.assert_act_deltas(e["p"], o, e["delta"], e["fresh"], f"{name}, {m}")


@pytest.mark.parametrize("name", SMALL_STEP)
def test_tanh_gelu_for_exact_gelu_in_the_small_step_regime(name):
    """bf16: the mirror passes and the mutant is rejected.  fp8: the route's documented bf16 rounding of the activation is of the two
    functions' distance, and its derived term covers mirror and mutant alike -- without the term the MIRROR is over the bound too, so no
    bound on the packed deltas can tell them apart there (the projection test on the GPU does)."""
    e = _evaluate_small_step(name)
    p, o = e["p"], e["mut"][am.TANH_FOR_ERF]
    am.assert_act_deltas(p, e["mirror"]["none"][0], e["delta"], e["fresh"], f"mirror | {name}, small step")
    if not p["fp8"]:
        with pytest.raises(AssertionError, match="segments over the bound"):
            am.assert_act_deltas(p, o, e["delta"], e["fresh"], f"{name}, small step, {am.TANH_FOR_ERF}")
    else:
        raw = float(seg_rel_err(e["mirror"]["none"][0], e["delta"], MLP_SEG_W1, e["cols"]).max())
        assert raw > 2 * am.ACT_SEG_BOUND, raw
        am.assert_act_deltas(p, o, e["delta"], e["fresh"], f"{name}, small step, {am.TANH_FOR_ERF} (under the term)")


def _mutant_errors():
    errs = {}
    for name in CASES:
        e = _evaluate(name)
        for m, o in e["mut"].items():
            if _counted(e, m):
                errs[(name, m)] = am.delta_err(e["p"], o, e["delta"], e["fresh"])
    for name in SMALL_STEP:
        e = _evaluate_small_step(name)
        if _counted(e, am.TANH_FOR_ERF):
            errs[(name + f", step {am.ERF_MUTANT_STEP}", am.TANH_FOR_ERF)] = am.delta_err(e["p"], e["mut"][am.TANH_FOR_ERF], e["delta"], e["fresh"])
    return errs


def test_separation_of_bound_and_weakest_mutant():
    errs = _mutant_errors()
    assert {m for _, m in errs} == {am.TANH_FOR_SILU, am.TANH_FOR_ERF, am.BIAS_ADDED, am.BIAS_DROPPED, am.BIAS_AFTER}
    weakest = min(errs, key=errs.get)
    floor = _floor()
    print(f"weakest counted mutant {weakest}: {errs[weakest]:.4f}; margin x floor {MLP_SEG_MARGIN * floor:.4f}; bound {am.ACT_SEG_BOUND:.4f}")
    assert MLP_SEG_MARGIN * floor <= 0.5 * errs[weakest] and am.ACT_SEG_BOUND <= 0.5 * errs[weakest], (weakest, errs[weakest])


if __name__ == "__main__":
    print("| case | quantity | mirror's worst segment (terms taken off) |\n|---|---|---|")
    for n in CASES:
        for q, v in _floors(_evaluate(n)).items():
            print(f"| {n} | {q} | {v:.4f} |")
    print(f"\nmaximum {_floor():.5f}\n")
    rows = {}
    for (name, m), v in _mutant_errors().items():
        key = (name.split(" ")[0], "small step" if "step 0." in name else name.split(", ")[1], m)
        r = rows.setdefault(key, [v, v])
        r[0], r[1] = min(r[0], v), max(r[1], v)
    print("| operands | regime | mutant | weakest case | strongest case |\n|---|---|---|---|---|")
    for (kind, regime, m), (lo, hi) in sorted(rows.items()):
        print(f"| {kind} | {regime} | {m} | {lo:.4f} | {hi:.4f} |")
