"""The gated feed-forward path without a GPU (tests/glu_method_model.py):

* the bf16 stand-ins pass the bounds the GPU tests assert -- the operator mirror the bound of tests/test_gpu_mlp_glu.py (fp32 torch under
  assert_close_bf16's defaults), the module emulation the bounds of tests/test_gpu_mlp_glu_e2e.py -- and every mutant exceeds them on the
  same inputs (halves swapped, activation applied to the product, cache subtracted before the product, up bias dropped, block means of
  the gate branch alone scored, block means of the up rows not copied);
* (the gated GEMM1 kernels compile for gfx950 without spills or scratch, six instantiations: tests/test_mlp_mm1_form_audit.py;)
* the fake kernel traces without a GPU and the C ABI lists the two new entries."""
import os
import re

import pytest
import torch

import glu_method_model as gm
import method_model as mm
from helpers import assert_close_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ operator mirror
OP_MUTANTS = ("halves_swapped", "act_on_product", "cache_before_product", "up_bias_dropped")


def _operator_problem(seed=334):
    """the second shape of the GPU operator test (M = 333, counts F / 0 / 336), on the CPU"""
    M, k, f, counts = 333, 256, 512, [512, 0, 336]
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape, scale: (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)   # noqa: E731
    p = dict(a=rnd(M, k, scale=0.5), wg=rnd(f, k, scale=0.06), wu=rnd(f, k, scale=0.06), bg=rnd(f, scale=0.1), bu=rnd(f, scale=0.1),
             cache=rnd(f, M, scale=0.3), inds=torch.stack([torch.randperm(f, generator=g) for _ in range(3)]).to(torch.int32),
             counts=torch.tensor(counts, dtype=torch.int32))
    return p


def _operator_check(p, act, c):
    """the assertions of test_every_group_against_fp32_torch on packed deltas `c`"""
    act32 = {"gelu_tanh": lambda x: torch.nn.functional.gelu(x, approximate="tanh"), "silu": torch.nn.functional.silu,
             "gelu": torch.nn.functional.gelu}[act]
    h = act32(p["a"].float() @ p["wg"].float().T + p["bg"].float()) * (p["a"].float() @ p["wu"].float().T + p["bu"].float())
    for g in range(3):
        rows, n = slice(g * 128, min(333, (g + 1) * 128)), int(p["counts"][g])
        cols = p["inds"][g, :n].long()
        assert (c[rows, n:] == 7.0).all()
        if n:
            assert_close_bf16(c[rows, :n], h[rows][:, cols] - p["cache"][cols][:, rows].float().T, what=f"group {g}")


@pytest.mark.parametrize("act", gm.ACTS)
def test_operator_mirror_passes_the_operator_bound_and_every_mutant_exceeds_it(act):
    p = _operator_problem()
    args = (p["a"], p["wg"], p["wu"], p["bg"], p["bu"], act, p["cache"], p["inds"], p["counts"])
    _operator_check(p, act, gm.mm1_glu_mirror(*args))
    for defect in OP_MUTANTS:
        with pytest.raises(AssertionError, match="elements off"):
            _operator_check(p, act, gm.mm1_glu_mirror(*args, defect=defect))


# ------------------------------------------------------------------------------------------------------------------ module emulation
@pytest.fixture(scope="module")
def runs():
    """route -> (checker over `GluEmulation` with the GPU test's assertions in force, trace of (step, layer, x, selection))"""
    out = {}
    for route in gm.ROUTES:
        trace = []
        out[route] = (gm.run_route(route, torch.device("cpu"), lambda li, w, act: gm.GluEmulation(w, act, gm.SCHEDULE, 0),
                                   floors=gm.GLU_FLOORS, eps=2 * gm.GLU_SELECTION_SHORTFALL, what=f"emulation {route}", trace=trace), trace)
    return out


@pytest.mark.parametrize("route", list(gm.ROUTES))
def test_emulation_holds_the_module_bounds(runs, route):
    """(asserted while the fixture ran: every call of every layer under MARGIN x floor, the cache bits outside the selection, the selection
    within 2 x the shortfall of the exact top-|S|)"""
    chk, trace = runs[route]
    assert ("output", 9) in chk.worst and ("refreshed", 1) in chk.worst and 0 < chk.shortfall <= 2 * gm.GLU_SELECTION_SHORTFALL
    kept = [r["step"] for r in trace if r["layer"] == 0 and r["sel"] is not None]
    assert kept == [s for s in range(gm.STEPS) if s % 10], "every step that is not a full step runs from a stored selection"
    for (name, ns), val in sorted(chk.worst.items()):
        bound = mm.MARGIN * gm.GLU_FLOORS[name][min(ns, max(gm.GLU_FLOORS[name]))]
        print(f"{route}: {name} after {ns} sparse steps {val:.5f} (bound {bound:.5f})")
        assert val <= bound


def _replay(route, trace, defect):
    """The mutant and the healthy model over the recorded inputs and selections (sequence 0); per assertion the worst ``error / bound`` of
    the mutant, rounded to bf16 where the module rounds, under the checker's own comparison."""
    act, bias, _ = gm.ROUTES[route]
    weights = [gm.glu_weights(li, bias) for li in range(gm.LAYERS)]
    every, cache = gm.SCHEDULE["full_step_every"], gm.SCHEDULE["block_mask_cache"]
    good, bad = gm.GluMethodModel(weights, act, every, cache), gm.GluMethodModel(weights, act, every, cache, defect=defect)
    ratios = {}
    for rec in trace:
        w2, b2 = weights[rec["layer"]][4:]
        sel = None if rec["sel"] is None else (rec["sel"][0][0], rec["sel"][1][0])
        args = (rec["step"], 0, rec["layer"], rec["x"][0], sel)
        res, mut = good.step(*args), bad.step(*args)
        chk = gm.GluChecker(good, weights, gm.N)
        chk.check_values(res, gm.bf(mut["o"]), gm.bf(mut["a"]), gm.bf(mut["o"]), w2, b2, "")
        for (name, ns), err in chk.worst.items():
            mm.record(ratios, name, err / (mm.MARGIN * gm.GLU_FLOORS[name][min(ns, max(gm.GLU_FLOORS[name]))]))
        if res["weight"] is not None:
            # what the method's top-k makes of the mutant's score, weighed with the healthy model's
            inds, counts = gm.topk_rows(gm.bf(mut["weight"]), 1 - gm.SCHEDULE["top_keys"], gm.SCHEDULE["counts_multiple_of"])
            short = 1.0 - min(mm.captured_fraction(res["weight"], inds, counts, gm.PASSED))
            mm.record(ratios, "selection", short / (2 * gm.GLU_SELECTION_SHORTFALL))
    return ratios


# mutant -> (route, assertions that must reject it, assertions that cannot see it)
MUTANTS = {
    "halves_swapped": ("silu", ("output", "cache", "refreshed"), ("selection",)),
    "act_on_product": ("silu", ("output", "cache", "refreshed"), ("selection",)),
    "cache_before_product": ("silu", ("output", "cache", "refreshed"), ("selection",)),
    "up_bias_dropped": ("gelu_tanh_bias", ("output", "cache", "refreshed"), ("selection",)),
    "gate_means_only": ("silu", ("selection",), ("output", "invariant", "cache", "refreshed")),
    "up_means_not_copied": ("silu", ("selection",), ("output", "invariant", "cache", "refreshed")),
}


def test_every_defect_of_the_model_has_a_mutant():
    assert set(MUTANTS) == set(gm.GLU_DEFECTS)


@pytest.mark.parametrize("defect", list(MUTANTS))
def test_module_mutant_is_rejected_and_inert_pairs_are_inert(runs, defect):
    route, counted, inert = MUTANTS[defect]
    ratios = _replay(route, runs[route][1], defect)
    print(f"mutant {defect} on {route}: " + ", ".join(f"{k} {v:.2f} x bound" for k, v in sorted(ratios.items())))
    for name in counted:      # the project's separation: margin x floor stays under half of every counted mutant's error
        assert ratios[name] >= 2.0, f"{defect} is not twice outside the {name} assertion: {ratios[name]:.3f} x the bound"
    for name in inert:
        assert ratios.get(name, 0.0) <= 1.0, f"{defect} is listed as inert for {name} but is rejected there ({ratios[name]:.3f} x the bound)"


# ------------------------------------------------------------------------------------------------------------------ plumbing
def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16 = torch.bfloat16
        a, w, c = torch.empty(2, 333, 256, dtype=bf16), torch.empty(512, 256, dtype=bf16), torch.empty(2, 333, 512, dtype=bf16)
        cache = torch.empty(2, 512, 336, dtype=bf16)[..., :333]
        inds, counts = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        assert torch.ops.chipmunk.csp_mlp_mm1_glu(a, w, w, c, None, None, cache, inds, counts, "silu", True) is None
        assert torch.ops.chipmunk.csp_mlp_mm1_glu(a[0], w, w, c[0], w[:, 0], None, cache[0], inds[0], counts[0], "gelu", False) is None
        with pytest.raises(RuntimeError, match="c must be"):
            torch.ops.chipmunk.csp_mlp_mm1_glu(a, w, w, c[0], None, None, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="unknown activation"):
            torch.ops.chipmunk.csp_mlp_mm1_glu(a, w, w, c, None, None, cache, inds, counts, "relu", True)


def test_abi_lists_the_gated_entries_and_refuses_bad_arguments():
    import ctypes
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    for name in ("chipmunk_csp_mlp_mm1_glu", "chipmunk_csp_mlp_mm1_glu_batched"):
        assert name in _native.SYMBOLS and re.search(rf"\b{name}\s*\(", header)
    for const, val in (("CHIPMUNK_ACT_GELU_TANH", 0), ("CHIPMUNK_ACT_SILU", 1), ("CHIPMUNK_ACT_GELU_ERF", 2)):
        assert re.search(rf"#define {const} {val}\b", header)
    lib, p, null = _native.lib(), ctypes.c_void_p(16), ctypes.c_void_p(0)

    def call(a=p, M=128, K=64, F=256, ldc=128, act=1, upd=0):
        return lib.chipmunk_csp_mlp_mm1_glu(a, p, p, p, null, null, p, p, p, M, K, F, ldc, act, upd, null), _native.last_error()
    for kw, text in ((dict(a=null), "null"), (dict(act=3), "unknown activation"), (dict(upd=2), "update_cache"), (dict(K=96), "multiple of 64"),
                     (dict(M=100, ldc=100), "pitch"), (dict(ldc=120), "pitch")):
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    rc = lib.chipmunk_csp_mlp_mm1_glu_batched(p, p, p, p, null, null, p, p, p, 100, 64, 256, 104, 1, 0, 2, ctypes.c_int64(100), null)
    assert rc == 1 and "batch stride" in _native.last_error()
    rc = lib.chipmunk_csp_mlp_mm1_glu_batched(p, p, p, p, null, null, p, p, p, 100, 64, 256, 104, 1, 0, 0, ctypes.c_int64(256 * 104), null)
    assert rc == 1 and "batch size" in _native.last_error()


def test_module_refuses_what_the_sparse_steps_cannot_honour():
    """construction only: no operator runs"""
    import chipmunk_amd  # noqa: F401
    from chipmunk.modules import SparseDiffGatedMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    lin = torch.nn.Linear
    counter = LayerCounter(1, 1)
    for act, code in ((torch.nn.SiLU(), "silu"), (torch.nn.GELU(approximate="tanh"), "gelu_tanh"), (torch.nn.GELU(), "gelu")):
        assert SparseDiffGatedMlp(0, counter, lin(64, 128, bias=False), lin(64, 128), act, lin(128, 64)).act_code == code
    for act in (torch.nn.ReLU(), torch.nn.Sigmoid(), "swish"):
        with pytest.raises(ValueError, match="unsupported activation"):
            SparseDiffGatedMlp(0, counter, lin(64, 128), lin(64, 128), act, lin(128, 64))
    with pytest.raises(ValueError, match="one shape"):
        SparseDiffGatedMlp(0, counter, lin(64, 128), lin(64, 192), torch.nn.SiLU(), lin(128, 64))
    fc1 = lin(64, 256)
    m = SparseDiffGatedMlp.from_fused(0, counter, fc1, torch.nn.SiLU(), lin(128, 64), gate_first=False)
    assert m.gate[0].data_ptr() == fc1.weight.data[128:].data_ptr() and m.up[1].data_ptr() == fc1.bias.data.data_ptr()
    # the parameters are read at every call: casting the Linear modules after wrapping rebinds param.data, and the module follows
    fc2 = m.fc2[0]
    before = m.fc2w_T
    assert m.fc2w_T is before, "the transposed fc2 weight is made once per weight tensor"
    fc1.double(), fc2.double()
    assert m.gate[0].dtype == torch.float64 and m.gate[0].data_ptr() == fc1.weight.data[128:].data_ptr()
    assert m.fc2w_T.dtype == torch.float64 and torch.equal(m.fc2w_T, fc2.weight.data.T)
    fc1.float(), fc2.float()
    # mlp.is_enabled off: the dense gated feed-forward
    from chipmunk_amd.util import config as cfg
    cfg.reset_to_base()
    try:
        cfg.GLOBAL_CONFIG["mlp"]["is_enabled"] = False
        x = torch.randn(1, 5, 64)
        g, u = x @ fc1.weight[128:].T + fc1.bias[128:], x @ fc1.weight[:128].T + fc1.bias[:128]
        assert torch.allclose(m(x), m.fc2[0](torch.nn.functional.silu(g) * u), atol=1e-6)
    finally:
        cfg.reset_to_base()
