"""fp8 row scales on the host (no GPU): the quantiser's chain on planted rows, F8Linear's row mode (weight scales, state dict, forward),
the config key and the three refusals, the new symbols / schema / fake kernels, and the fp32 mirror of the new GEMM1 epilogue against
fp64 with the four mutants the GPU bound has to reject (tests/mlp_rowscale_model.py).

Measured here (printed by test_the_mirror_floor_and_the_mutants): over the 18 cases x update none / store / scatter the mirror's worst
segment error is 0.0034 (packed deltas 0.0022; refreshed cache columns 0.0034, the stored bf16 activation of a 24-column segment), at
ORACLE_MLP_SEG_ERR = 0.0035 and under it, so the GPU test asserts the shipped MLP_SEG_BOUND = 0.007, a factor two above; the weakest
mutant of every kind lies at 0.55 or above (next row's scale 1.19, scale_a[0] 0.82, packed position 0.90, scale after the bias 0.56)."""
import os
import re

import pytest
import torch

import mlp_act_model as am
import mlp_rowscale_model as rm
from helpers import F8, MLP_SEG_BOUND, ORACLE_MLP_SEG_ERR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E5M2 = torch.float8_e5m2
NEW_SYMBOLS = ["chipmunk_quantize_fp8_rowwise", "chipmunk_csp_mlp_mm1_fp8_act_rs", "chipmunk_csp_mlp_mm1_fp8_act_rs_batched"]


def lin(i, o, bias=True):
    return torch.nn.Linear(i, o, bias=bias).bfloat16()


def f8(i, o, **kw):
    from chipmunk_amd.modules import F8Linear
    return F8Linear.from_linear(lin(i, o), **dict(dict(input_float8_dtype=F8), **kw))


# ------------------------------------------------------------------------------------------------------------------ ABI, schema, fakes
def test_the_new_entries_are_declared_exported_and_listed():
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in _native.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name)


def test_the_c_entries_refuse_bad_arguments_with_a_message():
    import ctypes
    from chipmunk_amd import _native
    lib = _native.lib()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    q = lambda x, K, rows=4: lib.chipmunk_quantize_fp8_rowwise(x, p, p, ctypes.c_int64(rows), K, ctypes.c_float(448.0), null)      # noqa: E731
    assert q(null, 128) == 1 and "null" in _native.last_error()
    assert q(p, 24) == 1 and "multiple of 16" in _native.last_error()
    assert q(p, 16384 + 16) == 1 and "16384" in _native.last_error()
    assert q(ctypes.c_void_p(4096 + 8), 128) == 1 and "aligned" in _native.last_error()
    assert q(p, 128, rows=0) == 0
    rs = lambda sa, act=0, upd=0, K=128: lib.chipmunk_csp_mlp_mm1_fp8_act_rs(p, p, p, null, p, p, p, sa, p, 200, K, 256, 200, act, upd, null)   # noqa: E731
    assert rs(null) == 1 and "null" in _native.last_error()
    assert rs(ctypes.c_void_p(4098)) == 1 and "4-byte aligned" in _native.last_error()
    assert rs(p, act=7) == 1 and "unknown activation" in _native.last_error()
    assert rs(p, upd=3) == 1 and "update_cache" in _native.last_error()
    assert rs(p, K=64) == 1 and "multiple of 128" in _native.last_error()


def test_schema_and_fake_kernels():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs.default._schema) == (
        "chipmunk::csp_mlp_mm1_fp8_act_rs(Tensor a, Tensor b, Tensor(c!) c, Tensor? bias, Tensor(pa!) pa_cache, Tensor indices, Tensor counts, "
        "Tensor scale_a, Tensor scale_b, str act, int update_cache) -> ()")
    with FakeTensorMode():
        x = torch.empty(2, 200, 128, dtype=torch.bfloat16)
        xq, recip = torch.ops.chipmunk.quantize_fp8_rowwise(x, 448.0)
        assert xq.shape == x.shape and xq.dtype == F8 and recip.shape == (2, 200) and recip.dtype == torch.float32
        a, w = torch.empty(200, 128, dtype=F8), torch.empty(256, 128, dtype=F8)
        c, cache = torch.empty(200, 256, dtype=torch.bfloat16), torch.empty(256, 200, dtype=torch.bfloat16)
        inds, cnt = torch.empty(2, 256, dtype=torch.int32), torch.empty(2, dtype=torch.int32)
        sa, sb = torch.empty(200), torch.empty(256)
        op = torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs
        op(a, w, c, None, cache, inds, cnt, sa, sb, "silu", 2)
        for bad_a, bad_b in ((torch.empty(1), sb), (sa, torch.empty(1)), (sa.double(), sb), (torch.empty(2, 100), sb), (sa, torch.empty(256, 1))):
            with pytest.raises(RuntimeError):
                op(a, w, c, None, cache, inds, cnt, bad_a, bad_b, "silu", 2)


# ------------------------------------------------------------------------------------------------------------------ quantiser chain
def test_the_quantiser_chain_on_planted_rows():
    """an all-zero row, a row whose amax lies below 1e-12 * 448, a row with one element of 3e38, a row of e4m3 rounding ties: the chain of
    tests/mlp_rowscale_model.quantize_chain, and F8Linear.quantize_input_rowwise (the torch route on the CPU) gives its bits"""
    K = 32
    x = torch.zeros(5, K)
    x[1] = torch.linspace(-1, 1, K) * 1e-10                 # amax 1e-10 < 448e-12: the scale saturates at 448
    x[2] = torch.linspace(-2, 2, K)
    x[2, 7] = 3e38
    x[3] = torch.linspace(-3, 3, K)
    x[4] = rm.quantizer_rows(1, K, 0)[0].float()
    x = x.to(torch.bfloat16)
    out, recip = rm.quantize_chain(x)
    f = out.float()
    assert recip.dtype == torch.float32 and torch.isfinite(recip).all() and not torch.isnan(f).any()
    assert (f[0] == 0).all() and recip[0] == 1.0 / torch.tensor(448.0)
    assert (f[1] == 0).all() and recip[1] == 1.0 / torch.tensor(448.0)                       # 448e-10 is under half of e4m3's 2^-9
    assert f[2, 7] == 448.0 and (f[2, :7] == 0).all() and (f[2, 8:] == 0).all()
    assert recip[2] == 1.0 / (torch.tensor(448.0) / x[2, 7].float())
    assert f[3].abs().max() == 448.0 and recip[3] == 1.0 / (torch.tensor(448.0) / torch.tensor(3.0))
    # ties to even, both signs, the subnormal binade included
    want = torch.tensor([448.0, 16.0, -20.0, 20.0, -24.0, 0.5, -0.5, 0.0, -0.0, 2.0 ** -8, 28.0, -28.0, 1.0, -1.25, 10.0, -10.0])
    assert recip[4] == 1.0 and torch.equal(f[4, :16], want)
    layer = f8(K, 8, scaling="row")
    xq, r = layer.quantize_input_rowwise(x.reshape(1, 5, K))
    assert xq.shape == (1, 5, K) and r.shape == (1, 5) and r.dtype == torch.float32
    assert torch.equal(xq[0].view(torch.uint8), out.view(torch.uint8)) and torch.equal(r[0], recip)
    with pytest.raises(RuntimeError, match="quantize_input_rowwise"):
        layer.quantize_input(x)
    with pytest.raises(RuntimeError, match="quantize_input"):
        f8(K, 8).quantize_input_rowwise(x)


# ------------------------------------------------------------------------------------------------------------------ F8Linear
def test_weight_scales_are_per_output_feature():
    torch.manual_seed(3)
    base = lin(64, 48)
    with torch.no_grad():
        base.weight.mul_(torch.logspace(0, 5, 48)[:, None].to(torch.bfloat16))        # output features five decades apart
    w = base.weight.data.float()
    row = f8_from(base, "row")
    assert row.scaling == "row" and row.scale.shape == (48, 1) and row.scale_reciprocal.shape == (48, 1) and row.scale.dtype == torch.float32
    want = (448.0 / w.abs().amax(dim=1, keepdim=True).clamp(min=1e-12)).clamp(max=448.0)
    assert torch.equal(row.scale, want) and torch.equal(row.scale_reciprocal, want.reciprocal())
    assert torch.equal(row.weight.data.view(torch.uint8), (w * want).clamp(-448.0, 448.0).to(F8).view(torch.uint8))
    full = w.abs().amax(dim=1) >= 1.0                                                 # (below that the scale saturates at 448)
    assert full.sum() > 30 and (row.weight.data.float().abs().amax(dim=1)[full] == 448.0).all()      # every such feature uses the whole range
    ten = f8_from(base, "tensor")
    assert ten.scaling == "tensor" and ten.scale.dim() == 0
    # the smallest feature survives row scaling and is crushed by the tensor's one scale
    deq = lambda m: m.weight.data.float() * m.scale_reciprocal      # noqa: E731
    err = lambda m: float((deq(m)[0] - w[0]).norm() / w[0].norm())  # noqa: E731
    assert err(row) < 0.05 < err(ten)
    with pytest.raises(ValueError, match="unknown scaling"):
        f8_from(base, "column")


def f8_from(linear, scaling):
    from chipmunk_amd.modules import F8Linear
    return F8Linear.from_linear(linear, input_float8_dtype=F8, scaling=scaling)


def test_forward_in_row_mode_is_the_documented_formula():
    torch.manual_seed(4)
    layer = f8(64, 48, scaling="row")
    x = (torch.randn(2, 5, 64) * torch.logspace(-1, 1, 5)[None, :, None]).to(torch.bfloat16)
    xq, sa = rm.quantize_chain(x.reshape(-1, 64))
    want = (xq.double() @ layer.weight.data.double().T) * sa.double()[:, None] * layer.scale_reciprocal.double().T + layer.bias.data.double()
    got = layer(x)
    assert got.dtype == torch.bfloat16 and got.shape == (2, 5, 48)
    torch.testing.assert_close(got.reshape(-1, 48).double(), want, atol=2e-2, rtol=2e-2)
    assert layer.input_scale is None and layer.trial_index == 0          # no calibration, nothing frozen


def test_state_dict_round_trips_of_both_granularities():
    from chipmunk_amd.modules import F8Linear
    torch.manual_seed(5)
    x = torch.randn(7, 64).to(torch.bfloat16)
    for scaling, n in (("row", 48), ("tensor", 1)):
        src = f8(64, 48, scaling=scaling)
        sd = src.state_dict()
        assert sd["scale"].numel() == n and sd["weight"].dtype == F8
        for built_as in ("tensor", "row"):      # the checkpoint's granularity decides, whatever the layer was built as
            dst = F8Linear(64, 48, dtype=torch.bfloat16, input_float8_dtype=F8, scaling=built_as)
            dst.load_state_dict(sd)
            assert dst.scaling == scaling and dst.scale.shape == src.scale.shape
            assert torch.equal(dst.weight.data.view(torch.uint8), src.weight.data.view(torch.uint8))
            assert torch.equal(dst.scale_reciprocal, src.scale_reciprocal)
            if scaling == "row":
                assert torch.equal(dst(x), src(x))
    # a float weight is quantised per the layer's mode
    base = lin(64, 48)
    for scaling in ("row", "tensor"):
        dst = F8Linear(64, 48, dtype=torch.bfloat16, input_float8_dtype=F8, scaling=scaling)
        dst.load_state_dict(base.state_dict())
        assert dst.scaling == scaling and dst.weight.dtype == F8 and dst.scale.numel() == (48 if scaling == "row" else 1)
        assert torch.equal(dst.weight.data.view(torch.uint8), f8_from(base, scaling).weight.data.view(torch.uint8))
    bad = dict(f8(64, 48, scaling="row").state_dict())
    bad["scale"] = bad["scale"][:7]
    with pytest.raises(RuntimeError, match="one scale, or one per output feature"):
        F8Linear(64, 48, dtype=torch.bfloat16).load_state_dict(bad)


# ------------------------------------------------------------------------------------------------------------------ config, refusals
def _block():
    blk = torch.nn.Module()
    blk.img_mlp = torch.nn.Sequential(lin(64, 128), torch.nn.GELU(approximate="tanh"), lin(128, 64))
    blk.txt_mlp = torch.nn.Sequential(lin(64, 128), torch.nn.GELU(approximate="tanh"), lin(128, 64))
    return blk


def test_the_key_defaults_to_tensor_and_recursive_swap_linears_passes_it(fresh_config, capsys):
    from chipmunk_amd.modules import F8Linear
    from chipmunk_amd.modules.mlp_fp8 import recursive_swap_linears
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.fp8_scaling"] == "tensor" and cfg.BASE_CONFIG["mlp"]["fp8_scaling"] == "tensor"
    assert cfg.amd_key("mlp", "fp8_scaling") == "tensor"
    torch.manual_seed(6)
    blk = _block()
    want = {n: f8_from(m, "tensor") for n, m in (("i0", blk.img_mlp[0]), ("t0", blk.txt_mlp[0]), ("t2", blk.txt_mlp[2]))}
    recursive_swap_linears(blk)
    # the layers it builds today: per-tensor scales, fc2 of the sparse image MLP left in bf16
    for n, m in (("i0", blk.img_mlp[0]), ("t0", blk.txt_mlp[0]), ("t2", blk.txt_mlp[2])):
        assert isinstance(m, F8Linear) and m.scaling == "tensor" and m.scale.dim() == 0 and torch.equal(m.scale, want[n].scale)
        assert torch.equal(m.weight.data.view(torch.uint8), want[n].weight.data.view(torch.uint8))
    assert not isinstance(blk.img_mlp[2], F8Linear)
    fresh_config["mlp"]["fp8_scaling"] = "row"
    fresh_config["mlp"]["fp8_fc2"] = True
    blk = _block()
    recursive_swap_linears(blk)
    assert blk.img_mlp[0].scaling == "row" and blk.txt_mlp[0].scaling == "row" and blk.txt_mlp[2].scaling == "row"
    assert blk.img_mlp[2].scaling == "tensor" and blk.img_mlp[2].scale.dim() == 0      # GEMM2's gather takes one scale
    blk = _block()
    recursive_swap_linears(blk, scaling="tensor")                                       # the keyword wins over the key
    assert blk.img_mlp[0].scaling == "tensor"
    fresh_config["mlp"]["fp8_scaling"] = "channel"
    with pytest.raises(ValueError, match="mlp.fp8_scaling"):
        recursive_swap_linears(_block())
    capsys.readouterr()


def test_the_modules_refuse_what_has_no_kernel(fresh_config):
    """construction only: a row-scaled fc2, row-scaled gated projections"""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    counter, silu, gelu = LayerCounter(1, 1), torch.nn.SiLU(), torch.nn.GELU(approximate="tanh")
    fresh_config["mlp"]["fp8_fc2"] = True
    row_fc2 = f8(256, 128, scaling="row")
    for make in (lambda: SparseDiffMlp(0, counter, lin(128, 256), gelu, row_fc2),
                 lambda: SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), silu, row_fc2)):
        with pytest.raises(ValueError, match="row-scaled fc2"):
            make()
    fc2 = lin(256, 128)
    for make in (lambda: SparseDiffGatedMlp(0, counter, f8(128, 256, scaling="row"), f8(128, 256, scaling="row"), silu, fc2),
                 lambda: SparseDiffGatedMlp(0, counter, f8(128, 256), f8(128, 256, scaling="row"), silu, fc2),
                 lambda: SparseDiffGatedMlp.from_fused(0, counter, f8(128, 512, scaling="row"), silu, fc2)):
        with pytest.raises(ValueError, match="row-scaled projection"):
            make()
    # what is taken: a row-scaled fc1 of the ungated module, per-tensor everything as before
    SparseDiffMlp(0, counter, f8(128, 256, scaling="row"), gelu, fc2)
    SparseDiffMlp(0, counter, f8(128, 256, scaling="row"), gelu, f8(256, 128))
    SparseDiffGatedMlp(0, counter, f8(128, 256), f8(128, 256), silu, fc2)


def test_ops_mlp_refuses_a_mixed_scale_pair():
    import importlib
    om = importlib.import_module("chipmunk_amd.ops.mlp")       # (chipmunk_amd.ops.mlp, the attribute, is run_e2e)
    M, K, F = 200, 128, 256
    a, w = torch.zeros(M, K).to(F8), torch.zeros(F, K).to(F8)
    c, cache = torch.zeros(M, F, dtype=torch.bfloat16), torch.zeros(F, M, dtype=torch.bfloat16)
    inds, cnt = torch.zeros(2, F, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    one, rows, cols = torch.tensor(1.0), torch.ones(M), torch.ones(F)
    for sa, sb in ((rows, one), (one, cols), (rows, torch.ones(F, 1)), (torch.ones(M - 1), cols), (torch.ones(2, M), cols)):
        with pytest.raises(ValueError, match="mixed pair"):
            om.csp_mlp_mm1_fp8(a, w, None, inds, cnt, cache, c, sa, sb, "silu")
        with pytest.raises(ValueError, match="mixed pair"):
            om.mm1_fp8_scatter(a, w, c, None, cache, inds, cnt, sa, sb, "silu")
    assert om._row_scales("t", a, w, rows, cols) and not om._row_scales("t", a, w, one, one) and not om._row_scales("t", a, w, one.reshape(1), one.reshape(1, 1))
    assert om._row_scales("t", torch.zeros(2, M, K).to(F8), w, torch.ones(2, M), cols)
    with pytest.raises(ValueError, match="unknown activation"):
        om.csp_mlp_mm1_fp8(a, w, None, inds, cnt, cache, c, rows, cols, "relu")


# ------------------------------------------------------------------------------------------------------------------ mirror, mutants
CASES = rm.rs_cases()
UPDATES = ("none", "store", "scatter")


@pytest.fixture(scope="module")
def measured():
    """case -> (problem, exact delta, exact fresh); computed once"""
    out = {}
    for name, args in CASES.items():
        p = rm.rs_problem(**args)
        out[name] = (p, *rm.rs_exact(p))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_inputs_make_a_misplaced_scale_visible(measured, name):
    rm.input_condition(measured[name][0])


def test_the_mirror_floor_and_the_mutants(measured):
    floor_d = floor_c = 0.0
    weakest = {m: float("inf") for m in rm.MUTANTS}
    for name, (p, delta, fresh) in measured.items():
        v = rm.rs_view(p)
        for upd in UPDATES:
            c, cache = rm.rs_mirror(p, upd)
            floor_d = max(floor_d, am.delta_err(v, c, delta, fresh))
            if upd != "none":
                floor_c = max(floor_c, am.assert_act_cache(v, cache, delta, fresh, f"mirror, update {upd} | {name}", accumulate=upd == "scatter"))
        for mut in rm.MUTANTS:
            if mut == rm.AFTER_BIAS and p["bias"] is None:
                continue
            err = am.delta_err(v, rm.rs_mirror(p, "none", mut)[0], delta, fresh)
            weakest[mut] = min(weakest[mut], err)
            assert err > MLP_SEG_BOUND, f"{name}: mutant '{mut}' has segment error {err:.4g}, inside the bound {MLP_SEG_BOUND}"
    print(f"mirror floor: packed deltas {floor_d:.4f}, refreshed cache columns {floor_c:.4f}; weakest mutants "
          + ", ".join(f"{m}: {e:.3g}" for m, e in weakest.items()))
    # the bound's rule (mlp_act_model.act_bound): a floor at or under ORACLE_MLP_SEG_ERR keeps MLP_SEG_BOUND, with its factor two of margin
    assert max(floor_d, floor_c) <= ORACLE_MLP_SEG_ERR and am.act_bound(max(floor_d, floor_c)) == MLP_SEG_BOUND


def test_constant_vectors_give_the_mirror_of_the_scalar_operator(measured):
    """the multiplication order is the scalar form's: with constant vectors the mirror has the bits of mlp_act_model.mm1_act_mirror"""
    p = dict(measured["M203 F128 silu"][0])
    p["sa"], p["sb"] = p["ra"].expand(p["M"]).contiguous(), p["rb"].expand(p["F"]).contiguous()
    for upd in UPDATES:
        c, cache = rm.rs_mirror(p, upd)
        c0, cache0 = am.mm1_act_mirror(rm.rs_view(p), upd)
        assert torch.equal(c.view(torch.int16), c0.view(torch.int16)) and torch.equal(cache.view(torch.int16), cache0.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ outlier tokens
def test_outlier_tokens_the_cpu_mirrors_put_row_scales_ahead_of_one_scale_per_tensor():
    """The inputs of tests/test_gpu_mlp_rowscale_e2e.py's outlier case (one token in sixteen scaled by 64), the quantisation alone: a full
    step's fc2(act(fc1(x))) with an e4m3 fc1 under both granularities against fp64 on the unquantised bf16 MLP.  (A sparse step adds the
    method's own staleness to both alike.)  The error is mlp_rowscale_model.rel_err, the mean over the tokens of the row-relative error.
    Measured: row scales 0.0376 - 0.0383, one scale per tensor 0.0379 - 0.0388, row scales ahead in all eight (layer, step) pairs by
    0.0001 - 0.0005: e4m3 is a floating-point format, a token 64 x below the tensor's amax keeps its three mantissa bits and only its
    smallest elements (under 2^-6 of the scaled range, about 1 % of a normal row) fall into the subnormals."""
    for li in range(am.LAYERS):
        for step in range(rm.E2E_STEPS):
            x = rm.e2e_input(step, li, 1, outliers=True)
            exact = rm.dense_exact(li, True, "gelu_tanh", x)
            row, ten = (rm.rel_err(rm.dense_quantised(li, True, "gelu_tanh", x, s), exact) for s in ("row", "tensor"))
            print(f"layer {li} step {step}: row scales {row:.4f}, one scale per tensor {ten:.4f}")
            assert row < ten
