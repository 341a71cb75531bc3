"""SparseDiffMlp over a row-scaled e4m3 fc1 (F8Linear scaling="row": one dynamic scale per token, one per fc1 column) on the device, and
F8Linear's row-mode forward.

1. The module against the fp64 model of the sparse-delta method (mlp_act_model.ActMethodModel fed the dequantised weight and the
   module's own row-quantised input): two layers, K = 256, F = 1024, N = 200 tokens (two groups, the last of 72 rows), a full step and
   three sparse steps, B = 1 and 2, tanh-GELU and SiLU, mlp.fused_scatter on and off.  Bounds: method_model.MLP_FLOORS x ROW_ERR_MARGIN
   and 2 x MLP_SELECTION_SHORTFALL_FP8, those of the existing fp8 module tests.
2. Outlier tokens (one in sixteen scaled by 64): against the fp64 evaluation of the UNQUANTISED bf16 MLP the row-scaled module's error
   is smaller than the tensor-scaled module's, on every step (the ordering only; tests/test_mlp_rowscale_host.py has it on the CPU
   mirror first).  The fp64 evaluation is the method's (mlp_act_model.ActMethodModel on the unquantised weights and inputs with the
   module's own selections): a full step is the dense MLP, a sparse step keeps the unselected columns of the last steps as the module does,
   so the distance is the quantisation error and not the staleness both modules share (0.32 of the dense MLP at these inputs' drift
   against 0.038 of quantisation error).  The error is the mean over the tokens of the row-relative error.
3. F8Linear.forward in row mode against fp64 on the dequantised operands, atol = rtol = 2e-2."""
import pytest
import torch

import method_model as mm
import mlp_act_model as am
import mlp_rowscale_model as rm
from helpers import F8, assert_close_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    assert torch.cuda.is_available()
    ot.gpu_tensors.clear()
    saved = ot._resident_bytes, ot._kept_offloaded_bytes
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    ot.gpu_tensors.clear()
    ot._resident_bytes, ot._kept_offloaded_bytes = saved


def module_factory():
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    counter = LayerCounter(am.LAYERS, 1)
    acts = {"gelu_tanh": torch.nn.GELU(approximate="tanh"), "silu": torch.nn.SiLU()}
    return lambda layer, fc1, fc2, act: SparseDiffMlp(layer, counter, fc1, acts[act], fc2, 6)


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


@pytest.mark.parametrize("fused", [True, False], ids=["fused scatter", "separate scatter"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("act,bias", [("gelu_tanh", True), ("silu", False)])
def test_row_scaled_module_against_the_method_model(dev, fresh_config, act, bias, B, fused):
    what = f"row scales {act}{'' if bias else ' no bias'} B{B} {'fused' if fused else 'separate'}"
    chk = rm.run_rows(dev, module_factory(), act, bias, B, fused_scatter=fused, floors=mm.MLP_FLOORS, eps=2 * mm.MLP_SELECTION_SHORTFALL_FP8, what=what)
    report(what, chk)
    assert ("output", 3) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    mod = chk.modules[0]
    fc1 = mod.fc1[0]
    assert fc1.scaling == "row" and fc1.scale_reciprocal.shape == (am.F, 1) and fc1.input_scale is None and fc1.trial_index == 0
    assert mod.storage.get_out_cache().shape[0] == B


def test_separate_scatter_gives_the_bits_of_the_fused_one(dev, fresh_config):
    outs = []
    for fused in (True, False):
        from chipmunk_amd.util import config as cfgmod
        from chipmunk_amd.util import layer_counter as lc
        cfgmod.reset_to_base()
        lc.singleton.__init__(0, 0)
        chk = rm.run_rows(dev, module_factory(), "silu", True, 2, fused_scatter=fused)
        st = chk.modules[1].storage
        outs.append([t.clone() for t in (st.get_out_cache(), st.get_sparse_act_T(), st.get_counts())])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


def test_outlier_tokens_row_scales_are_closer_to_the_unquantised_mlp_than_one_scale_per_tensor(dev, fresh_config):
    from chipmunk_amd.util import config as cfgmod
    from chipmunk_amd.util import layer_counter as lc
    errs = {}
    for scaling in ("row", "tensor"):
        cfgmod.reset_to_base()
        lc.singleton.__init__(0, 0)
        chk = rm.run_rows(dev, module_factory(), "gelu_tanh", True, 1, scaling=scaling, outliers=True)
        errs[scaling] = {key: rm.rel_err(out, chk.unquantised[key]) for key, out in chk.outs.items()}
        assert rm.rel_err(chk.unquantised[0, 0], rm.dense_exact(0, True, "gelu_tanh", chk.xs[0, 0])) < 1e-12        # a full step is the dense MLP
    for key in sorted(errs["row"]):
        print(f"outlier tokens, step {key[0]} layer {key[1]}: error against the unquantised MLP, row scales {errs['row'][key]:.4f}, "
              f"one scale per tensor {errs['tensor'][key]:.4f}")
    for key in errs["row"]:
        assert errs["row"][key] < errs["tensor"][key], f"step {key[0]} layer {key[1]}: {errs['row'][key]:.4g} (row) against {errs['tensor'][key]:.4g} (tensor)"


@pytest.mark.parametrize("shape", [(3, 128, 64), (257, 1536, 256)], ids=["3x128", "257x1536 to 256"])
def test_f8linear_forward_in_row_mode(dev, shape):
    from chipmunk_amd.modules import F8Linear
    from chipmunk_amd.modules.mlp_fp8 import scaled_mm_takes_row_scales
    M, K, N = shape
    g = torch.Generator().manual_seed(77 + M)
    lin = torch.nn.Linear(K, N).bfloat16()
    with torch.no_grad():
        lin.weight.mul_(torch.logspace(-1, 1, N)[:, None].to(torch.bfloat16))           # output features two decades apart
    layer = F8Linear.from_linear(lin.to(dev), input_float8_dtype=F8, scaling="row")
    x = (torch.randn(M, K, generator=g) * torch.logspace(-1, 1, M)[:, None]).to(torch.bfloat16).to(dev)      # tokens two decades apart
    xq, sa = layer.quantize_input_rowwise(x)
    want = (xq.double() @ layer.weight.data.double().T) * sa.double()[:, None] * layer.scale_reciprocal.double().T + layer.bias.data.double()
    got = layer(x)
    print(f"F8Linear row-mode forward on {dev}: torch._scaled_mm with [M, 1] / [1, N] scales {'taken' if scaled_mm_takes_row_scales(dev) else 'refused: matmul fallback'}")
    assert got.dtype == torch.bfloat16 and got.shape == (M, N)
    assert_close_bf16(got, want, what=f"F8Linear row-mode forward {shape}")
    assert torch.equal(layer(x.reshape(1, M, K))[0], got)
