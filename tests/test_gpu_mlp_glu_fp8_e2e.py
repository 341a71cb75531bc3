"""SparseDiffGatedMlp over F8Linear projections on the device against the fp64 model of the sparse-delta method for gated feed-forwards
(tests/glu_fp8_method_model.py, tests/glu_method_model.py).  The model takes the module's own quantised operands -- x_q times the layer's
reciprocal input scale, W_q times its reciprocal weight scale -- so quantisation error is not counted, as on the ungated fp8 route.

Two layers, K = 256, F = 1024, 13 steps of glu_method_model.SCHEDULE (full steps 0 and 10, a selection kept at step 11).  Routes: SiLU without
biases over two F8Linear layers at N = 1003 tokens, B = 1 (ragged last group, pitched cache); tanh-GELU with biases through `from_fused`
(one [2F, K] F8Linear) at N = 1024, B = 2; the first route again with the activation cache offloaded and not resident, the second again
with mlp.fused_scatter off.  Bounds: MARGIN x GLU_FLOORS for output, invariant, cache and refreshed columns; 2 x GLU_SELECTION_SHORTFALL_FP8 for the selection, a figure measured on
`Fp8GluEmulation`, which runs no chipmunk operator."""
import pytest
import torch

import glu_fp8_method_model as gfp
import glu_method_model as gm

pytestmark = pytest.mark.gpu
OFFLOADED = {"global_disable_offloading": False, "mlp.sparse_act_T": True, "keep_resident_if_fits": False}


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    assert torch.cuda.is_available()
    a = torch.zeros(16, gfp.K, device="cuda:0").to(torch.float8_e4m3fn)
    b = torch.zeros(gfp.F, gfp.K, device="cuda:0").to(torch.float8_e4m3fn)
    one = torch.ones((), device="cuda:0")
    try:        # torch's own fp8 GEMM, called as F8Linear calls it: its support varies with the ROCm build; nothing of the project runs here
        torch._scaled_mm(a, b.T, scale_a=one, scale_b=one, bias=torch.zeros(gfp.F, device="cuda:0", dtype=torch.bfloat16),
                         out_dtype=torch.bfloat16, use_fast_accum=True)
    except (RuntimeError, NotImplementedError) as e:
        pytest.skip(f"torch._scaled_mm fp8 unavailable here: {e}")
    ot.gpu_tensors.clear()
    saved = ot._resident_bytes, ot._kept_offloaded_bytes
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    ot.gpu_tensors.clear()
    ot._resident_bytes, ot._kept_offloaded_bytes = saved


def module_factory(counter):
    from chipmunk_amd.modules import SparseDiffGatedMlp

    def make(layer, projs, fc2, fused, act):
        if fused is None:
            return SparseDiffGatedMlp(layer, counter, projs[0], projs[1], gm.act_module(act), fc2, 6)
        return SparseDiffGatedMlp.from_fused(layer, counter, projs[0], gm.act_module(act), fc2, gate_first=fused)
    return make


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


@pytest.mark.parametrize("route,res,fused_scatter", [("silu_n1003", "resident", True), ("gelu_tanh_bias_fused_b2", "resident", True),
                                                     ("silu_n1003", "offloaded", True), ("gelu_tanh_bias_fused_b2", "resident", False)],
                         ids=["silu n1003", "gelu_tanh bias fused b2", "silu n1003 offloaded", "gelu_tanh bias fused b2 separate scatter"])
def test_gated_fp8_modules_against_the_method_model(dev, fresh_config, route, res, fused_scatter):
    from chipmunk_amd.util.layer_counter import LayerCounter
    gm.configure(fresh_config, OFFLOADED if res == "offloaded" else None, fused_scatter)
    what = f"glu fp8 {route}, {'fused' if fused_scatter else 'separate'} scatter, {res}"
    chk = gfp.run_route(route, dev, module_factory(LayerCounter(gfp.LAYERS, 1)), floors=gfp.GLU_FLOORS,
                        eps=2 * gfp.GLU_SELECTION_SHORTFALL_FP8, what=what)
    report(what, chk)
    assert ("output", 9) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    assert all(m.fp8 for m in chk.modules)
    holder = chk.modules[0].storage.sparse_act_T
    assert holder.is_resident() == (res == "resident")
