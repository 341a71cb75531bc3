"""SparseDiffMlp over an MXFP4 ``W4Linear`` ``fc1`` on the device: its outputs equal, bit for bit, those of the same module over an ``nn.Linear``
holding ``widened()`` -- tests/method_model.py's `flux` schedule at N = 1003 (a dense layer, full and sparse steps), ``mlp.fused_scatter`` on / off."""
import pytest
import torch

import method_model as mm
from test_gpu_mlp_w8_e2e import dev, widened_linear  # noqa: F401  (the fixture: fresh config, empty offload registry)

pytestmark = pytest.mark.gpu


def run_route(n, device, mxfp4, fused):      # the outputs of every call; the sparse layers' fc1 a W4Linear, or the nn.Linear over its widened weight
    from chipmunk_amd.modules import SparseDiffMlp, W4Linear
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    torch.cuda.synchronize()
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)
    ot.gpu_tensors.clear()
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    n_inv, steps, _every, _cache = mm.configure_mlp(cfg.GLOBAL_CONFIG, "flux")
    cfg.GLOBAL_CONFIG["offloading"].update({"global_disable_offloading": True})
    cfg.GLOBAL_CONFIG["mlp"]["fused_scatter"] = fused
    counter, gelu, mods, outs = lc.LayerCounter(mm.MLP_LAYERS, 1), torch.nn.GELU(approximate="tanh"), [], []
    for li in range(mm.MLP_LAYERS):
        torch.manual_seed(li)
        fc1, fc2 = torch.nn.Linear(mm.MLP_K, mm.MLP_F).to(device).bfloat16(), torch.nn.Linear(mm.MLP_F, mm.MLP_K).to(device).bfloat16()
        if li >= mm.MLP_DENSE_LAYERS:
            q = W4Linear.from_linear(fc1)
            fc1 = q if mxfp4 else widened_linear(q)
        mods.append(SparseDiffMlp(li, counter, fc1, gelu, fc2, 6))
    mm.drive(mods, n_inv, steps, lambda step, inv, li: (mm.mlp_input(step, inv, li, n, mm.MLP_K).to(device),),
             lambda step, inv, li, mod, args, out: outs.append(out.clone()))
    return outs


@pytest.mark.parametrize("fused", [True, False])
def test_module_outputs_are_those_of_the_widened_bf16_module(dev, fused):
    got, ref = run_route(1003, dev, True, fused), run_route(1003, dev, False, fused)
    assert len(got) == len(ref) == mm.MLP_ROUTES["flux"][1] * mm.MLP_LAYERS
    for i, (o, r) in enumerate(zip(got, ref)):
        assert torch.equal(o.view(torch.int16), r.view(torch.int16)), f"call {i} (step {i // mm.MLP_LAYERS}, layer {i % mm.MLP_LAYERS}): outputs differ"
