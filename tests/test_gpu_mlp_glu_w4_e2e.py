"""SparseDiffGatedMlp over MXFP4 ``W4Linear`` projections (``mlp.mxfp4_gated``): two layers, or one fused layer with the gate in either half;
``fc2`` bf16 or a ``W4LinearT``.  Every output equals, bit for bit, that of the same module over ``nn.Linear`` layers holding the widened weights --
tests/method_model.py's `flux` schedule at N = 1003, ``mlp.fused_scatter`` on / off."""
import pytest
import torch

import method_model as mm
from test_gpu_mlp_w8_e2e import dev, widened_linear  # noqa: F401  (the fixture: fresh config, empty offload registry)

pytestmark = pytest.mark.gpu


def run_route(n, device, source, w4_fc2, mxfp4, fused):      # the outputs of every call; the sparse layers in MXFP4, or nn.Linear over the widened weights
    from chipmunk_amd.modules import SparseDiffGatedMlp, W4Linear, W4LinearT
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
    cfg.GLOBAL_CONFIG["mlp"].update(fused_scatter=fused, mxfp4_gated=True, mxfp4_fc2=True)
    counter, silu, mods, outs = lc.LayerCounter(mm.MLP_LAYERS, 1), torch.nn.SiLU(), [], []
    linear = lambda i, o: torch.nn.Linear(i, o).to(device).bfloat16()      # noqa: E731
    for li in range(mm.MLP_LAYERS):
        torch.manual_seed(li)
        projs = [linear(mm.MLP_K, mm.MLP_F), linear(mm.MLP_K, mm.MLP_F)] if source == "two layers" else [linear(mm.MLP_K, 2 * mm.MLP_F)]
        fc2 = linear(mm.MLP_F, mm.MLP_K)
        if li >= mm.MLP_DENSE_LAYERS:
            quant = [W4Linear.from_linear(lin) for lin in projs]
            projs = quant if mxfp4 else [widened_linear(q) for q in quant]
            if w4_fc2:
                q2 = W4LinearT.from_linear(fc2)
                if mxfp4:
                    fc2 = q2
                else:
                    fc2.weight.data.copy_(q2.widened())      # the nn.Linear over the widened weight
        if source == "two layers":
            mods.append(SparseDiffGatedMlp(li, counter, *projs, silu, fc2, 6))
        else:
            mods.append(SparseDiffGatedMlp.from_fused(li, counter, projs[0], silu, fc2, gate_first=source == "fused, gate first"))
    mm.drive(mods, n_inv, steps, lambda step, inv, li: (mm.mlp_input(step, inv, li, n, mm.MLP_K).to(device),),
             lambda step, inv, li, mod, args, out: outs.append(out.clone()))
    assert all(m.w4 == mxfp4 and m.gate[0].dtype == (torch.uint8 if mxfp4 else torch.bfloat16) for m in mods[mm.MLP_DENSE_LAYERS:])
    return outs


@pytest.mark.parametrize("fused", [True, False], ids=["fused scatter", "scatter-add kernel"])
@pytest.mark.parametrize("w4_fc2", [False, True], ids=["bf16 fc2", "W4LinearT fc2"])
@pytest.mark.parametrize("source", ["two layers", "fused, gate first", "fused, up first"])
def test_module_outputs_are_those_of_the_widened_bf16_module(dev, source, w4_fc2, fused):
    got, ref = run_route(1003, dev, source, w4_fc2, True, fused), run_route(1003, dev, source, w4_fc2, False, fused)
    assert len(got) == len(ref) == mm.MLP_ROUTES["flux"][1] * mm.MLP_LAYERS
    for i, (o, r) in enumerate(zip(got, ref)):
        assert torch.equal(o.view(torch.int16), r.view(torch.int16)), f"call {i} (step {i // mm.MLP_LAYERS}, layer {i % mm.MLP_LAYERS}): outputs differ"
