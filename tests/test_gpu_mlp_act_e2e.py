"""SparseDiffMlp with SiLU, exact GELU and tanh-GELU, with and without an fc1 bias, on the device against the fp64 model of the
sparse-delta method (tests/mlp_act_model.py: `ActMethodModel`).

The layout of tests/test_gpu_mlp_glu_e2e.py: two layers, K = 256, F = 1024, N = 333 tokens (three groups, the last of 77 rows; a pitched
cache), 13 steps with full_step_every = 10, block_mask_cache = 2, first_n_dense_layers = 0, top_keys = 0.3 and the drifting inputs of
method_model.mlp_input.  After every call: the output, the activation cache, the output cache (against its own activation cache) and
the refreshed columns against the model, which takes the module's own selection; the bits of every cache element outside the
selection; the selection against the exact top-|S| of the model's score.  Bounds: method_model.MLP_FLOORS x ROW_ERR_MARGIN and
2 x MLP_SELECTION_SHORTFALL (2 x MLP_SELECTION_SHORTFALL_FP8 with an e4m3 fc1), the figures of the existing ungated route.

`ActEmulation` (the module's op sequence in torch, no chipmunk operator) runs beside the bf16 routes under the same bounds: a figure
of the module over a floor is a defect unless the emulation exceeds the floor too."""
import pytest
import torch

import mlp_act_model as am
import method_model as mm

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
    from cpu_ops import ExactGELU
    counter = LayerCounter(am.LAYERS, 1)
    # (tanh-GELU through the tests' subclass: activation_code goes by isinstance)
    acts = {"gelu_tanh": ExactGELU(approximate="tanh"), "silu": torch.nn.SiLU(), "gelu": torch.nn.GELU()}
    return lambda layer, fc1, fc2, act: SparseDiffMlp(layer, counter, fc1, acts[act], fc2, 6)


def eps_of(route):
    return 2 * (mm.MLP_SELECTION_SHORTFALL_FP8 if am.ROUTES[route][2] else mm.MLP_SELECTION_SHORTFALL)


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


@pytest.mark.parametrize("route", list(am.ROUTES))
def test_modules_against_the_method_model(dev, fresh_config, route):
    act, bias, fp8, B, offloaded = am.ROUTES[route]
    if fp8:
        from fp8_fc2_method_model import scaled_mm_available
        assert scaled_mm_available(dev) is None, "F8Linear's forward (torch._scaled_mm) does not run here"
    chk = am.run_route(route, dev, module_factory(), floors=mm.MLP_FLOORS, eps=eps_of(route), what=f"act {route}")
    report(f"act {route}", chk)
    assert ("output", 9) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    mod = chk.modules[0]
    assert mod.act_code == act and (mod.fc1[0].bias is None) == (not bias)
    assert mod.storage.sparse_act_T.is_resident() == (not offloaded)
    assert mod.storage.get_out_cache().shape[0] == B


@pytest.mark.parametrize("route", [r for r, v in am.ROUTES.items() if not v[2] and not v[4]])
def test_emulation_stays_inside_the_same_bounds(dev, fresh_config, route):
    """the torch-only comparator on the device, under the bounds the modules are held to"""
    chk = am.run_route(route, dev, lambda layer, fc1, fc2, act: am.ActEmulation(layer, fc1, fc2, act, fresh_config),
                       floors=mm.MLP_FLOORS, eps=eps_of(route), what=f"emulation {route}")
    report(f"emulation {route}", chk)
    assert ("output", 9) in chk.worst


def test_separate_scatter_gives_the_bits_of_the_fused_one(dev, fresh_config):
    """mlp.fused_scatter off: csp_mlp_mm1_act without update, then csp_mlp_mm2_and_scatter_add -- output cache and activation cache bit for bit"""
    outs = []
    for fused in (True, False):
        from chipmunk_amd.util import config as cfgmod
        from chipmunk_amd.util import layer_counter as lc
        cfgmod.reset_to_base()
        lc.singleton.__init__(0, 0)
        chk = am.run_route("gelu_nobias", dev, module_factory(), floors=mm.MLP_FLOORS, eps=eps_of("gelu_nobias"), fused_scatter=fused)
        st = chk.modules[1].storage
        outs.append([t.clone() for t in (st.get_out_cache(), st.get_sparse_act_T(), st.get_counts())])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
