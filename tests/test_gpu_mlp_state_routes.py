"""Which selection route a sparse step of ``SparseDiffMlp`` / ``SparseDiffGatedMlp`` takes on the device: for every setting of the two
fused-selection keys, one and two block means per group, whole and short last groups and ``mlp.top_p`` off and on, the operators that run
are those of the route ``select_route`` names, and exactly one route runs per selecting step.  (The values are the e2e tests'.)
"""
import itertools

import pytest
import torch

import glu_method_model as gm
import method_model as mm

pytestmark = pytest.mark.gpu
K, F = 64, 1024
SCHEDULE = dict(full_step_every=10, block_mask_cache=2, first_n_dense_layers=0, top_keys=0.3, random_keys=0.0, counts_multiple_of=256)
ROUTES = {"single": ["topk_delta_indices"], "group": ["topk_group_delta_indices"], "chain": ["topk_indices", "copy_indices"]}
SPIED = ("topk_indices", "topk_indices_p", "copy_indices", "topk_delta_indices_p", "topk_group_delta_indices", "topk_group_delta_indices_p")


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


@pytest.fixture()
def ran(monkeypatch):
    """the names of the selection operators in the order they ran; every spy passes its call on"""
    from chipmunk_amd import ops
    names = []

    def spy(name, fn):
        def through(*args, **kwargs):
            names.append(name)
            return fn(*args, **kwargs)
        return through

    for name in SPIED:
        monkeypatch.setattr(ops, name, spy(name, getattr(ops, name)))
    # (the single-row route without top_p is looked up in torch.ops.chipmunk, not in ops)
    monkeypatch.setattr(torch.ops.chipmunk, "topk_delta_indices", spy("topk_delta_indices", torch.ops.chipmunk.topk_delta_indices))
    return names


def linear(w, b, dev):
    lin = torch.nn.Linear(w.shape[1], w.shape[0])
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    return lin.to(dev).bfloat16()


def make_module(dev, gated):
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    wg, bg, wu, bu, w2, b2 = gm.glu_weights(0, True, K, F)
    if gated:
        return SparseDiffGatedMlp(0, LayerCounter(1, 1), linear(wg, bg, dev), linear(wu, bu, dev), torch.nn.SiLU(), linear(w2, b2, dev), 6)
    return SparseDiffMlp(0, LayerCounter(1, 1), linear(wg, bg, dev), torch.nn.GELU(approximate="tanh"), linear(w2, b2, dev), 6)


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("n", [256, 200])
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_selecting_steps_take_the_route_of_select_route(dev, ran, gated, n, r):
    from chipmunk_amd.modules.mlp import select_route
    from chipmunk_amd.util import config as cfgmod
    from chipmunk_amd.util import layer_counter as lc
    xs = [mm.mlp_input(step, 0, 0, n, K).to(dev) for step in range(3)]
    seen = set()
    for single_key, group_key, top_p in itertools.product((False, True), (False, True), (0.0, 0.6)):
        cfgmod.reset_to_base()
        lc.singleton.__init__(0, 0)
        cfg = cfgmod.GLOBAL_CONFIG
        cfg["num_model_invocations_per_inference_step"] = 1
        cfg["steps"] = 50
        cfg["offloading"].update({"global_disable_offloading": True})
        cfg["mlp"].update(SCHEDULE)
        cfg["mlp"].update(bm=128, mbm=128 // r, fused_topk_delta=single_key, fused_group_topk_delta=group_key, top_p=top_p,
                          top_p_min_keys=0.05)
        route = select_route(True, True, 2 * r if gated else r, single_key, group_key)
        want = [name + "_p" if top_p and name != "copy_indices" else name for name in ROUTES[route]]
        what = f"fused_topk_delta {single_key}, fused_group_topk_delta {group_key}, top_p {top_p}"
        mod = make_module(dev, gated)
        with torch.no_grad():
            del ran[:]
            out = mod(xs[0])
            assert ran == [], f"{what}: a full step selected"
            for x in xs[1:]:
                out = mod(x)
                assert ran == want, f"{what}: route {route} is {want}, ran {ran}"
                del ran[:]
        assert tuple(out.shape) == (1, n, K) and bool(torch.isfinite(out.float()).all())
        groups = (n + 127) // 128
        assert tuple(mod.storage.get_indices().shape) == (1, groups, F) and tuple(mod.storage.get_counts().shape) == (1, groups)
        assert int(mod.storage.get_counts().min()) > 0
        seen.add(route)
    assert seen == ({"chain", "group"} if gated or r > 1 else {"chain", "single"})
