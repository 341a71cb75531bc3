"""SparseDiffGatedMlp on the device against the fp64 model of the sparse-delta method for gated feed-forwards (tests/glu_method_model.py).

Two layers, K = 256, F = 1024 (the fewest columns `topk_indices` accepts), N = 333 tokens (three groups, the last of 77 rows; a pitched
cache), 13 steps with full_step_every = 10, block_mask_cache = 2, first_n_dense_layers = 0, top_keys = 0.3 and the drifting inputs of
method_model.mlp_input: a full step, nine sparse steps that each make a selection, the second full step, a selection made at step 12 and one
kept at step 11 (the `step >= 10` rule).  After every call: the output, the activation cache, the output cache (against its own activation
cache) and the refreshed columns against the model, which takes the module's own selection; the bits of every cache element outside the
selection; the selection against the exact top-|S| of the model's score.  Bounds: those of the ungated bf16 route (method_model.MLP_FLOORS x
ROW_ERR_MARGIN, 2 x MLP_SELECTION_SHORTFALL); the measured figures are recorded in tests/glu_method_model.py."""
import pytest
import torch

import glu_method_model as gm
import method_model as mm

pytestmark = pytest.mark.gpu
OFFLOADED = {"global_disable_offloading": False, "mlp.sparse_act_T": True, "keep_resident_if_fits": False}


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


def linear(w, b, dev):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
    with torch.no_grad():
        lin.weight.copy_(w)
        if b is not None:
            lin.bias.copy_(b)
    return lin.to(dev).bfloat16()


def module_factory(dev, counter, fused=None):
    from chipmunk_amd.modules import SparseDiffGatedMlp

    def make(layer, weights, act):
        wg, bg, wu, bu, w2, b2 = weights
        fc2 = linear(w2, b2, dev)
        if fused is None:
            return SparseDiffGatedMlp(layer, counter, linear(wg, bg, dev), linear(wu, bu, dev), gm.act_module(act), fc2, 6)
        halves = [(wg, bg), (wu, bu)] if fused else [(wu, bu), (wg, bg)]       # fused = gate_first
        fc1 = linear(torch.cat([h[0] for h in halves]), None if bg is None else torch.cat([h[1] for h in halves]), dev)
        return SparseDiffGatedMlp.from_fused(layer, counter, fc1, gm.act_module(act), fc2, gate_first=fused)
    return make


def run(dev, cfg, route, fused_scatter=True, offloading=None, fused=None, floors=gm.GLU_FLOORS, eps=None):
    from chipmunk_amd.util.layer_counter import LayerCounter
    gm.configure(cfg, offloading, fused_scatter)
    eps = 2 * gm.GLU_SELECTION_SHORTFALL if eps is None else eps
    return gm.run_route(route, dev, module_factory(dev, LayerCounter(gm.LAYERS, 1), fused), floors=floors, eps=eps, what=f"glu {route}")


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


@pytest.mark.parametrize("res", ["resident", "offloaded"])
@pytest.mark.parametrize("fused_scatter", [True, False], ids=["fused scatter", "separate scatter"])
@pytest.mark.parametrize("route", list(gm.ROUTES))
def test_gated_modules_against_the_method_model(dev, fresh_config, route, fused_scatter, res):
    what = f"glu {route}, {'fused' if fused_scatter else 'separate'} scatter, {res}"
    chk = run(dev, fresh_config, route, fused_scatter, OFFLOADED if res == "offloaded" else None)
    report(what, chk)
    assert ("output", 9) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    holder = chk.modules[0].storage.sparse_act_T
    assert holder.is_resident() == (res == "resident")


def test_from_fused_with_the_up_half_first_gives_the_bits_of_two_projections(dev, fresh_config):
    """one [2F, K] projection whose SECOND half is the gate: the module uses its halves as views, output and state bit for bit"""
    outs = []
    for fused in (None, False):
        from chipmunk_amd.util import config as cfgmod
        from chipmunk_amd.util import layer_counter as lc
        cfgmod.reset_to_base()
        lc.singleton.__init__(0, 0)
        chk = run(dev, cfgmod.GLOBAL_CONFIG, "gelu_tanh_bias", fused=fused)
        st = chk.modules[1].storage
        # the index rows are torch.empty past their counts (topk_indices writes the kept columns only): what lies there is whatever the
        # allocator handed out, so the lists are compared up to the counts, and the counts themselves
        inds, counts = st.get_indices(), st.get_counts()
        kept = torch.where(torch.arange(inds.shape[-1], device=inds.device) < counts[..., None], inds, torch.full_like(inds, -1))
        outs.append([t.clone() for t in (st.get_out_cache(), st.get_sparse_act_T(), kept, counts, st.get_blockmean_mid_cache())])
    fc1 = chk.modules[0].projs[0]      # (of the second run: one projection, its second half the gate, used in place)
    assert fc1.weight.shape[0] == 2 * gm.F and chk.modules[0].gate[0].data_ptr() == fc1.weight.data[gm.F:].data_ptr()
    assert int(outs[0][3].min()) > 0
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


def test_unsupported_activation_raises_at_construction(dev):
    from chipmunk_amd.modules import SparseDiffGatedMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    w = gm.glu_weights(0, True)
    with pytest.raises(ValueError, match="unsupported activation"):
        SparseDiffGatedMlp(0, LayerCounter(1, 1), linear(w[0], w[1], dev), linear(w[2], w[3], dev), torch.nn.ReLU(), linear(w[4], w[5], dev))
    with pytest.raises(ValueError, match="unsupported activation"):
        SparseDiffGatedMlp.from_fused(0, LayerCounter(1, 1), linear(torch.cat([w[0], w[2]]), None, dev), torch.nn.Tanh(), linear(w[4], w[5], dev))


def test_sparse_step_at_another_token_count_is_refused(dev, fresh_config):
    from chipmunk_amd.util.layer_counter import LayerCounter
    gm.configure(fresh_config)
    mod = module_factory(dev, LayerCounter(1, 1))(0, gm.glu_weights(0, False), "silu")
    with torch.no_grad():
        mod(mm.mlp_input(0, 0, 0, gm.N, gm.K).to(dev))
        with pytest.raises(RuntimeError, match="batch size 1 with 333 tokens"):
            mod(mm.mlp_input(1, 0, 0, gm.N + 1, gm.K).to(dev))
