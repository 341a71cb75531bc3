"""SparseDiffMlp / SparseDiffGatedMlp with ``mlp.top_p`` on the device.

The FLUX schedule of tests/method_model.py (K = 256, F = 1024, 1024 and 1003 tokens) with ``mlp.top_p = 0.4`` and ``mlp.top_p_min_keys =
0.05``, the AMD keys on (the fused delta kernel) and off (the plain operator + ``copy_indices``), the state resident and on the host: after
every call the output and the stored state against the fp64 method model at the project's floors times its margin (the floors pinned
without top-p: the method sets them, not the count); every stored selection against the rule's model (tests/mlp_top_p_model.py) over
block means recomputed here; and in at least half of the calls that make a selection some group stores fewer columns than
``ops.topk_indices`` gives for the same values -- otherwise the feature was not exercised.

Why 0.4: top-k at 0.3 of 1024 columns stores 512; a half-normal delta needs about 0.18 of the columns for 40 % of its mass, 180, which
pads to 256.  Confirmed on the CPU mirror (tests/test_mlp_top_p_host.py: 16 of 16 selection calls), so 0.4 it is.

One gated case: SparseDiffGatedMlp over two steps (a full step, then a sparse step that makes a selection) at the shape of
tests/test_gpu_mlp_glu_e2e.py, its stored selection against the model and its output at that file's bound."""
import pytest
import torch

import glu_method_model as gm
import method_model as mm
import mlp_top_p_model as tp

pytestmark = pytest.mark.gpu
TOP_P, MIN_KEYS = 0.4, 0.05
MLP_FLAGS = ("mlp.out_cache", "mlp.indices", "mlp.counts", "mlp.sparse_act_T", "mlp.blockmean_mid_cache")
# the first two residency set-ups of tests/test_gpu_method_model.py: nothing offloaded; every field through the host, the library's pinned pool
MLP_RESIDENCY = {
    "disabled": dict(global_disable_offloading=True),
    "host, native pool": dict({f: True for f in MLP_FLAGS}, global_disable_offloading=False, keep_resident_if_fits=False, native_host_pool=True),
}


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


@pytest.mark.parametrize("res", ["disabled", "host, native pool"])
@pytest.mark.parametrize("amd_keys", [True, False], ids=["fused delta kernel", "plain op + copy_indices"])
@pytest.mark.parametrize("n", [1024, 1003])
def test_mlp_route_with_top_p(dev, fresh_config, n, amd_keys, res):
    fresh_config["mlp"].update(top_p=TOP_P, top_p_min_keys=MIN_KEYS)
    what = f"mlp top_p {TOP_P}, n {n}, {'amd' if amd_keys else 'ref'}, {res}"
    trace = []
    chk = mm.run_mlp_route("flux", n, dev, torch.nn.Linear, torch.nn.GELU(approximate="tanh"), floors=mm.MLP_FLOORS, eps=None, what=what,
                           trace=trace, offloading=MLP_RESIDENCY[res], amd_keys=amd_keys)
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())))
    assert ("output", 3) in chk.worst
    made, smaller = tp.check_mlp_trace(trace, chk.modules, fresh_config["mlp"])
    print(f"{what}: {smaller} of {made} selection calls store fewer columns than top_keys alone in some group")
    assert made >= 8 and 2 * smaller >= made


def _linear(w, b, dev):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
    with torch.no_grad():
        lin.weight.copy_(w)
        if b is not None:
            lin.bias.copy_(b)
    return lin.to(dev).bfloat16()


def test_gated_module_with_top_p(dev, fresh_config):
    from chipmunk_amd.modules import SparseDiffGatedMlp
    from chipmunk_amd.modules.mlp import block_mean
    from chipmunk_amd.util.layer_counter import LayerCounter
    cfg = gm.configure(fresh_config)
    cfg.update(top_p=TOP_P, top_p_min_keys=MIN_KEYS)
    route = "gelu_tanh_bias"
    act, bias, _ = gm.ROUTES[route]
    counter = LayerCounter(gm.LAYERS, 1)
    weights = [gm.glu_weights(li, bias) for li in range(gm.LAYERS)]
    mods = [SparseDiffGatedMlp(li, counter, _linear(w[0], w[1], dev), _linear(w[2], w[3], dev), gm.act_module(act), _linear(w[4], w[5], dev), 6)
            for li, w in enumerate(weights)]
    model = gm.GluMethodModel(weights, act, gm.SCHEDULE["full_step_every"], gm.SCHEDULE["block_mask_cache"])
    chk = gm.GluChecker(model, weights, gm.N, gm.GLU_FLOORS, None, None, "glu top_p")
    x_of = gm.inputs_for(route, dev)
    means, sizes = {}, []

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (x_of(step, li),)

    def after(step, inv, li, mod, args, out):
        chk.after(step, inv, li, mod, args, out)            # the output and the state at the bounds of tests/test_gpu_mlp_glu_e2e.py
        x, rows = args[0], (gm.N + 127) // 128
        if step == 0:
            g, u = mod._pre(x)
            means[li] = mod._paired_block_means(block_mean(g, 128), block_mean(u, 128), rows)
            return
        pre = mod._paired_block_means(*mod._pre(block_mean(x, 128)), rows)
        score = (pre - means[li]).abs()
        score = score.reshape(1, -1, 2, score.shape[-1]).sum(dim=2)          # gate + up movement per group, as the module sums it
        st = mod.storage
        sizes.extend(tp.check_rows(st.get_indices()[0], st.get_counts()[0], score[0], 1 - cfg["top_keys"], TOP_P, MIN_KEYS,
                                   cfg["counts_multiple_of"], f"gated layer {li}"))
        assert int(st.get_counts().max()) <= 512

    mm.drive(mods, 1, 2, inputs, after)
    print("gated, top_p 0.4: kept columns per group", sizes, {k: round(v, 4) for k, v in sorted(chk.worst.items())})
    assert len(sizes) == gm.LAYERS * 3 and ("output", 1) in chk.worst
    assert min(sizes) < gm.PASSED                                            # fewer than the top_keys rule passes, somewhere
