"""``mlp.fused_group_topk_delta`` in the modules: a short schedule (a full step, then three sparse steps that each select) with the key on
and with it off gives the same bits -- outputs, stored indices and counts, block-mean cache, activation cache -- at every step, for
``SparseDiffGatedMlp`` (two rows per group) and ``SparseDiffMlp`` with ``bm = 2 mbm``; with the key on neither ``ops.topk_indices`` nor
``ops.copy_indices`` runs; and a ragged token count works on the ``bm > mbm`` route, its selection the model's.
"""
import pytest
import torch

import glu_fp8_method_model as gfp
import glu_method_model as gm
import group_delta_model as gdm
import method_model as mm

pytestmark = pytest.mark.gpu
K, F = 256, 1024
SCHEDULE = dict(full_step_every=10, block_mask_cache=2, first_n_dense_layers=0, top_keys=0.3, random_keys=0.0, counts_multiple_of=256)
STEPS = 4


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


def configure(key_on, bm=128, mbm=128):
    from chipmunk_amd.util import config as cfgmod
    from chipmunk_amd.util import layer_counter as lc
    cfgmod.reset_to_base()
    lc.singleton.__init__(0, 0)
    cfg = cfgmod.GLOBAL_CONFIG
    cfg["num_model_invocations_per_inference_step"] = 1
    cfg["steps"] = 50
    cfg["mlp"].update(SCHEDULE)
    cfg["mlp"].update(bm=bm, mbm=mbm, fused_group_topk_delta=key_on)
    cfg["offloading"].update({"global_disable_offloading": True})
    return cfg["mlp"]


def make_module(dev, gated):
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    wg, bg, wu, bu, w2, b2 = gm.glu_weights(0, True, K, F)
    if gated == "fp8":      # two e4m3 F8Linear projections, a bf16 fc2
        projs, fc2 = gfp.f8_layers((wg, bg, wu, bu, w2, b2), None, dev)
        return SparseDiffGatedMlp(0, LayerCounter(1, 1), projs[0], projs[1], torch.nn.SiLU(), fc2, 6)
    if gated:
        return SparseDiffGatedMlp(0, LayerCounter(1, 1), linear(wg, bg, dev), linear(wu, bu, dev), torch.nn.SiLU(), linear(w2, b2, dev), 6)
    return SparseDiffMlp(0, LayerCounter(1, 1), linear(wg, bg, dev), torch.nn.GELU(approximate="tanh"), linear(w2, b2, dev), 6)


def inputs(dev, step, n, b):
    return torch.cat([mm.mlp_input(step, s, 0, n, K) for s in range(b)]).to(dev)


def state(mod, out):
    """what a step leaves behind, as integer tensors (the index rows are torch.empty past their counts: compared up to the counts)"""
    st = mod.storage
    res = [out.clone().view(torch.int16), st.get_blockmean_mid_cache().clone().view(torch.int16), st.get_sparse_act_T().clone().view(torch.int16)]
    inds, counts = st.get_indices(), st.get_counts()
    if inds is not None:
        res += [torch.where(torch.arange(inds.shape[-1], device=inds.device) < counts[..., None], inds, torch.full_like(inds, -1)), counts.clone()]
    return res


def run_schedule(dev, gated, n, b, key_on, bm, mbm, monkeypatch=None):
    from chipmunk_amd import ops
    configure(key_on, bm, mbm)
    if key_on and monkeypatch is not None:      # the spy: the unfused chain's two operators must not run
        def forbidden(*a, **k):
            raise AssertionError("the unfused selection chain ran with mlp.fused_group_topk_delta on")
        monkeypatch.setattr(ops, "topk_indices", forbidden)
        monkeypatch.setattr(ops, "copy_indices", forbidden)
    mod = make_module(dev, gated)
    trace = []
    with torch.no_grad():
        for step in range(STEPS):
            trace.append(state(mod, mod(inputs(dev, step, n, b))))
    torch.cuda.synchronize()
    return trace


def assert_identical(on, off, what):
    names = ["output", "block-mean cache", "activation cache", "indices", "counts"]
    for step, (a, c) in enumerate(zip(on, off)):
        assert len(a) == len(c) == (3 if step == 0 else 5)
        for name, x, y in zip(names, a, c):
            assert torch.equal(x, y), f"{what}: {name} differs at step {step}"
    assert int(on[-1][4].min()) > 0


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("n", [384, 300])
def test_gated_module_key_on_equals_key_off(dev, monkeypatch, n, b):
    off = run_schedule(dev, True, n, b, False, 128, 128)
    on = run_schedule(dev, True, n, b, True, 128, 128, monkeypatch)
    assert_identical(on, off, f"gated N {n} B {b}")


def test_gated_fp8_module_key_on_equals_key_off(dev, monkeypatch):
    a = torch.zeros(16, K, device=dev).to(torch.float8_e4m3fn)
    w = torch.zeros(F, K, device=dev).to(torch.float8_e4m3fn)
    one = torch.ones((), device=dev)
    # torch's own fp8 GEMM, called as F8Linear calls it, has to exist in this build; nothing of the project runs in this line
    torch._scaled_mm(a, w.T, scale_a=one, scale_b=one, bias=torch.zeros(F, device=dev, dtype=torch.bfloat16), out_dtype=torch.bfloat16,
                     use_fast_accum=True)
    off = run_schedule(dev, "fp8", 300, 1, False, 128, 128)
    on = run_schedule(dev, "fp8", 300, 1, True, 128, 128, monkeypatch)
    assert_identical(on, off, "gated fp8 N 300")


def test_ungated_module_two_block_means_per_group_key_on_equals_key_off(dev, monkeypatch):
    off = run_schedule(dev, False, 384, 1, False, 128, 64)
    on = run_schedule(dev, False, 384, 1, True, 128, 64, monkeypatch)
    assert_identical(on, off, "ungated bm 128 mbm 64 N 384")


def test_ungated_module_ragged_token_count_selects_as_the_model(dev, monkeypatch):
    """N = 300, bm = 128, mbm = 64: five block-mean rows, three groups, the last with one row"""
    from chipmunk_amd.modules.mlp import block_mean
    cfg = configure(True, 128, 64)
    mod = make_module(dev, False)
    with torch.no_grad():
        mod(inputs(dev, 0, 300, 1))
        before = mod.storage.get_blockmean_mid_cache().clone()
        x = inputs(dev, 1, 300, 1)
        bmfc1 = mod.fc1[0](block_mean(x, 64))
        assert before.shape == bmfc1.shape == (1, 5, F)
        out = mod(x)
    torch.cuda.synchronize()
    assert out.shape == (1, 300, K) and bool(torch.isfinite(out.float()).all())
    inds, counts, cache = gdm.run(bmfc1, before, 2, 1 - cfg["top_keys"], cfg["counts_multiple_of"], fill=-1)
    got_i, got_c = mod.storage.get_indices().cpu(), mod.storage.get_counts().cpu()
    assert got_i.shape == (1, 3, F) and torch.equal(got_c, counts)
    listed = torch.arange(F) < counts[..., None]
    assert torch.equal(torch.where(listed, got_i, torch.full_like(got_i, -1)), torch.where(listed, inds, torch.full_like(inds, -1)))
    assert torch.equal(mod.storage.get_blockmean_mid_cache().cpu().view(torch.int16), cache.view(torch.int16))
