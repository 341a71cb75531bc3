"""``csp_mlp_mm1_fp8_w4`` ("MXFP4 fc1 under e4m3 activations") on the GPU.
(1) Bits on exact sums (a in halves, |a| <= 2; block bytes 126 .. 129; bias in halves: products multiples of 1/8, sums under 384 * 2 * 6 * 4, 18 bits):
``csp_mlp_mm1_act`` on ``a.to(bf16)`` / ``widened()``.  (2) fp64, helpers.MLP_SEG_BOUND; a constant row vector.  (3) Refusals.  (4) The module."""
import functools

import pytest
import torch

import method_model as mm
import test_gpu_mlp_w4 as w4
import test_gpu_mlp_w8 as w8
from helpers import MLP_ACTS as ACTS, MLP_SEG_BOUND, MLP_SEG_W1, assert_segs_close, mm1_exact
from test_gpu_mlp_w4_e2e import dev, run_route  # noqa: F401  (the fixture: fresh config, empty offload registry)

pytestmark = pytest.mark.gpu

E4M3, F = torch.float8_e4m3fn, 512
COUNTS = {40: ((33,),), 128: ((65,),), 1003: ((0, 1, 32, 33, 64, 65, F, 200), (F, 65, 0, 33, 1, 64, 32, 424))}


@functools.lru_cache(maxsize=None)
def problem(M, K, B, f=F, exact=True, counts=None):
    # tests/test_gpu_mlp_w4.py's problem around e4m3 activations p["aq"] (p["a"]: their bf16 widening): (1)'s exact-sum inputs, or row-quantised normal ones
    from chipmunk_amd.modules import W4Linear
    from chipmunk_amd.modules.mlp_fp8 import quantize_rowwise_torch
    g = torch.Generator().manual_seed(31 * M + K + B)
    if exact:
        aq, sa = (torch.randint(-4, 5, (B, M, K), generator=g) * 0.5).to(E4M3), torch.ones(B, M)
        layer = W4Linear.from_mx(torch.randint(0, 256, (f, K // 2), generator=g, dtype=torch.uint8),
                                 torch.randint(126, 130, (f, K // 32), generator=g, dtype=torch.uint8))
        bias = (torch.randint(-16, 17, (f,), generator=g) * 0.5).to(torch.bfloat16)
    else:
        aq, sa = quantize_rowwise_torch(torch.randn(B, M, K, generator=g) * torch.logspace(-1, 1, M)[:, None], 448.0)
        lin = torch.nn.Linear(K, f, bias=False)
        lin.weight.data = torch.randn(f, K, generator=g) * 0.06
        layer, bias = W4Linear.from_linear(lin), (torch.randn(f, generator=g) * 0.1).to(torch.bfloat16)
    p = dict(w4.problem(M, K, B, f=f, seed=int(exact), counts=counts or COUNTS[M][:B], layer=layer))
    p.update({k: t.to(p["a"].device) for k, t in dict(aq=aq, sa=sa, bias=bias, a=aq.to(torch.bfloat16)).items()})
    return p


def run(p, s, scale_a, bias, act, upd):
    _, c, cache, inds, cnt = w8.operands(p, s)
    torch.ops.chipmunk.csp_mlp_mm1_fp8_w4(p["aq"] if p["B"] > 1 else p["aq"][0], p["w4"], p["sc"], c, bias, cache, inds, cnt, scale_a, act, upd)


def run_both(p, layout, bias, act, upd, what):      # this form and the bf16 form on the widened operands from equal states
    s, ref = w8.fresh_state(p, layout), w8.fresh_state(p, layout)
    run(p, s, p["sa"] if p["B"] > 1 else p["sa"][0], bias, act, upd)
    a, c, cache, inds, cnt = w8.operands(p, ref)
    torch.ops.chipmunk.csp_mlp_mm1_act(a, p["wide"], c, bias, cache, inds, cnt, act, bool(upd))
    w8.check_untouched(p, s, what, cache_written=upd)
    w8.assert_same(p, s, ref, what)


BIT_CASES = ([(1003, 384, 1, "column", act, upd) for act in ACTS for upd in (0, 1)] +
             [(40, 128, 1, "column", "gelu_tanh", 1), (40, 128, 1, "group", "silu", 0), (128, 256, 1, "column", "gelu", 1), (128, 256, 1, "group", "gelu_tanh", 1),
              (1003, 384, 2, "column", "gelu_tanh", 1), (1003, 384, 2, "group", "silu", 1), (1003, 384, 1, "group", "gelu", 0)])


@pytest.mark.parametrize("M,K,B,layout,act,upd", BIT_CASES)
def test_bits_on_exact_sums(dev, M, K, B, layout, act, upd):
    p = problem(M, K, B)
    assert len(p["w4"].unique()) == 256 and len(p["sc"].unique()) == 4 and len(p["aq"].view(torch.uint8).unique()) == 9
    for bias in (None, p["bias"]):
        run_both(p, layout, bias, act, upd, f"M {M} K {K} B {B} {layout} {act} update {upd} bias {bias is not None}")


def test_bits_through_the_tail_split(dev):
    f = ((2 * torch.cuda.get_device_properties(0).multi_processor_count // 8) // 2 + 1) * 128
    lists = ((2048, 0, 1024, 3072, 512, 256, 4096, f), (256, f, 0, 1024, 2048, 552, f, f))
    p = problem(1003, 256, 2, f=f, counts=tuple(tuple(min(c, f) for c in row) for row in lists))
    run_both(p, "column", p["bias"], "gelu_tanh", 1, "tail split")


@pytest.mark.parametrize("K,act,rows", [(384, act, True) for act in ACTS] + [(384, "gelu_tanh", False), (1536, "silu", True)])
def test_segments_against_the_fp64_contract(dev, K, act, rows):
    p = problem(1003, K, 1, exact=False)
    sa = p["sa"][0] if rows else p["sa"][0, 500:501].clone()      # (the scalar form: one row's number for all; the reference takes the same)
    s = w8.fresh_state(p, "column")
    run(p, s, sa, p["bias"], act, 1)
    w8.check_untouched(p, s, f"fp64 {act}", cache_written=True)
    exact, _ = mm1_exact(p["aq"][0].double() * sa.double()[:, None], p["wide"], p["bias"], p["cache0"][0], p["inds"][0], p["cnt"][0], act)
    assert_segs_close(s["c"][0], exact, MLP_SEG_BOUND, f"csp_mlp_mm1_fp8_w4 {act}: packed deltas", width=MLP_SEG_W1, cols=p["cols"][0])
    if not rows:      # the same number for every row, as a vector: the same bits
        ref = w8.fresh_state(p, "column")
        run(p, ref, sa.expand(1003).contiguous(), p["bias"], act, 1)
        w8.assert_same(p, s, ref, "constant row scales")


def test_refusals_write_nothing(dev):
    p = problem(128, 256, 1)
    a, w4, sc, sa, f = p["aq"][0], p["w4"], p["sc"], p["sa"][0], p["F"]
    off = lambda t: torch.zeros(t.numel() + 1, dtype=torch.uint8, device=dev)[1:].view(t.shape)      # noqa: E731  (one byte off every alignment)
    bad = {"K off its multiple": dict(a=a[:, :64].contiguous(), w4=w4[:, :32].contiguous(), sc=sc[:, :2].contiguous()),
           "unknown act": dict(act="relu"), "update_cache 2": dict(upd=2), "update_cache -1": dict(upd=-1),
           "scale_a of 127": dict(sa=sa[:127].contiguous()), "scale_a of [2]": dict(sa=sa[:2].contiguous()), "scale_a in fp64": dict(sa=sa.double()),
           "b off 4-byte alignment": dict(w4=off(w4)), "scale_b off 4-byte alignment": dict(sc=off(sc)), "a in bf16": dict(a=p["a"][0])}
    for what, change in bad.items():
        s = w8.fresh_state(p, "column")
        k = dict(dict(a=a, w4=w4, sc=sc, sa=sa, act="silu", upd=1), **change)
        with pytest.raises((RuntimeError, ValueError)):
            torch.ops.chipmunk.csp_mlp_mm1_fp8_w4(k["a"], k["w4"], k["sc"], s["c"][0], p["bias"], s["cache"][0], p["inds"][0], p["cnt"][0], k["sa"], k["act"], k["upd"])
        assert (s["c_buf"] == w8.SENT).all() and torch.equal(s["cache"], p["cache0"]), f"{what}: refused, but c or the cache was written"


def run_module(n, device, fused, key, steps=6):
    """tests/test_gpu_mlp_w4_e2e.py's route over `steps` steps: the outputs of every call; key on: every sparse step is also made by hand on copies of its state"""
    from chipmunk_amd import ops
    from chipmunk_amd.modules import SparseDiffMlp, W4Linear
    from chipmunk_amd.modules.mlp import activation_cache_view
    from chipmunk_amd.util import config as cfg, layer_counter as lc
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    torch.cuda.synchronize()
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)
    ot.gpu_tensors.clear()
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    n_inv, _steps, _every, _cache = mm.configure_mlp(cfg.GLOBAL_CONFIG, "flux")
    cfg.GLOBAL_CONFIG["offloading"].update({"global_disable_offloading": True})
    cfg.GLOBAL_CONFIG["mlp"].update(fused_scatter=fused, mxfp4_fp8_act=key)
    counter, gelu, mods, outs, before, by_hand = lc.LayerCounter(mm.MLP_LAYERS, 1), torch.nn.GELU(approximate="tanh"), [], [], {}, []
    for li in range(mm.MLP_LAYERS):
        torch.manual_seed(li)
        fc1, fc2 = torch.nn.Linear(mm.MLP_K, mm.MLP_F).to(device).bfloat16(), torch.nn.Linear(mm.MLP_F, mm.MLP_K).to(device).bfloat16()
        fc1 = W4Linear.from_linear(fc1) if li >= mm.MLP_DENSE_LAYERS else fc1
        mods.append(SparseDiffMlp(li, counter, fc1, gelu, fc2, 6))

    def inputs(step, inv, li):
        st = mods[li].storage
        if key and li >= mm.MLP_DENSE_LAYERS and not counter.should_do_full_mlp_step():      # the state a sparse step starts from
            before[li] = st.get_sparse_act_T().clone(), st.get_out_cache().clone()
        return (mm.mlp_input(step, inv, li, n, mm.MLP_K).to(device),)

    def after(step, inv, li, mod, args, out):
        outs.append(out.clone())
        if li in before:
            act_T, out_cache = before.pop(li)
            fc1, (xq, sa) = mod.fc1[0], mod.fc1[0].quantize_input_rowwise(args[0])
            ops.mlp(x=xq[0], fc1w=fc1.weight.data, fc1b=fc1.bias.data, fc2w_T=mod.fc2w_T[0], indices=mod.storage.get_indices()[0],
                    counts=mod.storage.get_counts()[0], sparse_act_T=activation_cache_view(act_T, n, False), cached_out=out_cache[0],
                    num_sms_scatter_add=6, mm1_scale_a=sa[0], fc1_scale=fc1.block_scale, act="gelu_tanh")
            assert torch.equal(out_cache.view(torch.int16), out.view(torch.int16)), f"step {step} layer {li}: the module's sparse step is not the hand-called chain"
            by_hand.append((step, li))
    mm.drive(mods, n_inv, steps, inputs, after)
    return outs, by_hand


@pytest.mark.parametrize("fused", [True, False])
def test_module_sparse_steps_are_the_hand_called_chain(dev, fused):
    on, by_hand = run_module(1003, dev, fused, True)
    assert len(by_hand) == 4 * (mm.MLP_LAYERS - mm.MLP_DENSE_LAYERS)      # steps 1, 2, 3 and 5 of 6 are sparse (full_step_every = 4)
    off, ref = run_module(1003, dev, fused, False)[0], run_route(1003, dev, False, fused)      # (the parent's path: the module over the widened nn.Linear)
    assert all(torch.equal(o.view(torch.int16), r.view(torch.int16)) for o, r in zip(off, ref)), "key off: not the bits of the module over the widened weight"
    assert not all(torch.equal(o, r) for o, r in zip(on, off)), "key on: the sparse steps still run on bf16 activations"
