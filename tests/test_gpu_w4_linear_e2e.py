"""SparseDiffMlp over an MXFP4 ``W4Linear`` ``fc1`` with ``mlp.w4_stream_rows`` at the probe's row count, on the `flux` schedule at N = 1003
(that of tests/test_gpu_mlp_w4_e2e.py): the block-mean probes of the selecting steps, and only they, run ``ops.w4_linear``; the outputs stay
inside the bounds tests/test_gpu_w8_linear_e2e.py applies (fp64 method model on the widened weights, ``MLP_FLOORS`` x 2, selection shortfall
2 x ``MLP_SELECTION_SHORTFALL``); with the key at 0 nothing streams and the outputs are the parent's, bit for bit."""
import pytest
import torch

import method_model as mm
import test_gpu_w8_linear_e2e as w8

pytestmark = pytest.mark.gpu
N = 1003
dev = w8.dev      # the same fixture: fresh config, cleared storage


def run(device, key, calls, what):
    """-> (checker, (step, layer) of every sparse call, the outputs of every call); `calls` collects the row counts ops.w4_linear sees"""
    import chipmunk_amd.ops
    from chipmunk_amd.modules import SparseDiffMlp, W4Linear
    from chipmunk_amd.util import layer_counter as lc
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    w8._reset()
    n_inv, steps, every, cache = mm.configure_mlp(GLOBAL_CONFIG, "flux")
    GLOBAL_CONFIG["offloading"].update({"global_disable_offloading": True})
    GLOBAL_CONFIG["mlp"]["w4_stream_rows"] = key
    counter, gelu, mods, weights = lc.LayerCounter(mm.MLP_LAYERS, 1), torch.nn.GELU(approximate="tanh"), [], []
    for li in range(mm.MLP_LAYERS):
        torch.manual_seed(li)
        fc1, fc2 = torch.nn.Linear(mm.MLP_K, mm.MLP_F).to(device).bfloat16(), torch.nn.Linear(mm.MLP_F, mm.MLP_K).to(device).bfloat16()
        if li >= mm.MLP_DENSE_LAYERS:
            fc1 = W4Linear.from_linear(fc1)
        mods.append(SparseDiffMlp(li, counter, fc1, gelu, fc2, 6))
        w1 = fc1.widened() if isinstance(fc1, W4Linear) else fc1.weight.data
        weights.append((w1.double(), fc1.bias.data.double(), fc2.weight.data.double(), fc2.bias.data.double()))
    model = mm.MlpMethodModel(weights, every, cache, GLOBAL_CONFIG["mlp"]["bm"])
    chk = w8.e2e.W8Checker(model, weights, N, 1, mm.MLP_DENSE_LAYERS, mm.MLP_PASSED, mm.MLP_FLOORS, 2 * mm.MLP_SELECTION_SHORTFALL,
                           lambda mod, x, full: x, what)
    sparse, outs = [], []

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (mm.mlp_input(step, inv, li, N, mm.MLP_K).to(device),)

    def after(step, inv, li, mod, args, out):
        outs.append(out.clone())
        chk.after(step, inv, li, mod, args, out)
        if li >= mm.MLP_DENSE_LAYERS and not model.is_full(step):
            sparse.append((step, li))
    real = chipmunk_amd.ops.w4_linear
    chipmunk_amd.ops.w4_linear = lambda x, *a, **kw: calls.append(x.numel() // x.shape[-1]) or real(x, *a, **kw)
    try:
        mm.drive(mods, n_inv, steps, inputs, after)
    finally:
        chipmunk_amd.ops.w4_linear = real
    return chk, sparse, outs


def test_the_probes_stream_and_key_off_gives_the_parents_bits(dev, monkeypatch):
    from chipmunk_amd.modules import W4Linear
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    probe_rows, calls = (N + GLOBAL_CONFIG["mlp"]["mbm"] - 1) // GLOBAL_CONFIG["mlp"]["mbm"], []
    chk, sparse, _ = run(dev, probe_rows, calls, f"mlp w4 fc1 flux, n {N}, w4_stream_rows {probe_rows}")
    w8.e2e.report(f"w4_stream_rows {probe_rows}", chk)
    assert ("output", 3) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    cache = mm.MLP_ROUTES["flux"][3]      # a step >= 10 off the block_mask_cache grid reuses the stored selection
    selecting = [(step, li) for step, li in sparse if not (step % cache != 0 and step >= 10)]
    assert 0 < len(selecting) < len(sparse), "the schedule holds selecting steps and a step that reuses its selection"
    assert calls == [probe_rows] * len(selecting), (calls, probe_rows, len(selecting))
    # the key at 0: nothing streams, and the outputs are those of the parent's forward, written out
    calls.clear()
    off = run(dev, 0, calls, "key 0")[2]
    assert calls == [] and off
    monkeypatch.setattr(W4Linear, "forward", lambda self, x: torch.nn.functional.linear(
        x, self.widened() if x.dtype == torch.bfloat16 else self.widened().to(x.dtype), self.bias))
    parent = run(dev, 0, calls, "parent forward")[2]
    assert len(off) == len(parent) and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(off, parent))
