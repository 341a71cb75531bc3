"""SparseDiffGatedMlp over weight-only ``W8Linear`` projections (``mlp.w8_gated``) on the device against the fp64 model of the sparse-delta
method for gated feed-forwards (tests/glu_method_model.py) evaluated on the WIDENED weights: a ``W8Linear`` is the bf16 linear layer over
``weight.to(bf16) * scale_reciprocal`` (exact: power-of-two scales), so there is no quantisation error to set aside and no residue -- the
plain gated model, the floors ``MLP_FLOORS`` x 2 and 2 x ``MLP_SELECTION_SHORTFALL``, the bounds tests/test_gpu_mlp_glu_e2e.py holds the
bf16 gated route to.

Two layers over the schedule of tests/glu_method_model.py (13 steps, full steps 0 and 10, a selection kept at step 11) at N = 1003, B = 1
(ragged last group, pitched cache) and N = 1024, B = 2; layer 1 scales its projections per tensor, layer 2 per row.  Once through
``from_fused`` (one ``[2F, K]`` ``W8Linear``, its ``[2F]`` scale split like its weight), once with a ``W8Linear`` ``fc2`` under
``mlp.fp8_fc2`` (GEMM2 gathers e4m3 rows as well), once with ``mlp.w8_stream_rows`` on (the block-mean probe streams the e4m3 weights).
Dense and full steps and the block-mean probe go through ``W8Linear.forward``, the sparse steps through ``csp_mlp_mm1_glu_w8``.

Selections: with two projections (and the probe through ``F.linear``) they are those of the same module over the widened bf16
``nn.Linear``s, index for index.  The fused constructor's dense call is one GEMM of another shape, and the streamed probe sums in another
order than the vendor GEMM (tests/test_gpu_w8_linear_e2e.py), so near-ties may fall differently there: those runs are held to the model's
selection bound only.  With the key off the constructor raises.

Measured on one MI355X, worst over the five runs: output 0.0093 (bound 0.0104), out_cache against its own activation cache 0.0096 (0.0104),
activation cache 0.0056 at a full step (0.0066) and 0.0050 after (0.0054), refreshed columns 0.0034 (0.0048), selection shortfall 0.00009
with the streamed probe and 0.00006 without (0.00018): the figures of the bf16 gated route (tests/glu_method_model.py)."""
import pytest
import torch

import glu_method_model as gm
import method_model as mm

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


def _clear():
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    ot.gpu_tensors.clear()
    ot._resident_bytes = ot._kept_offloaded_bytes = 0


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    assert torch.cuda.is_available()
    saved = ot._resident_bytes, ot._kept_offloaded_bytes
    _clear()
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


def widened_linear(q):
    """the bf16 nn.Linear a W8Linear stands for"""
    lin = torch.nn.Linear(q.in_features, q.out_features, bias=q.bias is not None).to(q.weight.device).bfloat16()
    with torch.no_grad():
        lin.weight.copy_(q.widened())
        if q.bias is not None:
            lin.bias.copy_(q.bias)
    return lin


def run_route(n, batch, device, weight_only, act="silu", bias=False, fused=None, w8_fc2=False, stream_rows=0, floors=None, eps=None, what=""):
    """gm.SCHEDULE with `batch` sequences of `n` tokens per call; weight_only: the projections (and, `w8_fc2`, fc2) are W8Linear, otherwise
    the nn.Linear over the same widened weights.  fused: None = two projections, True / False = one [2F, K] projection and whether its first
    half is the gate.  Returns (checker, selections per sparse call)."""
    from chipmunk_amd.modules import SparseDiffGatedMlp, W8Linear
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    from chipmunk_amd.util.layer_counter import LayerCounter
    gm.configure(GLOBAL_CONFIG)
    GLOBAL_CONFIG["mlp"].update(w8_gated=True, fp8_fc2=bool(w8_fc2), w8_stream_rows=stream_rows)
    counter = LayerCounter(gm.LAYERS, 1)
    mods, weights = [], []
    take = lambda q: q if weight_only else widened_linear(q)      # noqa: E731
    for li in range(gm.LAYERS):
        wg, bg, wu, bu, w2, b2 = gm.glu_weights(li, bias)
        scaling = "tensor" if li == 0 else "row"
        fc2 = linear(w2, b2, device)
        q2 = W8Linear.from_linear(fc2) if w8_fc2 else None
        if fused is None:
            qg, qu = W8Linear.from_linear(linear(wg, bg, device), scaling=scaling), W8Linear.from_linear(linear(wu, bu, device), scaling=scaling)
            wide = [(qg.widened().double(), bg), (qu.widened().double(), bu)]
            mod = SparseDiffGatedMlp(li, counter, take(qg), take(qu), gm.act_module(act), fc2 if q2 is None else take(q2), 6)
        else:
            halves = [(wg, bg), (wu, bu)] if fused else [(wu, bu), (wg, bg)]
            q1 = W8Linear.from_linear(linear(torch.cat([h[0] for h in halves]), None if bg is None else torch.cat([h[1] for h in halves]), device),
                                      scaling=scaling)
            w = q1.widened().double()
            first, second = w[: gm.F], w[gm.F:]
            wide = [(first, bg), (second, bu)] if fused else [(second, bg), (first, bu)]
            mod = SparseDiffGatedMlp.from_fused(li, counter, take(q1), gm.act_module(act), fc2 if q2 is None else take(q2), gate_first=fused)
        mods.append(mod)
        w2d = (q2.widened() if q2 is not None else fc2.weight.data).double()
        weights.append((wide[0][0], wide[0][1], wide[1][0], wide[1][1], w2d, fc2.bias.data.double()))    # (the biases are bf16 values already)
    model = gm.GluMethodModel(weights, act, gm.SCHEDULE["full_step_every"], gm.SCHEDULE["block_mask_cache"])
    chk = gm.GluChecker(model, weights, n, floors, eps, None, what)
    selections = []

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (torch.cat([mm.mlp_input(step, b, li, n, gm.K) for b in range(batch)]).to(device),)

    def after(step, inv, li, mod, args, out):
        chk.after(step, inv, li, mod, args, out)
        if not model.is_full(step):
            selections.append((step, li, mod.storage.get_indices().clone(), mod.storage.get_counts().clone()))

    mm.drive(mods, 1, gm.STEPS, inputs, after)
    chk.modules = mods
    return chk, selections


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


# (tokens, batch, activation, biases, fused, W8Linear fc2, mlp.w8_stream_rows)
CASES = {"n1003 b1": (1003, 1, "silu", False, None, False, 0), "n1024 b2": (1024, 2, "gelu_tanh", True, None, False, 0),
         "from_fused": (1003, 1, "gelu_tanh", True, True, False, 0), "w8 fc2": (1003, 1, "silu", False, None, True, 0),
         "stream rows": (1024, 2, "gelu", True, None, False, 64)}


@pytest.mark.parametrize("case", list(CASES))
def test_gated_module_over_weight_only_projections_against_the_method_model(dev, case, monkeypatch):
    import sys
    import chipmunk_amd.ops
    from chipmunk_amd.modules import W8Linear
    n, batch, act, bias, fused, w8_fc2, stream = CASES[case]
    what = f"glu w8 {case}: n {n}, b {batch}, {act}{', biases' if bias else ''}"
    ops_mlp = sys.modules["chipmunk_amd.ops.mlp"]
    seen, streamed = [], []
    real_glu_w8, real_stream = ops_mlp.mm1_glu_w8, chipmunk_amd.ops.w8_linear

    def spy(x, w_gate, w_up, scale_gate, scale_up, *a, **kw):
        seen.append((x.dtype, w_gate.dtype, w_up.dtype, tuple(scale_gate.shape), tuple(scale_up.shape)))
        return real_glu_w8(x, w_gate, w_up, scale_gate, scale_up, *a, **kw)

    def stream_spy(x, *a, **kw):
        streamed.append(x.numel() // x.shape[-1])
        return real_stream(x, *a, **kw)
    monkeypatch.setattr(ops_mlp, "mm1_glu_w8", spy)
    monkeypatch.setattr(chipmunk_amd.ops, "w8_linear", stream_spy)
    chk, sel = run_route(n, batch, dev, True, act, bias, fused, w8_fc2, stream, floors=mm.MLP_FLOORS, eps=2 * mm.MLP_SELECTION_SHORTFALL,
                         what=what)
    report(what, chk)
    assert ("output", 9) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    # the sparse steps ran the gated weight-only GEMM1 on bf16 x and the e4m3 weights, layer 1 with one scale, layer 2 with one per row
    assert len(seen) == len(sel) > 0 and all(s[:3] == (torch.bfloat16, E4M3, E4M3) for s in seen), seen
    assert {s[3] for s in seen} == {s[4] for s in seen} == {(), (gm.F,)}, "both scale granularities ran"
    for m in chk.modules:
        assert m.w8 and not m.fp8 and all(isinstance(p, W8Linear) for p in m.projs) and len(m.projs) == (1 if fused is not None else 2)
        assert (m.fc2w_T.dtype == E4M3) == w8_fc2
    probe_rows = batch * ((n + 127) // 128)
    assert (probe_rows in streamed) == (stream > 0), "mlp.w8_stream_rows applies to the block-mean probe, and nothing streams without it"
    if fused is not None or stream:
        return
    # the same modules over the widened bf16 nn.Linear make the same selections
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    torch.cuda.synchronize()
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)
    _clear()
    seen.clear()
    _, ref = run_route(n, batch, dev, False, act, bias, fused, w8_fc2, stream, what=what + " (widened bf16)")
    assert not seen and len(sel) == len(ref) > 0
    for (step, li, inds, counts), (step_r, li_r, inds_r, counts_r) in zip(sel, ref):
        assert (step, li) == (step_r, li_r) and torch.equal(counts, counts_r), f"step {step} layer {li}: counts differ"
        live = torch.arange(inds.shape[-1], device=inds.device) < counts[..., None]
        assert torch.equal(inds[live], inds_r[live]), f"step {step} layer {li}: selected columns differ"


def test_key_off_the_constructor_raises(dev, fresh_config):
    from chipmunk_amd.modules import SparseDiffGatedMlp, W8Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    wg, bg, wu, bu, w2, b2 = gm.glu_weights(0, True)
    q = lambda w, b: W8Linear.from_linear(linear(w, b, dev))      # noqa: E731
    assert not fresh_config["mlp"]["w8_gated"]
    with pytest.raises(ValueError, match="only the ungated GEMM1 has a weight-only form"):
        SparseDiffGatedMlp(0, LayerCounter(1, 1), q(wg, bg), q(wu, bu), torch.nn.SiLU(), linear(w2, b2, dev))
    with pytest.raises(ValueError, match="only the ungated GEMM1 has a weight-only form"):
        SparseDiffGatedMlp.from_fused(0, LayerCounter(1, 1), q(torch.cat([wg, wu]), torch.cat([bg, bu])), torch.nn.SiLU(), linear(w2, b2, dev))
    fresh_config["mlp"]["w8_gated"] = True
    with pytest.raises(ValueError, match="mixed pair"):
        SparseDiffGatedMlp(0, LayerCounter(1, 1), q(wg, bg), linear(wu, bu, dev), torch.nn.SiLU(), linear(w2, b2, dev))
    assert SparseDiffGatedMlp(0, LayerCounter(1, 1), q(wg, bg), q(wu, bu), torch.nn.SiLU(), linear(w2, b2, dev)).w8
