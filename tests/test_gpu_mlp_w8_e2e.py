"""SparseDiffMlp over a weight-only ``W8Linear`` ``fc1`` (``mlp.fp8_weight_only``) on the device against the fp64 model of the sparse-delta
method (tests/method_model.py) evaluated on the WIDENED weights: a ``W8Linear`` is the bf16 linear layer over ``weight.to(bf16) *
scale_reciprocal`` (exact: power-of-two scales), so there is no quantisation error to set aside and no residue -- the plain model, the
floors ``MLP_FLOORS`` x 2 and the existing selection bound, as tests/test_gpu_mlp_fp8_fc2_e2e.py holds its routes to.

The `flux` schedule at N = 1003, B = 1 (ragged last group, pitched cache) and N = 1024, B = 2; once more with a ``W8Linear`` ``fc2`` under
``mlp.fp8_fc2`` (GEMM2 gathers e4m3 rows as well) and once with the activation cache offloaded.  Sparse layer 1 scales its ``fc1`` per
tensor, layer 2 per output feature.  Dense and full steps and the block-mean probe go through ``W8Linear.forward``, the sparse steps through
``csp_mlp_mm1_w8``; the selections are those of the same modules over the widened bf16 ``nn.Linear``, index for index."""
import pytest
import torch

import fp8_fc2_method_model as f2
import method_model as mm

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


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


class W8Checker(f2.Fc2Checker):
    """`Fc2Checker` (any batch size, dense layers in front) without its residue: no layer quantises an activation here"""

    def after(self, step, inv, layer, module, args, out):
        x = args[0]
        full = self.model.is_full(step)
        w = [t.to(x.device).double() for t in self.weights[layer]]
        w2, b2 = w[-2], w[-1]
        if layer < self.dense_layers:
            for b in range(x.shape[0]):
                exact = mm.gelu_tanh(x[b].double() @ w[0].T + w[1]) @ w2.T + b2
                self._check("output", 0, mm.rel_rows(out[b], exact), f"step {step} invocation {inv} sequence {b} layer {layer}")
            return
        st = module.storage
        out = out.clone()       # (the module hands back the output cache's slot itself)
        mm.reload_current(st)
        stored = st.get_sparse_act_T()
        assert stored.shape[-1] == (self.n + 7) // 8 * 8 and (stored[..., self.n:] == 0).all(), f"step {step} layer {layer}: padding columns of the cache"
        for b in range(x.shape[0]):
            seq = inv * self.batch + b
            where = f"step {step} invocation {inv} sequence {b} layer {layer}"
            sel = None if full else (st.get_indices()[b], st.get_counts()[b])
            res = self.model.step(step, seq, layer, x[b], sel)
            act_t = stored[b][:, : self.n]
            self.check_values(res, out[b], act_t.T, st.get_out_cache()[b], w2, b2, where, 0.0)
            if not full:
                same = (act_t.view(torch.int16) == self.pre[b][:, : self.n].view(torch.int16)) | res["refreshed"].T
                assert same.all(), f"{where}: {int((~same).sum())} cache elements outside the selection changed"
            if res["weight"] is not None:
                frac = min(mm.captured_fraction(res["weight"], sel[0], sel[1], self.passed))
                self.shortfall = max(self.shortfall, 1.0 - frac)
                if self.eps is not None:
                    assert 1.0 - frac <= self.eps, f"{where}: the selection captures {frac:.4f} of what the exact top-|S| captures"


def widened_linear(q):
    """the bf16 nn.Linear a W8Linear stands for"""
    lin = torch.nn.Linear(q.in_features, q.out_features, bias=q.bias is not None).to(q.weight.device).bfloat16()
    with torch.no_grad():
        lin.weight.copy_(q.widened())
        if q.bias is not None:
            lin.bias.copy_(q.bias)
    return lin


def run_route(n, batch, device, weight_only, w8_fc2=False, offloading=None, floors=None, eps=None, what=""):
    """the `flux` schedule of tests/method_model.py with `batch` sequences per call; weight_only: the sparse layers' fc1 (and, `w8_fc2`, fc2)
    are W8Linear, otherwise the nn.Linear over the same widened weights.  Returns (checker, selections per sparse call)."""
    from chipmunk_amd.modules import SparseDiffMlp, W8Linear
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    from chipmunk_amd.util.layer_counter import LayerCounter
    n_inv, steps, every, cache = mm.configure_mlp(GLOBAL_CONFIG, "flux")
    GLOBAL_CONFIG["offloading"].update(offloading or {"global_disable_offloading": True})
    GLOBAL_CONFIG["mlp"]["fp8_fc2"] = bool(w8_fc2)
    counter, gelu = LayerCounter(mm.MLP_LAYERS, 1), torch.nn.GELU(approximate="tanh")
    mods, weights = [], []
    for li in range(mm.MLP_LAYERS):
        w1, b1, w2, b2 = mm.mlp_weights(li, mm.MLP_K, mm.MLP_F)
        fc1, fc2 = torch.nn.Linear(mm.MLP_K, mm.MLP_F), torch.nn.Linear(mm.MLP_F, mm.MLP_K)
        with torch.no_grad():
            for prm, val in ((fc1.weight, w1), (fc1.bias, b1), (fc2.weight, w2), (fc2.bias, b2)):
                prm.copy_(val)
        fc1, fc2 = fc1.to(device).bfloat16(), fc2.to(device).bfloat16()
        if li >= mm.MLP_DENSE_LAYERS:
            q1 = W8Linear.from_linear(fc1, scaling="row" if li % 2 == 0 else "tensor")
            fc1 = q1 if weight_only else widened_linear(q1)
            if w8_fc2:
                q2 = W8Linear.from_linear(fc2)
                fc2 = q2 if weight_only else widened_linear(q2)
        wide = lambda lay: lay.widened().double() if isinstance(lay, W8Linear) else lay.weight.data.double()      # noqa: E731
        mods.append(SparseDiffMlp(li, counter, fc1, gelu, fc2, 6))
        weights.append((wide(fc1), fc1.bias.data.double(), wide(fc2), fc2.bias.data.double()))
    model = mm.MlpMethodModel(weights, every, cache, GLOBAL_CONFIG["mlp"]["bm"])
    chk = W8Checker(model, weights, n, batch, mm.MLP_DENSE_LAYERS, mm.MLP_PASSED, floors, eps, lambda mod, x, full: x, what)
    selections = []

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (torch.cat([mm.mlp_input(step, inv * batch + b, li, n, mm.MLP_K) for b in range(batch)]).to(device),)

    def after(step, inv, li, mod, args, out):
        chk.after(step, inv, li, mod, args, out)
        if li >= mm.MLP_DENSE_LAYERS and not model.is_full(step):
            selections.append((step, li, mod.storage.get_indices().clone(), mod.storage.get_counts().clone()))

    mm.drive(mods, n_inv, steps, inputs, after)
    chk.modules = mods
    return chk, selections


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


CASES = [(1003, 1, False, "resident"), (1024, 2, False, "resident"), (1003, 1, True, "resident"), (1003, 1, False, "offloaded")]


@pytest.mark.parametrize("n,batch,w8_fc2,res", CASES, ids=[f"n{n} b{b}{' w8 fc2' if f else ''} {r}" for n, b, f, r in CASES])
def test_module_over_a_weight_only_fc1_against_the_method_model(dev, n, batch, w8_fc2, res):
    from chipmunk_amd.modules import W8Linear
    what = f"mlp w8 fc1 flux, n {n}, b {batch}{', w8 fc2' if w8_fc2 else ''}, {res}"
    offloading = f2.OFFLOADED if res == "offloaded" else None
    chk, sel = run_route(n, batch, dev, True, w8_fc2, offloading, floors=mm.MLP_FLOORS, eps=2 * mm.MLP_SELECTION_SHORTFALL, what=what)
    report(what, chk)
    assert ("output", 3) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    for m in chk.modules[mm.MLP_DENSE_LAYERS:]:
        assert isinstance(m.fc1[0], W8Linear) and m.fc1[0].weight.dtype == E4M3
        assert (m.fc2w_T[0].dtype == E4M3) == w8_fc2
    assert chk.modules[-1].storage.sparse_act_T.is_resident() == (res == "resident")
    assert {tuple(m.fc1[0].scale_reciprocal.shape) for m in chk.modules[mm.MLP_DENSE_LAYERS:]} == {(), (mm.MLP_F,)}, "both scale granularities ran"
    # the same modules over the widened bf16 nn.Linear make the same selections
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    torch.cuda.synchronize()
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)
    ot.gpu_tensors.clear()
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    _, ref = run_route(n, batch, dev, False, w8_fc2, offloading, what=what + " (widened bf16)")
    assert len(sel) == len(ref) > 0
    for (step, li, inds, counts), (step_r, li_r, inds_r, counts_r) in zip(sel, ref):
        assert (step, li) == (step_r, li_r) and torch.equal(counts, counts_r), f"step {step} layer {li}: counts differ"
        live = torch.arange(inds.shape[-1], device=inds.device) < counts[..., None]
        assert torch.equal(inds[live], inds_r[live]), f"step {step} layer {li}: selected columns differ"


def test_the_sparse_steps_run_the_weight_only_gemm1(dev, monkeypatch):
    """csp_mlp_mm1_w8 is what a sparse step launches (with the fused scatter and without it), and no bf16 GEMM1 runs beside it"""
    import sys
    import chipmunk_amd.ops  # noqa: F401
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    ops_mlp = sys.modules["chipmunk_amd.ops.mlp"]             # (the package exports run_e2e under the module's name)
    seen = []
    real_w8, real_mm1 = ops_mlp.mm1_w8, ops_mlp.mm1_scatter

    def spy(x, fc1w, fc1_scale, *a, **kw):
        seen.append((x.dtype, fc1w.dtype, tuple(fc1_scale.shape), kw.get("update_cache")))
        return real_w8(x, fc1w, fc1_scale, *a, **kw)
    monkeypatch.setattr(ops_mlp, "mm1_w8", spy)
    for fused in (True, False):
        from chipmunk_amd.util import config as cfg
        from chipmunk_amd.util import layer_counter as lc
        from chipmunk_amd.util.storage import offloaded_tensor as ot
        torch.cuda.synchronize()
        cfg.reset_to_base()
        lc.singleton.__init__(0, 0)
        ot.gpu_tensors.clear()
        ot._resident_bytes = ot._kept_offloaded_bytes = 0
        GLOBAL_CONFIG["mlp"]["fused_scatter"] = fused
        seen.clear()
        chk, _ = run_route(1003, 1, dev, True, floors=mm.MLP_FLOORS, eps=2 * mm.MLP_SELECTION_SHORTFALL, what=f"fused_scatter {fused}")
        assert seen and all(s[0] == torch.bfloat16 and s[1] == E4M3 and s[3] == fused for s in seen), seen
        assert {s[2] for s in seen} == {(), (mm.MLP_F,)}
    assert real_mm1 is ops_mlp.mm1_scatter
