"""The sparse-delta MLP with an fp8 ``fc2`` (``mlp.fp8_fc2``: an e4m3 ``F8Linear`` whose weight rows the sparse steps' GEMM2 gathers as
they are), for tests/test_gpu_mlp_fp8_fc2_e2e.py.  method_model.py, glu_method_model.py and glu_fp8_method_model.py are imported, not edited.

What changes in the method: a full step computes ``O = Q(A) W2^T + b2`` -- ``fc2`` quantises its input -- while every sparse step adds
``(A_new - A_old) W2^T`` of the UNQUANTISED bf16 deltas.  So ``O`` is no longer ``A W2^T + b2`` of the current activations but carries the
full step's quantisation residue ``(Q(A_full) - A_full) W2^T`` until the next full step.  The fp64 models of the imported helpers are used
as they are (their ``a``, ``fresh``, ``refreshed`` and ``weight`` do not involve ``fc2``) and `Fc2Checker` adds that residue to what they
return, from the module's own quantised operands, so that quantisation error is not counted:

* ``W2``: the layer's e4m3 weight times its reciprocal scale;
* at a full step, the activation as ``fc2`` quantised it: the module's bf16 activation (read back from the activation cache the step
  stored) through ``F8Linear.quantize_input``'s torch chain with the input scale the layer held at that call (it is still calibrating
  over the first calls), times the reciprocal input scale;
* the quantised ``x`` and ``fc1`` weights where ``fc1`` is fp8, as on the existing fp8 routes.

`Fc2Emulation` is the module's op sequence in torch (no chipmunk operator): a reference for the bounds, run by the GPU test beside the
module.  Bounds: ``MARGIN x MLP_FLOORS`` (``GLU_FLOORS`` for the gated route) and the selection shortfall of the corresponding existing
route.  Measured on an MI355X (docs/EXPERIMENTS_r13.md): module and emulation stay inside every floor, so none is pinned anew.
"""
import torch

import glu_fp8_method_model as gfp
import glu_method_model as gm
import method_model as mm

F8 = torch.float8_e4m3fn
OFFLOADED = {"global_disable_offloading": False, "mlp.sparse_act_T": True, "keep_resident_if_fits": False}


def scaled_mm_available(device):
    """torch's own fp8 GEMM, called as F8Linear calls it: its support varies with the ROCm build; nothing of the project runs here.
    Returns None, or the reason it is unavailable."""
    a = torch.zeros(16, mm.MLP_K, device=device).to(F8)
    b = torch.zeros(mm.MLP_F, mm.MLP_K, device=device).to(F8)
    one = torch.ones((), device=device)
    try:
        torch._scaled_mm(a, b.T, scale_a=one, scale_b=one, bias=torch.zeros(mm.MLP_F, device=device, dtype=torch.bfloat16),
                         out_dtype=torch.bfloat16, use_fast_accum=True)
    except (RuntimeError, NotImplementedError) as e:
        return str(e)
    return None


def f8_fc2(fc2):
    from chipmunk_amd.modules.mlp_fp8 import F8Linear
    return F8Linear.from_linear(fc2, input_float8_dtype=F8)


def dequantised_weight(lay):
    return lay.weight.data.double() * lay.scale_reciprocal.double()


def quantised_input(lay, act):
    """[n, f] fp64: bf16 `act` as `lay` quantised it in the call that just ended (F8Linear.quantize_input's torch chain with the scale the
    call left behind), times the reciprocal input scale"""
    q = (act * lay.input_scale).clamp(-lay.input_max_value, lay.input_max_value).to(lay.input_float8_dtype)
    return q.double() * lay.input_scale_reciprocal.double()


class Fc2Checker(mm.MlpChecker):
    """`MlpChecker` / `GluChecker` for modules whose ``fc2`` is an e4m3 F8Linear: any batch size (sequence b of invocation i is the
    model's invocation ``i B + b``), `dense_layers` dense layers in front, ``operand(module, x, full) -> [B, ...]`` what the model takes
    per sequence; the model's ``o`` and the invariant take the full step's quantisation residue (module docstring)."""

    def __init__(self, model, weights, n, batch, dense_layers, passed, floors=None, eps=None, operand=None, what=""):
        super().__init__(model, weights, n, floors, eps, operand, what)
        self.batch, self.dense_layers, self.passed, self.residue = batch, dense_layers, passed, {}

    def before(self, module, step, layer):
        self.pre = None
        if layer >= self.dense_layers and not self.model.is_full(step):
            self.pre = module.storage.get_sparse_act_T().clone()

    def check_values(self, res, out, act, out_cache, w2, b2, where, carried):
        ns = res["nsparse"]
        self._check("output", ns, mm.rel_rows(out, res["o"]), where)
        self._check("invariant", ns, mm.rel_rows(out_cache, act.double() @ w2.T + b2 + carried), where)
        self._check("cache", ns, mm.rel_rows(act, res["a"]), where)
        if ns > 0:
            self._check("refreshed", ns, mm.rel_rows(act, res["fresh"], res["refreshed"]), where)

    def after(self, step, inv, layer, module, args, out):
        x = args[0]
        full = self.model.is_full(step)
        w = [None if t is None else t.to(x.device).double() for t in self.weights[layer]]
        w2, b2 = w[-2], w[-1]
        xm = self.operand(module, x, full)
        if layer < self.dense_layers:       # (ungated, bf16: the dense layers in front keep their nn.Linear)
            for b in range(x.shape[0]):
                exact = mm.gelu_tanh(xm[b].double() @ w[0].T + w[1]) @ w2.T + b2
                self._check("output", 0, mm.rel_rows(out[b], exact), f"step {step} invocation {inv} sequence {b} layer {layer}")
            return
        st, fc2 = module.storage, module.fc2[0]
        out = out.clone()       # (the module hands back the output cache's slot itself)
        mm.reload_current(st)
        stored = st.get_sparse_act_T()
        assert stored.shape[-1] == (self.n + 7) // 8 * 8 and (stored[..., self.n:] == 0).all(), f"step {step} layer {layer}: padding columns of the cache"
        for b in range(x.shape[0]):
            seq = inv * self.batch + b
            where = f"step {step} invocation {inv} sequence {b} layer {layer}"
            sel = None if full else (st.get_indices()[b], st.get_counts()[b])
            res = self.model.step(step, seq, layer, xm[b], sel)
            act_t = stored[b][:, : self.n]
            if full:
                act = act_t.T                                   # the module's bf16 activation, as fc2 got it
                qa = quantised_input(fc2, act)
                # (what O carries beyond the model's A W2^T + b2, what out_cache carries beyond act_cache^T W2^T + b2)
                self.residue[(layer, seq)] = ((qa - res["a"]) @ w2.T, (qa - act.double()) @ w2.T)
            to_model, to_cache = self.residue[(layer, seq)]
            res = dict(res, o=res["o"] + to_model)
            self.check_values(res, out[b], act_t.T, st.get_out_cache()[b], w2, b2, where, to_cache)
            if not full:
                same = (act_t.view(torch.int16) == self.pre[b][:, : self.n].view(torch.int16)) | res["refreshed"].T
                assert same.all(), f"{where}: {int((~same).sum())} cache elements outside the selection changed"
            if res["weight"] is not None:
                frac = min(mm.captured_fraction(res["weight"], sel[0], sel[1], self.passed))
                self.shortfall = max(self.shortfall, 1.0 - frac)
                if self.eps is not None:
                    assert 1.0 - frac <= self.eps, f"{where}: the selection captures {frac:.4f} of what the exact top-|S| captures"


# ------------------------------------------------------------------------------------------------------------------ ungated routes
def build_mlps(device, fp8_fc1, make_module):
    """mm.build_mlps with an e4m3 F8Linear fc2 (and, for `fp8_fc1`, fc1) behind the dense layers; ``make_module(layer, fc1, fc2)``."""
    from chipmunk_amd.modules.mlp_fp8 import F8Linear
    mods, weights = [], []
    for li in range(mm.MLP_LAYERS):
        w1, b1, w2, b2 = mm.mlp_weights(li, mm.MLP_K, mm.MLP_F)
        fc1, fc2 = torch.nn.Linear(mm.MLP_K, mm.MLP_F), torch.nn.Linear(mm.MLP_F, mm.MLP_K)
        with torch.no_grad():
            for prm, val in ((fc1.weight, w1), (fc1.bias, b1), (fc2.weight, w2), (fc2.bias, b2)):
                prm.copy_(val)
        fc1, fc2 = fc1.to(device).bfloat16(), fc2.to(device).bfloat16()
        w1m, w2m = fc1.weight.data.double(), fc2.weight.data.double()
        if li >= mm.MLP_DENSE_LAYERS:
            if fp8_fc1:
                fc1 = F8Linear.from_linear(fc1, input_float8_dtype=F8)
                w1m = dequantised_weight(fc1)
            fc2 = f8_fc2(fc2)
            w2m = dequantised_weight(fc2)
        mods.append(make_module(li, fc1, fc2))
        weights.append((w1m, fc1.bias.data.double(), w2m, fc2.bias.data.double()))
    return mods, weights


def run_mlp_route(route, n, batch, device, make_module, floors=None, eps=None, what="", offloading=None):
    """`mm.run_mlp_route` over ``mm.MLP_ROUTES_GPU[route]`` with `batch` sequences per call and an fp8 fc2 (``mlp.fp8_fc2`` on)."""
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    n_inv, steps, every, cache = mm.configure_mlp(GLOBAL_CONFIG, route)
    GLOBAL_CONFIG["offloading"].update(offloading or {})
    GLOBAL_CONFIG["mlp"]["fp8_fc2"] = True
    mods, weights = build_mlps(device, route == "wan_fp8", make_module)
    model = mm.MlpMethodModel(weights, every, cache, GLOBAL_CONFIG["mlp"]["bm"])
    chk = Fc2Checker(model, weights, n, batch, mm.MLP_DENSE_LAYERS, mm.MLP_PASSED, floors, eps, lambda mod, x, full: mm.fp8_operand(mod, x),
                     what or route)

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (torch.cat([mm.mlp_input(step, inv * batch + b, li, n, mm.MLP_K) for b in range(batch)]).to(device),)

    mm.drive(mods, n_inv, steps, inputs, chk.after)
    chk.modules = mods
    return chk


# ------------------------------------------------------------------------------------------------------------------ gated route
def run_glu_route(route, device, make_module, floors=None, eps=None, what="", offloading=None, fused_scatter=True):
    """`gfp.run_route` (F8Linear projections) with an fp8 fc2; ``make_module(layer, projs, fc2, fused, act)``."""
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    gm.configure(GLOBAL_CONFIG, offloading, fused_scatter)
    GLOBAL_CONFIG["mlp"]["fp8_fc2"] = True
    act, bias, B, n, fused = gfp.ROUTES[route]
    mods, weights = [], []
    for li in range(gfp.LAYERS):
        projs, fc2 = gfp.f8_layers(gm.glu_weights(li, bias), fused, device)
        w = gfp.model_weights(projs, fc2, fused)
        fc2 = f8_fc2(fc2)
        weights.append(w[:4] + (dequantised_weight(fc2), w[5]))
        mods.append(make_module(li, projs, fc2, fused, act))
    model = gfp.Fp8GluMethodModel(weights, act, gfp.SCHEDULE["full_step_every"], gfp.SCHEDULE["block_mask_cache"])
    chk = Fc2Checker(model, weights, n, B, 0, gm.PASSED, floors, eps, gfp.fp8_operands, what or route)

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (torch.cat([mm.mlp_input(step, b, li, n, gfp.K) for b in range(B)]).to(device),)

    mm.drive(mods, 1, gfp.STEPS, inputs, chk.after)
    chk.modules = mods
    return chk


# ------------------------------------------------------------------------------------------------------------------ emulation
class Fc2Emulation:
    """SparseDiffMlp's op sequence with a bf16 fc1 and an e4m3 F8Linear fc2 (mbm == bm == 128, one model invocation per step) in torch,
    bf16 wherever the module holds bf16, exact sums inside a GEMM or a mean; full steps through fc2's own forward (torch._scaled_mm),
    the selection through `glu_method_model.topk_rows`, the sparse GEMM2 as ``bf16(bf16((delta @ f(W2q)^T[cols]) s) + out)`` on the
    e4m3 weight.  No chipmunk operator (run it with ``mlp.fused_fp8_quantize`` off, so that fc2 quantises with the torch chain)."""

    def __init__(self, layer, fc1, fc2, cfg, dense_layers):
        assert cfg["num_model_invocations_per_inference_step"] == 1 and fc1.weight.dtype == torch.bfloat16
        self.fc1, self.fc2, self.cfg, self.dense = [fc1], [fc2], cfg["mlp"], layer < dense_layers
        self.storage, self.calls = gm._Store(), 0

    means = gm.GluEmulation.means
    lin = gm.GluEmulation.lin

    def __call__(self, x):
        bf = gm.bf
        fc1, fc2 = self.fc1[0], self.fc2[0]
        w1, b1 = fc1.weight.data, fc1.bias.data
        if self.dense:
            return self.lin(bf(mm.gelu_tanh(self.lin(x, w1, b1).double())), fc2.weight.data, fc2.bias.data)
        step, v = self.calls, self.storage.v
        self.calls += 1
        B, n, _ = x.shape
        if step % self.cfg["full_step_every"] == 0:
            mid = self.lin(x, w1, b1)
            h = bf(mm.gelu_tanh(mid.double()))
            out = fc2(h)
            ld = (n + 7) // 8 * 8
            cache = torch.zeros(B, h.shape[-1], ld, dtype=torch.bfloat16, device=x.device)
            cache[..., :n] = h.transpose(1, 2)
            v.update(sparse_act_T=cache, out_cache=out, blockmean_mid_cache=self.means(mid))
            return out
        if not (step % self.cfg["block_mask_cache"] != 0 and step >= 10 and "indices" in v):
            pre = self.lin(self.means(x), w1, b1)
            bmc = v["blockmean_mid_cache"]
            score = bf(bf(pre.double() - bmc.double()).abs())
            inds, counts = gm.topk_rows(score.reshape(-1, score.shape[-1]).cpu(), 1 - self.cfg["top_keys"], self.cfg["counts_multiple_of"])
            inds, counts = inds.reshape(score.shape).to(x.device), counts.reshape(score.shape[:2]).to(x.device)
            sel = torch.stack([mm.selection_mask(inds[b], counts[b], inds.shape[1], inds.shape[2], 1) for b in range(B)])
            v["blockmean_mid_cache"] = torch.where(sel, pre, bmc)
            v["indices"], v["counts"] = inds, counts
        w2q, s2 = fc2.weight.data.double(), fc2.scale_reciprocal.double()
        out, cache = v["out_cache"].clone(), v["sparse_act_T"].clone()
        for b in range(B):
            inds, counts = v["indices"][b], v["counts"][b]
            for g in range(inds.shape[0]):
                rows, cnt = slice(g * 128, min(n, (g + 1) * 128)), int(counts[g])
                cols = inds[g, :cnt].long()
                old = cache[b][cols][:, rows].double().T
                dg = bf(mm.gelu_tanh(x[b, rows].double() @ w1[cols].double().T + b1[cols].double()) - old)     # GEMM1: one bf16 rounding
                cache[b][cols, rows] = bf(old.T + dg.double().T)                                              # scatter-add, bf16
                out[b, rows] = bf(bf((dg.double() @ w2q.T[cols]) * s2).double() + out[b, rows].double())      # GEMM2 on the e4m3 rows
        v.update(sparse_act_T=cache, out_cache=out)
        return out
