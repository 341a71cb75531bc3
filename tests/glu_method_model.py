"""The sparse-delta method for GATED feed-forwards, ``fc2(act(x Wg^T + bg) * (x Wu^T + bu))``, in fp64 (`GluMethodModel`: `MlpMethodModel`'s
step with ``fresh = act(h_g) * h_u`` and the block means of both pre-activations), the checker the GPU test runs after every
SparseDiffGatedMlp call (`GluChecker`), and two bf16 stand-ins in plain torch that call no chipmunk operator:

* `mm1_glu_mirror`: the gated GEMM1 operator (exact sums of bf16 operands, act * up - cache, one bf16 rounding);
* `GluEmulation`: the module's whole op sequence with every tensor rounded to bf16 where the module rounds: a bf16 reference for the
  module bounds (`GLU_FLOORS`).

``defect=`` turns model / mirror into one of the mutants of tests/test_mlp_glu_host.py.
"""
import torch

import method_model as mm

ACTS = ("gelu_tanh", "silu", "gelu")
GLU_DEFECTS = ("halves_swapped", "act_on_product", "cache_before_product", "up_bias_dropped", "gate_means_only", "up_means_not_copied")

# the module test: two layers, 333 tokens (three groups, the last of 77 rows; a pitched cache), 13 steps.  F = 1024 is the fewest
# columns `topk_indices` takes (its quantile is read off the first 1024 columns of a row), so the module cannot run at the operator
# test's F = 512.
K, F, N, LAYERS, STEPS = 256, 1024, 333, 2, 13
SCHEDULE = dict(full_step_every=10, block_mask_cache=2, first_n_dense_layers=0, top_keys=0.3, random_keys=0.0, counts_multiple_of=256)
PASSED = F - int(F * (1 - SCHEDULE["top_keys"]))       # columns that pass the method's threshold (see method_model.MLP_PASSED)
# route -> (activation, biases, batch size)
ROUTES = {"silu": ("silu", False, 1), "gelu_tanh_bias": ("gelu_tanh", True, 1), "silu_b2": ("silu", False, 2)}


def act64(name, x):
    if name == "gelu_tanh":
        return mm.gelu_tanh(x)
    if name == "silu":
        return x * torch.sigmoid(x)
    assert name == "gelu", name
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def act_module(name):
    return {"gelu_tanh": torch.nn.GELU(approximate="tanh"), "silu": torch.nn.SiLU(), "gelu": torch.nn.GELU()}[name]


def glu_weights(layer, bias, k=K, f=F):
    """(Wg [f, k], bg [f] | None, Wu, bu | None, W2 [k, f], b2 [k]) rounded to bf16 (as the module holds them), in fp32"""
    wg, bg, w2, b2 = mm.mlp_weights(layer, k, f, seed=0)
    wu, bu, _, _ = mm.mlp_weights(layer, k, f, seed=1)
    r = lambda t: t.to(torch.bfloat16).float()      # noqa: E731
    return r(wg), r(bg) if bias else None, r(wu), r(bu) if bias else None, r(w2), r(b2)


def paired_means(hg, hu, bm):
    """[n, f] gate / up pre-activations -> [2 G, f]: rows 2i / 2i + 1 = gate / up mean of block i"""
    g, u = mm.block_mean64(hg, bm), mm.block_mean64(hu, bm)
    return torch.stack([g, u], dim=1).reshape(2 * g.shape[0], g.shape[1])


# ------------------------------------------------------------------------------------------------------------------ fp64 model
class GluMethodModel(mm.MlpMethodModel):
    """``weights[layer] = (Wg, bg | None, Wu, bu | None, W2, b2)``; schedule and selection handling of `MlpMethodModel` (mbm == bm)."""

    def __init__(self, weights, act, full_step_every, block_mask_cache, bm=128, defect=None):
        assert defect is None or defect in GLU_DEFECTS, defect
        assert act in ACTS, act
        self.w = [tuple(None if t is None else t.double() for t in w) for w in weights]
        self.act, self.full_every, self.mask_cache, self.bm, self.defect = act, full_step_every, block_mask_cache, bm, defect
        self.state = {}

    def pre(self, layer, x):
        wg, bg, wu, bu, w2, b2 = (None if t is None else t.to(x.device) for t in self.w[layer])
        zero = torch.zeros(wg.shape[0], dtype=torch.float64, device=x.device)
        bg, bu = zero if bg is None else bg, zero if bu is None else bu
        return x.double() @ wg.T + bg, x.double() @ wu.T + bu, bu, w2, b2

    def step(self, step, inv, layer, x, sel=None):
        """As `MlpMethodModel.step`; ``weight`` [g, f] is the sum of |Bm_new - Bm_cache| over the group's gate and up rows."""
        hg, hu, bu, w2, b2 = self.pre(layer, x)
        key = (layer, inv)
        st = self.state.setdefault(key, {})
        fresh = act64(self.act, hg) * hu
        n, f = fresh.shape
        if self.is_full(step):
            st.update(o=fresh @ w2.T + b2, bm=paired_means(hg, hu, self.bm), nsparse=0, a=fresh)
            return dict(o=st["o"], a=fresh, fresh=fresh, refreshed=torch.ones_like(fresh, dtype=torch.bool), weight=None, nsparse=0)
        weight = None
        if not self.reuses_selection(step, key):
            bm_new = paired_means(hg, hu, self.bm)
            diff = (bm_new - st["bm"]).abs()
            weight = diff[0::2] if self.defect == "gate_means_only" else diff[0::2] + diff[1::2]
            st["sel"] = sel
            gm = mm.selection_mask(sel[0], sel[1], sel[0].shape[0], f, 1).repeat_interleave(2, dim=0)
            if self.defect == "up_means_not_copied":
                gm[1::2] = False
            st["bm"] = torch.where(gm, bm_new, st["bm"])
        inds, counts = st["sel"]
        m = mm.selection_mask(inds, counts, n, f, self.bm)
        st["nsparse"] += 1
        new = fresh
        if self.defect == "halves_swapped":
            new = act64(self.act, hu) * hg
        elif self.defect == "act_on_product":
            new = act64(self.act, hg * hu)
        elif self.defect == "up_bias_dropped":
            new = act64(self.act, hg) * (hu - bu)
        elif self.defect == "cache_before_product":
            new = st["a"] + (act64(self.act, hg) - st["a"]) * hu
        a = torch.where(m, new, st["a"])
        o = a @ w2.T + b2
        st.update(o=o, a=a)
        return dict(o=o, a=a, fresh=fresh, refreshed=m, weight=weight, nsparse=st["nsparse"])


# ------------------------------------------------------------------------------------------------------------------ bf16 stand-ins
def bf(t):
    return t.to(torch.bfloat16)


# (Sums and activations of the stand-ins are taken in fp64 and rounded ONCE to bf16 where the module rounds: torch's own fp32 / bf16 CPU
# kernels round differently with the thread count and the instruction set, see tests/cpu_ops.py.)
def mm1_glu_mirror(a, wg, wu, bg, bu, act, cache, inds, counts, sentinel=7.0, defect=None):
    """The gated GEMM1 operator in plain torch (exact sums, one bf16 rounding of the result).  a [M, K], wg / wu [F, K], bg / bu [F] | None,
    cache [F, M] (all bf16), inds [G, F], counts [G] -> packed deltas [M, F] bf16 (columns at or past the count hold `sentinel`)."""
    M, f = a.shape[0], wg.shape[0]
    c = torch.full((M, f), sentinel, dtype=torch.bfloat16, device=a.device)
    for g in range(inds.shape[0]):
        rows, n = slice(g * 128, min(M, (g + 1) * 128)), int(counts[g])
        cols = inds[g, :n].long()
        w0, w1, b0, b1 = (wu, wg, bu, bg) if defect == "halves_swapped" else (wg, wu, bg, bu)
        hg = a[rows].double() @ w0[cols].double().T + (0 if b0 is None else b0[cols].double())
        hu = a[rows].double() @ w1[cols].double().T + (0 if b1 is None or defect == "up_bias_dropped" else b1[cols].double())
        old = cache[cols][:, rows].double().T
        if defect == "act_on_product":
            d = act64(act, hg * hu) - old
        elif defect == "cache_before_product":
            d = (act64(act, hg) - old) * hu
        else:
            d = act64(act, hg) * hu - old
        c[rows, :n] = bf(d)
    return c


def topk_rows(w, sparsity, multiple_of):
    """`topk_indices` without random keys on [R, F] rows: the threshold is element int(1024 sparsity) of the ascending first 1024 values,
    columns at or above it are kept in ascending order, and the count is rounded up to `multiple_of` with the last rejected column of
    every residue mod 1024, residues ascending."""
    R, f = w.shape
    inds, counts = torch.full((R, f), -1, dtype=torch.int32), torch.zeros(R, dtype=torch.int32)
    for r in range(R):
        row = w[r].float()
        thr = row[:1024].sort().values[int(1024 * sparsity)]
        keep = row >= thr
        kept = torch.nonzero(keep).flatten()
        rejected = torch.nonzero(~keep).flatten()
        last = {}
        for c in rejected.tolist():
            last[c % 1024] = c
        pad = (-kept.numel()) % multiple_of
        lst = torch.cat([kept, torch.tensor([last[t] for t in sorted(last)][:pad], dtype=torch.long)])
        inds[r, : lst.numel()] = lst.to(torch.int32)
        counts[r] = lst.numel()
    return inds, counts


class _Store:
    """the getters of MlpStorage over plain attributes; nothing is offloaded, so the protocol calls have nothing to do"""

    def __init__(self):
        self.v = {}

    def __getattr__(self, name):
        if name.startswith("get_"):
            return lambda: self.v.get(name[4:])
        if name in ("load_async", "load_async_wait", "complete_cur_layer"):
            return lambda: None
        raise AttributeError(name)


class GluEmulation:
    """SparseDiffGatedMlp's op sequence (mbm == bm == 128, fused scatter or not: the same arithmetic) in torch on any device, bf16 wherever
    the module holds bf16, exact sums inside a GEMM or a mean.  B >= 1."""

    def __init__(self, weights, act, cfg, counter_steps):
        self.w, self.act, self.cfg = weights, act, cfg
        self.storage, self.calls, self.every = _Store(), 0, counter_steps

    def lin(self, x, w, b):
        return bf(x.double() @ w.double().T + (0 if b is None else b.double()))

    def means(self, t):
        return bf(torch.stack([t[:, a:a + 128].double().mean(dim=1) for a in range(0, t.shape[1], 128)], dim=1))

    def paired(self, g, u):
        return torch.stack([g, u], dim=2).reshape(g.shape[0], 2 * g.shape[1], g.shape[2])

    def __call__(self, x):
        wg, bg, wu, bu, w2, b2 = (None if t is None else bf(t.to(x.device)) for t in self.w)
        step, v = self.calls, self.storage.v
        self.calls += 1
        B, n, _ = x.shape
        if step % self.cfg["full_step_every"] == 0:
            g, u = self.lin(x, wg, bg), self.lin(x, wu, bu)
            h = bf(bf(act64(self.act, g.double())).double() * u.double())
            out = self.lin(h, w2, b2)
            ld = (n + 7) // 8 * 8
            cache = torch.zeros(B, h.shape[-1], ld, dtype=torch.bfloat16, device=x.device)
            cache[..., :n] = h.transpose(1, 2)
            v.update(sparse_act_T=cache, out_cache=out, blockmean_mid_cache=self.paired(self.means(g), self.means(u)))
            return out
        if not (step % self.cfg["block_mask_cache"] != 0 and step >= 10 and "indices" in v):
            bmx = self.means(x)
            pre = self.paired(self.lin(bmx, wg, bg), self.lin(bmx, wu, bu))
            bmc = v["blockmean_mid_cache"]
            mdiff = bf(bf(pre.double() - bmc.double()).abs())
            score = bf(mdiff.double().reshape(B, -1, 2, mdiff.shape[-1]).sum(dim=2))
            inds, counts = topk_rows(score.reshape(-1, score.shape[-1]).cpu(), 1 - self.cfg["top_keys"], self.cfg["counts_multiple_of"])
            inds, counts = inds.reshape(score.shape).to(x.device), counts.reshape(score.shape[:2]).to(x.device)
            gm = torch.stack([mm.selection_mask(inds[b], counts[b], inds.shape[1], inds.shape[2], 1) for b in range(B)])
            v["blockmean_mid_cache"] = torch.where(gm.repeat_interleave(2, dim=1), pre, bmc)
            v["indices"], v["counts"] = inds, counts
        out, cache = v["out_cache"].clone(), v["sparse_act_T"].clone()
        for b in range(B):
            inds, counts = v["indices"][b], v["counts"][b]
            d = mm1_glu_mirror(x[b], wg, wu, bg, bu, self.act, cache[b][:, :n], inds, counts)
            for g in range(inds.shape[0]):
                rows, cnt = slice(g * 128, min(n, (g + 1) * 128)), int(counts[g])
                cols = inds[g, :cnt].long()
                dg = d[rows, :cnt]
                cache[b][cols, rows] = bf(cache[b][cols][:, rows].double() + dg.double().T)            # scatter-add, bf16
                out[b, rows] = bf(bf(dg.double() @ w2.T[cols].double()).double() + out[b, rows].double())  # GEMM2: bf16(acc) + C in bf16
        v.update(sparse_act_T=cache, out_cache=out)
        return out


# ------------------------------------------------------------------------------------------------------------------ checker, driver
# The bounds are those of the ungated bf16 route: method_model.MLP_FLOORS (indexed by the sparse steps since the full step, the last
# entry, three, standing for every longer run) x ROW_ERR_MARGIN, and 2 x MLP_SELECTION_SHORTFALL.  The gated route stays inside them, on
# the MI355X and in `GluEmulation` alike -- worst over all routes, both scatter settings, resident and offloaded (the two agree to the
# digits shown): output 0.0056 at a full step rising to 0.0092 after nine sparse steps in a row (bound 0.0104), out_cache against its
# own activation cache 0.0020 -> 0.0092 (0.0104), activation cache 0.0050 -> 0.0032 (0.0066 -> 0.0054), refreshed columns at most
# 0.0036 (0.0048), selection shortfall 0.000062 (0.00018).  tests/test_mlp_glu_host.py holds the emulation to them and shows every
# mutant outside.
GLU_FLOORS = mm.MLP_FLOORS
GLU_SELECTION_SHORTFALL = mm.MLP_SELECTION_SHORTFALL


class GluChecker(mm.MlpChecker):
    """`MlpChecker` for SparseDiffGatedMlp (or `GluEmulation`): no dense first layer, any batch size (sequence b is the model's
    invocation b), the gated model's weight in the selection check."""

    def before(self, module, step, layer):
        self.pre = None if self.model.is_full(step) else module.storage.get_sparse_act_T().clone()

    def after(self, step, inv, layer, module, args, out):
        x = args[0]
        w2, b2 = (t.to(x.device) for t in self.weights[layer][4:])
        st = module.storage
        out = out.clone()       # (the module hands back the output cache's slot itself)
        mm.reload_current(st)
        full = self.model.is_full(step)
        stored = st.get_sparse_act_T()
        assert stored.shape[-1] == (self.n + 7) // 8 * 8 and (stored[..., self.n:] == 0).all(), f"step {step} layer {layer}: padding columns of the cache"
        for b in range(x.shape[0]):
            where = f"step {step} sequence {b} layer {layer}"
            sel = None if full else (st.get_indices()[b], st.get_counts()[b])
            res = self.model.step(step, b, layer, x[b], sel)
            act_t = stored[b][:, : self.n]
            self.check_values(res, out[b], act_t.T, st.get_out_cache()[b], w2, b2, where)
            if not full:
                same = (act_t.view(torch.int16) == self.pre[b][:, : self.n].view(torch.int16)) | res["refreshed"].T
                assert same.all(), f"{where}: {int((~same).sum())} cache elements outside the selection changed"
            if res["weight"] is not None:
                frac = min(mm.captured_fraction(res["weight"], sel[0], sel[1], PASSED))
                self.shortfall = max(self.shortfall, 1.0 - frac)
                if self.eps is not None:
                    assert 1.0 - frac <= self.eps, f"{where}: the selection captures {frac:.4f} of what the exact top-|S| captures"


def configure(cfg, offloading=None, fused_scatter=True):
    cfg["num_model_invocations_per_inference_step"] = 1
    cfg["steps"] = 50
    cfg["mlp"].update(SCHEDULE)
    cfg["mlp"]["fused_scatter"] = fused_scatter
    cfg["offloading"].update(offloading or {"global_disable_offloading": True})
    return cfg["mlp"]


def inputs_for(route, device):
    B = ROUTES[route][2]
    return lambda step, layer: torch.cat([mm.mlp_input(step, b, layer, N, K) for b in range(B)]).to(device)


def run_route(route, device, make_module, floors=None, eps=None, what="", trace=None, defect=None):
    """Drive LAYERS modules from ``make_module(layer, weights, act)`` over the schedule by the integration protocol, with the checker's
    assertions after every call (call `configure` first).  Returns the checker."""
    act, bias, _B = ROUTES[route]
    weights = [glu_weights(li, bias) for li in range(LAYERS)]
    mods = [make_module(li, weights[li], act) for li in range(LAYERS)]
    model = GluMethodModel(weights, act, SCHEDULE["full_step_every"], SCHEDULE["block_mask_cache"], defect=defect)
    chk = GluChecker(model, weights, N, floors, eps, None, what or route)
    x_of = inputs_for(route, device)

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (x_of(step, li),)

    def after(step, inv, li, mod, args, out):
        if trace is not None:
            mm.reload_current(mod.storage)
            sel = None if model.is_full(step) else (mod.storage.get_indices().clone(), mod.storage.get_counts().clone())
            trace.append(dict(step=step, layer=li, x=args[0], sel=sel))
        chk.after(step, inv, li, mod, args, out)

    mm.drive(mods, 1, STEPS, inputs, after)
    chk.modules = mods
    return chk
