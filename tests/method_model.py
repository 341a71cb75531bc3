"""The sparse-delta method in fp64: what SparseDiffAttn / SparseDiffMlp compute over a schedule with CHANGING inputs, stated in plain torch
on any device.  No chipmunk operator is called by the models; the read-back helpers use the public storage getters and ``ops.bitunpack``.

The models take the module's own selection S as input (read back after each step that sets it), so that ties in a top-k and the
hash-random keys cannot matter: the models state what follows from S, the selection itself is held to the exact top-|S| separately.
State is kept per (layer, model invocation).  ``defect=`` turns a model into one of the mutants of tests/test_method_model_cpu.py.
"""
import math

import torch

import helpers

ATTN_DEFECTS = ("delta_persists", "cache_wrong_sign", "cache_before_subtraction", "stale_mask_after_recompute", "stale_kv",
                "other_invocation", "pipeline_slot_layer", "ragged_and_text_rows_no_delta", "kept_list_cut_to_128")
MLP_DEFECTS = ("stale_full_activations", "other_invocation_activations", "last_group_cache_stale", "delta_twice",
               "other_layer_indices_on_cached_mask", "bias_again", "block_means_not_copied")
PIPELINE_DEPTH = 2      # chipmunk_amd.util.storage.offloaded_tensor.PIPELINE_DEPTH: layers l and l +- 2 share a device slot


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31 - 1))


DRIFT = 1.0 / 3.0     # every step mixes a fixed base with fresh noise of a third of its size: a stale-state defect is then far above rounding


def mlp_input(step, inv, layer, n, k, seed=0):
    """x ``[1, n, k]`` bf16 (CPU): base of (layer, invocation) + DRIFT x fresh noise of (step, layer, invocation)."""
    base = torch.randn(1, n, k, generator=_gen(seed, 1, layer, inv))
    return (base + DRIFT * torch.randn(1, n, k, generator=_gen(seed, 2, layer, inv, step))).to(torch.bfloat16)


def mlp_weights(layer, k, f, seed=0):
    """(W1 [f, k], b1 [f], W2 [k, f], b2 [k]) fp32, uniform in +-1/sqrt(fan_in) as torch.nn.Linear draws them."""
    g = _gen(seed, 3, layer)
    u = lambda *shape, fan: (torch.rand(*shape, generator=g) * 2 - 1) / fan ** 0.5      # noqa: E731
    return u(f, k, fan=k), u(f, fan=k), u(k, f, fan=f), u(k, fan=f)


def attn_input(step, inv, layer, h, n, seed=0, gain=1.6):
    """q, k, v ``[1, h, n, 128]`` bf16 (CPU), base + DRIFT x noise as `mlp_input`; `gain` on q widens the score spread so that the
    column sums differ by far more than their bf16 rounding and a top-k over them means something."""
    out = []
    for j in range(3):
        base = torch.randn(1, h, n, 128, generator=_gen(seed, 4 + j, layer, inv))
        t = base + DRIFT * torch.randn(1, h, n, 128, generator=_gen(seed, 7 + j, layer, inv, step))
        out.append(((gain if j == 0 else 1.0) * t).to(torch.bfloat16))
    return out


# ------------------------------------------------------------------------------------------------------------------ MLP
def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def block_mean64(h, mbm):
    """[n, f] fp64 -> [ceil(n / mbm), f]: mean over the rows present of every block."""
    return torch.stack([h[a:a + mbm].mean(dim=0) for a in range(0, h.shape[0], mbm)])


def selection_mask(inds, counts, n, f, bm):
    """[n, f] bool: row i refreshes the columns ``inds[i // bm, :counts[i // bm]]``."""
    g = inds.shape[0]
    m = torch.zeros(g, f, dtype=torch.bool, device=inds.device)
    for i in range(g):
        m[i, inds[i, : int(counts[i])].long()] = True
    return m.repeat_interleave(bm, dim=0)[:n]


def captured_fraction(weight, inds, counts, passed=None):
    """Per group: weight captured by the listed columns / weight captured by the exact top-|S| (1 when nothing can be captured).
    ``passed``: the number of columns the method's threshold admits, where the listed count is that number rounded up to a multiple with
    columns that did NOT pass: the comparison is then between the ``passed`` heaviest listed columns and the exact top-``passed``, so
    that the padding neither counts as shortfall nor hides one."""
    out = []
    for g in range(weight.shape[0]):
        c = int(counts[g])
        listed = weight[g, inds[g, :c].long().unique()]
        if passed is not None:
            c = min(passed, c)
            listed = listed.sort(descending=True).values[:c]
        got = listed.sum()
        best = weight[g].sort(descending=True).values[:c].sum()
        out.append(float(got / best) if float(best) > 0 else 1.0)
    return out


class MlpMethodModel:
    """fp64 sparse-delta MLP.  ``weights[layer] = (W1, b1, W2, b2)`` (any float dtype; for the fp8 route W1 is the module's quantised
    weight times its reciprocal scale and the `x` handed to `step` is the module's quantised input times its reciprocal scale:
    quantisation error is not counted).  Schedule: full steps every ``full_step_every``; from step 10 on a sparse step whose number is
    no multiple of ``block_mask_cache`` keeps the previous selection and leaves the block means alone."""

    def __init__(self, weights, full_step_every, block_mask_cache, bm=128, defect=None):
        assert defect is None or defect in MLP_DEFECTS, defect
        self.w = [tuple(t.double() for t in w) for w in weights]
        self.full_every, self.mask_cache, self.bm, self.defect = full_step_every, block_mask_cache, bm, defect
        self.state = {}

    def is_full(self, step):
        return step % self.full_every == 0

    def reuses_selection(self, step, key):
        return step % self.mask_cache != 0 and step >= 10 and "sel" in self.state.get(key, {})

    def _act_key(self, layer, inv):
        return (layer, 0) if self.defect == "other_invocation_activations" else (layer, inv)

    def step(self, step, inv, layer, x, sel=None):
        """x [n, k]; sel = (inds [g, f], counts [g]) the module stored for this step (ignored on a full step; on a step that keeps its
        selection the stored one is what the module has, pass it all the same).  Returns a dict: ``o`` [n, c] the output, ``a`` [n, f] the
        activations the cache must hold, ``fresh`` [n, f], ``refreshed`` [n, f] bool, ``weight`` [g, f] |Bm_new - Bm_cache| BEFORE the update
        (None on full and kept-selection steps), ``nsparse`` sparse steps since the last full one."""
        w1, b1, w2, b2 = (t.to(x.device) for t in self.w[layer])
        key, akey = (layer, inv), self._act_key(layer, inv)
        st = self.state.setdefault(key, {})
        ast = self.state.setdefault(akey, {})
        h = x.double() @ w1.T + b1
        fresh = gelu_tanh(h)
        n, f = fresh.shape
        if self.is_full(step):
            st.update(o=fresh @ w2.T + b2, bm=block_mean64(h, self.bm), nsparse=0)
            ast["a"] = fresh
            ast["a_full"] = fresh
            return dict(o=st["o"], a=fresh, fresh=fresh, refreshed=torch.ones_like(fresh, dtype=torch.bool), weight=None, nsparse=0)
        reused = self.reuses_selection(step, key)
        weight = None
        if not reused:
            bm_new = block_mean64(h, self.bm)
            weight = (bm_new - st["bm"]).abs()
            st["sel"] = sel
            gm = selection_mask(sel[0], sel[1], sel[0].shape[0], f, 1)
            if self.defect != "block_means_not_copied":
                st["bm"] = torch.where(gm, bm_new, st["bm"])
        elif self.defect == "other_layer_indices_on_cached_mask":
            other = self.state.get((layer + 1, inv), self.state.get((layer - 1, inv)))
            st["sel"] = other["sel"]
        inds, counts = st["sel"]
        m = selection_mask(inds, counts, n, f, self.bm)
        st["nsparse"] += 1
        if self.defect is None:
            a = torch.where(m, fresh, ast["a"])
            o = a @ w2.T + b2                       # == o_prev + (a - a_prev) W2^T exactly: the method's delta form
        else:
            base = ast["a_full"] if self.defect == "stale_full_activations" else ast["a"]
            delta = torch.where(m, fresh - base, torch.zeros_like(fresh))
            o = st["o"] + (2.0 if self.defect == "delta_twice" else 1.0) * (delta @ w2.T)
            if self.defect == "bias_again":
                o = o + b2
            a = base + delta
            if self.defect == "last_group_cache_stale":
                last = (n - 1) // self.bm * self.bm
                a = torch.cat([a[:last], base[last:]])
        st["o"] = o
        ast["a"] = a
        return dict(o=o, a=a, fresh=fresh, refreshed=m, weight=weight, nsparse=st["nsparse"])


def read_mlp_selection(storage):
    """(inds [g, f] int32, counts [g]) of the current model invocation, from the public getters (B == 1)."""
    return storage.get_indices()[0], storage.get_counts()[0]


# ------------------------------------------------------------------------------------------------------------------ attention
def kept_from_mask(mask, multiple_of):
    """bool mask [1, h, g, n] -> (inds [1, h, g, n] int32, counts [1, h, g]): the True columns ascending; the method rounds a count up to a
    multiple of ``multiple_of`` with the first False columns (what both the reference's and this build's mask-to-indices do)."""
    _, hh, gg, n = mask.shape
    inds = torch.zeros(1, hh, gg, n, dtype=torch.int32, device=mask.device)
    counts = torch.zeros(1, hh, gg, dtype=torch.int32, device=mask.device)
    cols = torch.arange(n, device=mask.device, dtype=torch.int32)
    for h in range(hh):
        for g in range(gg):
            row = mask[0, h, g]
            on, off = cols[row], cols[~row]
            pad = min((-on.numel()) % multiple_of, off.numel())
            lst = torch.cat([on, off[:pad]])
            inds[0, h, g, : lst.numel()] = lst
            counts[0, h, g] = lst.numel()
    return inds, counts


def read_attn_selection_compressed(module, inv, n, multiple_of):
    """Compressed route: the stored bit-packed mask of invocation `inv` -> (mask [1, h, g, n] bool, inds, counts)."""
    from chipmunk_amd import ops
    mask = ops.bitunpack(module.storage.get_indices(), module.mask_shape[inv])[..., :n]
    return (mask,) + kept_from_mask(mask, multiple_of)


def read_attn_selection_flux(module):
    """FLUX route: stored (indices, counts)."""
    return module.storage.get_indices(), module.storage.get_counts()


class AttnMethodModel:
    """fp64 sparse-delta attention.  The caller names what the method does at this (step, layer) through `kind` (see `kind_of`)."""

    def __init__(self, first_n_dense_layers, full_steps, recompute_mask, defect=None):
        assert defect is None or defect in ATTN_DEFECTS, defect
        self.first_dense, self.full_steps, self.recompute, self.defect = first_n_dense_layers, set(full_steps), recompute_mask, defect
        self.state = {}

    def kind_of(self, step, layer):
        if layer < self.first_dense:
            return "dense"
        if step not in self.full_steps:
            return "sparse"
        if step == 0:
            return "first"
        return "mask" if (step == 1 or self.recompute) else "full"

    def _sparse(self, q, k, v, sel):
        inds, counts = sel
        if self.defect == "kept_list_cut_to_128":
            counts = counts.clone()
            counts[0, 0, 0] = (int(counts[0, 0, 0]) - 1) // 128 * 128
        return helpers.attn_exact(q, k, v, inds, counts, with_top=True)

    def column_sums(self, q, k, p):
        """cs [1, h, g, n] fp64: sum over the 192 rows of a group of exp(s_ij) p_i (p from the previous full step)."""
        s = q.double() @ k.double().transpose(-1, -2) / q.shape[-1] ** 0.5
        w = torch.exp(s) * p[..., None]
        n = w.shape[-2]
        pad = (-n) % helpers.GROUP_ROWS
        w = torch.nn.functional.pad(w, (0, 0, 0, pad))
        return w.view(*w.shape[:2], -1, helpers.GROUP_ROWS, w.shape[-1]).sum(dim=-2)

    def step(self, step, inv, layer, q, k, v, sel=None, n_video=None):
        """Returns a dict: ``o`` the output; ``allow`` [1, h, n] the derived part of the row allowance that is NOT the flat bound (see
        `allowance`); ``cache`` after a step that stores one; ``cs`` the column sums on a mask step; ``kind``."""
        kind = self.kind_of(step, layer)
        st = self.state.setdefault((layer, inv), {})
        if kind in ("dense", "first", "mask", "full"):
            dense, dtop = helpers.attn_exact(q, k, v, with_top=True)
        res = dict(kind=kind)
        if kind == "dense":
            return dict(res, o=dense, evals=[(dense, dtop)], sums=[])
        if kind == "first":
            s = q.double() @ k.double().transpose(-1, -2) / q.shape[-1] ** 0.5
            st["p"] = 1.0 / torch.exp(s).sum(-1)
            return dict(res, o=dense, evals=[(dense, dtop)], sums=[])
        if kind in ("mask", "full"):
            if kind == "mask":
                res["cs"] = self.column_sums(q, k, st["p"])
                s = q.double() @ k.double().transpose(-1, -2) / q.shape[-1] ** 0.5
                st["p"] = 1.0 / torch.exp(s).sum(-1)
                if not (self.defect == "stale_mask_after_recompute" and "sel" in st):
                    st["sel"] = sel
            sp, stop = self._sparse(q, k, v, st["sel"])
            cache = dense - sp
            if self.defect == "cache_wrong_sign":
                cache = sp - dense
            if self.defect == "cache_before_subtraction":
                cache = dense
            st.update(cache=cache, cache_evals=[(dense, dtop), (sp, stop)], k=k, v=v)
            return dict(res, o=dense, cache=cache, cache_evals=st["cache_evals"], evals=[(dense, dtop)], sums=[])
        # sparse step
        src = st
        if self.defect == "other_invocation":
            src = self.state.get((layer, 1 - inv), st)
        if self.defect == "pipeline_slot_layer":
            src = self.state.get((layer + PIPELINE_DEPTH, inv), self.state.get((layer - PIPELINE_DEPTH, inv), st))
        ks, vs = (st["k"], st["v"]) if self.defect == "stale_kv" else (k, v)
        sp, stop = self._sparse(q, ks, vs, src["sel"])
        if self.defect == "ragged_and_text_rows_no_delta":
            n = q.shape[2]
            first = min((n - 1) // helpers.GROUP_ROWS * helpers.GROUP_ROWS, n if n_video is None else n_video)
            sp = sp.clone()
            sp[:, :, first:] = 0
        o = src["cache"] + sp
        if self.defect == "delta_persists":
            st["cache"] = o
        st["k"], st["v"] = k, v
        return dict(res, o=o, cache=st["cache"], evals=st["cache_evals"] + [(sp, stop)], sums=[st["cache"], o])


def allowance(res, flat=helpers.ROW_ERR_BOUND, per_sparse_eval=0.0):
    """Row-relative allowance [1, h, n] for an attention output, derived from what the model has: every attention evaluation that entered
    the value may be off by ``flat`` + its `top_key_term` relative to ITS OWN norm, and every stored bf16 sum by 2^-8 of its norm; the
    total is taken relative to the norm of the exact output.  ``per_sparse_eval``: added to `flat` for the gathered evaluations when the
    shipped dispatch may fold the scale into Q (docs/TEST_SENSITIVITY.md records that fold's cost)."""
    o = res["o"]
    den = o.norm(dim=-1)
    tot = torch.zeros_like(den)
    for i, (e, top) in enumerate(res["evals"]):
        f = flat + (per_sparse_eval if i > 0 else 0.0)
        tot = tot + (f + helpers.top_key_term(e, top)) * e.norm(dim=-1)
    for s in res["sums"]:
        tot = tot + helpers.BF16_EPS * s.norm(dim=-1)
    return torch.where(den > 0, tot / den, torch.zeros_like(den))


# ------------------------------------------------------------------------------------------------------------------ driver
def drive(modules, n_inv, steps, inputs, after):
    """The integration protocol of INTEGRATION.md / tools/wan_workload.py over ``steps`` inference steps: per step every model invocation,
    per invocation every layer: ``load_async_wait()`` of the layer (not before the very first call), ``load_async()`` of the layer that
    follows, the call, ``after(step, inv, layer, module, args, out)`` (assertions; the layer's state is still that of this invocation),
    then ``storage.complete_cur_layer()``.  ``inputs(step, inv, layer)`` gives the call's arguments."""
    first = True
    with torch.no_grad():
        for step in range(steps):
            for inv in range(n_inv):
                for li, mod in enumerate(modules):
                    if not first:
                        mod.storage.load_async_wait()
                    first = False
                    modules[(li + 1) % len(modules)].storage.load_async()
                    args = inputs(step, inv, li)
                    out = mod(*args)
                    after(step, inv, li, mod, args, out)
                    mod.storage.complete_cur_layer()


def reload_current(storage, unsuppress=None, read=None):
    """Bring the layer's stored state of the CURRENT invocation back into its device slots with the protocol's own ``load_async`` /
    ``load_async_wait``, so that the public getters show what was just stored (a host-resident field's getter shows the slot as last
    loaded, not what `set_*` sent to the host since).  Holder state is left as the module set it.  The one exception is the read of a
    mask whose load the module has suppressed (it kept the index rows the mask unpacks to): ``unsuppress`` names that holder, the flag
    is cleared for this one load and for ``read()`` (whose result is returned) and SET AGAIN before returning, so that every later
    protocol ``load_async`` and every module call see the flag as shipped."""
    was = unsuppress is not None and unsuppress.is_suppressed()
    if was:
        unsuppress.suppress_current(False)
    try:
        storage.load_async()
        storage.load_async_wait()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return read() if read is not None else None
    finally:
        if was:
            unsuppress.suppress_current(True)


# ------------------------------------------------------------------------------------------------------------------ MLP: schedules, checker
MARGIN = helpers.ROW_ERR_MARGIN
MLP_K, MLP_F, MLP_DENSE_LAYERS, MLP_LAYERS = 256, 1024, 1, 3
# route -> (model invocations, steps, full_step_every, block_mask_cache).  flux: step 11 keeps its selection (cached-mask branch) and up
# to three sparse steps run in a row; wan: two invocations with different inputs
MLP_ROUTES = {"flux": (1, 13, 4, 2), "wan": (2, 7, 4, 2)}
MLP_TOP_KEYS = 0.3                                              # as shipped
# columns that pass the method's threshold (the value at rank int(F x sparsity) of the ascending row, ties aside): 308 of 1024; the
# stored count is that rounded up to counts_multiple_of = 256 with columns that did not pass
MLP_PASSED = MLP_F - int(MLP_F * (1 - MLP_TOP_KEYS))
MLP_ROUTES_GPU = dict(MLP_ROUTES, wan_fp8=(2, 7, 4, 2))       # the fp8 GEMM1 of the shipped Wan file: GPU only (torch._scaled_mm)


def configure_mlp(cfg, route):
    n_inv, steps, every, cache = MLP_ROUTES_GPU[route]
    cfg["num_model_invocations_per_inference_step"] = n_inv
    cfg["steps"] = 50
    cfg["mlp"].update(dict(top_keys=MLP_TOP_KEYS, random_keys=0.0, full_step_every=every, block_mask_cache=cache,
                           first_n_dense_layers=MLP_DENSE_LAYERS, counts_multiple_of=256))
    return n_inv, steps, every, cache


def record(table, key, value):
    table[key] = max(table.get(key, 0.0), float(value))


def rel_rows(got, exact, mask=None):
    """worst row-relative error, optionally over the masked elements of every row only (rows without any are skipped)"""
    got, exact = got.double(), exact.double()
    if mask is not None:
        got, exact = got * mask, exact * mask
        rows = mask.any(dim=-1)
        got, exact = got[rows], exact[rows]
    if exact.numel() == 0:
        return 0.0
    return float(helpers.row_rel_err(got, exact).max())


class MlpChecker:
    """The assertions of the GPU test after every SparseDiffMlp call, against `model`; tests/test_method_model_cpu.py runs the same object
    over the CPU oracle (to pin the floors) and over the mutants (to prove they are rejected).  ``floors[name][nsparse]``; with
    ``floors=None`` nothing is asserted and `worst` collects the figures.  ``operand(module, x) -> x for the model``."""

    def __init__(self, model, weights, n, floors=None, eps=None, operand=None, what=""):
        self.model, self.weights, self.n, self.floors, self.eps, self.operand, self.what = model, weights, n, floors, eps, operand, what
        self.worst, self.shortfall, self.pre = {}, 0.0, None

    def before(self, module, step, layer):
        """snapshot of the activation cache as a sparse step is about to see it"""
        self.pre = None
        if layer >= MLP_DENSE_LAYERS and not self.model.is_full(step):
            self.pre = module.storage.get_sparse_act_T().clone()

    def _check(self, name, nsparse, err, where):
        record(self.worst, (name, nsparse), err)
        if self.floors is not None:
            bound = MARGIN * self.floors[name][min(nsparse, max(self.floors[name]))]
            helpers._record_row_err(f"{self.what} {name} {where}", err, bound)
            assert err <= bound, f"{self.what} {where}: {name} error {err:.4g} > {bound:.4g} ({nsparse} sparse steps since the full step)"

    def check_values(self, res, out, act, out_cache, w2, b2, where):
        """out [n, c], act [n, f] (the cache, token-major view), out_cache [n, c] against the model's `res`"""
        ns = res["nsparse"]
        self._check("output", ns, rel_rows(out, res["o"]), where)
        self._check("invariant", ns, rel_rows(out_cache, act.double() @ w2.double().T + b2.double()), where)
        self._check("cache", ns, rel_rows(act, res["a"]), where)
        if ns > 0:
            self._check("refreshed", ns, rel_rows(act, res["fresh"], res["refreshed"]), where)

    def after(self, step, inv, layer, module, args, out):
        where = f"step {step} invocation {inv} layer {layer}"
        x = args[0]
        w1, b1, w2, b2 = (t.to(x.device) for t in self.weights[layer])
        xm = (self.operand(module, x) if self.operand else x)[0]
        if layer < MLP_DENSE_LAYERS:
            exact = gelu_tanh(xm.double() @ w1.double().T + b1.double()) @ w2.double().T + b2.double()
            self._check("output", 0, rel_rows(out[0], exact), where)
            return
        st = module.storage
        out = out.clone()       # (the module hands back the output cache's slot itself)
        reload_current(st)
        full = self.model.is_full(step)
        res = self.model.step(step, inv, layer, xm, None if full else read_mlp_selection(st))
        stored = st.get_sparse_act_T()
        assert stored.shape[-1] == (self.n + 7) // 8 * 8 and (stored[..., self.n:] == 0).all(), f"{where}: padding columns of the cache"
        act_t = stored[0][:, : self.n]
        self.check_values(res, out[0], act_t.T, st.get_out_cache()[0], w2, b2, where)
        if not full:
            # every element outside the refreshed (rows, columns) keeps the bits it had when the call began
            same = (act_t.view(torch.int16) == self.pre[0][:, : self.n].view(torch.int16)) | res["refreshed"].T
            assert same.all(), f"{where}: {int((~same).sum())} cache elements outside the selection changed"
        if res["weight"] is not None:
            inds, counts = read_mlp_selection(st)
            frac = min(captured_fraction(res["weight"], inds, counts, MLP_PASSED))
            self.shortfall = max(self.shortfall, 1.0 - frac)
            if self.eps is not None:
                assert 1.0 - frac <= self.eps, f"{where}: the selection captures {frac:.4f} of what the exact top-|S| captures"


def build_mlps(route, device, linear, gelu, fp8=False):
    """(modules, weights per layer as the model takes them, counter) for the route's schedule; call `configure_mlp` first."""
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    counter = LayerCounter(MLP_LAYERS, 1)
    mods, weights = [], []
    for li in range(MLP_LAYERS):
        w1, b1, w2, b2 = mlp_weights(li, MLP_K, MLP_F)
        fc1, fc2 = linear(MLP_K, MLP_F), linear(MLP_F, MLP_K)
        with torch.no_grad():
            for prm, val in ((fc1.weight, w1), (fc1.bias, b1), (fc2.weight, w2), (fc2.bias, b2)):
                prm.copy_(val)
        fc1, fc2 = fc1.to(device).bfloat16(), fc2.to(device).bfloat16()
        if fp8 and li >= MLP_DENSE_LAYERS:
            from chipmunk_amd.modules.mlp_fp8 import F8Linear
            fc1 = F8Linear.from_linear(fc1, input_float8_dtype=torch.float8_e4m3fn)
            w1m = fc1.weight.data.double() * fc1.scale_reciprocal.double()
        else:
            w1m = fc1.weight.data.double()
        mods.append(SparseDiffMlp(li, counter, fc1, gelu, fc2, 6))
        weights.append((w1m, fc1.bias.data.double(), fc2.weight.data.double(), fc2.bias.data.double()))
    return mods, weights


def fp8_operand(module, x):
    """the module's own quantised input times its reciprocal scale (bf16 x when the layer's fc1 is not fp8)"""
    fc1 = module.fc1[0]
    if fc1.weight.dtype != torch.float8_e4m3fn:
        return x
    xq = (x * fc1.input_scale).clamp(-fc1.input_max_value, fc1.input_max_value).to(torch.float8_e4m3fn)
    return xq.double() * fc1.input_scale_reciprocal.double()


def run_mlp_route(route, n, device, linear, gelu, model_defect=None, floors=None, eps=None, fp8=False, what="", trace=None,
                  offloading=None, amd_keys=True):
    """Drive the route's modules by the integration protocol with the checker's assertions after every call.  Returns the checker."""
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    n_inv, steps, every, cache = configure_mlp(GLOBAL_CONFIG, route)
    GLOBAL_CONFIG["offloading"].update(offloading or {})
    if not amd_keys:
        for key in AMD_MLP_KEYS:
            GLOBAL_CONFIG["mlp"][key] = False
    mods, weights = build_mlps(route, device, linear, gelu, fp8)
    model = MlpMethodModel(weights, every, cache, GLOBAL_CONFIG["mlp"]["bm"], defect=model_defect)
    chk = MlpChecker(model, weights, n, floors, eps, fp8_operand if fp8 else None, what or route)

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (mlp_input(step, inv, li, n, MLP_K).to(device),)

    def after(step, inv, li, mod, args, out):
        if trace is not None and li >= MLP_DENSE_LAYERS:
            reload_current(mod.storage)
            full = model.is_full(step)
            trace.append(dict(step=step, inv=inv, layer=li, x=args[0],
                              sel=None if full else tuple(t.clone() for t in read_mlp_selection(mod.storage))))
        chk.after(step, inv, li, mod, args, out)

    drive(mods, n_inv, steps, inputs, after)
    chk.modules = mods
    return chk


# ------------------------------------------------------------------------------------------------------------------ attention: schedules, checker
ATTN_H, ATTN_VID, ATTN_TXT = 2, (4, 12, 16), 64
ATTN_N = ATTN_VID[0] * ATTN_VID[1] * ATTN_VID[2] + ATTN_TXT          # 832: five 192-row groups, the last of 64 rows, text rows present
ATTN_SPARSE_LAYERS = 3
# route -> (shipped file, steps, full steps, overrides of the attn section)
ATTN_ROUTES = {
    "hunyuan": ("hunyuan_c3.yml", 7, {0, 1, 4}, dict(full_step_schedule={0, 1, 4}, top_keys=0.15, random_keys=0.0)),
    "flux": ("flux_c2.yml", 6, {0, 1, 4}, dict(full_step_every=4, full_step_schedule=None)),
    "wan": ("wan_c5.yml", 6, {0, 1, 4}, dict(full_step_every=4, full_step_schedule=None, top_keys=0.15, random_keys=0.0, local_voxels=1)),
}
AMD_ATTN_KEYS = ("fused_packed_mask_to_indices", "sorted_indices", "fused_residual", "fused_topk_mask", "fused_colsum_topk",
                 "keep_unpacked_indices", "keep_unpacked_indices_offloaded", "ragged_mask_to_indices")
AMD_MLP_KEYS = ("fused_topk_delta", "fused_block_mean", "fused_fp8_quantize", "fused_scatter")


def configure_attn(cfg, route, root, amd_keys=True, token_major=False):
    """The shipped file of the route, its schedule shortened; returns (invocations, steps, full steps, dense layers)."""
    import os
    from chipmunk_amd.util import config as config_mod
    shipped, steps, full, over = ATTN_ROUTES[route]
    config_mod.load_from_file(os.path.join(root, "configs", shipped))
    cfg["steps"] = 50
    cfg["attn"].update(over)
    cfg["attn"]["token_major_output"] = token_major
    if not amd_keys:
        for key in AMD_ATTN_KEYS:
            cfg["attn"][key] = False
    return cfg["num_model_invocations_per_inference_step"], steps, full, cfg["attn"]["first_n_dense_layers"]


class AttnChecker:
    """The assertions of the GPU test after every SparseDiffAttn call (see MlpChecker).  The output and the stored cache are held to the
    derived per-row `allowance`: the asserted figure is the worst ``row error / allowance`` (<= 1).  ``per_sparse_eval``: see `allowance`."""

    def __init__(self, model, n_video, multiple_of, compressed, eps=None, assert_on=True, per_sparse_eval=0.0, what="", static=None):
        self.model, self.n_video, self.multiple_of, self.compressed = model, n_video, multiple_of, compressed
        self.eps, self.assert_on, self.extra, self.what, self.static = eps, assert_on, per_sparse_eval, what, static
        self.worst, self.shortfall, self.pre, self.suppressed_sparse_steps, self.sparse_calls = {}, 0.0, None, 0, 0

    def before(self, module, step, layer):
        self.pre = None
        if self.model.kind_of(step, layer) == "sparse":
            self.pre = module.storage.get_out_cache().clone()

    def ratio(self, got, res):
        allow = allowance(res, per_sparse_eval=self.extra)
        err = helpers.row_rel_err(got, res["o"])
        return float(torch.where(err == 0, torch.zeros_like(err), err / allow).max())

    def _check(self, name, kind, ratio, where):
        record(self.worst, (name, kind), ratio)
        helpers._record_row_err(f"{self.what} {name} {where} (error / allowance)", ratio, 1.0)
        if self.assert_on:
            assert ratio <= 1.0, f"{self.what} {where}: {name} row error is {ratio:.3f} x its derived allowance ({kind} step)"

    def check_values(self, res, out, cache, where):
        self._check("output", res["kind"], self.ratio(out, res), where)
        if cache is not None and res["kind"] in ("mask", "full"):
            self._check("cache", res["kind"], self.ratio(cache, dict(o=res["cache"], evals=res["cache_evals"], sums=[res["cache"]])), where)

    def after(self, step, inv, layer, module, args, out):
        where = f"step {step} invocation {inv} layer {layer}"
        q, k, v = args
        out = out.clone()       # a sparse step may hand back the pipeline slot itself: the reload below would refill it
        kind = self.model.kind_of(step, layer)
        st = module.storage
        sel = mask = None
        self.sparse_calls += kind == "sparse"
        if kind == "sparse" and self.compressed and st.indices.is_suppressed():
            self.suppressed_sparse_steps += 1       # the module ran this step from its kept index rows, the mask's load suppressed
        if kind == "mask" and self.compressed:
            # (only the read of the mask a mask step just stored may need its suppressed load; the flag is set again inside)
            mask, inds, counts = reload_current(st, st.indices, lambda: read_attn_selection_compressed(module, inv, q.shape[2], self.multiple_of))
            sel = (inds, counts)
        elif kind in ("mask", "full", "sparse"):
            reload_current(st)
            if kind == "mask":
                sel = read_attn_selection_flux(module)
        res = self.model.step(step, inv, layer, q, k, v, sel, self.n_video)
        self.check_values(res, out, st.get_out_cache() if kind in ("mask", "full") else None, where)
        if kind == "sparse":
            now = st.get_out_cache()
            assert now.shape == self.pre.shape and torch.equal(now.view(torch.int16), self.pre.view(torch.int16)), \
                f"{where}: a sparse step changed the stored cache"
        if kind == "mask":
            self.check_selection(res["cs"], sel, mask, where)

    def check_selection(self, cs, sel, mask, where):
        inds, counts = sel
        _, hh, gg, n = cs.shape
        for h in range(hh):
            groups = list(range(gg))
            if mask is not None and self.static is not None:
                static, sparse_groups = self.static
                srow = static[0, min(h, static.shape[1] - 1), :, :n].to(mask.device)
                assert (mask[0, h] | ~srow).all(), f"{where} head {h}: the selection does not contain the static mask"
                flags = sparse_groups[0, min(h, sparse_groups.shape[1] - 1), :, 0].to(mask.device)
                for g in range(gg):
                    if not bool(flags[g]):
                        assert torch.equal(mask[0, h, g], srow[g]), f"{where} head {h} group {g}: a group flagged non-sparse keeps its static mask, nothing else"
                groups = [g for g in groups if bool(flags[g])]
            if groups:
                gi = torch.tensor(groups, device=cs.device)
                frac = min(captured_fraction(cs[0, h, gi], inds[0, h, gi], counts[0, h, gi]))
                self.shortfall = max(self.shortfall, 1.0 - frac)
                if self.eps is not None:
                    assert 1.0 - frac <= self.eps, f"{where} head {h}: the selection captures {frac:.4f} of what the exact top-|S| captures"


def run_attn_route(route, device, root, amd_keys=True, token_major=False, model_defect=None, eps=None, assert_on=True,
                   per_sparse_eval=0.0, what="", trace=None, offloading=None):
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.modules import attn as attn_mod
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    from chipmunk_amd.util.layer_counter import LayerCounter
    n_inv, steps, full, dense_layers = configure_attn(GLOBAL_CONFIG, route, root, amd_keys, token_major)
    GLOBAL_CONFIG["offloading"].update(offloading or {})
    cfg = GLOBAL_CONFIG["attn"]
    layers = dense_layers + ATTN_SPARSE_LAYERS
    counter = LayerCounter(layers, 1)
    mods = [SparseDiffAttn(i, counter) for i in range(layers)]
    compressed = bool(cfg["should_compress_indices"])
    static = None
    if compressed:
        torch.manual_seed(5)
        mods[0].initialize_static_mask(ATTN_VID, ATTN_TXT, ATTN_H, device)
        static = (attn_mod.singleton_static_mask, attn_mod.singleton_video_query_groups)
    multiple_of = 128 if cfg["pad_qkv_before_kernel"] else cfg["counts_multiple_of"]
    tk = int(multiple_of * round(cfg["top_keys"] * ATTN_N / multiple_of))
    assert tk > 0, "the schedule would exercise only the static mask"
    model = AttnMethodModel(dense_layers, full, bool(cfg["recompute_mask"]), defect=model_defect)
    chk = AttnChecker(model, ATTN_N - ATTN_TXT, multiple_of, compressed, eps, assert_on, per_sparse_eval, what or route, static)

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return tuple(t.to(device) for t in attn_input(step, inv, li, ATTN_H, ATTN_N))

    def after(step, inv, li, mod, args, out):
        torch.manual_seed(1000 * step + 10 * li + inv)
        chk.after(step, inv, li, mod, args, out)
        if trace is not None:
            st = model.state.get((li, inv), {})
            trace.append(dict(step=step, inv=inv, layer=li, sel=st.get("sel") if model.kind_of(step, li) == "mask" else None))

    drive(mods, n_inv, steps, inputs, after)
    chk.modules = mods
    return chk


# ------------------------------------------------------------------------------------------------------------------ pinned floors
# The CPU oracle (the reference's roundings) against the models over the schedules above, worst row, rounded up to two digits;
# tests/test_method_model_cpu.py pins them and shows them tight.  MLP: [quantity][sparse steps since the last full step].
MLP_FLOORS = {
    "output": {0: 0.0041, 1: 0.0040, 2: 0.0046, 3: 0.0052},         # module output against the model's O
    "invariant": {0: 0.0020, 1: 0.0034, 2: 0.0043, 3: 0.0052},      # out_cache against act_cache^T W2^T + b2 of the module's own cache
    "cache": {0: 0.0033, 1: 0.0029, 2: 0.0027, 3: 0.0027},          # activation cache against the model's A, whole rows
    "refreshed": {1: 0.0026, 2: 0.0024, 3: 0.0025},                 # ... on the refreshed columns alone, against the fresh activation
}
# 1 - (|Bm_new - Bm_cache| captured by the MLP_PASSED heaviest columns of the stored selection) / (captured by the exact top-MLP_PASSED):
# what the bf16 rounding of the block means moves across the threshold.  (Against the exact top-|S| of all 512 listed columns the mirror
# "falls short" by 0.13, all of it the 204 columns that pad 308 to 512: that comparison cannot tell a stale selection from padding.)
MLP_SELECTION_SHORTFALL = 0.00009
# the fp8 route has no CPU mirror (torch._scaled_mm); its block means are quantised on their own, apart from x: measured on an MI355X over
# N = 1024, 1003 and both switch settings, worst 0.005379, rounded up
MLP_SELECTION_SHORTFALL_FP8 = 0.0054
# attention: worst (row error / derived allowance) of the oracle per (quantity, kind of step); the allowance already holds the margin
ATTN_RATIO_FLOORS = {("output", "dense"): 0.43, ("output", "first"): 0.39, ("output", "mask"): 0.40, ("output", "full"): 0.40,
                     ("output", "sparse"): 0.20, ("cache", "mask"): 0.26, ("cache", "full"): 0.26}
# 1 - (fp64 column-sum weight captured by the stored selection) / (captured by the exact top-|S|), sparse groups only.  The compressed
# routes add 1 % random keys and round the count up to 128 with keys that were not selected; FLUX stores the plain top-k
ATTN_SELECTION_SHORTFALL = {"hunyuan": 0.13, "flux": 0.000093, "wan": 0.13}
