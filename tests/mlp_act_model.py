"""The ungated sparse MLP with any of the three kernel activations and an optional fc1 bias (``csp_mlp_mm1_act`` /
``csp_mlp_mm1_fp8_act``, ``SparseDiffMlp(..., nn.SiLU() | nn.GELU() | nn.GELU("tanh"))``), for tests/test_mlp_act_host.py,
tests/test_gpu_mlp_act.py and tests/test_gpu_mlp_act_e2e.py.  helpers.py, method_model.py and glu_method_model.py are imported, not
edited.

Operator level: the case list (`act_cases`), a plain-torch mirror of the new epilogue arithmetic (`mm1_act_mirror`: fp32 sums, then the
roundings in the operator's order), the mutants the checker has to reject (`act_mutants`) and the bound the GPU test asserts
(`ACT_SEG_BOUND`, derived by the rule in `act_bound`).

Module level: the fp64 model of the method with an activation by name and an optional bias (`ActMethodModel`), its checker, the route
table, and `ActEmulation`, the module's op sequence in torch (no chipmunk operator; bf16 fc1 only: an fp8 fc1 runs torch._scaled_mm and
calibrates its input scale over its own calls, so a second consumer of the layer would change what the module sees).
"""
import torch

import glu_method_model as gm
import method_model as mm
from helpers import (BF16_EPS, F8, MLP_ACTS, MLP_BM, MLP_SEG_BOUND, MLP_SEG_MARGIN, MLP_SEG_W1, ORACLE_MLP_SEG_ERR, assert_segs_close,
                     gathered_cache, mlp_exact_args, mlp_group_cols, mlp_problem, mm1_exact, refreshed_cache_term, seg_rel_err, seg_term)

SENT = 7.0


def bf(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ operator: cases
def act_cases():
    """name -> `helpers.mlp_problem` arguments (gated=False): M = 333 (three groups, the last of 77 rows, cache pitch 336) and 1000 (eight
    groups, one empty), F = 512, K = 320 / 256 bf16 and 384 e4m3, the counts of helpers.MLP_COUNTS; every activation, with and without a
    bias, both cache regimes."""
    out = {}
    for M in (333, 1000):
        for regime in ("random", "previous step"):
            for fp8 in (False, True):
                K = 384 if fp8 else 320 if M == 333 else 256
                for act in MLP_ACTS:
                    for biases in (True, False):
                        name = f"{'fp8' if fp8 else 'bf16'} {act}{'' if biases else ' no bias'} M{M} K{K}, {regime} cache"
                        out[name] = dict(M=M, K=K, F=512, seed=500 + len(out), regime=regime, act=act, fp8=fp8, gated=False, biases=biases)
    return out


def exact(p, **over):
    """(delta, fresh) of problem p in fp64 by the operator's definition (helpers.mm1_exact), with operands overridden"""
    q = dict(p, **over)
    return mm1_exact(q["a"], q["w"], q["bias"], q["cache0"], q["inds"], q["cnt"], **mlp_exact_args(q))


def small_step_problem(args, step):
    """The previous-step regime of `helpers.mlp_problem` with a step size of choice (mlp_problem's own is 0.05): the cache holds bf16 of
    the activations of x0, the operator sees x0 + step * randn.  Built from the random-regime problem of the same arguments, whose `a`
    is x0 as the operator reads it."""
    p = mlp_problem(**dict(args, regime="random"))
    every = torch.arange(p["F"], dtype=torch.int32).expand(p["G"], p["F"])
    fresh0 = mm1_exact(p["a"], p["w"], p["bias"], torch.zeros(p["F"], p["M"]), every, [p["F"]] * p["G"], **mlp_exact_args(p))[1]
    p["cache0"] = bf(fresh0.T).contiguous()
    noise = torch.randn(p["M"], p["K"], generator=torch.Generator().manual_seed(args["seed"] + 77)) * step
    if p["fp8"]:
        p["a"] = ((p["a"].float() * p["ra"] + noise) / p["ra"]).clamp(-448.0, 448.0).to(F8)
    else:
        p["a"] = bf(p["a"].float() + noise)
    p["regime"] = f"previous step, step {step}"
    return p


# ------------------------------------------------------------------------------------------------------------------ operator: mirror
def act32(act, x):
    """the activation in fp32 torch"""
    fn = torch.nn.functional
    return fn.silu(x) if act == "silu" else fn.gelu(x, approximate="tanh" if act == "gelu_tanh" else "none")


def mm1_act_mirror(p, update="none"):
    """The new GEMM1 forms in plain torch, fp32 sums and then the roundings in the operator's order (include/chipmunk_hip.h, "Ungated
    activations"):  bf16  c = bf16(act(sum + bias) - cache);  fp8  t = bf16(act((sum * scale_a) * scale_b + bias)), c = bf16(t - cache).
    A null bias is zero.  update: "none", "scatter" (cache = bf16(cache + c), what csp_scatter_add does) or, fp8 only, "store"
    (cache = t).  Returns (c [M, F] bf16 with `SENT` at and past the counts, cache [F, M] bf16)."""
    assert update in ("none", "scatter") or (update == "store" and p["fp8"])
    M, f = p["M"], p["F"]
    c = torch.full((M, f), SENT, dtype=torch.bfloat16)
    cache = p["cache0"].clone()
    a, w = p["a"].float(), p["w"].float()
    for g in range(p["G"]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(p["cnt"][g])
        if n == 0:
            continue
        col = p["inds"][g, :n].long()
        acc = a[rows] @ w[col].T
        b = 0.0 if p["bias"] is None else p["bias"][col].float()
        old = cache[col][:, rows].float().T
        if p["fp8"]:
            t = bf(act32(p["act"], (acc * p["ra"]) * p["rb"] + b))
            d = bf(t.float() - old)
        else:
            t = None
            d = bf(act32(p["act"], acc + b) - old)
        c[rows, :n] = d
        if update != "none":
            cache[col, rows] = (t if update == "store" else bf(old + d.float())).T
    return c, cache


# ------------------------------------------------------------------------------------------------------------------ operator: mutants
TANH_FOR_SILU, TANH_FOR_ERF = "tanh-GELU where SiLU was asked", "tanh-GELU where exact GELU was asked"
BIAS_ADDED, BIAS_DROPPED, BIAS_AFTER = "bias added when it is null", "bias dropped when it is given", "the bias added after the activation"


def other_bias(p):
    """a bias vector of the problems' scale (0.1) for a problem that has none"""
    return bf(torch.randn(p["F"], generator=torch.Generator().manual_seed(4242)) * 0.1)


def packed_bias(p, bias):
    """bias in the packed layout of the deltas: [M, F] fp64 with [m, j] = bias[inds[g, j]], 0 at and past the counts"""
    out = torch.zeros(p["M"], p["F"], dtype=torch.float64)
    for g in range(p["G"]):
        n = int(p["cnt"][g])
        out[g * MLP_BM:(g + 1) * MLP_BM, :n] = bias[p["inds"][g, :n].long()].double()
    return out


def stored(p, res):
    """(delta, fresh) of a mutant -> what the operator would store: one rounding of the delta (bf16), or the bf16 activation minus the
    cache, rounded again (fp8)"""
    d, f = res
    return bf(bf(f).double() - (f - d)) if p["fp8"] else bf(d)


def act_mutants(p):
    """name -> packed deltas (bf16): the exact fp64 result with ONE defect, rounded where the operator rounds"""
    mut = {}
    if p["act"] == "silu":
        mut[TANH_FOR_SILU] = stored(p, exact(p, act="gelu_tanh"))
    if p["act"] == "gelu":
        mut[TANH_FOR_ERF] = stored(p, exact(p, act="gelu_tanh"))
    if p["bias"] is None:
        mut[BIAS_ADDED] = stored(p, exact(p, bias=other_bias(p)))
    else:
        mut[BIAS_DROPPED] = stored(p, exact(p, bias=None))
        d0, f0 = exact(p, bias=None)
        pb = packed_bias(p, p["bias"])
        mut[BIAS_AFTER] = stored(p, (d0 + pb, f0 + pb))
    return mut


def delta_term(p, delta, fresh, cols):
    """the derived term of the packed deltas: none for bf16 (one rounding); the ungated fp8 route rounds the activation to bf16 and
    subtracts in bf16, 2^-8 ||fresh_seg|| / ||delta_seg|| (tests/test_gpu_mlp_accuracy.py, test_ungated_fp8_gemm1)"""
    return seg_term(fresh, delta, MLP_SEG_W1, cols) if p["fp8"] else None


def delta_err(p, got, delta, fresh):
    """worst segment error of packed deltas `got` against the exact ones, the derived term taken off"""
    cols = mlp_group_cols(p["cnt"], p["M"])
    err = seg_rel_err(got, delta, MLP_SEG_W1, cols)
    term = delta_term(p, delta, fresh, cols)
    return float((err if term is None else err - term).max())


# ------------------------------------------------------------------------------------------------------------------ operator: the bound
def act_bound(floor):
    """The rule of the MLP accuracy tests (docs/TEST_SENSITIVITY.md): a mirror floor at or under ORACLE_MLP_SEG_ERR keeps the shipped bound
    MLP_SEG_BOUND; above it the bound is MLP_SEG_MARGIN x the measured floor."""
    return MLP_SEG_BOUND if floor <= ORACLE_MLP_SEG_ERR else MLP_SEG_MARGIN * floor


# Measured by tests/test_mlp_act_host.py over `act_cases` (all 48; update off / scatter / store, derived terms taken off): the mirror's
# worst segment is 0.0034 (fp8, the cache that holds the bf16 activation itself; packed deltas 0.0032), under ORACLE_MLP_SEG_ERR = 0.0035,
# so the GPU bound is the shipped one.  That file asserts this constant against the rule.
ACT_SEG_BOUND = MLP_SEG_BOUND
# The exact-GELU / tanh-GELU mutant is counted on the bf16 route in a previous-step regime with this step: the two functions differ by
# 5e-4 at most, so the deltas have to be small for the difference to show.  Checked on the CPU before it was fixed (weakest case per
# step: 0.05 -> 0.0054, 0.02 -> 0.0128, 0.01 -> 0.0251, 0.005 -> 0.0558 against 2 x bound = 0.014); tests/test_mlp_act_host.py holds it.
# The fp8 route rounds the activation to bf16 before it subtracts (2^-9 |act|, about the two functions' distance): its derived term covers
# the mutant in every regime, so there the two are told apart by projection (tests/test_gpu_mlp_act.py), as for the gated operators.
ERF_MUTANT_STEP = 0.01


def assert_act_deltas(p, got, delta, fresh, what):
    cols = mlp_group_cols(p["cnt"], p["M"])
    return assert_segs_close(got, delta, ACT_SEG_BOUND, f"{what}: packed deltas", extra=delta_term(p, delta, fresh, cols), cols=cols)


def assert_act_cache(p, cache, delta, fresh, what, accumulate=True):
    """the refreshed cache columns against the fresh fp64 activation (tests/test_gpu_mlp_accuracy.py, assert_cache): bf16(cache + delta)
    inherits the delta's error and is rounded once more (helpers.refreshed_cache_term; act_rounded on the fp8 route); not accumulate:
    the cache is the bf16 activation itself"""
    cols = mlp_group_cols(p["cnt"], p["M"])
    got = gathered_cache(cache, p["inds"], p["cnt"])
    term = refreshed_cache_term(got, fresh, delta, ACT_SEG_BOUND, MLP_SEG_W1, cols, p["fp8"]) if accumulate else None
    return assert_segs_close(got, fresh, ACT_SEG_BOUND, f"{what}: refreshed cache columns", extra=term, cols=cols)


def gelu_projection(got, want_tanh, want_erf):
    """sum((got - want_tanh) * d) / sum(d * d), d = want_erf - want_tanh: 0 for a tanh-GELU result, 1 for an exact-GELU one, up to the
    rounding of `got`, which averages out over the elements (tests/test_gpu_mlp_glu.py)"""
    d = (want_erf - want_tanh).double()
    return float(((got.double() - want_tanh.double()) * d).sum() / (d * d).sum())


# ------------------------------------------------------------------------------------------------------------------ module: model
# the layout of the gated module test (tests/test_gpu_mlp_glu_e2e.py): two layers, K = 256, F = 1024, N = 333, 13 steps,
# full_step_every = 10, block_mask_cache = 2, no dense layer in front, top_keys = 0.3
K, F, N, LAYERS, STEPS, SCHEDULE, PASSED = gm.K, gm.F, gm.N, gm.LAYERS, gm.STEPS, gm.SCHEDULE, gm.PASSED
# route -> (activation, fc1 bias, e4m3 fc1, batch size, activation cache offloaded)
ROUTES = {
    "silu_bias": ("silu", True, False, 1, False),
    "gelu_nobias": ("gelu", False, False, 1, False),
    "gelu_tanh_nobias": ("gelu_tanh", False, False, 1, False),
    "silu_fp8": ("silu", True, True, 1, False),
    "silu_bias_b2": ("silu", True, False, 2, False),
    "gelu_nobias_offloaded": ("gelu", False, False, 1, True),
}
OFFLOADED = {"global_disable_offloading": False, "mlp.sparse_act_T": True, "keep_resident_if_fits": False}


def act_weights(layer, bias):
    """(W1 [F, K], b1 [F] | None, W2 [K, F], b2 [K]) rounded to bf16 (as the module holds them), in fp32"""
    w1, b1, w2, b2 = mm.mlp_weights(layer, K, F)
    r = lambda t: t.to(torch.bfloat16).float()      # noqa: E731
    return r(w1), r(b1) if bias else None, r(w2), r(b2)


class ActMethodModel(mm.MlpMethodModel):
    """`MlpMethodModel` (its defect-free step) with ``fresh = act(x W1^T + b1)`` for an activation by name and b1 that may be None"""

    def __init__(self, weights, act, full_step_every, block_mask_cache, bm=128):
        assert act in MLP_ACTS, act
        self.w = [tuple(None if t is None else t.double() for t in w) for w in weights]
        self.act, self.full_every, self.mask_cache, self.bm, self.defect = act, full_step_every, block_mask_cache, bm, None
        self.state = {}

    def step(self, step, inv, layer, x, sel=None):
        w1, b1, w2, b2 = (None if t is None else t.to(x.device) for t in self.w[layer])
        key = (layer, inv)
        st = self.state.setdefault(key, {})
        h = x.double() @ w1.T
        if b1 is not None:
            h = h + b1
        fresh = gm.act64(self.act, h)
        n, f = fresh.shape
        if self.is_full(step):
            st.update(o=fresh @ w2.T + b2, bm=mm.block_mean64(h, self.bm), nsparse=0, a=fresh)
            return dict(o=st["o"], a=fresh, fresh=fresh, refreshed=torch.ones_like(fresh, dtype=torch.bool), weight=None, nsparse=0)
        weight = None
        if not self.reuses_selection(step, key):
            bm_new = mm.block_mean64(h, self.bm)
            weight = (bm_new - st["bm"]).abs()
            st["sel"] = sel
            st["bm"] = torch.where(mm.selection_mask(sel[0], sel[1], sel[0].shape[0], f, 1), bm_new, st["bm"])
        inds, counts = st["sel"]
        m = mm.selection_mask(inds, counts, n, f, self.bm)
        st["nsparse"] += 1
        a = torch.where(m, fresh, st["a"])
        o = a @ w2.T + b2
        st.update(o=o, a=a)
        return dict(o=o, a=a, fresh=fresh, refreshed=m, weight=weight, nsparse=st["nsparse"])


class ActChecker(gm.GluChecker):
    """`GluChecker` (no dense first layer, any batch size) for SparseDiffMlp: weights (W1, b1 | None, W2, b2), and the model takes the
    module's own quantised input where fc1 is fp8 (`method_model.fp8_operand`)."""

    def after(self, step, inv, layer, module, args, out):
        x = args[0]
        w2, b2 = (t.to(x.device) for t in self.weights[layer][2:])
        st = module.storage
        out = out.clone()       # (the module hands back the output cache's slot itself)
        mm.reload_current(st)
        full = self.model.is_full(step)
        stored_t = st.get_sparse_act_T()
        assert stored_t.shape[-1] == (self.n + 7) // 8 * 8 and (stored_t[..., self.n:] == 0).all(), f"step {step} layer {layer}: padding columns of the cache"
        xm = self.operand(module, x) if self.operand else x
        for b in range(x.shape[0]):
            where = f"step {step} sequence {b} layer {layer}"
            sel = None if full else (st.get_indices()[b], st.get_counts()[b])
            res = self.model.step(step, b, layer, xm[b], sel)
            act_t = stored_t[b][:, : self.n]
            self.check_values(res, out[b], act_t.T, st.get_out_cache()[b], w2, b2, where)
            if not full:
                same = (act_t.view(torch.int16) == self.pre[b][:, : self.n].view(torch.int16)) | res["refreshed"].T
                assert same.all(), f"{where}: {int((~same).sum())} cache elements outside the selection changed"
            if res["weight"] is not None:
                frac = min(mm.captured_fraction(res["weight"], sel[0], sel[1], PASSED))
                self.shortfall = max(self.shortfall, 1.0 - frac)
                if self.eps is not None:
                    assert 1.0 - frac <= self.eps, f"{where}: the selection captures {frac:.4f} of what the exact top-|S| captures"


def linear(w, b, dev):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
    with torch.no_grad():
        lin.weight.copy_(w)
        if b is not None:
            lin.bias.copy_(b)
    return lin.to(dev).bfloat16()


def run_route(route, device, make_module, floors=None, eps=None, what="", fused_scatter=True):
    """Drive LAYERS modules from ``make_module(layer, fc1, fc2, act)`` over the schedule by the integration protocol with the checker's
    assertions after every call.  Returns the checker (``chk.modules``: the modules)."""
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    act, bias, fp8, B, offloaded = ROUTES[route]
    gm.configure(GLOBAL_CONFIG, OFFLOADED if offloaded else None, fused_scatter)
    mods, weights = [], []
    for li in range(LAYERS):
        w1, b1, w2, b2 = act_weights(li, bias)
        fc1, fc2 = linear(w1, b1, device), linear(w2, b2, device)
        w1m = fc1.weight.data.double()
        if fp8:
            from chipmunk_amd.modules.mlp_fp8 import F8Linear
            fc1 = F8Linear.from_linear(fc1, input_float8_dtype=F8)
            w1m = fc1.weight.data.double() * fc1.scale_reciprocal.double()
        weights.append((w1m, None if b1 is None else fc1.bias.data.double(), fc2.weight.data.double(), fc2.bias.data.double()))
        mods.append(make_module(li, fc1, fc2, act))
    model = ActMethodModel(weights, act, SCHEDULE["full_step_every"], SCHEDULE["block_mask_cache"])
    chk = ActChecker(model, weights, N, floors, eps, mm.fp8_operand if fp8 else None, what or route)

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        return (torch.cat([mm.mlp_input(step, b, li, N, K) for b in range(B)]).to(device),)

    mm.drive(mods, 1, STEPS, inputs, chk.after)
    chk.modules = mods
    return chk


# ------------------------------------------------------------------------------------------------------------------ module: emulation
class ActEmulation:
    """SparseDiffMlp's op sequence with a bf16 fc1 / fc2 (mbm == bm == 128, one model invocation per step, fused scatter or not: the
    same arithmetic) in torch on any device: bf16 wherever the module holds bf16, exact sums inside a GEMM or a mean, the selection
    through `glu_method_model.topk_rows`.  No chipmunk operator.  B >= 1."""

    def __init__(self, layer, fc1, fc2, act, cfg):
        assert fc1.weight.dtype == torch.bfloat16 and fc2.weight.dtype == torch.bfloat16
        self.fc1, self.fc2, self.act, self.cfg = [fc1], [fc2], act, cfg["mlp"]
        self.storage, self.calls = gm._Store(), 0

    means = gm.GluEmulation.means
    lin = gm.GluEmulation.lin

    def __call__(self, x):
        fc1, fc2 = self.fc1[0], self.fc2[0]
        w1, b1 = fc1.weight.data, None if fc1.bias is None else fc1.bias.data
        w2, b2 = fc2.weight.data, fc2.bias.data
        step, v = self.calls, self.storage.v
        self.calls += 1
        B, n, _ = x.shape
        if step % self.cfg["full_step_every"] == 0:
            mid = self.lin(x, w1, b1)
            h = bf(gm.act64(self.act, mid.double()))
            out = self.lin(h, w2, b2)
            cache = torch.zeros(B, h.shape[-1], (n + 7) // 8 * 8, dtype=torch.bfloat16, device=x.device)
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
        out, cache = v["out_cache"].clone(), v["sparse_act_T"].clone()
        for b in range(B):
            inds, counts = v["indices"][b], v["counts"][b]
            for g in range(inds.shape[0]):
                rows, cnt = slice(g * 128, min(n, (g + 1) * 128)), int(counts[g])
                cols = inds[g, :cnt].long()
                old = cache[b][cols][:, rows].double().T
                h = x[b, rows].double() @ w1[cols].double().T + (0 if b1 is None else b1[cols].double())
                dg = bf(gm.act64(self.act, h) - old)                                                          # GEMM1: one bf16 rounding
                cache[b][cols, rows] = bf(old.T + dg.double().T)                                              # scatter-add, bf16
                out[b, rows] = bf(bf(dg.double() @ w2.T[cols].double()).double() + out[b, rows].double())     # GEMM2: bf16(acc) + C in bf16
        v.update(sparse_act_T=cache, out_cache=out)
        return out
