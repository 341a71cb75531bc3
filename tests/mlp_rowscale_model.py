"""The fp8 GEMM1 with one scale per token row and one per fc1 column (``csp_mlp_mm1_fp8_act_rs``), the row-wise input quantiser
(``quantize_fp8_rowwise``) and ``F8Linear(scaling="row")``, for tests/test_mlp_rowscale_host.py, tests/test_gpu_mlp_rowscale.py,
tests/test_gpu_quantize_fp8_rowwise.py and tests/test_gpu_mlp_rowscale_e2e.py.  helpers.py and mlp_act_model.py are imported, not edited.

Operator level: problems whose scale vectors make a misplaced scale visible (`rs_problem`), the operator's definition in fp64
(`rs_exact`), a plain-torch fp32 mirror of the new epilogue (`rs_mirror`) with its four mutants, and the quantiser's chain (`quantize_chain`).

Module level: an fp64 model of SparseDiffMlp over a row-scaled fc1 is mlp_act_model.ActMethodModel fed the dequantised weight and the
module's own row-quantised input (`row_operand`).
"""
import torch

import method_model as mm_
import mlp_act_model as am
from helpers import F8, MLP_BM, mlp_act64, mlp_group_cols, mlp_problem

bf = am.bf
FP8_MAX = 448.0

# ------------------------------------------------------------------------------------------------------------------ quantiser


def quantize_chain(x, max_value=FP8_MAX):
    """chipmunk_quantize_fp8_rowwise by its definition, in torch (fp32; on the CPU the division is IEEE's): returns (e4m3 [rows, K],
    scale_recip fp32 [rows]).  The quotient is tensor / tensor: torch evaluates `number / tensor` as reciprocal-then-multiply, two
    roundings (448 / 3 comes out one ulp high), which is not the division the contract states."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    scale = (torch.full_like(amax, max_value) / torch.clamp(amax, min=1e-12)).clamp(max=max_value)
    out = (xf * scale[:, None]).clamp(-max_value, max_value).to(F8)
    return out, 1.0 / scale


def quantizer_rows(rows, K, seed):
    """bf16 [rows, K]: row r spans the magnitudes 1e-3 .. 1e3 (10^(-3 + 6 r / rows) x randn); planted rows -- an all-zero row, a row of
    e4m3 rounding ties (its amax is 448, so the scale is exactly 1 and the row holds midpoints between e4m3 neighbours: 17, 19, 21, 23 in
    the binade of spacing 2, 0.5 + 1/32 in the one of spacing 1/16, the half of the smallest subnormal 2^-10, each with both signs), a row whose
    largest value sits in its last element."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (-3.0 + 6.0 * torch.arange(rows) / max(rows, 1))
    x = (torch.randn(rows, K, generator=g) * mag[:, None]).to(torch.bfloat16)
    ties = torch.tensor([448.0, 17.0, -19.0, 21.0, -23.0, 0.53125, -0.53125, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 27.0, -29.0, 1.0625, -1.1875, 9.5, -10.5])
    if rows >= 2:
        x[rows // 2] = 0
    x[0] = ties.repeat(K // 16).to(torch.bfloat16)
    if rows >= 3:
        x[rows - 1, K - 1] = 1000.0
    return x


# ------------------------------------------------------------------------------------------------------------------ operator: problems
ROW_PATTERN = (0.4, 1.0, 2.5, 1.0)        # scale of token row m relative to the tensor's: neighbours differ by 2.5 x
COL_PATTERN = (0.5, 1.25)                 # ... of fc1 column i (by its parity): 2.5 x
BIAS_SCALE = 0.3                          # against a pre-activation of 0.5 * 0.06 * sqrt(K = 128) = 0.34 x the scale patterns

# name -> (M, F, counts, act, bias): K = 128; M = 128 (one group), 200 (a ragged last group of 72 rows; whole runs of four rows: the 16-byte
# row-scale read) and 203 (75 rows, cache pitch 208, M % 4 != 0: the clamped single reads); counts that end inside a 64-column tile, the
# short last segment at least 16 columns wide as in helpers.MLP_COUNTS (the error of a segment of 8 elements is hardly an average: one
# bf16 rounding alone reaches 0.0035 there)
SHAPES = {"M128 F64": (128, 64, [40]), "M200 F256": (200, 256, [144, 208]), "M203 F128": (203, 128, [128, 24])}


def rs_cases():
    out = {}
    for shape, (M, F, counts) in SHAPES.items():
        for act in ("gelu_tanh", "silu", "gelu"):
            for biases in (True, False):
                out[f"{shape} {act}{'' if biases else ' no bias'}"] = dict(M=M, F=F, counts=counts, act=act, biases=biases, seed=700 + len(out))
    return out


def rs_problem(M, F, counts, act, biases, seed, K=128):
    """`helpers.mlp_problem` (fp8, ungated, random cache) with scale VECTORS in place of the two numbers: sa [M] = ra * ROW_PATTERN[m % 4],
    sb [F] = rb * COL_PATTERN[i % 2], and index lists that alternate odd and even columns (odd first), so that neighbouring kept columns'
    scales differ by 2.5 x and the scale at packed position j is never that of column idx[g, j].  The operands stay the e4m3 tensors: the
    operator's definition holds for any scale vectors.  The bias is BIAS_SCALE randn."""
    p = mlp_problem(M=M, K=K, F=F, seed=seed, regime="random", act=act, fp8=True, gated=False, biases=biases, counts=counts)
    g = torch.Generator().manual_seed(seed + 1)
    odd, even = torch.arange(1, F, 2), torch.arange(0, F, 2)
    inds = []
    for _ in range(p["G"]):
        o, e = odd[torch.randperm(F // 2, generator=g)], even[torch.randperm(F // 2, generator=g)]
        inds.append(torch.stack([o, e], dim=1).reshape(-1))
    p["inds"] = torch.stack(inds).to(torch.int32)
    p["sa"] = (p["ra"] * torch.tensor(ROW_PATTERN).repeat((M + 3) // 4)[:M]).float().contiguous()
    p["sb"] = (p["rb"] * torch.tensor(COL_PATTERN).repeat(F // 2)).float().contiguous()
    if biases:
        p["bias"] = bf(torch.randn(F, generator=g) * BIAS_SCALE)
    return p


def input_condition(p):
    """The condition on the inputs that makes the mutants visible (checked, not measured): neighbouring rows' and neighbouring kept columns'
    scales differ by a factor >= 2, the scale at packed position j is not that of column idx[g, j], the indices are not the identity, and
    the bias is not small against the pre-activation (rms ratio >= 0.25)."""
    sa, sb = p["sa"].double(), p["sb"].double()
    r = sa[1:] / sa[:-1]
    assert (torch.maximum(r, 1 / r) >= 2).all()
    for g in range(p["G"]):
        n = int(p["cnt"][g])
        col = p["inds"][g, :n].long()
        c = sb[col][1:] / sb[col][:-1]
        assert (torch.maximum(c, 1 / c) >= 2).all()
        m = sb[:n] / sb[col]
        assert (torch.maximum(m, 1 / m) >= 2).all()
        assert not torch.equal(col, torch.arange(n))
    if p["bias"] is not None:
        h = rs_pre(p, bias=False)
        live = torch.arange(p["F"]) < mlp_group_cols(p["cnt"], p["M"])[:, None]
        assert p["bias"].double().pow(2).mean().sqrt() >= 0.25 * h[live].pow(2).mean().sqrt()


def rs_pre(p, bias=True):
    """the pre-activation in fp64, packed layout [M, F], 0 at and past the counts"""
    h = torch.zeros(p["M"], p["F"], dtype=torch.float64, device=p["a"].device)
    ad, wd = p["a"].double(), p["w"].double()
    for g in range(p["G"]):
        rows, n = slice(g * MLP_BM, min(p["M"], (g + 1) * MLP_BM)), int(p["cnt"][g])
        if n == 0:
            continue
        col = p["inds"][g, :n].long()
        v = (ad[rows] @ wd[col].T) * p["sa"][rows, None].double() * p["sb"][col][None, :].double()
        h[rows, :n] = v + p["bias"][col].double() if bias and p["bias"] is not None else v
    return h


def rs_exact(p):
    """(delta, fresh) of the operator by its definition in fp64 (include/chipmunk_hip.h, "fp8 row scales"), packed layout"""
    h = rs_pre(p)
    live = torch.arange(p["F"], device=h.device) < mlp_group_cols(p["cnt"], p["M"]).to(h.device)[:, None]
    fresh = torch.where(live, mlp_act64(p["act"], h), torch.zeros_like(h))
    old = torch.zeros_like(h)
    for g in range(p["G"]):
        rows, n = slice(g * MLP_BM, min(p["M"], (g + 1) * MLP_BM)), int(p["cnt"][g])
        old[rows, :n] = p["cache0"][p["inds"][g, :n].long()][:, rows].double().T
    return fresh - old, fresh


# ------------------------------------------------------------------------------------------------------------------ operator: mirror
NEXT_ROW, FIRST_ROW, PACKED_COL, AFTER_BIAS = ("the row scale of row m + 1 used for row m", "scale_a[0] used for every row",
                                               "the column scale taken at packed position j", "the column scale applied after the bias")
MUTANTS = (NEXT_ROW, FIRST_ROW, PACKED_COL, AFTER_BIAS)


def rs_mirror(p, update="none", mutant=None):
    """The new epilogue in plain torch, fp32 sums and then the operator's roundings (mlp_act_model.mm1_act_mirror with the scale vectors):
    t = bf16(act((sum * sa[m]) * sb[idx[g, j]] + bias[idx[g, j]])), c = bf16(t - cache).  update "none" | "store" (cache = t) | "scatter"
    (cache = bf16(cache + c)).  mutant: one of MUTANTS.  Returns (c [M, F] bf16 with am.SENT at and past the counts, cache [F, M])."""
    assert update in ("none", "store", "scatter") and (mutant is None or mutant in MUTANTS)
    M, f = p["M"], p["F"]
    c = torch.full((M, f), am.SENT, dtype=torch.bfloat16)
    cache = p["cache0"].clone()
    a, w = p["a"].float(), p["w"].float()
    for g in range(p["G"]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(p["cnt"][g])
        if n == 0:
            continue
        col = p["inds"][g, :n].long()
        acc = a[rows] @ w[col].T
        m = torch.arange(rows.start, rows.stop)
        sa = p["sa"][(m + 1).clamp(max=M - 1)] if mutant == NEXT_ROW else p["sa"][0].expand(len(m)) if mutant == FIRST_ROW else p["sa"][m]
        sb = p["sb"][:n] if mutant == PACKED_COL else p["sb"][col]
        b = 0.0 if p["bias"] is None else p["bias"][col].float()
        pre = ((acc * sa[:, None]) + b) * sb[None, :] if mutant == AFTER_BIAS else (acc * sa[:, None]) * sb[None, :] + b
        old = cache[col][:, rows].float().T
        t = bf(am.act32(p["act"], pre))
        d = bf(t.float() - old)
        c[rows, :n] = d
        if update != "none":
            cache[col, rows] = (t if update == "store" else bf(old + d.float())).T
    return c, cache


def rs_view(p):
    """p as mlp_act_model's checkers read it (an fp8 problem: the activation is rounded to bf16 before the subtraction)"""
    return dict(p, fp8=True)


# ------------------------------------------------------------------------------------------------------------------ module
def row_operand(module, x):
    """the module's own row-quantised input, dequantised, in fp64 (what the fp64 model of a row-scaled fc1 is fed)"""
    xq, recip = module.fc1[0].quantize_input_rowwise(x)
    return xq.double() * recip.double().unsqueeze(-1)


def outlier_tokens(x, every=16, gain=64.0):
    """x [B, N, K] with one token in `every` scaled by `gain`"""
    x = x.clone()
    x[:, ::every] = (x[:, ::every].float() * gain).to(x.dtype)
    return x


E2E_N, E2E_STEPS = 200, 4       # two groups, the last of 72 rows; a full step and three sparse steps (am.SCHEDULE: full_step_every = 10)


def e2e_input(step, li, B, n=E2E_N, outliers=False):
    x = torch.cat([mm_.mlp_input(step, b, li, n, am.K) for b in range(B)])
    return outlier_tokens(x) if outliers else x


def run_rows(device, make_module, act, bias, B, fused_scatter=True, floors=None, eps=None, scaling="row", outliers=False, what=""):
    """mlp_act_model.run_route for an e4m3 fc1 built with `scaling`: am.LAYERS modules from ``make_module(layer, fc1, fc2, act)`` over
    E2E_STEPS steps of E2E_N tokens by the integration protocol, the checker's assertions after every call (floors None: nothing is
    asserted against the model).  The fp64 model gets the dequantised weight and, per call, the module's own quantised input.  Returns
    the checker (``chk.modules``, ``chk.outs``: the outputs per (step, layer), ``chk.xs``: the inputs, ``chk.unquantised``: the outputs of
    the same fp64 model on the UNQUANTISED bf16 weights and inputs with the module's own selections -- what the method computes without
    fp8, staleness of the unselected columns included, so that a module's distance from it is its quantisation error alone)."""
    from chipmunk_amd.modules.mlp_fp8 import F8Linear
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    am.gm.configure(GLOBAL_CONFIG, None, fused_scatter)
    mods, weights = [], []
    for li in range(am.LAYERS):
        w1, b1, w2, b2 = am.act_weights(li, bias)
        fc1, fc2 = am.linear(w1, b1, device), am.linear(w2, b2, device)
        fc1 = F8Linear.from_linear(fc1, input_float8_dtype=F8, scaling=scaling)
        w1m = fc1.weight.data.double() * fc1.scale_reciprocal.double()
        weights.append((w1m, None if b1 is None else fc1.bias.data.double(), fc2.weight.data.double(), fc2.bias.data.double()))
        mods.append(make_module(li, fc1, fc2, act))
    model = am.ActMethodModel(weights, act, am.SCHEDULE["full_step_every"], am.SCHEDULE["block_mask_cache"])
    operand = row_operand if scaling == "row" else mm_.fp8_operand
    chk = am.ActChecker(model, weights, E2E_N, floors, eps, operand, what)
    chk.outs, chk.xs, chk.unquantised = {}, {}, {}
    plain = am.ActMethodModel([am.act_weights(li, bias) for li in range(am.LAYERS)], act, am.SCHEDULE["full_step_every"], am.SCHEDULE["block_mask_cache"])

    def inputs(step, inv, li):
        chk.before(mods[li], step, li)
        chk.xs[step, li] = e2e_input(step, li, B, outliers=outliers).to(device)
        return (chk.xs[step, li],)

    def after(step, inv, li, mod, args, out):
        chk.outs[step, li] = out.clone()
        chk.after(step, inv, li, mod, args, out)
        st = mod.storage
        sels = [None if plain.is_full(step) else (st.get_indices()[b], st.get_counts()[b]) for b in range(B)]
        chk.unquantised[step, li] = torch.stack([plain.step(step, b, li, args[0][b], sels[b])["o"] for b in range(B)])

    mm_.drive(mods, 1, E2E_STEPS, inputs, after)
    chk.modules = mods
    return chk


def dense_exact(li, bias, act, x):
    """fc2(act(fc1(x))) of layer li in fp64 on the UNQUANTISED bf16 weights"""
    w1, b1, w2, b2 = (None if t is None else t.double().to(x.device) for t in am.act_weights(li, bias))
    h = x.double() @ w1.T
    return mlp_act64(act, h if b1 is None else h + b1) @ w2.T + b2


def rel_err(got, exact):
    """mean over the token rows of ||got_row - exact_row|| / ||exact_row||: every token counts alike (in one norm over the whole tensor
    the outlier tokens, 64 x the rest, are all that shows)"""
    return float(((got.double() - exact).norm(dim=-1) / exact.norm(dim=-1)).mean())


def dense_quantised(li, bias, act, x, scaling, tensor_amax=None):
    """the CPU mirror of a full step with an e4m3 fc1: fc2(bf16(act(bf16(fc1 on the quantised operands)))) in fp64 sums, per-row / per-feature
    scales ("row") or one scale each ("tensor"; tensor_amax: the input amax the frozen scale was calibrated on)"""
    w1, b1, w2, b2 = (None if t is None else t.double() for t in am.act_weights(li, bias))
    xf, wf = x.float(), w1.float()
    if scaling == "row":
        xq, sa = quantize_chain(xf.reshape(-1, xf.shape[-1]))
        xd = (xq.double() * sa.double()[:, None]).reshape(x.shape)
        ws = (FP8_MAX / wf.abs().amax(dim=1, keepdim=True).clamp(min=1e-12)).clamp(max=FP8_MAX)
    else:
        s = (FP8_MAX / torch.clamp(xf.abs().max() if tensor_amax is None else tensor_amax, min=1e-12)).clamp(max=FP8_MAX)
        xd = (x * s).clamp(-FP8_MAX, FP8_MAX).to(F8).double() / s.double()
        ws = (FP8_MAX / wf.abs().max().clamp(min=1e-12)).clamp(max=FP8_MAX)
    wd = (wf * ws).clamp(-FP8_MAX, FP8_MAX).to(F8).double() / ws.double()
    h = bf(xd @ wd.T + (0 if b1 is None else b1)).double()
    return bf(bf(mlp_act64(act, h)).double() @ w2.T + b2)
