"""What the column-sum kernels compute, in plain torch (no chipmunk operator), and the numbers of their error bound.

``cs[b, h, g, j] = sum_{i in group g} exp(s_ij) p_i`` is a sum of positive terms, so every element has a small RELATIVE error and the
bf16 roundings on its path can be counted from the source.  Per element, against `helpers.colsum_exact` (fp64):

    |cs - x| / x  <=  rounds[g] * 2^-8  +  FP32_TERM[family]  (+ FOLD_TERM[family] where the route folds the scale into bf16 q)

Three route families, each with a MIRROR here that rounds where the kernel rounds:

* ``fused``  -- attn64.hip MODE 3, then cs_combine_kernel or topk_mask_kernel<..., PARTS>.  fp32 summands, added in fp32 over a 64-row
  wave and across the waves of a set (``(cs_own + x1) + x2``), ONE bf16 rounding per partial row; the one or two partial rows of a group
  (attn_params.h `colsum_part_rows`, copied below as `part_rows`) added in fp32 and rounded again.  One partial row: one effective
  rounding (the second, of a bf16 value, is exact).  Two partial rows: two.  The summand is ``exp2(s c + log2 p)`` with unit weights,
  ``exp2(s c - m c) * exp2(m c + log2 p)`` with a fixed reference point or the running maximum (`ref`).
* ``wave``   -- colsum64_kernel (attn64.hip): one wave per group, one rounding; q is multiplied by SCALE_LOG2E and rounded to bf16
  first (``val[e] = (__bf16)((float)val[e] * SCALE_LOG2E)``), ``log2 p`` is the accumulator's initial value.
* ``general`` -- attn.hip's CSONLY pass: four waves of 48 rows, partial sums added in fp32 as ``(a0 + a1) + (a2 + a3)``, one rounding
  (`f32_to_bf16_bits(tot)`); it folds the scale in the same way (``qf[qb][ks][e] = (__bf16)((float)qf[qb][ks][e] * SCALE_LOG2E)``).

The constants are measured and pinned by tests/test_colsum_metric_cpu.py; docs/TEST_SENSITIVITY.md, "Column sums", has the tables."""
import math

import torch

GROUP_ROWS = 192
WAVE_ROWS = 64
BF16_EPS = 2.0 ** -8
C32 = float(torch.tensor(0.08838834764, dtype=torch.float32) * torch.tensor(1.44269504089, dtype=torch.float32))   # SCALE_LOG2E as compiled

FAMILY = {"general": "general", "two_pass": "wave", "fused": "fused", "fused_weighted": "fused", "fused_runmax": "fused",
          "fused_per_head": "fused"}
FUSED_REF = {"fused": "unit", "fused_per_head": "unit", "fused_weighted": "fixed", "fused_runmax": "rowmax"}

# FP32_TERM: twice the worst element error of the family's mirror with its bf16 roundings (and the fold) switched off -- fp32 scores,
# exp2 and sums in the kernel's stated order -- against fp64, over the case matrix of tests/test_colsum_metric_cpu.py.
FP32_WORST = {"fused": 1.4e-6, "wave": 1.0e-6, "general": 1.0e-6}
FP32_TERM = {fam: 2 * w for fam, w in FP32_WORST.items()}
# FOLD_TERM: twice the worst element error of the mirror with bf16(q * SCALE_LOG2E) and no other rounding (the routes that fold).  The
# error of one score is averaged over the rows that carry a group's sum, so the short last groups set it (8 rows at Nq = 200); with
# the degenerate p of the batched case (x 1e6 on every 11th row: 17 or 18 rows carry a group) it has a figure of its own.
FOLD_WORST = {"randn p": 0.0035, "degenerate p": 0.0055}
FOLD_TERM = {regime: 2 * w for regime, w in FOLD_WORST.items()}
# The fold is a documented rounding of an INPUT, so its exact effect can be stated: the routes that fold are ALSO held against the fp64
# column sums over bf16(q * SCALE_LOG2E) (`fold_q`, the remaining scale in fp64: FOLD_SCALE_MUL), under the bound without FOLD_TERM.
FOLD_SCALE_MUL = math.log(2.0) * math.sqrt(128.0)
# SEG_FLOOR: the mirrors' worst (group, 64-key tile) segment error per rounds class (against the folded reference where the route
# folds; the short segments of the k_lens cases -- a single column at length 65 -- set the class of two roundings); the bound is twice
# that.  SEG_FLOOR_PLAIN: the folding routes against plain fp64, per p regime.
SEG_FLOOR = {1: 0.0026, 2: 0.0037}
SEG_FLOOR_PLAIN = {"randn p": 0.0025, "degenerate p": 0.0031}
SEG_MARGIN = 2.0
# L_FP32_ERR: worst relative error of an fp32 mirror of the normaliser l (fp32 scores, fp32 exp2, a sequential fp32 sum in key order)
# against fp64 (set by the 33 000-key case); the kernels add in another order, hence the margin of 4.
L_FP32_ERR = 8.3e-6
L_MARGIN = 4.0


def fold_q(q):
    """``bf16(q * SCALE_LOG2E)`` as colsum64_kernel and the CSONLY pass form it (fp32 product, one rounding)"""
    return (q.float() * torch.tensor(C32, dtype=torch.float32, device=q.device)).to(torch.bfloat16)


def p_regime(regime):
    return "degenerate p" if regime == "degenerate p" else "randn p"


def part_rows(j, nwg):
    """`colsum_part_rows` of csrc/attn_params.h, the same arithmetic: the one or two partial rows of group j among the 2 * nwg rows of
    its (batch, head)."""
    a = (3 * j) >> 2
    w0 = 3 * j - 4 * a
    r0 = 2 * a + (1 if w0 else 0)
    r1 = 2 * (a + 1)
    return [r0, r1] if (w0 >= 2 and a + 1 < nwg) else [r0]


def block_row(wb):
    """the partial row that 64-row wave block `wb` of a (batch, head) is added into (attn64.hip: the first nA = 3 - (4a mod 3) waves of
    workgroup a are its first set)"""
    a, w = wb // 4, wb % 4
    return 2 * a + (0 if w < 3 - (4 * a) % 3 else 1)


def group_sets(nq):
    """per group the wave blocks of each of its partial rows: [[blocks of row r0], [blocks of row r1]] (blocks past Nq left out)"""
    nwg, G = (nq + 255) // 256, (nq + GROUP_ROWS - 1) // GROUP_ROWS
    out = []
    for j in range(G):
        rows = part_rows(j, nwg)
        blocks = [wb for wb in (3 * j, 3 * j + 1, 3 * j + 2) if wb < 4 * nwg]
        sets = [[wb for wb in blocks if block_row(wb) == r] for r in rows]
        assert sorted(sum(sets, [])) == blocks and all(sets), (nq, j, rows, blocks)
        out.append(sets)
    return out


def rounds(route, nq):
    """bf16 roundings on the path of an element of group g: [G] floats"""
    G = (nq + GROUP_ROWS - 1) // GROUP_ROWS
    if FAMILY[route] != "fused":
        return [1.0] * G
    return [float(len(part_rows(j, (nq + 255) // 256))) for j in range(G)]


def folds(route):
    return FAMILY[route] != "fused"


def elem_terms(route, regime="randn p", folded_reference=False):
    """(fp32 term, extra) of `helpers.assert_colsums_close` for a route: extra is FOLD_TERM of the p regime where the route folds and
    the reference is plain fp64, else 0"""
    return FP32_TERM[FAMILY[route]], (FOLD_TERM[p_regime(regime)] if folds(route) and not folded_reference else 0.0)


def elem_bound(route, nq, regime="randn p", folded_reference=False):
    """[G] the asserted element bound per group"""
    f, e = elem_terms(route, regime, folded_reference)
    return [r * BF16_EPS + f + e for r in rounds(route, nq)]


def seg_bound(route, nq, regime="randn p", folded_reference=False):
    """[G] the asserted segment bound per group"""
    if folds(route) and not folded_reference:
        return [SEG_MARGIN * SEG_FLOOR_PLAIN[p_regime(regime)]] * len(rounds(route, nq))
    return [SEG_MARGIN * SEG_FLOOR[int(r)] for r in rounds(route, nq)]


def _bf16(x):
    return x.float().to(torch.bfloat16).to(x.dtype)


def _lengths(k, k_lens):
    return [k.shape[2] if k_lens is None else max(1, min(k.shape[2], int(k_lens[b]))) for b in range(k.shape[0])]


def _p_rows(p, B, H, Nq):
    return p.reshape(B, H, -1)[..., :Nq]


def summands32(q, k, p, ref="unit", fold=False):
    """fp32 summands of one (batch, head) as the kernels form them: q ``[Nq, D]``, k ``[L, D]`` bf16, p ``[Nq]`` fp32 -> ``[Nq, L]``.
    A row with p <= 0 adds exactly nothing (``log2 p`` is replaced by -1e30)."""
    qf, kf = q.float(), k.float()
    lp = torch.where(p > 0, torch.log2(p.float().clamp_min(1e-45)), torch.full_like(p.float(), -1.0e30))
    c = torch.tensor(C32, dtype=torch.float32, device=q.device)
    if fold:
        return torch.exp2((qf * c).to(torch.bfloat16).float() @ kf.T + lp[:, None])
    s = qf @ kf.T
    if ref == "unit":
        return torch.exp2(s * c + lp[:, None])
    m = (qf.norm(dim=-1) * kf.norm(dim=-1).max())[:, None] if ref == "fixed" else s.max(dim=-1, keepdim=True).values
    w = torch.exp2(m * c + lp[:, None]).clamp_max(1.0e37)
    return torch.exp2(s * c - m * c) * w


def _blocks(e, rows):
    """[Nq, L] -> [ceil(Nq / rows), L]: fp32 (or fp64) sums over consecutive `rows`-row blocks, the last one short"""
    n = e.shape[0]
    nb = (n + rows - 1) // rows
    return torch.nn.functional.pad(e, (0, 0, 0, nb * rows - n)).view(nb, rows, -1).sum(1)


def combine(blocks, family, nq, bf16=True, second=1.0):
    """per-64-row-block sums ``[..., NB, Nk]`` (NB >= ceil(Nq / 64)) -> column sums ``[..., G, Nk]``, rounded where the family rounds
    (bf16 False: nowhere).  fused: blocks of a set added in wave order, one rounding per partial row, the rows added and rounded;
    `second` multiplies a group's second partial row (a defect: 0 = dropped, 2 = added twice).  wave / general: one rounding."""
    rnd = _bf16 if bf16 else (lambda x: x)
    G = (nq + GROUP_ROWS - 1) // GROUP_ROWS
    out = []
    sets = group_sets(nq)
    nb = 4 * ((nq + 255) // 256)
    if blocks.shape[-2] < nb:          # (the wave blocks past Nq of the last workgroup add nothing)
        blocks = torch.nn.functional.pad(blocks, (0, 0, 0, nb - blocks.shape[-2]))
    for j in range(G):
        if family == "fused":
            parts = []
            for s in sets[j]:
                acc = blocks[..., s[0], :]
                for wb in s[1:]:
                    acc = acc + blocks[..., wb, :]
                parts.append(rnd(acc))
            tot = parts[0] if len(parts) == 1 else parts[0] + second * parts[1]
        else:
            tot = blocks[..., 3 * j:3 * j + 3, :].sum(-2)
        out.append(rnd(tot))
    return torch.stack(out, dim=-2)


def mirror(route, q, k, p, k_lens=None, bf16=True, fold=None):
    """The route's column sums as its kernels form them (module docstring): ``[B, H, G, Nk]`` fp32.  bf16 False: the roundings of the
    sums switched off; fold: whether q * SCALE_LOG2E is rounded to bf16 first (None: as the family does)."""
    fam = FAMILY[route]
    fold = (fam != "fused") if fold is None else fold
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]
    G = (Nq + GROUP_ROWS - 1) // GROUP_ROWS
    pr = _p_rows(p, B, H, Nq)
    out = torch.zeros(B, H, G, Nk, dtype=torch.float32, device=q.device)
    for b, L in enumerate(_lengths(k, k_lens)):
        for h in range(H):
            e = summands32(q[b, h], k[b, h, :L], pr[b, h], FUSED_REF.get(route, "unit"), fold)
            if fam == "fused":
                cs = combine(_blocks(e, WAVE_ROWS), fam, Nq, bf16)
            elif fam == "wave":
                cs = _blocks(e, GROUP_ROWS)
            else:
                w = torch.nn.functional.pad(_blocks(e, 48), (0, 0, 0, 4 * G - (Nq + 47) // 48)).view(G, 4, L)
                cs = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
            out[b, h, :, :L] = _bf16(cs) if bf16 and fam != "fused" else cs
    return out


def l_mirror32(q, k, k_lens=None):
    """the normaliser ``l = 1 / sum_j exp(s_ij)`` in fp32: fp32 scores, fp32 exp2, a SEQUENTIAL fp32 sum in key order: ``[B, H, Nq]``"""
    B, H, Nq, _ = q.shape
    c = torch.tensor(C32, dtype=torch.float32, device=q.device)
    out = torch.zeros(B, H, Nq, dtype=torch.float32, device=q.device)
    for b, L in enumerate(_lengths(k, k_lens)):
        for h in range(H):
            e = torch.exp2((q[b, h].float() @ k[b, h, :L].float().T) * c).T.contiguous()      # [L, Nq]
            acc = torch.zeros(Nq, dtype=torch.float32, device=q.device)
            for j in range(L):
                acc = acc + e[j]
            out[b, h] = 1.0 / acc
    return out


def l_exact(q, k, k_lens=None):
    """``1 / sum_j exp(q_i . k_j / sqrt(D))`` in fp64: ``[B, H, Nq]``"""
    B, H, Nq, D = q.shape
    out = torch.zeros(B, H, Nq, dtype=torch.float64, device=q.device)
    for b, L in enumerate(_lengths(k, k_lens)):
        for h in range(H):
            out[b, h] = 1.0 / torch.exp((q[b, h].double() @ k[b, h, :L].double().T) / math.sqrt(D)).sum(-1)
    return out


def exact_blocks(q, k, p, k_lens=None, scale_mul=1.0, hook=None):
    """fp64 per-64-row-block sums of the exact summands ``exp(s_ij) p_i``: ``[B, H, 3 G, Nk]``, 0 for rows past Nq and columns past the
    lengths.  hook(E, b, h) may change one (batch, head)'s ``[Nq, L]`` summands in place: the defects of the CPU file."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    G = (Nq + GROUP_ROWS - 1) // GROUP_ROWS
    pr = _p_rows(p, B, H, Nq).double()
    out = torch.zeros(B, H, 3 * G, Nk, dtype=torch.float64, device=q.device)
    for b, L in enumerate(_lengths(k, k_lens)):
        for h in range(H):
            e = torch.exp((q[b, h].double() @ k[b, h, :L].double().T) * (scale_mul / math.sqrt(D))) * pr[b, h, :, None]
            if hook is not None:
                hook(e, b, h)
            w = _blocks(e, WAVE_ROWS)
            out[b, h, :w.shape[0], :L] = w
    return out


# --------------------------------------------------------------------------- the case matrix shared by the CPU and the GPU file (CPU tensors)
SHAPES = {          # name -> (Nq, Nk, H)
    "1000x1000": (1000, 1000, 2),        # six groups: all four `part_rows` phases, a 40-row last group, the `a + 1 < nwg` cut on it
    "777x200": (777, 200, 2),            # a ragged key tile, more rows than keys
    "960x64": (960, 64, 2),              # one key tile
    "200x192": (200, 192, 2),            # exactly three key tiles, an 8-row last group
    "260x1000": (260, 1000, 2),          # fewer rows than keys
    "448x33000": (448, 33000, 1),        # the signal is 0.006: smaller than the absolute tolerance the suite used
}
REGIMES = ("previous step", "own l")
KLENS_CASES = {     # tests/test_gpu_attn_klens.py: (n, its two length sets); B = 3, H = 2
    "general": (416, ([416, 33, 1], [32, 97, 415])),
    "wave64": (448, ([448, 65, 64], [129, 63, 1])),
}


def _randn_bf16(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def problem(shape, regime):
    """q0 / k / v as tests/test_gpu_attn64.py::test_colsum64_vs_oracle draws them.  "previous step": the call sees
    ``q = bf16(q0 + 0.1 randn)`` and p = the normaliser of q0.  "own l": q = q0 and p = its own exact normaliser (every group's sums
    then add up to its row count).  p is ``[B, H, Nq, 1]`` fp32."""
    nq, nk, H = SHAPES[shape]
    q0, k, v = _randn_bf16(1, H, nq, 128, seed=nq), _randn_bf16(1, H, nk, 128, seed=nk + 1), _randn_bf16(1, H, nk, 128, seed=nk + 2)
    q = q0
    if regime == "previous step":
        q = (q0.float() + 0.1 * torch.randn(q0.shape, generator=torch.Generator().manual_seed(3))).to(torch.bfloat16)
    else:
        assert regime == "own l", regime
    return dict(q=q, q0=q0, k=k, v=v, p=l_exact(q0, k).float()[..., None], k_lens=None, regime=regime, nq=nq, nk=nk)


def degenerate_problem():
    """tests/test_gpu_attn64.py::test_fused_colsum_strided_batched_and_degenerate_p: B = 2, ``[B, N, H, D]`` storage viewed as
    ``[B, H, N, D]``; p = the call's own normaliser with zeros on rows 5::7 (they must add exactly nothing) and x 1e6 on rows 3::11"""
    B, H, N = 2, 3, 640
    q, k, v = [_randn_bf16(B, N, H, 128, seed=s).permute(0, 2, 1, 3) for s in (51, 52, 53)]
    p = l_exact(q, k).float()
    p[:, :, 5::7] = 0.0
    p[:, :, 3::11] *= 1.0e6
    return dict(q=q, q0=q, k=k, v=v, p=p[..., None].contiguous(), k_lens=None, regime="degenerate p", nq=N, nk=N)


def klens_problem(kind, which):
    """the inputs and one of the two length sets of tests/test_gpu_attn_klens.py; p = the exact normaliser over the valid keys"""
    n, lens = KLENS_CASES[kind]
    q, k, v = [_randn_bf16(3, 2, n, 128, seed=n + s) for s in (1, 2, 3)]
    kl = list(lens[which])
    return dict(q=q, q0=q, k=k, v=v, p=l_exact(q, k, kl).float()[..., None], k_lens=kl, regime="own l", nq=n, nk=n)


def cpu_cases():
    """name -> () -> problem: every input set of the GPU file"""
    out = {f"{s}, {r}": (lambda s=s, r=r: problem(s, r)) for s in SHAPES for r in REGIMES}
    out["640x640 batched, degenerate p"] = degenerate_problem
    for kind in KLENS_CASES:
        for which in (0, 1):
            out[f"k_lens {kind} {KLENS_CASES[kind][1][which]}"] = (lambda kind=kind, which=which: klens_problem(kind, which))
    return out
