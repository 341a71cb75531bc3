"""The three row-wise normalisation operators by their definitions, in fp64 and plain torch (no chipmunk operator: CPU or device
tensors alike), the input families that reach what `randn * const` rows never contain, and the mutants -- the exact result with
one defect, rounded where the operator rounds -- that the segment bound of docs/TEST_SENSITIVITY.md, "Row-wise norm kernels", must
reject.  tests/test_rowwise_metric_cpu.py pins the constants below; tests/test_gpu_rowwise_accuracy.py asserts them on the device.

Definitions (ops/qkv.py, the kernel headers of csrc/indexed_io.hip and csrc/rowwise.hip):

* per-head RMSNorm (`qkv_split_norm`): ``x / sqrt(mean_128(x^2) + eps) * weight``, then for tokens ``< rope_rows`` the rotation of
  pairs (2i, 2i+1) by the pair's angle: ``(re c - im s, re s + im c)``; output ``[1, H, n, 128]``.
* row-wide RMSNorm (`split_heads_rownorm`): the same with the mean over ``heads * 128`` columns of a part, per part norm and rope flags,
  a weight of either dtype (widened exactly); output ``[B, H, n, 128]`` per part.
* `residual_ln_modulate`: ``x' = x + gate * y``; ``xm = shift + (x' - mean) / sqrt(var + eps) * (1 + scale)``, biased variance;
  ``1 + scale`` is the bf16 tensor the reference materialises (an input rounding, taken as the input it is)."""
import math

import torch

EPS = 1e-6
SEG_W = 128                    # the metric's segment: one head row of an RMSNorm output, 128 consecutive columns of xm

# ---- floors: the worst segment of each operator's CPU path (the reference's op sequence) against the exact references, over every
# family and case of tests/test_rowwise_metric_cpu.py (which pins them: test_floor_constants_are_tight), few-element segments taken out, rounded up.
# The number of bf16 roundings on an element's path orders them: one rounding is 2^-8 / sqrt(3) = 0.0023 rms.
FLOOR_LN = 0.0036                                              # bf16(xn), bf16(shift + xn * bf16(1 + scale))
FLOOR_HEAD = {False: 0.0036, True: 0.0046}                     # bf16(x r), bf16(* w) (, bf16 after the rotation)
FLOOR_WIDE = {("none", False): 0.0022, ("none", True): 0.0036,     # weight kind of the part, rotated token or not
              ("bf16", False): 0.0035, ("bf16", True): 0.0044,
              ("fp32", False): 0.0037, ("fp32", True): 0.0036}
MARGIN = 2.0                   # what a correct kernel may do differently: the order of the sums, an fp32 rotation


# ---- the derived term of a segment with a handful of elements.  A floor is a statement about 128 independent roundings: their relative
# L2 error is 2^-8 / sqrt(3) per rounding, within a few per cent.  A segment with at most FEW non-zero elements, or one dominated by a
# single element (`few_element_segments`) -- the one element of a one-hot row, in ``xm`` the one large element of such a row, the 8 columns
# of ``xm`` behind a multiple of 128, a row of C = 8 -- has no such average: its error is the error of its worst element, up to 2^-8 per
# rounding on the path, and the largest over many such segments grows with their number (8 209 rows of 8 columns on the device, 70 here).  For those segments the bound is the worst case itself, read from the source, not a constant
# measured on the CPU: ``roundings * 2^-8`` for the RMSNorm operators (csrc/indexed_io.hip `round_bf16_pair(a, b)`, `pack_bf16x2(a * w,
# b * w)`, `pack_bf16x2(re * cr + ...)`; csrc/rowwise.hip `round_bf16_pair(re, im)` twice and `pack_bf16x2` in `rownorm_rows`), and for ``xm``
# ``2^-8 (||xn (1 + scale)||_seg + ||xm||_seg) / ||xm||_seg``: `round_bf16_pair(a, b)` on the normalised value, whose error the
# modulation carries, and `pack_bf16x2` on the sum (csrc/rowwise.hip, residual_ln_modulate_kernel).  HARD_SLACK covers the compounding
# ((1 + 2^-8)^3 - 1 = 3 * 2^-8 * 1.004) and the fp32 statistics (relative 1e-6).  Every other segment keeps MARGIN * floor.
FEW = 8
BF16_EPS = 2.0 ** -8
HARD_SLACK = 1.01
ROUNDINGS_HEAD = {False: 2, True: 3}
ROUNDINGS_WIDE = {("none", False): 1, ("none", True): 2, ("bf16", False): 2, ("bf16", True): 3, ("fp32", False): 2, ("fp32", True): 2}


def _pick(cond, a, b):
    return cond.double() * (a - b) + b


def _segs(t, width):
    pad = (-t.shape[-1]) % width
    return torch.nn.functional.pad(t, (0, pad)).unflatten(-1, (-1, width))


def few_element_segments(exact, width=None):
    """bool per segment (``exact.shape[:-1]``, or ``[..., segments]`` with `width`): at most FEW elements of the exact segment are non-zero,
    or its largest element alone holds a quarter or more of its sum of squares (of 128 normal values the largest holds 1 / 19 on average and a
    quarter with probability 1e-6; the one large element of a LayerNorm row that is zero elsewhere holds all but 1e-4)"""
    s = _segs(exact, exact.shape[-1] if width is None else width)
    few = ((s != 0).sum(-1) <= FEW) | (4.0 * s.abs().amax(-1).pow(2) >= s.pow(2).sum(-1))
    return few[..., 0] if width is None else few


def bound_ln(exact, prod):
    """(bound per segment of ``xm``, few-element mask).  prod: the exact ``xn * (1 + scale)``"""
    few = few_element_segments(exact, SEG_W)
    den = _segs(exact, SEG_W).norm(dim=-1)
    hard = HARD_SLACK * BF16_EPS * (1.0 + _segs(prod, SEG_W).norm(dim=-1) / den.clamp_min(1e-300))
    return torch.where(few, hard, torch.full_like(hard, MARGIN * FLOOR_LN)), few


def _bound_rms(floors, roundings, rotated, exact):
    few = few_element_segments(exact)
    rotated = rotated.to(exact.device)
    return torch.where(few, HARD_SLACK * BF16_EPS * _pick(rotated, roundings[0], roundings[1]), MARGIN * _pick(rotated, floors[0], floors[1])), few


def bound_head(rotated, exact):
    """rotated: bool ``[1, H, n]``, the rotated output rows -> (bound per segment, few-element mask)"""
    return _bound_rms((FLOOR_HEAD[True], FLOOR_HEAD[False]), (ROUNDINGS_HEAD[True], ROUNDINGS_HEAD[False]), rotated, exact)


def bound_wide(kind, rotated, exact):
    return _bound_rms((FLOOR_WIDE[(kind, True)], FLOOR_WIDE[(kind, False)]), (ROUNDINGS_WIDE[(kind, True)], ROUNDINGS_WIDE[(kind, False)]), rotated, exact)


def weight_kind(w):
    return "none" if w is None else "bf16" if w.dtype == torch.bfloat16 else "fp32"


def rotated_tokens(B, H, n, rope_rows, flag=True, device="cpu"):
    """[B, H, n] bool: the output rows that were rotated"""
    return ((torch.arange(n, device=device) < (rope_rows if flag else 0))[None, None, :]).expand(B, H, n)


# ------------------------------------------------------------------------------------------------ defects
EPS_ABSENT, EPS_X10, EPS_OUTSIDE = "eps absent", "eps x 10", "eps outside the square root"
STATS_ROW, STATS_HEAD = "statistics of row r+1", "statistics of head h+1"
HEAD_FOR_ROW, ROW_FOR_HEAD = "per-head statistics where row-wide is meant", "row-wide statistics where per-head is meant"
LAST8_OUT, LAST_HEAD_OUT = "last 8 columns left out of the sum", "last head left out of the sum"
LAST8_TWICE, DIVISOR = "last 8 columns counted twice", "divisor 512 * NV instead of C"
NO_MEAN_IN_VAR, SCALE_FOR_ONE, SHIFT_SCALE_SWAPPED = "mean not subtracted in the variance", "scale where 1 + scale is meant", "shift and scale exchanged"
GATE_TWICE, XM_BEFORE_RESIDUAL = "gate * y added twice", "xm from the row before the residual"
W_COL8, Q_ON_K, ROT_BEFORE_WEIGHT = "weight of column c+8", "the q weight on k", "rotation before the weight product"
ROT_NEXT_TOKEN, ROT_BOUNDARY, ROT_SIGN = "table row of token t+1", "row rope_rows rotated, row rope_rows - 1 not", "opposite sign of sin"
ROT_HALF, ROT_UNFLAGGED = "pairs (i, i+64)", "a part without the flag rotated"
SCALE_102, SCALE_101, UNBIASED = "scale x 1.02 on every 128th row", "scale x 1.01 on every 128th row", "unbiased variance (C - 1)"
NO_DEFECT = "no defect"

EPS_DEFECTS = (EPS_ABSENT, EPS_X10, EPS_OUTSIDE)
RECORDED = (SCALE_101, UNBIASED)
# operator -> its counted defects
DEFECTS = {
    "head": EPS_DEFECTS + (STATS_ROW, STATS_HEAD, ROW_FOR_HEAD, LAST8_OUT, LAST8_TWICE, W_COL8, Q_ON_K, ROT_BEFORE_WEIGHT, ROT_NEXT_TOKEN,
                           ROT_BOUNDARY, ROT_SIGN, ROT_HALF, ROT_UNFLAGGED, SCALE_102),
    "wide": EPS_DEFECTS + (STATS_ROW, HEAD_FOR_ROW, LAST8_OUT, LAST_HEAD_OUT, LAST8_TWICE, DIVISOR, W_COL8, Q_ON_K, ROT_BEFORE_WEIGHT,
                           ROT_NEXT_TOKEN, ROT_BOUNDARY, ROT_SIGN, ROT_HALF, ROT_UNFLAGGED, SCALE_102),
    "ln": EPS_DEFECTS + (STATS_ROW, LAST8_OUT, LAST8_TWICE, DIVISOR, NO_MEAN_IN_VAR, SCALE_FOR_ONE, SHIFT_SCALE_SWAPPED, GATE_TWICE,
                         XM_BEFORE_RESIDUAL, SCALE_102),
}
# defect -> the families on which it is counted (it must exceed the bound in every case of them where it is not provably inert).
# eps: only rows whose mean square is near eps see it.  A defect that moves one 8-column piece's share of a row's sum is counted where
# one column can carry the row (special); on the other families every column carries 1 / C of the sum, so at C >= 384 it moves
# the result by less than a rounding: recorded there, never counted.
ALL = ("iid", "ladder", "head_ladder", "special")
FAMILIES = {d: ALL for ops in DEFECTS.values() for d in ops}
FAMILIES.update({d: ("ladder", "special") for d in EPS_DEFECTS})
FAMILIES.update({LAST8_OUT: ("special",), LAST8_TWICE: ("special",)})


def _bf(t):
    return t.to(torch.bfloat16).double()


def _every_128th(rows, device):
    return torch.arange(rows, device=device) % 128 == 0


# ------------------------------------------------------------------------------------------------ RMSNorm + rotation
def _rotate(v, cos, sin, rope_rows, defect=None):
    """v [B, n, H, 128] fp64: tokens < rope_rows rotated, pair (2i, 2i+1) by the angle both of its table entries carry"""
    r, n = int(rope_rows), v.shape[1]
    if r == 0 or cos is None:
        return v
    dev = v.device
    c, s = cos[:r, 0::2].double(), sin[:r, 0::2].double()
    if defect == ROT_SIGN:
        s = -s
    if defect == ROT_NEXT_TOKEN:
        c, s = torch.roll(c, -1, 0), torch.roll(s, -1, 0)
    rows = table = torch.arange(r, device=dev)
    if defect == ROT_BOUNDARY:
        rows = torch.cat([rows[:r - 1], torch.arange(r, min(r + 1, n), device=dev)])
        table = torch.cat([table[:r - 1], torch.full((rows.numel() - (r - 1),), r - 1, device=dev)])
    sel = v[:, rows]
    cc, sn = c[table][None, :, None, :], s[table][None, :, None, :]
    if defect == ROT_HALF:
        re, im = sel[..., :64], sel[..., 64:]
        new = torch.cat([re * cc - im * sn, re * sn + im * cc], dim=-1)
    else:
        re, im = sel[..., 0::2], sel[..., 1::2]
        new = torch.stack([re * cc - im * sn, re * sn + im * cc], dim=-1).flatten(-2)
    out = v.clone()
    out[:, rows] = new
    return out


def _rms_part(x, weight, eps, wide, normed, rope, cos, sin, rope_rows, rounded, defect):
    """one part ``x [B, n, H, 128]`` -> ``[B, H, n, 128]`` fp64.  rounded: bf16 where the operator rounds (after the normalisation, after
    a bf16 weight product, at the end); an fp32 weight keeps its product unrounded."""
    v = x.double()
    B, n, H, D = v.shape
    rnd = _bf if rounded else (lambda t: t)
    if normed:
        sq = v * v
        if defect == LAST8_OUT:
            (sq[:, :, H - 1, D - 8:] if wide else sq[..., D - 8:]).zero_()
        if defect == LAST_HEAD_OUT:
            sq[:, :, H - 1].zero_()
        use_wide = wide != (defect in (HEAD_FOR_ROW, ROW_FOR_HEAD))
        ss = sq.sum((-2, -1), keepdim=True) if use_wide else sq.sum(-1, keepdim=True)
        if defect == LAST8_TWICE:
            ss = ss + (sq[:, :, H - 1:, D - 8:].sum((-2, -1), keepdim=True) if use_wide else sq[..., D - 8:].sum(-1, keepdim=True))
        div = 512 * ((H + 3) // 4) if defect == DIVISOR else H * D if use_wide else D
        ms = ss / div
        if defect == STATS_ROW:
            ms = torch.roll(ms.reshape(B * n, -1), -1, 0).reshape(ms.shape)
        if defect == STATS_HEAD:
            ms = torch.roll(ms, -1, 2)
        e = eps * {EPS_ABSENT: 0.0, EPS_X10: 10.0}.get(defect, 1.0)
        r = 1.0 / (ms.sqrt() + eps) if defect == EPS_OUTSIDE else 1.0 / (ms + e).sqrt()
        if defect in (SCALE_102, SCALE_101):
            f = 1.02 if defect == SCALE_102 else 1.01
            r = r * _pick(_every_128th(B * n, v.device), f, 1.0).reshape(B, n, 1, 1)
        v = rnd(v * r)
    w = None
    if weight is not None:
        w = weight.double().flatten()
        if defect == W_COL8:
            w = torch.roll(w, -8)
        w = w.reshape(-1, D)
    rot_rows = rope_rows if rope else 0
    if defect == ROT_BEFORE_WEIGHT:
        v = _rotate(v, cos, sin, rot_rows)
    if w is not None:
        v = v * w
        if rounded and weight.dtype == torch.bfloat16:
            v = _bf(v)
    if defect != ROT_BEFORE_WEIGHT:
        v = _rotate(v, cos, sin, rot_rows, defect)
    return rnd(v).permute(0, 2, 1, 3).contiguous()


def rms_head_exact(qkv, q_weight, k_weight, heads, eps=EPS, cos=None, sin=None, rounded=False, defect=None):
    """`qkv_split_norm` by its definition: ``qkv [n, >= 3 * heads * 128]`` -> ``[q, k, v]``, each ``[1, heads, n, 128]`` fp64"""
    n = qkv.shape[0]
    parts = qkv[:, :3 * heads * 128].reshape(1, n, 3, heads, 128)
    r = 0 if cos is None else cos.shape[0]
    ws = [q_weight, q_weight if defect == Q_ON_K else k_weight]
    out = [_rms_part(parts[:, :, p], ws[p], eps, False, True, True, cos, sin, r, rounded, defect) for p in range(2)]
    out.append(_rms_part(parts[:, :, 2], None, eps, False, False, defect == ROT_UNFLAGGED, cos, sin, r, rounded, None))
    return out


def rms_row_exact(x, heads, weights, norm, rope, eps=EPS, cos=None, sin=None, rounded=False, defect=None):
    """`split_heads_rownorm` by its definition: ``x [B, n, >= parts * heads * 128]`` -> per part ``[B, heads, n, 128]`` fp64"""
    parts, C = len(norm), heads * 128
    B, n = x.shape[0], x.shape[1]
    r = 0 if cos is None else cos.shape[0]
    ws = list(weights)[:parts] + [None] * (parts - len(weights))
    if defect == Q_ON_K and parts >= 2 and norm[1]:
        ws[1] = ws[0]
    out = []
    for p in range(parts):
        rp = bool(rope[p]) != (defect == ROT_UNFLAGGED and not rope[p])
        part = x[:, :, p * C:(p + 1) * C].reshape(B, n, heads, 128)
        out.append(_rms_part(part, ws[p], eps, True, bool(norm[p]), rp, cos, sin, r, rounded, defect if norm[p] or rope[p] else None))
    return out


# ------------------------------------------------------------------------------------------------ residual + LayerNorm + modulate
def residual_exact(x, y, gate):
    """fp64 ``x + gate * y`` (``x`` itself without ``y``)"""
    return x.double() if y is None else x.double() + gate.double() * y.double()


def nearest_bf16_violations(got, exact):
    """the number of elements of ``got`` that are not A nearest bf16 of ``exact``: ``|got - e| <= |bf16(e) - e|``"""
    g = got.to(exact.device).double()
    return int((~((g - exact).abs() <= (_bf(exact) - exact).abs())).sum())


def ln_modulate_exact(x, y, gate, shift, scale, eps=EPS, x_out=None, rounded=False, defect=None, with_prod=False):
    """``xm [rows, C]`` fp64 (with_prod: and ``xn * (1 + scale)``, the ingredient of `bound_ln`).  The LayerNorm input is ``x_out`` where given (the bf16 the operator returned for the residual; its own
    check is `nearest_bf16_violations`), else bf16 of the fp64 residual, else ``x``."""
    rnd = _bf if rounded else (lambda t: t)
    if y is None:
        base = x.double()
    elif defect == XM_BEFORE_RESIDUAL:
        base = x.double()
    elif defect == GATE_TWICE:
        base = _bf(x.double() + 2.0 * gate.double() * y.double())
    else:
        base = x_out.double() if x_out is not None else _bf(residual_exact(x, y, gate))
    rows, C = base.shape
    cw = torch.ones(C, dtype=torch.float64, device=base.device)
    if defect == LAST8_OUT:
        cw[C - 8:] = 0.0
    if defect == LAST8_TWICE:
        cw[C - 8:] = 2.0
    div = 512 * ((C + 511) // 512) if defect == DIVISOR else C
    mean = (base * cw).sum(-1, keepdim=True) / div
    cen = base - mean
    var = ((base if defect == NO_MEAN_IN_VAR else cen).pow(2) * cw).sum(-1, keepdim=True) / ((C - 1) if defect == UNBIASED else div)
    if defect == STATS_ROW:
        mean, var = torch.roll(mean, -1, 0), torch.roll(var, -1, 0)
        cen = base - mean
    e = eps * {EPS_ABSENT: 0.0, EPS_X10: 10.0}.get(defect, 1.0)
    rstd = 1.0 / (var.sqrt() + eps) if defect == EPS_OUTSIDE else 1.0 / (var + e).sqrt()
    if defect in (SCALE_102, SCALE_101):
        rstd = rstd * _pick(_every_128th(rows, base.device), 1.02 if defect == SCALE_102 else 1.01, 1.0)[:, None]
    xn = rnd(cen * rstd)
    one = (1 + scale).double()                                  # the bf16 tensor of the reference: an input rounding
    sh = shift.double()
    if defect == SCALE_FOR_ONE:
        one = scale.double()
    if defect == SHIFT_SCALE_SWAPPED:
        sh, one = scale.double(), (1 + shift).double()
    return (rnd(sh + xn * one), xn * one) if with_prod else rnd(sh + xn * one)


# ------------------------------------------------------------------------------------------------ input families
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _randn(shape, g):
    return torch.randn(*shape, generator=g, device=g.device)


def ladder_scale(rows, device="cpu"):
    """row r scaled by 2^((5 r) mod 21 - 12): neighbours differ by 2^5 or more; 2^-12 .. 2^8"""
    return torch.pow(2.0, ((5 * torch.arange(rows, device=device)) % 21 - 12).double()).float()


def head_ladder_scale(rows, heads, device="cpu"):
    """head h of row r scaled by 2^((3 ((h + r) mod H)) mod 11 - 5): ``[rows, heads]``; the heaviest head rotates with the row"""
    hh = (torch.arange(heads, device=device)[None, :] + torch.arange(rows, device=device)[:, None]) % heads
    return torch.pow(2.0, ((3 * hh) % 11 - 5).double()).float()


def special_rows(rows, kinds, sweep=None):
    """row number -> kind index: kind i at rows 5 + i, 64 + i, `sweep` + 3 + i (a row of the grid's second sweep) and rows - 1 - i (the
    tensor's last rows; the very last is kind 0, the all-zero row).  Later entries win."""
    out = {}
    for i in range(kinds):
        for r in (5 + i, 64 + i) + (() if sweep is None else (sweep + 3 + i,)):
            if 0 <= r < rows:
                out[r] = i
    for i in reversed(range(kinds)):
        if rows - 1 - i >= 0:
            out[rows - 1 - i] = i
    return out


def rms_inputs(family, B, n, heads, parts, extra, seed, wide, sweep=None, device="cpu"):
    """``x [B, n, parts * heads * 128 + extra]`` bf16.  special: 0 all-zero row, 1 only column 0 of every part non-zero, 2 only the
    last column of every part (and of its last head); the one value is about sqrt(C eps), so that the row's mean square is eps."""
    g = _gen(seed, device)
    R, C = B * n, heads * 128
    t = _randn((R, parts, heads, 128), g) * 1.7
    tail = _randn((R, extra), g) * 1.7
    if family == "ladder":
        t = t * ladder_scale(R, device)[:, None, None, None]
    elif family == "head_ladder":
        t = t * head_ladder_scale(R, heads, device)[:, None, :, None]
    elif family == "special":
        v = float(torch.tensor(math.sqrt((C if wide else 128) * EPS)).to(torch.bfloat16))
        for r, kind in special_rows(R, 3, sweep).items():
            t[r] = 0.0
            if kind == 1:
                t[r, :, 0, 0] = v
            if kind == 2:
                t[r, :, heads - 1, 127] = -v
    else:
        assert family == "iid", family
    return torch.cat([t.reshape(R, parts * C), tail], dim=1).to(torch.bfloat16).reshape(B, n, parts * C + extra)


def rms_weight(C, dtype, seed, device="cpu"):
    return (1 + 0.1 * _randn((C,), _gen(seed, device))).to(dtype)


def rope_tables(rope_rows, seed, device="cpu"):
    """(cos, sin) fp32 ``[rope_rows, 128]``, both entries of a pair carrying its angle; random angles, row 1 of angle 0 and row 2 of
    pi / 2 (a table of one or two rows: its last row pi / 2)"""
    if not rope_rows:
        return None, None
    ang = torch.rand(rope_rows, 64, generator=_gen(seed, device), device=device, dtype=torch.float64) * 6.28
    if rope_rows >= 3:
        ang[1], ang[2] = 0.0, math.pi / 2
    else:
        ang[rope_rows - 1] = math.pi / 2
    return (ang.cos().float().repeat_interleave(2, dim=1).contiguous(), ang.sin().float().repeat_interleave(2, dim=1).contiguous())


def rope_row_choices(n):
    """{0, 1, n, a value not divisible by 4}"""
    odd = next((r for r in range(n - 1, 0, -1) if r % 4), None)
    return sorted({0, 1, n} | ({odd} if odd else set()))


def ln_inputs(family, rows, C, residual, seed, sweep=None, device="cpu"):
    """x, y, gate, shift, scale (bf16; y and gate None without the residual).  special: 0 all-zero row, 1 / 2 only column 0 / the last
    column non-zero (about sqrt(C eps): a variance of eps), 3 a constant row 3.0, 4 a row of mean 100 and sd 4; y is 0 on those rows."""
    g = _gen(seed, device)
    x = _randn((rows, C), g) * 2.0 + 0.3
    y = _randn((rows, C), g)
    gate, shift, scale = 0.5 * _randn((C,), g), 0.2 * _randn((C,), g), 0.2 * _randn((C,), g)
    if family == "ladder":
        s = ladder_scale(rows, device)[:, None]
        x, y = x * s, y * s
    elif family == "special":
        v = float(torch.tensor(math.sqrt(C * EPS)).to(torch.bfloat16))
        for r, kind in special_rows(rows, 5, sweep).items():
            y[r] = 0.0
            if kind < 3:
                x[r] = 0.0
                if kind == 1:
                    x[r, 0] = v
                if kind == 2:
                    x[r, C - 1] = -v
            elif kind == 3:
                x[r] = 3.0
            else:
                x[r] = 100.0 + 2.0 * (x[r] - 0.3)
    else:
        assert family == "iid", family
    b = lambda t: t.to(torch.bfloat16)      # noqa: E731
    return b(x), (b(y) if residual else None), (b(gate) if residual else None), b(shift), b(scale)


# ------------------------------------------------------------------------------------------------ cases
QKV_SHAPES = [(1, 1, 0), (37, 3, 64), (1200, 4, 0), (3700, 24, 0)]          # (n, heads, extra); the last: 266 400 segments > one sweep of 262 144
QKV_SWEEP_TOKENS = 262144 // (3 * 24)                                        # the first token of the capped grid's second sweep at 24 heads
WIDE_HEADS = [1, 2, 5, 7, 12, 13, 33, 40, 41, 61, 64]                         # NV 1, 1, 2, 2, 3, 4, 9, 10, 11, 16, 16; HELD up to NV 10
WIDE_WEIGHTS = {"none": [None] * 3, "bf16": [torch.bfloat16] * 3, "fp32": [torch.float32] * 3, "mixed": [torch.float32, torch.bfloat16, None]}
LN_COLS = [8, 520, 1032, 2568, 3080, 5128, 3072, 8192]                       # a vector past the row at all but the last two
LN_ROWS = 70


def wide_flags(parts, rope_rows):
    """the flags of tests/test_gpu_wan_glue.py: the last part of a two- or three-part row is copied, the others normalised and, with a table, rotated"""
    norm = [True] if parts == 1 else [p < parts - 1 for p in range(parts)]
    return norm, [nm and rope_rows > 0 for nm in norm]


def wide_weights(kind, norm, C, seed, device="cpu"):
    kinds = WIDE_WEIGHTS[kind]
    return [rms_weight(C, kinds[p], seed + p, device) if norm[p] and kinds[p] is not None else None for p in range(len(norm))]
