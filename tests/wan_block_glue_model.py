"""Wan's block glue (`ops.residual_ln_modulate_f32`, csrc/rowwise.hip `residual_ln_modulate_f32_kernel`) by its definition, in fp64 and
plain torch (no chipmunk operator: CPU or device tensors alike), the seeded input families of tests/rowwise_model.py with vectors that
differ between the sequences of a batch, and the mutants -- the exact result with one defect, rounded where the operator rounds -- that
the segment bound must reject.  tests/test_wan_block_glue_cpu.py pins the constants below on the CPU path (the reference's torch
sequence); tests/test_gpu_wan_block_glue.py asserts them on the device.  docs/TEST_SENSITIVITY.md, "Wan block glue".

Definition (reference examples/wan/wan/modules/model.py:100-110, 317-334; include/chipmunk_hip.h):

* ``x_out = fp32(fp32(x) + fp32(fp32(y) * gate))``, ``fp32(x) + fp32(y)`` without a gate, ``x`` itself without ``y``.  This is a
  condition on bits (`residual_f32` is torch's fp32 formula), not a tolerance; the LayerNorm below takes ``x_out`` as the input it is.
* ``xn = (x_out - mean) / sqrt(var + eps)`` over the columns, biased variance.
* ``xm = xn * (1 + scale) + shift`` with the sequence's vectors, or ``xn * weight + bias``; rounded ONCE, to bf16.  Only for a bf16 ``x``
  without ``y`` and with a modulation ``xn`` is rounded to bf16 before (WanLayerNorm's ``.type_as``): the class with two roundings."""
import math

import torch

import rowwise_model as rm

EPS = rm.EPS
SEG_W = rm.SEG_W               # the metric's segment: 128 consecutive columns of xm, the last one short
MARGIN = rm.MARGIN             # what a correct kernel may do differently: the order of the sums, one fma for fp32's two roundings

# ---- floors: the worst full segment of the CPU path against fp64 over every case of tests/test_wan_block_glue_cpu.py (which pins them:
# test_floor_constants_are_tight), rounded up.  One bf16 rounding is 2^-8 / sqrt(3) = 0.0023 rms of a segment.
FLOOR = {"one": 0.0025, "two": 0.0034}          # roundings on an element's path: bf16(xm) | bf16(xn), bf16(xm)


def rounding_class(x, y, affine):
    return "two" if x.dtype == torch.bfloat16 and y is None and not affine else "one"


def bound(cls, exact, prod):
    """(bound per segment of ``xm``, few-element mask).  A segment of a handful of elements (`rowwise_model.few_element_segments`: the 8
    columns behind a multiple of 128, a row of C = 8, the one large element of a one-hot row) has no average over 128 roundings: its
    bound is the worst case of the roundings on its path, ``2^-8`` for the last one and, in the class with two, ``2^-8 ||xn * mult|| /
    ||xm||`` for the rounding of ``xn`` that the multiplication carries (prod: the exact ``xn * mult``); `rowwise_model.HARD_SLACK` covers
    the fp32 statistics and evaluation.  Every other segment: ``MARGIN * FLOOR[cls]``."""
    few = rm.few_element_segments(exact, SEG_W)
    den = rm._segs(exact, SEG_W).norm(dim=-1)
    carried = rm._segs(prod, SEG_W).norm(dim=-1) / den.clamp_min(1e-300) if cls == "two" else torch.zeros_like(den)
    hard = rm.HARD_SLACK * rm.BF16_EPS * (1.0 + carried)
    return torch.where(few, hard, torch.full_like(hard, MARGIN * FLOOR[cls])), few


# ------------------------------------------------------------------------------------------------ defects
SEQ0, SEQ_NEXT = "sequence 0's vectors for every sequence", "vectors of sequence b + 1"
GATE_ON_X, SCALE_FOR_ONE, SHIFT_SCALE_SWAPPED = "gate applied to x", "scale where 1 + scale is meant", "shift and scale exchanged"
EPS_ABSENT, STATS_FROM_X, BIAS_DROPPED = "eps absent", "statistics of x instead of x_out", "bias dropped"
BF16_POINTS = "residual_ln_modulate's bf16 rounding points on a bf16-rounded stream"
BF16_ONE_PLUS_SCALE, UNBIASED, XN_ROUNDED = "bf16(1 + scale) alone", "unbiased variance (C - 1)", "xn rounded to bf16 where it is not"
NO_DEFECT = "no defect"

DEFECTS = (SEQ0, SEQ_NEXT, GATE_ON_X, SCALE_FOR_ONE, SHIFT_SCALE_SWAPPED, EPS_ABSENT, STATS_FROM_X, BIAS_DROPPED, BF16_POINTS)
RECORDED = (BF16_ONE_PLUS_SCALE, UNBIASED, XN_ROUNDED)          # cannot clear 2 x the bound everywhere: printed, never counted
ALL = ("iid", "ladder", "special")
# defect -> the families it is counted on.  eps: only rows whose variance is near eps see it.  The bf16 stream: only a row whose mean is
# large against its spread (the mean-100 row: bf16 keeps 100 to 0.25, a sixteenth of the row's standard deviation) -- on rows of mean 0.3
# and sd 2 three more roundings add 0.004 in all, under twice the bound: recorded there.
FAMILIES = {d: ALL for d in DEFECTS}
FAMILIES.update({EPS_ABSENT: ("ladder", "special"), BF16_POINTS: ("special",)})


def applies(d, t):
    """whether defect `d` can touch the case of inputs `t` (`glue_inputs`) at all; where it cannot, the mutant is the undamaged result
    bit for bit"""
    x, y, gate, affine = t["x"], t["y"], t["gate"], t["weight"] is not None
    if d in (SEQ0, SEQ_NEXT):                                        # one vector for all, or one sequence: nothing to confuse
        return any(v is not None and v.dim() > 1 and v.shape[0] > 1 for v in (gate, t["shift"], t["scale"]))
    if d == GATE_ON_X:
        return y is not None and gate is not None
    if d == STATS_FROM_X:
        return y is not None
    if d in (SCALE_FOR_ONE, SHIFT_SCALE_SWAPPED, BF16_ONE_PLUS_SCALE):
        return not affine
    if d == BIAS_DROPPED:
        return affine
    if d == XN_ROUNDED:
        return rounding_class(x, y, affine) == "one"
    return True


def counted(d, t, family):
    """whether defect `d` must be at twice the bound or more on the case of inputs `t` of `family`.  The bf16 rounding points are counted
    where the stream is not bf16 already: a bf16 x without y IS the bf16 stream, and what is left (bf16 vectors, bf16(1 + scale)) is recorded"""
    if d == BF16_POINTS and not (t["x"].dtype == torch.float32 or t["y"] is not None):
        return False
    return d in DEFECTS and family in FAMILIES[d] and applies(d, t)


def _bf(t):
    return t.to(torch.bfloat16).double()


def _seq(v, B, C):
    """a per-sequence vector ``[C]``, ``[B, C]`` or ``[B, 1, C]`` as fp64 ``[B, 1, C]``"""
    return v.double().reshape(-1, 1, C).expand(B, 1, C)


# ------------------------------------------------------------------------------------------------ the operator
def residual_f32(x, y, gate):
    """``x_out`` by torch's fp32 formula (model.py:327, 331, 334): ``[B, L, C]`` fp32, ``None`` without ``y``"""
    if y is None:
        return None
    B, C = x.shape[0], x.shape[-1]
    return x.float() + (y.float() if gate is None else y.float() * gate.float().reshape(-1, 1, C).expand(B, 1, C))


def glue_exact(x, y, gate, shift, scale, weight, bias, eps=EPS, x_out=None, rounded=False, defect=None, with_prod=False):
    """``xm [B, L, C]`` fp64 (with_prod: and ``xn * mult``, the ingredient of `bound`).  The LayerNorm input is ``x_out`` where given (the
    fp32 tensor the operator returned, checked bit for bit on its own), else `residual_f32`, else ``x``.  rounded: bf16 where the operator
    rounds."""
    B, L, C = x.shape
    affine = weight is not None
    rnd = _bf if rounded else (lambda t: t)
    two = rounded and rounding_class(x, y, affine) == "two"
    pick = lambda v: None if v is None else _seq(v, B, C)      # noqa: E731
    g, sh, sc = pick(gate), pick(shift), pick(scale)
    if defect == SEQ0:
        g, sh, sc = [None if v is None else v[:1].expand(B, 1, C) for v in (g, sh, sc)]
    if defect == SEQ_NEXT:
        g, sh, sc = [None if v is None else torch.roll(v, -1, 0) for v in (g, sh, sc)]
    xd = x.double()
    if y is None:
        base = xd
    elif defect == GATE_ON_X and g is not None:
        base = (x.float() * g.float() + y.float()).double()
    elif defect in (SEQ0, SEQ_NEXT) and g is not None:
        base = (x.float() + y.float() * g.float()).double()                  # fp32 as `residual_f32`: bit-inert where the vectors are shared
    elif defect == BF16_POINTS:
        base = _bf(_bf(xd) + (y.double() if g is None else _bf(g) * y.double()))
    else:
        base = (x_out if x_out is not None else residual_f32(x, y, gate)).double()
    if defect == BF16_POINTS and y is None:
        base = _bf(xd)
    stat = xd if (defect == STATS_FROM_X and y is not None) else base
    mean = stat.mean(-1, keepdim=True)
    var = (stat - mean).pow(2).sum(-1, keepdim=True) / ((C - 1) if defect == UNBIASED else C)
    rstd = 1.0 / (var + (0.0 if defect == EPS_ABSENT else eps)).sqrt()
    xn = (base - mean) * rstd
    if two or (rounded and defect in (BF16_POINTS, XN_ROUNDED)):
        xn = _bf(xn)
    if affine:
        mult, add = weight.double(), bias.double()
        if defect == BIAS_DROPPED:
            add = torch.zeros_like(add)
        if defect == BF16_POINTS:
            mult, add = _bf(mult), _bf(add)
    else:
        mult, add = 1.0 + sc, sh
        if defect == SCALE_FOR_ONE:
            mult = sc
        if defect == SHIFT_SCALE_SWAPPED:
            mult, add = 1.0 + sh, sc
        if defect == BF16_POINTS:
            mult, add = _bf(1.0 + _bf(sc)), _bf(sh)
        if defect == BF16_ONE_PLUS_SCALE:
            mult = _bf(mult)
    prod = xn * mult
    out = rnd(prod + add)
    return (out, prod) if with_prod else out


# ------------------------------------------------------------------------------------------------ inputs
RESIDUALS = ("none", "gated", "ungated")
MODS = ("vec", "seq", "affine")           # modulation [C] | modulation [B, C] (gate [B, 1, C]) | affine weight / bias


def refused(xdtype, residual):
    return xdtype == torch.bfloat16 and residual == "ungated"


def glue_inputs(family, B, L, C, xdtype, residual, mod, seed, sweep=None, device="cpu"):
    """dict(x, y, gate, shift, scale, weight, bias).  ``x [B, L, C]`` of `xdtype`; ``y`` bf16 or None; vectors fp32, of order 1, drawn
    independently per sequence (``mod == "vec"``: one ``[C]`` vector for all).  Families as `rowwise_model.ln_inputs`: iid rows (mean 0.3,
    sd 2); ladder: row r scaled by 2^((5 r) mod 21 - 12); special: 0 all-zero row, 1 / 2 only column 0 / the last column non-zero (about
    sqrt(C eps): a variance of eps), 3 a constant row 3.0 -- y is 0 on those --, 4 a row of mean 100 and sd 4 (y kept)."""
    g = rm._gen(seed, device)
    rows = B * L
    x = rm._randn((rows, C), g) * 2.0 + 0.3
    y = rm._randn((rows, C), g)
    gate, shift, scale = rm._randn((B, 1, C), g), rm._randn((B, C), g), 0.5 * rm._randn((B, C), g)
    weight, bias = 1.0 + 0.3 * rm._randn((C,), g), rm._randn((C,), g)
    if family == "ladder":
        s = rm.ladder_scale(rows, device)[:, None]
        x, y = x * s, y * s
    elif family == "special":
        v = float(torch.tensor(math.sqrt(C * EPS)).to(torch.bfloat16))
        for r, kind in rm.special_rows(rows, 5, sweep).items():
            if kind < 4:
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
    out = dict(x=x.to(xdtype).reshape(B, L, C).contiguous(), y=None, gate=None, shift=None, scale=None, weight=None, bias=None)
    if residual != "none":
        out["y"] = y.to(torch.bfloat16).reshape(B, L, C).contiguous()
        if residual == "gated":
            out["gate"] = gate if mod != "vec" else gate[0, 0].contiguous()
    if mod == "affine":
        out["weight"], out["bias"] = weight, bias
    elif mod == "seq":
        out["shift"], out["scale"] = shift, scale
    else:
        out["shift"], out["scale"] = shift[0].contiguous(), scale[0].contiguous()
    return out


# ------------------------------------------------------------------------------------------------ cases
COLS = [8, 520, 1032, 1536, 2568, 5120, 5128, 8192]     # NV 1, 2, 3, 3, 6, 10, 11, 16 on the classes 2, 3, 6, 10, 16: vectors held up to 6
BATCH, SEQ_LEN = 2, 35                                  # 70 rows; a wave's row walk crosses the sequence boundary off a multiple of four
SWEEP_CASE = (3, 2800, 520)                             # 8 400 rows over the capped grid's 8 192 waves
