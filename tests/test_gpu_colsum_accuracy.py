"""The column sums of dense_colsum_attn and the fused mask step against plain fp64 (helpers.colsum_exact), element by element.

``cs[b, h, g, j] = sum_{i in group g} exp(s_ij) p_i`` decides which keys every sparse step keeps.  It is a sum of positive terms, so
each element is held to a RELATIVE bound that is read off the source (tests/colsum_model.py):

    |cs - x| / x  <=  rounds[g] * 2^-8 + FP32_TERM          rounds[g] = 1 or 2 partial rows (fused routes), 1 (one wave / one block per group)

The two routes that round ``q * SCALE_LOG2E`` to bf16 before the scores (colsum64_kernel: "two_pass"; attn.hip's CSONLY pass: "general")
are held to that bound against fp64 over the folded q -- the exact effect of that documented rounding -- and to the bound plus the pinned
FOLD_TERM against plain fp64.  Beside the element bound: the (group, 64-key tile) segment error under twice the mirrors' floor, ``l``
under 4 x an fp32 mirror's error, and with p = the call's own normaliser every group's sums add up to its row count.
tests/test_colsum_metric_cpu.py pins every constant and proves that the bound rejects 1 % defects; docs/TEST_SENSITIVITY.md, "Column
sums", has the measured figures.

Columns at and past Nk of the ``[B, H, G, max(Nq, Nk)]`` tensor when Nq > Nk: include/chipmunk_hip.h promises nothing for them ("columns
j >= Nk are left untouched", and the tensor is uninitialised), so nothing is asserted."""
import contextlib
import functools
import os

import pytest
import torch

import colsum_model as cm
from helpers import BF16_EPS, assert_colsums_close, colsum_exact

pytestmark = pytest.mark.gpu

ROUTES = {
    "general": dict(attn_dense64=2, attn_colsum64=2),
    "two_pass": dict(attn_dense64=1, attn_colsum64=1, attn_fused_colsum=2),
    "fused": dict(attn_dense64=1, attn_colsum64=1),
    "fused_weighted": dict(attn_dense64=1, attn_colsum64=1, attn_fused_colsum=3),
    "fused_runmax": dict(attn_dense64=1, attn_colsum64=1, attn_nomax=2),
    "fused_per_head": dict(attn_dense64=1, attn_colsum64=1, attn_fused_colsum=4),
}
LONG = "448x33000"          # one head, the routes that take long launches (the 64-row kernels)
MATRIX = [(r, s) for s in cm.SHAPES for r in ROUTES if s != LONG or r != "general"]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def options(**kw):
    from chipmunk_amd import _native
    try:
        for name, value in kw.items():
            _native.set_option(name, value)
        yield
    finally:
        for name in kw:
            _native.set_option(name, 0)


def _on_device(c):
    """the problem's tensors on the GPU plus its fp64 references, built once: x (plain), lx; xf (folded q) on first use"""
    dev = torch.device("cuda:0")
    c = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    c["x"] = colsum_exact(c["q"], c["k"], c["p"], c["k_lens"])
    c["lx"] = cm.l_exact(c["q"], c["k"], c["k_lens"])
    return c


def _folded(c):
    if "xf" not in c:
        c["xf"] = colsum_exact(cm.fold_q(c["q"]), c["k"], c["p"], c["k_lens"], scale_mul=cm.FOLD_SCALE_MUL)
    return c["xf"]


@functools.lru_cache(maxsize=None)
def _problem(shape, regime):
    return _on_device(cm.problem(shape, regime))


@functools.lru_cache(maxsize=None)
def _degenerate():
    return _on_device(cm.degenerate_problem())


@functools.lru_cache(maxsize=None)
def _klens(kind, which):
    return _on_device(cm.klens_problem(kind, which))


def _log(line):
    path = os.environ.get("CHIPMUNK_ROW_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check(route, c, cs, l, what, l_guard=True):
    nq, nk, regime = c["nq"], c["nk"], c["regime"]
    B, H = c["q"].shape[:2]
    G = (nq + 191) // 192
    assert cs.dtype == torch.bfloat16 and cs.shape[:3] == (B, H, G) and cs.shape[3] >= nk, cs.shape
    cs = cs[..., :nk]
    rounds = cm.rounds(route, nq)
    fp32, extra = cm.elem_terms(route, regime)
    assert_colsums_close(cs, c["x"], rounds, extra, f"{route}, {what}", fp32, cm.seg_bound(route, nq, regime))
    if cm.folds(route):
        assert_colsums_close(cs, _folded(c), rounds, None, f"{route}, folded reference, {what}", fp32, cm.seg_bound(route, nq, regime, True))
    if c["k_lens"] is not None:
        for b, L in enumerate(c["k_lens"]):
            assert not cs[b, :, :, L:].float().any(), f"{route}, {what}: column sums past k_lens[{b}] = {L} are not exactly 0"
    if regime == "own l":
        # p = the call's own normaliser: a group's sums add up to its row count, within rounds[g] * 2^-8 (each column is, and the terms
        # are positive; the fold's and the fp32 part's errors average out over the columns: measured 0.0007 at most)
        rows = torch.tensor([min(192, nq - g * 192) for g in range(G)], dtype=torch.float64, device=cs.device)
        bound = torch.tensor(rounds, dtype=torch.float64, device=cs.device) * BF16_EPS
        off = (cs.double().sum(-1) - rows).abs() / rows
        print(f"{route}, {what}: group totals off their row counts by {float(off.max()):.5f} at most")
        assert (off <= bound).all(), f"{route}, {what}: a group's column sums add up to its row count +- {float(off.max()):.5f}"
    # l: relative error against fp64 under L_MARGIN x the fp32 mirror's
    lerr = float(((l[..., :nq, 0].double() - c["lx"]).abs() / c["lx"]).max())
    print(f"{route}, {what}: l worst relative error {lerr:.3g} (bound {cm.L_MARGIN * cm.L_FP32_ERR:.3g})")
    _log(f"l {route}, {what}\t{lerr:.3g}\t{cm.L_MARGIN * cm.L_FP32_ERR:.3g}")
    if l_guard:
        assert lerr <= cm.L_MARGIN * cm.L_FP32_ERR, f"{route}, {what}: l off by {lerr:.3g} (relative)"
    torch.testing.assert_close(l[..., :nq, 0].double(), c["lx"], rtol=1e-3, atol=0)


@pytest.mark.parametrize("regime", cm.REGIMES)
@pytest.mark.parametrize("route,shape", MATRIX)
def test_column_sums(dev, route, shape, regime):
    c = _problem(shape, regime)
    with options(**ROUTES[route]):
        o, cs, l = torch.ops.chipmunk.dense_colsum_attn(c["q"], c["k"], c["v"], c["p"])
    _check(route, c, cs, l, f"{shape}, {regime}")


@pytest.mark.parametrize("route", list(ROUTES))
def test_column_sums_batched_token_major_degenerate_p(dev, route):
    """B = 2 on [B, N, H, D] storage; rows 5::7 have p = 0 and add exactly nothing (the reference leaves them out: were they counted,
    a seventh of every sum would be wrong), rows 3::11 have p x 1e6 and carry the sums"""
    c = _degenerate()
    assert c["q"].stride(1) == 128 and not c["q"].is_contiguous()
    with options(**ROUTES[route]):
        o, cs, l = torch.ops.chipmunk.dense_colsum_attn(c["q"], c["k"], c["v"], c["p"])
    _check(route, c, cs, l, "640x640 batched, degenerate p")


KLENS_RUNS = ([("general", "general", w, nan) for w in (0, 1) for nan in (False, True)] +
              [(r, "wave64", 0, nan) for r in ("fused", "two_pass", "fused_weighted") for nan in (False, True)] +
              [(r, "wave64", 1, False) for r in ("fused", "two_pass", "fused_weighted")])      # sub-tile lengths: finite padding (chipmunk_hip.h)


@pytest.mark.parametrize("route,kind,which,nan_padding", KLENS_RUNS)
def test_column_sums_with_key_lengths(dev, route, kind, which, nan_padding):
    """the length sets of tests/test_gpu_attn_klens.py: valid columns under the element bound, columns past the length exactly 0, NaN in
    the padding wherever that file allows it"""
    from chipmunk_amd import ops
    c = _klens(kind, which)
    k, v = c["k"], c["v"]
    if nan_padding:
        k, v = k.clone(), v.clone()
        for b, L in enumerate(c["k_lens"]):
            k[b, :, L:] = float("nan")
            v[b, :, L:] = float("nan")
    kl = torch.tensor(c["k_lens"], dtype=torch.int32, device=dev)
    with options(**ROUTES[route]):
        o, cs, l = ops.dense_colsum_attn(c["q"], k, v, c["p"], False, kl)
    assert torch.isfinite(cs.float()).all()
    _check(route, c, cs, l, f"k_lens {c['k_lens']}, NaN padding {nan_padding}")


@pytest.mark.parametrize("shape,k_top", [("1000x1000", 128), (LONG, 2048)])
def test_mask_step_without_cs_against_exact_column_sums(dev, shape, k_top):
    """`ops.dense_colsum_topk_mask` (random part 0, no static mask, all groups on) against `colsum_exact`, not against another kernel.

    The kernel selects the k_top largest of its own sums c~, each within delta of the exact x: ``c~ = x (1 + e)``, ``|e| <= delta`` (the
    asserted element bound of the fused route, per group).  (1) For a selected column s and an unselected u, ``c~_s >= c~_u``, hence
    ``x_s (1 + delta) >= x_u (1 - delta)``: no unselected column exceeds the smallest selected one by more than
    ``(1 + delta) / (1 - delta)``.  (2) For the selected set S and the exact top-k set T:
    ``sum_S x >= sum_S c~ / (1 + delta) >= sum_T c~ / (1 + delta) >= sum_T x (1 - delta) / (1 + delta) >= (1 - 2 delta) sum_T x``
    (and ``sum_S x <= sum_T x`` by definition): the selected mass is within 2 delta of the exact top-k mass."""
    from chipmunk_amd import ops
    c = _problem(shape, "previous step")
    with options(**ROUTES["fused"]):
        o, mask, l = ops.dense_colsum_topk_mask(c["q"], c["k"], c["v"], c["p"], k_top, 0.0, None, None)
    x = c["x"]
    assert mask.shape == x.shape and mask.dtype == torch.bool
    assert (mask.sum(-1) == k_top).all(), "exactly k_top columns per row"
    delta = torch.tensor(cm.elem_bound("fused", c["nq"]), dtype=torch.float64, device=x.device).view(1, 1, -1)
    inf = torch.full_like(x, float("inf"))
    smallest_kept = torch.where(mask, x, inf).min(-1).values
    largest_left = torch.where(mask, -inf, x).max(-1).values
    ratio = largest_left / smallest_kept
    top = x.topk(k_top, dim=-1).values.sum(-1)
    short = 1.0 - torch.where(mask, x, torch.zeros_like(x)).sum(-1) / top
    print(f"mask step {shape}: largest unselected / smallest selected {float(ratio.max()):.5f} (allowed {float(((1 + delta) / (1 - delta)).max()):.5f}), "
          f"mass short of the exact top-{k_top} by {float(short.max()):.2e} (allowed {float(2 * delta.max()):.4f})")
    _log(f"mask step {shape}\t{float(ratio.max()):.6f}\t{float(((1 + delta) / (1 - delta)).max()):.6f}\t{float(short.max()):.3g}")
    assert (ratio <= (1 + delta) / (1 - delta)).all(), f"an unselected column is {float(ratio.max()):.4f} x the smallest selected one"
    # (-1e-12: the two fp64 sums add the same values in another order)
    assert (short >= -1e-12).all() and (short <= 2 * delta).all(), f"selected mass {float(short.max()):.4g} short of the exact top-k mass"
    lerr = float(((l[..., :c["nq"], 0].double() - c["lx"]).abs() / c["lx"]).max())
    assert lerr <= cm.L_MARGIN * cm.L_FP32_ERR, lerr
