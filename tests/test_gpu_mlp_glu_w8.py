"""``csp_mlp_mm1_glu_w8`` -- the gated GEMM1 over e4m3 gate / up weights with bf16 activations ("Gated weight-only GEMM1") --
on the GPU.

(a) Bits against the bf16 gated kernel.  With power-of-two scales (one number, or one per weight row; gate and up different) and no biases
    the packed deltas and the updated cache are ``csp_mlp_mm1_glu``'s on the two widened weights, bit for bit, sentinels and padding
    included: the lane / byte / k mapping of the widened fragments and which weight a DMA piece gathers from are conditions, not
    tolerances.  The weights hold every finite e4m3 byte.  K = 64 (one k step, shorter than the ring), 192 (odd against the ring depth of
    3) and 1536; M = 40, 128 and 1003 (last group of 107 rows); F = 1024; counts 0, 1, 32, 33, 64, 65, 1000 and 1024 mixed in one call (the
    gated tile is 64 packed columns: 32 / 33 and 64 / 65 are its edges); the three activations; update_cache 0 / 1; a batch of two; both
    cache layouts; two separate weights, and the halves of one ``[2F, K]`` tensor in both orders.
(b) Bits against the ungated weight-only kernel.  ``w_up`` all zero bytes with ``bias_up = 1`` makes u exactly 1.0 and
    ``fma(act(g), 1, -c)`` round as ``act(g) - c``: with general scales (no powers of two) and a gate bias the result is the BITS of
    ``csp_mlp_mm1_w8`` with the gate's weight, scale and bias -- the gate branch's scale gather, bias order and epilogue, no tolerance.
    tanh-GELU only, and the reason lies in the UNGATED kernel: its epilogue is ``act(h) - c`` in C++, and tanh-GELU ends in an fma of its own
    (``fma(-x, r, x)``), so ``act(h)`` is a rounded fp32 number before the subtraction -- the premise of the comparison.  SiLU (``x * r``)
    and the exact GELU (``(0.5 x) * (erf + 1)``) end in a multiplication, which hipcc's default contraction may fuse with the subtraction
    into ``fma(x, r, -c)``: the ungated kernel then never rounds ``act(h)`` on its own, while the gated form must (``d = fma(act(g), u,
    -c)`` has act(g) as an operand).  Observed on an MI355X: with SiLU the two kernels' packed deltas differ (K 192, per-row scales,
    column-major, update off); with tanh-GELU they are bit-equal.  SiLU and the exact GELU are covered by (a), bit for bit against the
    bf16 gated kernel, and by (c).
(c) With biases on both branches and general scales every 64-column segment of every row of the deltas and of the refreshed cache columns
    is held against the fp64 definition (tests/mlp_glu_w8_model.py) under helpers.MLP_SEG_BOUND, the bound tests/test_gpu_mlp_accuracy.py
    holds the bf16 gated form to: the same arithmetic class plus one fp32 multiply per branch (2^-24 relative).  No new constant.
    tests/test_mlp_glu_w8_host.py proves the metric against six mutants.
(d) A zero bias vector gives the bits of no bias, a constant scale vector those of the number, the fused scatter those of the unfused
    sequence, a batch those of its slices, a second run those of the first; nothing at or past M, at or past a count, in the cache's
    padding or in a column that was not selected is written."""
import functools

import pytest
import torch

from helpers import MLP_BM, MLP_SEG_BOUND, MLP_SEG_W1, assert_segs_close, gathered_cache, refreshed_cache_term
from mlp_glu_w8_model import mm1_glu_w8_exact
from mlp_w8_model import E4M3, every_byte_weight

pytestmark = pytest.mark.gpu

SENT = 7.0
F = 1024
ACTS = ("gelu_tanh", "silu", "gelu")
COUNTS = {40: [[33]], 128: [[1000]], 1003: [[0, 1, 32, 33, 64, 65, 1000, 1024], [1024, 65, 0, 1000, 1, 33, 64, 520]]}
SOURCES = ("two weights", "fused, gate first", "fused, up first")


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def problem(M, K, B):
    """inputs on the device: a [B, M, K] bf16, two every-byte e4m3 weights (and the two as halves of one [2F, K] tensor), a random cache
    [B, F, M], one index permutation per group, power-of-two scales"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * M + K)
    G = (M + MLP_BM - 1) // MLP_BM
    counts = COUNTS[M][:B]
    assert len(counts) == B and all(len(c) == G for c in counts)
    p = dict(M=M, K=K, B=B, F=F, G=G, ldc=(M + 7) // 8 * 8)
    p["a"] = (torch.randn(B, M, K, generator=g) * 0.25).to(torch.bfloat16).to(dev)
    p["wg"], p["wu"] = every_byte_weight(F, K, seed=M + K).to(dev), every_byte_weight(F, K, seed=M + K + 1).to(dev)
    p["fused"] = torch.cat([p["wg"].view(torch.uint8), p["wu"].view(torch.uint8)]).view(E4M3)       # [2F, K]: gate first
    p["cache0"] = (torch.randn(B, F, M, generator=g) * 0.3).to(torch.bfloat16).to(dev)
    p["bg"] = (torch.randn(F, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    p["bu"] = (torch.randn(F, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    p["inds"] = torch.stack([torch.stack([torch.randperm(F, generator=g) for _ in range(G)]) for _ in range(B)]).to(torch.int32).to(dev)
    p["cnt"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    p["cols"] = p["cnt"].long().repeat_interleave(MLP_BM, dim=1)[:, :M]                  # [B, M]: the live columns of every row
    # power-of-two reciprocal scales, gate and up different: |w| <= 448 -> <= 0.44 and below
    p["s1"] = (torch.tensor([2.0 ** -10], device=dev), torch.tensor([2.0 ** -11], device=dev))
    p["sv"] = tuple(torch.ldexp(torch.ones(F), -(9 + torch.randint(0, 5, (F,), generator=g))).to(dev) for _ in range(2))
    assert not torch.equal(*p["sv"])
    return p


def weights(p, source):
    """(w_gate, w_up) e4m3 [F, K]: two tensors, or the halves of one [2F, K] tensor in either order (views, rows K apart)"""
    if source == "two weights":
        return p["wg"], p["wu"]
    lo, hi = p["fused"][:F], p["fused"][F:]
    return (lo, hi) if source == "fused, gate first" else (hi, lo)


def fresh_state(p, layout):
    """c and the cache as views of buffers with sentinels: rows behind c, the cache's padding [M, ldc) and a row behind it (column-major),
    or the rows of the last group at or past M (group-major)"""
    dev, B, M, G, ldc = p["a"].device, p["B"], p["M"], p["G"], p["ldc"]
    c_buf = torch.full((B * M + MLP_BM, F), SENT, dtype=torch.bfloat16, device=dev)
    c = c_buf[: B * M].view(B, M, F)
    if layout == "column":
        cache_buf = torch.full((B, F + 1, ldc), SENT, dtype=torch.bfloat16, device=dev)
        cache_buf[:, :F, :M] = p["cache0"]
        cache = cache_buf[:, :F, :M]
    else:
        rows = torch.full((B, G * MLP_BM, F), SENT, dtype=torch.bfloat16, device=dev)
        rows[:, :M] = p["cache0"].transpose(1, 2)
        cache_buf = rows.view(B, G, MLP_BM, F).transpose(2, 3).contiguous()               # [B, G, F, 128]
        cache = cache_buf
    return dict(c=c, c_buf=c_buf, cache=cache, cache_buf=cache_buf, layout=layout)


def operands(p, s, b=None):
    """(a, c, cache, inds, cnt) as the operators take them: 2-D for one sequence (or sequence b of a batch), the 3-D batch otherwise"""
    if p["B"] == 1 or b is not None:
        b = 0 if b is None else b
        return p["a"][b], s["c"][b], s["cache"][b], p["inds"][b], p["cnt"][b]
    return p["a"], s["c"], s["cache"], p["inds"], p["cnt"]


def run_w8(p, s, w, scales, biases, act, upd, b=None):
    a, c, cache, inds, cnt = operands(p, s, b)
    torch.ops.chipmunk.csp_mlp_mm1_glu_w8(a, w[0], w[1], scales[0], scales[1], c, biases[0], biases[1], cache, inds, cnt, act, upd)


def widened(w8, scale):
    sb = scale.to(torch.bfloat16)
    wide = w8.to(torch.bfloat16) * (sb[:, None] if sb.numel() > 1 else sb)
    assert torch.equal(wide.double(), w8.double() * (scale.double()[:, None] if scale.numel() > 1 else scale.double())), "widening is exact"
    return wide


def run_bf16(p, s, w, scales, biases, act, upd):
    a, c, cache, inds, cnt = operands(p, s)
    torch.ops.chipmunk.csp_mlp_mm1_glu(a, widened(w[0], scales[0]), widened(w[1], scales[1]), c, biases[0], biases[1], cache, inds, cnt, act, upd)


def cache_cm(p, s):
    """the cache as [B, F, M], whatever its layout"""
    if s["layout"] == "column":
        return s["cache"]
    B, G = p["B"], p["G"]
    return s["cache"].transpose(2, 3).reshape(B, G * MLP_BM, F)[:, : p["M"]].transpose(1, 2)


def check_untouched(p, s, what, cache_written):
    B, M = p["B"], p["M"]
    assert (s["c_buf"][B * M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    past = torch.arange(F, device=s["c"].device) >= p["cols"][..., None]
    assert (s["c"][past] == SENT).all(), f"{what}: packed columns at or past a count were written"
    if s["layout"] == "column":
        assert (s["cache_buf"][:, F] == SENT).all() and (s["cache_buf"][:, :F, M:] == SENT).all(), f"{what}: cache padding was written"
    else:
        tail = s["cache_buf"].transpose(2, 3).reshape(B, -1, F)[:, M:]
        assert (tail == SENT).all(), f"{what}: rows of the last group at or past M were written"
    now = cache_cm(p, s)
    if not cache_written:
        assert torch.equal(bits(now), bits(p["cache0"])), f"{what}: the cache was written"
    else:       # a column that no group row selected keeps its bits
        for b in range(B):
            for g in range(p["G"]):
                rows = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM))
                keep = torch.ones(F, dtype=torch.bool, device=now.device)
                keep[p["inds"][b, g, : int(p["cnt"][b, g])].long()] = False
                assert torch.equal(bits(now[b, keep][:, rows]), bits(p["cache0"][b, keep][:, rows])), f"{what}: an unselected column changed"


def assert_same(s, ref, what, other="csp_mlp_mm1_glu on the widened weights"):
    assert torch.equal(bits(s["c_buf"]), bits(ref["c_buf"])), f"{what}: packed deltas differ from {other}"
    assert torch.equal(bits(s["cache_buf"]), bits(ref["cache_buf"])), f"{what}: the cache differs from {other}"


# ------------------------------------------------------------------------------------------------ (a) bits of the bf16 gated kernel
BIT_CASES = ([(1003, 1536, 1, "column", act, upd) for act in ACTS for upd in (False, True)] +
             [(40, 64, 1, "column", "gelu_tanh", True), (40, 64, 1, "group", "silu", False),
              (128, 192, 1, "column", "gelu", True), (128, 64, 1, "group", "gelu_tanh", True),
              (1003, 192, 2, "column", "gelu_tanh", True), (1003, 192, 2, "group", "silu", True), (1003, 64, 2, "column", "gelu", False),
              (1003, 1536, 1, "group", "silu", True), (1003, 192, 1, "group", "gelu", False)])


@pytest.mark.parametrize("M,K,B,layout,act,upd", BIT_CASES)
def test_bits_of_the_bf16_gated_form_on_the_widened_weights(dev, M, K, B, layout, act, upd):
    p = problem(M, K, B)
    for kind in ("s1", "sv"):
        for source in SOURCES:
            s, ref = fresh_state(p, layout), fresh_state(p, layout)
            w = weights(p, source)
            run_w8(p, s, w, p[kind], (None, None), act, upd)
            run_bf16(p, ref, w, p[kind], (None, None), act, upd)
            what = f"M {M} K {K} B {B} {layout} {act} update {upd} scales {'number' if kind == 's1' else 'vector'}, {source}"
            check_untouched(p, s, what, cache_written=upd)
            assert_same(s, ref, what)


# ------------------------------------------------------------------------------------------------ general scales
@functools.lru_cache(maxsize=None)
def model_problem(K, vector):
    """M = 1003: a 0.5, weights 0.06 randn quantised with 448 / amax scales (per row, or one: no powers of two), biases 0.1 / 0.3, cache 0.3"""
    p = dict(problem(1003, K, 1))
    dev = p["a"].device
    g = torch.Generator().manual_seed(77 + K)
    p["a"] = (torch.randn(1, 1003, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    for name, mul in (("g", 1.0), ("u", 1.3)):
        w = torch.randn(F, K, generator=g) * 0.06 * mul
        amax = w.abs().amax(dim=1) if vector else w.abs().amax().reshape(1)
        recip = (amax / 448.0).float()
        p["w" + name] = (w / (recip[:, None] if vector else recip)).clamp(-448, 448).to(E4M3).to(dev)
        p["s" + name] = recip.to(dev)
        assert not (torch.frexp(recip)[0] == 0.5).any(), "the scales must not be powers of two"
    p["bu"] = (torch.randn(F, generator=g) * 0.3).to(torch.bfloat16).to(dev)
    return p


# ------------------------------------------------------------------------------------------------ (b) bits of the ungated weight-only kernel
@pytest.mark.parametrize("K,vector,layout", [(192, True, "column"), (1536, False, "group"), (64, True, "group"), (1536, True, "column")])
def test_a_unit_up_branch_gives_the_bits_of_the_ungated_weight_only_kernel(dev, K, vector, layout, act="gelu_tanh"):
    p = model_problem(K, vector)
    zeros, ones = torch.zeros(F, K, dtype=torch.uint8, device=dev).view(E4M3), torch.ones(F, dtype=torch.bfloat16, device=dev)
    for upd in (False, True):
        s, ref = fresh_state(p, layout), fresh_state(p, layout)
        run_w8(p, s, (p["wg"], zeros), (p["sg"], p["su"]), (p["bg"], ones), act, upd)
        a, c, cache, inds, cnt = operands(p, ref)
        torch.ops.chipmunk.csp_mlp_mm1_w8(a, p["wg"], p["sg"], c, p["bg"], cache, inds, cnt, act, upd)
        what = f"unit up branch, K {K} {'vector' if vector else 'number'} {layout} {act} update {upd}"
        check_untouched(p, s, what, cache_written=upd)
        assert_same(s, ref, what, other="csp_mlp_mm1_w8 with the gate's weight, scale and bias")


# ------------------------------------------------------------------------------------------------ (c) fp64 model
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K,vector", [(192, True), (1536, True), (1536, False)])
def test_segments_against_the_fp64_definition(dev, K, vector, act):
    p = model_problem(K, vector)
    exact, fresh = mm1_glu_w8_exact(p["a"][0], p["wg"], p["wu"], p["sg"], p["su"], p["bg"], p["bu"], p["cache0"][0], p["inds"][0],
                                    p["cnt"][0], act)
    cols = p["cols"][0]
    for layout, upd in (("column", False), ("column", True), ("group", True)):
        s = fresh_state(p, layout)
        run_w8(p, s, (p["wg"], p["wu"]), (p["sg"], p["su"]), (p["bg"], p["bu"]), act, upd)
        what = f"csp_mlp_mm1_glu_w8 K {K} {'vector' if vector else 'number'} {act} {layout} update {upd}"
        check_untouched(p, s, what, cache_written=upd)
        worst = assert_segs_close(s["c"][0], exact, MLP_SEG_BOUND, f"{what}: packed deltas", width=MLP_SEG_W1, cols=cols)
        print(f"{what}: worst {MLP_SEG_W1}-column segment error {worst:.5f} (bound {MLP_SEG_BOUND})")
        if upd:      # the refreshed columns against the fresh activation, as tests/test_gpu_mlp_accuracy.py::assert_cache
            got = gathered_cache(cache_cm(p, s)[0], p["inds"][0], p["cnt"][0])
            term = refreshed_cache_term(got, fresh, exact, MLP_SEG_BOUND, MLP_SEG_W1, cols)
            worst = assert_segs_close(got, fresh, MLP_SEG_BOUND, f"{what}: refreshed cache columns", extra=term, cols=cols)
            print(f"{what}: refreshed cache columns, worst error less its term {worst:.5f} (bound {MLP_SEG_BOUND})")


# ------------------------------------------------------------------------------------------------ (d) consistency
@pytest.mark.parametrize("layout", ["column", "group"])
def test_zero_biases_are_no_biases_and_constant_vectors_are_the_numbers(dev, layout):
    p = problem(1003, 192, 1)
    w = weights(p, "two weights")
    zero = torch.zeros(F, dtype=torch.bfloat16, device=dev)
    ng, nu = torch.tensor([0.00123], device=dev), torch.tensor([0.00217], device=dev)                   # no powers of two
    base = fresh_state(p, layout)
    run_w8(p, base, w, (ng, nu), (None, None), "silu", True)
    check_untouched(p, base, "numbers, no biases", cache_written=True)
    vg, vu = ng.expand(F).contiguous(), nu.expand(F).contiguous()
    for what, scales, biases in (("zero bias vectors", (ng, nu), (zero, zero)), ("a zero gate bias", (ng, nu), (zero, None)),
                                 ("constant scale vectors", (vg, vu), (None, None)), ("a constant gate vector", (vg, nu), (None, None)),
                                 ("a constant up vector", (ng, vu), (None, None)), ("a second run", (ng, nu), (None, None))):
        s = fresh_state(p, layout)
        run_w8(p, s, w, scales, biases, "silu", True)
        assert torch.equal(bits(s["c_buf"]), bits(base["c_buf"])) and torch.equal(bits(s["cache_buf"]), bits(base["cache_buf"])), what


@pytest.mark.parametrize("layout", ["column", "group"])
def test_fused_scatter_is_the_unfused_sequence_and_a_batch_is_its_slices(dev, layout):
    from chipmunk_amd import ops
    from chipmunk_amd.ops.mlp import scatter_add_gm
    p = problem(1003, 192, 2)
    w, scales, biases = weights(p, "fused, up first"), p["sv"], (p["bg"], p["bu"])
    fused = fresh_state(p, layout)
    run_w8(p, fused, w, scales, biases, "gelu_tanh", True)
    check_untouched(p, fused, "fused scatter", cache_written=True)
    # update_cache 0, then the scatter-add of the packed deltas
    seq = fresh_state(p, layout)
    run_w8(p, seq, w, scales, biases, "gelu_tanh", False)
    check_untouched(p, seq, "update_cache 0", cache_written=False)
    if layout == "column":
        ops.scatter_add(seq["c"], seq["cache"], p["inds"], p["cnt"], 6)
    else:
        scatter_add_gm(seq["c"], seq["cache"], p["inds"], p["cnt"])
    assert_same(fused, seq, f"{layout}: fused scatter", other="update_cache 0 followed by the scatter-add")
    # the batch against one launch per sequence on the slices
    slices = fresh_state(p, layout)
    for b in range(p["B"]):
        run_w8(p, slices, w, scales, biases, "gelu_tanh", True, b=b)
    assert_same(fused, slices, f"{layout}: the batch", other="one launch per sequence")


def test_the_operator_refuses_what_the_kernel_does_not_take(dev):
    p = problem(128, 64, 1)
    s = fresh_state(p, "column")
    a, c, cache, inds, cnt = operands(p, s)
    op = torch.ops.chipmunk.csp_mlp_mm1_glu_w8
    s1 = p["s1"][0]
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        op(a, p["wg"].to(torch.bfloat16), p["wu"], s1, s1, c, None, None, cache, inds, cnt, "gelu_tanh", False)
    with pytest.raises(RuntimeError, match="scale_gate and scale_up"):
        op(a, p["wg"], p["wu"], s1, p["sv"][0][:7].contiguous(), c, None, None, cache, inds, cnt, "gelu_tanh", False)
    with pytest.raises(RuntimeError, match="unknown activation"):
        op(a, p["wg"], p["wu"], s1, s1, c, None, None, cache, inds, cnt, "relu", False)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        op(a[:, :32].contiguous(), p["wg"][:, :32].contiguous(), p["wu"][:, :32].contiguous(), s1, s1, c, None, None, cache, inds, cnt,
           "gelu_tanh", False)
    check_untouched(p, s, "refused calls", cache_written=False)
    assert (s["c"] == SENT).all()
