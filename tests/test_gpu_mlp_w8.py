"""``csp_mlp_mm1_w8`` -- GEMM1 over an e4m3 ``fc1`` weight with bf16 activations ("Weight-only fc1") -- on the GPU.

(a) Bits.  With a power-of-two ``scale_b`` (one number, or one per fc1 row) and no bias, the packed deltas and the updated cache are
    ``csp_mlp_mm1_act``'s on ``W.to(bf16) * scale_b``, bit for bit, sentinels included: the lane / byte / k mapping of the widened
    fragments is a condition, not a tolerance.  The weights hold every finite e4m3 byte.  K = 64 (one k step, shorter than the ring), 192
    (odd against the ring depth of 3) and 1536; M = 40 (one group under 64 rows), 128 and 1003 (last group of 107 rows); F = 1024; counts
    0, 1, 64, 65, 1000 and 1024 mixed in one call; the three activations; update_cache 0 / 1; a batch of two; both cache layouts.  One
    more launch shape reaches the tail split (64 x 64 sub-tiles), which F = 1024 does not: 16 groups x (slots / 2 + 1) column tiles.
(b) With a bias and scales that are no powers of two every 128-column (and every 64-column) segment of every row is held against the fp64
    definition (tests/mlp_w8_model.py) under helpers.MLP_SEG_BOUND, the bound tests/test_gpu_mlp_accuracy.py holds the ungated bf16 form
    to: the same arithmetic class plus one fp32 multiply (2^-24 relative, four orders below the bound).  No new constant.
(c) A zero bias vector gives the bits of no bias, a constant scale vector those of the number; nothing at or past M, at or past a count,
    in the cache's padding or in a column that was not selected is written."""
import functools

import pytest
import torch

from helpers import MLP_BM, MLP_SEG_BOUND, MLP_SEG_W1, assert_segs_close, gathered_cache, refreshed_cache_term
from mlp_w8_model import E4M3, every_byte_weight, mm1_w8_exact

pytestmark = pytest.mark.gpu

SENT = 7.0
F = 1024
ACTS = ("gelu_tanh", "silu", "gelu")
COUNTS = {40: [[65]], 128: [[1000]], 1003: [[0, 1, 64, 65, 1000, 1024, 128, 1024], [1024, 65, 0, 1000, 1, 64, 1024, 520]]}


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def problem(M, K, B, f=F, seed=0, counts=None):
    """inputs on the device: a [B, M, K] bf16, an every-byte e4m3 weight, a random cache [B, f, M], one index permutation per group"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * M + K + seed)
    G = (M + MLP_BM - 1) // MLP_BM
    counts = [list(c) for c in counts] if counts is not None else COUNTS[M][:B]
    assert len(counts) == B and all(len(c) == G for c in counts)
    p = dict(M=M, K=K, B=B, F=f, G=G, ldc=(M + 7) // 8 * 8)
    p["a"] = (torch.randn(B, M, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    p["w8"] = every_byte_weight(f, K, seed=M + K).to(dev)
    p["cache0"] = (torch.randn(B, f, M, generator=g) * 0.3).to(torch.bfloat16).to(dev)
    p["bias"] = (torch.randn(f, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    p["inds"] = torch.stack([torch.stack([torch.randperm(f, generator=g) for _ in range(G)]) for _ in range(B)]).to(torch.int32).to(dev)
    p["cnt"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    p["cols"] = p["cnt"].long().repeat_interleave(MLP_BM, dim=1)[:, :M]                  # [B, M]: the live columns of every row
    # power-of-two reciprocal scales: |w| <= 448 -> <= 0.44 and below
    p["s1"] = torch.tensor([2.0 ** -10], device=dev)
    p["sv"] = torch.ldexp(torch.ones(f), -(8 + torch.randint(0, 5, (f,), generator=g))).to(dev)
    return p


def fresh_state(p, layout):
    """c and the cache as views of buffers with sentinels: rows behind c, the cache's padding [M, ldc) and a row behind it (column-major),
    or the rows of the last group at or past M (group-major)"""
    dev, B, M, f, G, ldc = p["a"].device, p["B"], p["M"], p["F"], p["G"], p["ldc"]
    c_buf = torch.full((B * M + MLP_BM, f), SENT, dtype=torch.bfloat16, device=dev)
    c = c_buf[: B * M].view(B, M, f)
    if layout == "column":
        cache_buf = torch.full((B, f + 1, ldc), SENT, dtype=torch.bfloat16, device=dev)
        cache_buf[:, :f, :M] = p["cache0"]
        cache = cache_buf[:, :f, :M]
    else:
        rows = torch.full((B, G * MLP_BM, f), SENT, dtype=torch.bfloat16, device=dev)
        rows[:, :M] = p["cache0"].transpose(1, 2)
        cache_buf = rows.view(B, G, MLP_BM, f).transpose(2, 3).contiguous()               # [B, G, f, 128]
        cache = cache_buf
    return dict(c=c, c_buf=c_buf, cache=cache, cache_buf=cache_buf, layout=layout)


def operands(p, s):
    """(a, c, cache, inds, cnt) as the operators take them: 2-D for one sequence, the 3-D batch otherwise"""
    if p["B"] == 1:
        return p["a"][0], s["c"][0], s["cache"][0], p["inds"][0], p["cnt"][0]
    return p["a"], s["c"], s["cache"], p["inds"], p["cnt"]


def run_w8(p, s, scale, bias, act, upd):
    a, c, cache, inds, cnt = operands(p, s)
    torch.ops.chipmunk.csp_mlp_mm1_w8(a, p["w8"], scale, c, bias, cache, inds, cnt, act, upd)


def run_bf16(p, s, scale, bias, act, upd):
    a, c, cache, inds, cnt = operands(p, s)
    sb = scale.to(torch.bfloat16)
    wide = p["w8"].to(torch.bfloat16) * (sb[:, None] if sb.numel() > 1 else sb)
    assert torch.equal(wide.double(), p["w8"].double() * (scale.double()[:, None] if scale.numel() > 1 else scale.double())), "widening is exact"
    torch.ops.chipmunk.csp_mlp_mm1_act(a, wide, c, bias, cache, inds, cnt, act, upd)


def cache_cm(p, s):
    """the cache as [B, F, M], whatever its layout"""
    if s["layout"] == "column":
        return s["cache"]
    B, G, f = p["B"], p["G"], p["F"]
    return s["cache"].transpose(2, 3).reshape(B, G * MLP_BM, f)[:, : p["M"]].transpose(1, 2)


def check_untouched(p, s, what, cache_written):
    B, M, f = p["B"], p["M"], p["F"]
    assert (s["c_buf"][B * M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    past = torch.arange(f, device=s["c"].device) >= p["cols"][..., None]
    assert (s["c"][past] == SENT).all(), f"{what}: packed columns at or past a count were written"
    if s["layout"] == "column":
        assert (s["cache_buf"][:, f] == SENT).all() and (s["cache_buf"][:, :f, M:] == SENT).all(), f"{what}: cache padding was written"
    else:
        tail = s["cache_buf"].transpose(2, 3).reshape(B, -1, f)[:, M:]
        assert (tail == SENT).all(), f"{what}: rows of the last group at or past M were written"
    now = cache_cm(p, s)
    if not cache_written:
        assert torch.equal(bits(now), bits(p["cache0"])), f"{what}: the cache was written"
    else:       # a column that no group row selected keeps its bits
        for b in range(B):
            for g in range(p["G"]):
                rows = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM))
                keep = torch.ones(f, dtype=torch.bool, device=now.device)
                keep[p["inds"][b, g, : int(p["cnt"][b, g])].long()] = False
                assert torch.equal(bits(now[b, keep][:, rows]), bits(p["cache0"][b, keep][:, rows])), f"{what}: an unselected column changed"


def assert_same(p, s, ref, what):
    assert torch.equal(bits(s["c_buf"]), bits(ref["c_buf"])), f"{what}: packed deltas differ from csp_mlp_mm1_act on the widened weight"
    assert torch.equal(bits(s["cache_buf"]), bits(ref["cache_buf"])), f"{what}: the cache differs from csp_mlp_mm1_act on the widened weight"


# ------------------------------------------------------------------------------------------------ (a) bits
BIT_CASES = ([(1003, 1536, 1, "column", act, upd) for act in ACTS for upd in (False, True)] +
             [(40, 64, 1, "column", "gelu_tanh", True), (40, 64, 1, "group", "silu", False),
              (128, 192, 1, "column", "gelu", True), (128, 64, 1, "group", "gelu_tanh", True),
              (1003, 192, 2, "column", "gelu_tanh", True), (1003, 192, 2, "group", "silu", True), (1003, 64, 2, "column", "gelu", False),
              (1003, 1536, 1, "group", "gelu_tanh", True), (1003, 192, 1, "group", "gelu", False)])


@pytest.mark.parametrize("M,K,B,layout,act,upd", BIT_CASES)
def test_bits_of_the_bf16_form_on_the_widened_weight(dev, M, K, B, layout, act, upd):
    p = problem(M, K, B)
    for kind in ("s1", "sv"):
        s, ref = fresh_state(p, layout), fresh_state(p, layout)
        run_w8(p, s, p[kind], None, act, upd)
        run_bf16(p, ref, p[kind], None, act, upd)
        what = f"M {M} K {K} B {B} {layout} {act} update {upd} scale {'number' if kind == 's1' else 'vector'}"
        check_untouched(p, s, what, cache_written=upd)
        assert_same(p, s, ref, what)


@pytest.mark.parametrize("layout", ["column", "group"])
def test_bits_through_the_tail_split(dev, layout):
    """16 groups x (slots / 2 + 1) column tiles: every XCD keeps two leftover tiles and hands them out as 64 x 64 sub-tiles (the launch
    shape of tests/test_gpu_mlp_batched.py::test_tail_split_across_a_batch_boundary), the last group ragged (107 rows: a sub-tile of 43)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt = (2 * cus // 8) // 2 + 1
    f = nt * 128
    lists = ((2048, 0, 1024, 3072, 512, 256, 4096, f), (256, f, 0, 1024, 2048, 512, f, f))
    lists = tuple(tuple(min(c, f) for c in row) for row in lists)
    p = problem(1003, 192, 2, f=f, seed=7, counts=lists)
    for kind in ("s1", "sv"):
        s, ref = fresh_state(p, layout), fresh_state(p, layout)
        run_w8(p, s, p[kind], None, "gelu_tanh", True)
        run_bf16(p, ref, p[kind], None, "gelu_tanh", True)
        check_untouched(p, s, f"tail split {layout} {kind}", cache_written=True)
        assert_same(p, s, ref, f"tail split {layout} {kind}")


# ------------------------------------------------------------------------------------------------ (b) fp64 model
@functools.lru_cache(maxsize=None)
def model_problem(K, vector):
    """M = 1003: a 0.5, weights 0.06 randn quantised with 448 / amax scales (per row, or one: no powers of two), bias 0.1, cache 0.3"""
    p = dict(problem(1003, K, 1))
    g = torch.Generator().manual_seed(77 + K)
    w = torch.randn(F, K, generator=g) * 0.06
    amax = w.abs().amax(dim=1) if vector else w.abs().amax().reshape(1)
    recip = (amax / 448.0).float()
    p["w8"] = (w / (recip[:, None] if vector else recip)).clamp(-448, 448).to(E4M3).to(p["a"].device)
    p["scale"] = recip.to(p["a"].device)
    frac = torch.frexp(recip)[0]
    assert not (frac == 0.5).any(), "the scales must not be powers of two"
    return p


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K,vector", [(192, True), (1536, True), (1536, False)])
def test_segments_against_the_fp64_definition(dev, K, vector, act):
    p = model_problem(K, vector)
    exact, fresh = mm1_w8_exact(p["a"][0], p["w8"], p["scale"], p["bias"], p["cache0"][0], p["inds"][0], p["cnt"][0], act)
    cols = p["cols"][0]
    for layout, upd in (("column", False), ("column", True), ("group", True)):
        s = fresh_state(p, layout)
        run_w8(p, s, p["scale"], p["bias"], act, upd)
        what = f"csp_mlp_mm1_w8 K {K} {'vector' if vector else 'number'} {act} {layout} update {upd}"
        check_untouched(p, s, what, cache_written=upd)
        for width in (128, MLP_SEG_W1):
            worst = assert_segs_close(s["c"][0], exact, MLP_SEG_BOUND, f"{what}: packed deltas, {width}-column segments", width=width, cols=cols)
            print(f"{what}: worst {width}-column segment error {worst:.5f} (bound {MLP_SEG_BOUND})")
        if upd:      # the refreshed columns against the fresh activation, as tests/test_gpu_mlp_accuracy.py::assert_cache
            got = gathered_cache(cache_cm(p, s)[0], p["inds"][0], p["cnt"][0])
            term = refreshed_cache_term(got, fresh, exact, MLP_SEG_BOUND, MLP_SEG_W1, cols)
            assert_segs_close(got, fresh, MLP_SEG_BOUND, f"{what}: refreshed cache columns", extra=term, cols=cols)


# ------------------------------------------------------------------------------------------------ (c) independence
@pytest.mark.parametrize("layout", ["column", "group"])
def test_zero_bias_is_no_bias_and_a_constant_vector_is_the_number(dev, layout):
    p = problem(1003, 192, 1)
    zero = torch.zeros(F, dtype=torch.bfloat16, device=dev)
    number = torch.tensor([0.00123], device=dev)                   # no power of two
    base = fresh_state(p, layout)
    run_w8(p, base, number, None, "gelu_tanh", True)
    check_untouched(p, base, "number, no bias", cache_written=True)
    for what, scale, bias in (("zero bias vector", number, zero), ("constant scale vector", number.expand(F).contiguous(), None),
                              ("0-dim-like one-element scale", number.clone(), None)):
        s = fresh_state(p, layout)
        run_w8(p, s, scale, bias, "gelu_tanh", True)
        assert torch.equal(bits(s["c_buf"]), bits(base["c_buf"])) and torch.equal(bits(s["cache_buf"]), bits(base["cache_buf"])), what


def test_the_operator_refuses_what_the_kernel_does_not_take(dev):
    p = problem(128, 64, 1)
    s = fresh_state(p, "column")
    a, c, cache, inds, cnt = operands(p, s)
    op = torch.ops.chipmunk.csp_mlp_mm1_w8
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        op(a, p["w8"].to(torch.bfloat16), p["s1"], c, None, cache, inds, cnt, "gelu_tanh", False)
    with pytest.raises(RuntimeError, match="scale_b"):
        op(a, p["w8"], p["sv"][:7].contiguous(), c, None, cache, inds, cnt, "gelu_tanh", False)
    with pytest.raises(RuntimeError, match="unknown activation"):
        op(a, p["w8"], p["s1"], c, None, cache, inds, cnt, "relu", False)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        op(a[:, :32].contiguous(), p["w8"][:, :32].contiguous(), p["s1"], c, None, cache, inds, cnt, "gelu_tanh", False)
    check_untouched(p, s, "refused calls", cache_written=False)
    assert (s["c"] == SENT).all()
