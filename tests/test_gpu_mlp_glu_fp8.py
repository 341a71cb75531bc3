"""The gated fp8 GEMM1 operator ``chipmunk::csp_mlp_mm1_glu_fp8``: for e4m3 a, Wg, Wu and reciprocal scales ra, rbg, rbu
c = bf16(fma(act((a Wg^T) ra rbg + bg), (a Wu^T) ra rbu + bu, -cache)) on the kept columns, optionally followed by the scatter-add of c into the
cache ("Gated MLPs").  K = 256, F = 512; shapes, NaN slack rows behind a, the sentinel 7.0 in everything the operator must not
write, the canary row behind the cache and NaN in the cache padding are those of tests/test_gpu_mlp_glu.py.

1. an exactly representable problem (small integers as e4m3, power-of-two scales, biases in 1/64): the BITS of the bf16 gated kernel on
   the dequantised operands -- every partial sum on either side is exact in fp32 in any order, so this is a condition, not a tolerance;
2. every group against fp32 torch on random data under the project's fp8 GEMM1 tolerance (atol = rtol = 3e-2), weight scales 2.5 x apart,
   three activations x four bias combinations; the cache bit for bit;
3. the fused scatter = update off followed by csp_scatter_add; 4. a batch = its slices; 5. run to run; 6. refusals."""
import pytest
import torch

import glu_fp8_method_model as gfp

pytestmark = pytest.mark.gpu

BM = 128
K, F = 256, 512
SENT = 7.0
SHAPES = [
    (129, 144, [0, F]),
    (333, 336, [F, 0, 336]),
    (1000, 1000, [F, 0, 208, 16, 40, 512, 64, 272]),
]
IDS = [f"M{m}-ld{l}" for m, l, _ in SHAPES]
ACTS = ["gelu_tanh", "silu", "gelu"]
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def with_slack(rows, fill):
    """[M, C] tensor -> its copy as the [:M] view of a [M + 128, C] buffer whose slack rows hold `fill` (returns buffer, view)."""
    buf = torch.full((rows.shape[0] + BM, rows.shape[1]), fill, dtype=torch.float32, device=rows.device).to(rows.dtype)
    buf[: rows.shape[0]] = rows
    return buf, buf[: rows.shape[0]]


def fresh_state(p):
    """Mutable tensors of one launch: c (packed deltas out) and the cache, as views of buffers with canaries."""
    dev, M, f, ldc = p["cache0"].device, p["M"], p["f"], p["ldc"]
    cache_buf = torch.full((f + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)      # padding [M, ldc) = NaN
    cache_buf[f] = SENT                                                                           # the canary row
    cache_buf[:f, :M] = p["cache0"]
    c_buf, c = with_slack(torch.full((M, f), SENT, dtype=torch.bfloat16, device=dev), SENT)
    return dict(c=c, c_buf=c_buf, cache=cache_buf[:f, :M], cache_buf=cache_buf)


def random_problem(dev, M, ldc, counts, seed):
    p = gfp.fp8_problem(dev, M, counts, seed, k=K, f=F)
    p["ldc"] = ldc
    p["a_buf"], p["a"] = with_slack(p["a"], float("nan"))
    return p


def glu8(p, s, act, update, bg="bg", bu="bu"):
    torch.ops.chipmunk.csp_mlp_mm1_glu_fp8(p["a"], p["wg"], p["wu"], s["c"], p[bg] if bg else None, p[bu] if bu else None, s["cache"],
                                           p["inds"], p["cnt"], p["ra"], p["rbg"], p["rbu"], act, update)
    torch.cuda.synchronize()


def check_canaries(p, s, what):
    M, f = p["M"], p["f"]
    assert (s["c_buf"][M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    assert (s["cache_buf"][f] == SENT).all(), f"{what}: the row behind the cache's F * ldc elements was written"
    assert torch.isnan(p["a_buf"][M:].float()).all(), f"{what}: the input's slack rows changed"


# ------------------------------------------------------------------------------------------------ 1. the bf16 gated kernel's bits
EXACT_SCALES = (2.0 ** -4, 2.0 ** -3, 2.0 ** -2)      # scale_a, scale_b_gate, scale_b_up
_exact = {}


def exact_problem(dev, M, ldc, counts, seed):
    """a, Wg, Wu integers in [-4, 4] (exact in e4m3), scales 2^-4 / 2^-3 / 2^-2, biases multiples of 1/64 in [-1, 1] (exact in bf16);
    `a16`, `wg16`, `wu16`: the dequantised operands, exact in bf16.  Every partial sum of a gate (up) product is a multiple of 2^-7 (2^-6)
    below 2^24 such units on both sides: exact in fp32 in any order, so both kernels' epilogues see the same fp32 numbers."""
    key = (M, ldc, tuple(counts), seed)
    if key not in _exact:
        G = (M + BM - 1) // BM
        g = torch.Generator(device=dev).manual_seed(seed)
        ints = lambda *shape: torch.randint(-4, 5, shape, device=dev, generator=g).float()      # noqa: E731
        a, wg, wu = ints(M, K), ints(F, K), ints(F, K)
        sa, sg, su = EXACT_SCALES
        p = {"M": M, "G": G, "ldc": ldc, "counts": counts, "f": F}
        p["a_buf"], p["a"] = with_slack(a.to(F8), float("nan"))
        p["wg"], p["wu"] = wg.to(F8), wu.to(F8)
        p["a16_buf"], p["a16"] = with_slack((a * sa).to(torch.bfloat16), float("nan"))
        p["wg16"], p["wu16"] = (wg * sg).to(torch.bfloat16), (wu * su).to(torch.bfloat16)
        assert torch.equal(p["a"].float(), a) and torch.equal(p["a16"].float(), a * sa) and torch.equal(p["wu16"].float(), wu * su)
        p["ra"], p["rbg"], p["rbu"] = (torch.tensor([s], device=dev) for s in EXACT_SCALES)
        p["bg"], p["bu"] = ((torch.randint(-64, 65, (F,), device=dev, generator=g).float() / 64).to(torch.bfloat16) for _ in range(2))
        p["cache0"] = (torch.randn(F, M, device=dev, generator=g) * 0.3).to(torch.bfloat16)
        p["inds"] = torch.stack([torch.randperm(F, device=dev, generator=g) for _ in range(G)]).to(torch.int32)
        p["cnt"] = torch.tensor(counts, dtype=torch.int32, device=dev)
        _exact[key] = p
    return _exact[key]


@pytest.mark.parametrize("update", [False, True], ids=["update off", "scatter"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,ldc,counts", SHAPES, ids=IDS)
def test_exact_problem_gives_the_bits_of_the_bf16_gated_kernel(dev, M, ldc, counts, act, update):
    p = exact_problem(dev, M, ldc, counts, seed=M)
    ref, got = fresh_state(p), fresh_state(p)
    torch.ops.chipmunk.csp_mlp_mm1_glu(p["a16"], p["wg16"], p["wu16"], ref["c"], p["bg"], p["bu"], ref["cache"], p["inds"], p["cnt"], act, update)
    glu8(p, got, act, update)
    check_canaries(p, got, "fp8 gated")
    assert torch.equal(bits(got["c"]), bits(ref["c"])), "packed deltas differ from the bf16 gated kernel's on the dequantised operands"
    assert torch.equal(bits(got["cache"]), bits(ref["cache"])), "the cache differs from the bf16 gated kernel's"
    assert update or torch.equal(bits(got["cache"]), bits(p["cache0"]))


def make_batch(B, M, ldc, ps):
    """B problems with shared weights, biases and scales as one batch: a [B, M, K], cache the [:, :F, :M] view of [B, F + 1, ldc] (a canary
    row behind every sequence, so the batch stride exceeds F * ldc), indices [B, G, F], counts [B, G]."""
    dev = ps[0]["cache0"].device
    batch = dict(a=torch.stack([q["a"].view(torch.uint8) for q in ps]).view(F8), inds=torch.stack([q["inds"] for q in ps]),
                 cnt=torch.stack([q["cnt"] for q in ps]))

    def state():
        cache_buf = torch.full((B, F + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
        cache_buf[:, F] = SENT
        for b, q in enumerate(ps):
            cache_buf[b, :F, :M] = q["cache0"]
        c_buf = torch.full((B * M + BM, F), SENT, dtype=torch.bfloat16, device=dev)
        return dict(c=c_buf[: B * M].view(B, M, F), c_buf=c_buf, cache=cache_buf[:, :F, :M], cache_buf=cache_buf)
    return batch, state


def test_exact_batch_of_two_gives_the_bits_of_the_bf16_gated_batch(dev):
    M, ldc, counts = SHAPES[1]
    p = exact_problem(dev, M, ldc, counts, seed=M)
    q = dict(exact_problem(dev, M, ldc, [336, F, 0], seed=M + 7))
    a2, a16_2 = q["a"], q["a16"]                            # the second sequence: its own rows, cache, indices and counts
    ps = [p, dict(q)]
    batch, state = make_batch(2, M, ldc, ps)
    a16 = torch.stack([p["a16"], a16_2])
    assert torch.equal(batch["a"][1].float(), a2.float())
    ref, got = state(), state()
    torch.ops.chipmunk.csp_mlp_mm1_glu(a16, p["wg16"], p["wu16"], ref["c"], p["bg"], p["bu"], ref["cache"], batch["inds"], batch["cnt"],
                                       "silu", True)
    torch.ops.chipmunk.csp_mlp_mm1_glu_fp8(batch["a"], p["wg"], p["wu"], got["c"], p["bg"], p["bu"], got["cache"], batch["inds"],
                                           batch["cnt"], p["ra"], p["rbg"], p["rbu"], "silu", True)
    torch.cuda.synchronize()
    assert torch.equal(bits(got["c_buf"]), bits(ref["c_buf"])), "packed deltas differ from the bf16 gated batch's"
    assert torch.equal(bits(got["cache"]), bits(ref["cache"])) and (got["cache_buf"][:, F] == SENT).all()
    assert not torch.equal(bits(got["cache"][1]), bits(q["cache0"])), "the second sequence's cache took its scatter-add"


# ------------------------------------------------------------------------------------------------ 2. fp32 torch, every group
@pytest.mark.parametrize("biases", [("bg", "bu"), ("bg", None), (None, "bu"), (None, None)], ids=["both biases", "gate bias", "up bias", "no bias"])
@pytest.mark.parametrize("act", ACTS)
def test_every_group_against_fp32_torch(dev, act, biases):
    """want = act((a_q Wg_q^T) ra rbg + bg) * ((a_q Wu_q^T) ra rbu + bu) - cache in fp32 from the same quantised operands, under
    atol = rtol = 3e-2 (the project's fp8 GEMM1 tolerance)."""
    bg, bu = biases
    for (M, ldc, counts), sid in zip(SHAPES, IDS):
        p = random_problem(dev, M, ldc, counts, seed=M + 1)
        cache0 = p["cache0"]
        h = gfp.want_fp32(p, act, bg, bu)                              # [M, F], every column: shared by both update settings
        for update in (False, True):
            s = fresh_state(p)
            glu8(p, s, act, update, bg=bg, bu=bu)
            what = f"{act}, {sid}, update {update}"
            check_canaries(p, s, what)
            ratios = gfp.group_ratios(p, s["c"], h, SENT)              # (asserts the sentinel in the packed columns past every count)
            print(f"{what}: worst error / tolerance per group with kept columns {', '.join(f'{r:.3f}' for r in ratios)}")
            assert all(r <= 1.0 for r in ratios), f"{what}: packed deltas outside atol = rtol = 3e-2 of fp32 torch ({max(ratios):.3f} x)"
            for g in range(p["G"]):
                rows, n = slice(g * BM, min(M, (g + 1) * BM)), counts[g]
                cols, rest = p["inds"][g, :n].long(), p["inds"][g, n:].long()
                if update:
                    new = (cache0[cols][:, rows].float() + s["c"][rows, :n].float().T).to(torch.bfloat16)
                    assert torch.equal(s["cache"][cols][:, rows], new), f"{what}: group {g}: cache != bf16(cache + delta)"
                    assert torch.equal(s["cache"][rest][:, rows], cache0[rest][:, rows]), f"{what}: group {g}: unselected cache columns changed"
            if not update:
                assert torch.equal(bits(s["cache"]), bits(cache0)), f"{what}: the cache was written"


# ------------------------------------------------------------------------------------------------ 3. - 5.
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,ldc,counts", SHAPES, ids=IDS)
def test_fused_scatter_equals_the_unfused_sequence(dev, M, ldc, counts, act):
    p = random_problem(dev, M, ldc, counts, seed=M + 2)
    fused, two = fresh_state(p), fresh_state(p)
    glu8(p, fused, act, True)
    glu8(p, two, act, False)
    torch.ops.chipmunk.csp_scatter_add(two["c"].unsqueeze(0), two["cache"].unsqueeze(0), p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0), 6)
    torch.cuda.synchronize()
    assert torch.equal(bits(fused["c"]), bits(two["c"])), "packed deltas differ"
    assert torch.equal(bits(fused["cache"]), bits(two["cache"])), "the cache differs from update off + csp_scatter_add"


def random_batch(dev, B, M, ldc, counts_per_seq, seed):
    ps = [random_problem(dev, M, ldc, counts_per_seq[b], seed) for b in range(B)]      # one seed: shared weights, biases and scales ...
    g = torch.Generator(device=dev).manual_seed(seed + 100)
    for q in ps[1:]:                                                                  # ... and rows, cache and indices of their own
        rows = (q["a"].float()[torch.randperm(M, device=dev, generator=g)]).to(F8)
        q["a_buf"], q["a"] = with_slack(rows, float("nan"))
        q["cache0"] = q["cache0"][:, torch.randperm(M, device=dev, generator=g)].contiguous()
        q["inds"] = torch.stack([torch.randperm(F, device=dev, generator=g) for _ in range(q["G"])]).to(torch.int32)
    return ps, *make_batch(B, M, ldc, ps)


@pytest.mark.parametrize("update", [False, True], ids=["update off", "scatter"])
def test_batch_of_three_equals_its_slices(dev, update):
    M, ldc, _ = SHAPES[1]
    ps, batch, state = random_batch(dev, 3, M, ldc, [[F, 0, 336], [0, 0, 0], [64, 272, F]], seed=21)
    p = ps[0]
    got, ref = state(), state()
    assert got["cache"].stride(0) > F * ldc
    op = torch.ops.chipmunk.csp_mlp_mm1_glu_fp8
    op(batch["a"], p["wg"], p["wu"], got["c"], p["bg"], None, got["cache"], batch["inds"], batch["cnt"], p["ra"], p["rbg"], p["rbu"], "silu", update)
    for b in range(3):
        op(batch["a"][b], p["wg"], p["wu"], ref["c"][b], p["bg"], None, ref["cache"][b], batch["inds"][b], batch["cnt"][b], p["ra"], p["rbg"],
           p["rbu"], "silu", update)
    torch.cuda.synchronize()
    assert torch.equal(bits(got["c_buf"]), bits(ref["c_buf"])), "packed deltas of the batch differ from the per-sequence launches'"
    assert torch.equal(bits(got["cache"]), bits(ref["cache"])), "the cache of the batch differs from the per-sequence launches'"
    assert (got["cache_buf"][:, F] == SENT).all() and (got["c"][1] == SENT).all(), "a canary row or the all-zero sequence was written"
    assert not (got["c"][2][:BM, :64] == SENT).any()
    assert not torch.equal(bits(got["c"][2][:BM, :64]), bits(got["c"][0][:BM, :64])), "the sequences have rows of their own"


@pytest.mark.parametrize("act", ACTS)
def test_three_launches_from_the_same_state_give_the_same_bits(dev, act):
    M, ldc, counts = SHAPES[2]
    p = random_problem(dev, M, ldc, counts, seed=5)
    runs = []
    for _ in range(3):
        s = fresh_state(p)
        glu8(p, s, act, True)
        runs.append((bits(s["c_buf"]), bits(s["cache"])))
    assert all(torch.equal(x, y) for r in runs[1:] for x, y in zip(r, runs[0]))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_problem_and_write_nothing(dev):
    M, ldc, counts = SHAPES[1]
    p = random_problem(dev, M, ldc, counts, seed=3)
    s = fresh_state(p)
    op = torch.ops.chipmunk.csp_mlp_mm1_glu_fp8
    sc = (p["ra"], p["rbg"], p["rbu"])
    bf16 = torch.bfloat16
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):      # bf16 operands: those are csp_mlp_mm1_glu's
        op(p["a"].to(bf16), p["wg"].to(bf16), p["wu"].to(bf16), s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], *sc, "silu", False)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        cut = lambda t: t[:, :192].contiguous()      # noqa: E731
        op(cut(p["a"]), cut(p["wg"]), cut(p["wu"]), s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], *sc, "silu", False)
    with pytest.raises(RuntimeError, match="one-element float32 tensors on the GPU"):      # a scale on the host
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], p["ra"].cpu(), p["rbg"], p["rbu"], "silu", False)
    with pytest.raises(RuntimeError, match="one-element float32 tensors on the GPU"):      # a scale of another dtype
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], p["ra"], p["rbg"].double(), p["rbu"], "silu", False)
    with pytest.raises(RuntimeError, match="one-element float32 tensors on the GPU"):
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], p["ra"], p["rbg"], p["rbu"].to(bf16), "silu", True)
    with pytest.raises(RuntimeError, match="unknown activation"):
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], *sc, "relu", False)
    contiguous = p["cache0"].contiguous()                    # [F, 333]: columns 666 bytes apart
    with pytest.raises(RuntimeError, match="pitch"):
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], contiguous, p["inds"], p["cnt"], *sc, "silu", True)
    assert torch.equal(bits(contiguous), bits(p["cache0"]))
    ps, batch, state = random_batch(dev, 3, M, ldc, [counts] * 3, seed=4)
    sb = state()
    with pytest.raises(RuntimeError, match="a and c must both be"):      # c of the wrong rank for a batch
        op(batch["a"], p["wg"], p["wu"], sb["c"][0], p["bg"], p["bu"], sb["cache"], batch["inds"], batch["cnt"], *sc, "silu", True)
    with pytest.raises(RuntimeError, match="batch size"):
        op(batch["a"][:2], p["wg"], p["wu"], sb["c"][:2], p["bg"], p["bu"], sb["cache"], batch["inds"][:2], batch["cnt"][:2], *sc, "silu", True)
    torch.cuda.synchronize()
    assert (s["c_buf"] == SENT).all() and (sb["c_buf"] == SENT).all(), "a refused call wrote packed deltas"
    assert torch.equal(bits(s["cache"]), bits(p["cache0"])) and (s["cache_buf"][F] == SENT).all(), "a refused call wrote the cache"
    from chipmunk_amd import ops
    with pytest.raises(ValueError, match="float8_e4m3fn operands only"):
        ops.mm1_glu_fp8(p["a"].to(bf16), p["wg"].to(bf16), p["wu"].to(bf16), s["c"], None, None, "silu", s["cache"], p["inds"], p["cnt"], *sc)
