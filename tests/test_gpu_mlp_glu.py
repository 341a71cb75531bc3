"""The gated GEMM1 operator ``chipmunk::csp_mlp_mm1_glu``: c = bf16(act(a Wg^T + bg) * (a Wu^T + bu) - cache) on the kept columns, optionally
followed by the scatter-add of c into the cache ("Gated MLPs").  K = 256, F = 512.

Problem generator, NaN slack rows behind a, the sentinel 7.0 in everything the operator must not write and the canary row behind the cache
are those of tests/test_gpu_mlp_ragged.py.  Shapes: a one-row last group under a pitch wider than ceil8(M); counts of 0 and F; partial
64-column tiles (208, 16, 40, 272) and a count that ends inside an 8-column store (40); eight groups.

1. the up branch as the constant 1 (W_up = 0, bias_up = 1) under tanh-GELU: the BITS of the ungated kernel, with and without the scatter;
2. every group against fp32 torch for the three activations and the four bias combinations, independent random W_gate / W_up;
   and exact GELU against tanh-GELU by projection on their difference (the tolerance cannot tell them apart);
3. the fused scatter = update off followed by csp_scatter_add; 4. a batch = its slices; 5. run to run; 6. refusals."""
import pytest
import torch

from helpers import assert_close_bf16

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


def make_problem(dev, M, ldc, counts, seed, k=K, f=F):
    G = (M + BM - 1) // BM
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape, scale: (torch.randn(*shape, device=dev, generator=g) * scale).to(torch.bfloat16)   # noqa: E731
    p = {"M": M, "G": G, "ldc": ldc, "counts": counts, "f": f}
    a = rnd(M, k, scale=0.5)
    p["wg"], p["wu"] = rnd(f, k, scale=0.06), rnd(f, k, scale=0.06)
    p["bg"], p["bu"] = rnd(f, scale=0.1), rnd(f, scale=0.1)
    p["cache0"] = rnd(f, M, scale=0.3)
    p["inds"] = torch.stack([torch.randperm(f, device=dev, generator=g) for _ in range(G)]).to(torch.int32)
    p["cnt"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    p["a_buf"], p["a"] = with_slack(a, float("nan"))
    return p


def fresh_state(p):
    """Mutable tensors of one launch: c (packed deltas out) and the cache, as views of buffers with canaries."""
    dev, M, f, ldc = p["cache0"].device, p["M"], p["f"], p["ldc"]
    cache_buf = torch.full((f + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)      # padding [M, ldc) = NaN
    cache_buf[f] = SENT                                                                           # the canary row
    cache_buf[:f, :M] = p["cache0"]
    c_buf, c = with_slack(torch.full((M, f), SENT, dtype=torch.bfloat16, device=dev), SENT)
    return dict(c=c, c_buf=c_buf, cache=cache_buf[:f, :M], cache_buf=cache_buf)


def glu(p, s, act, update, bg="bg", bu="bu", wu="wu"):
    torch.ops.chipmunk.csp_mlp_mm1_glu(p["a"], p["wg"], p[wu], s["c"], p[bg] if bg else None, p[bu] if bu else None, s["cache"],
                                       p["inds"], p["cnt"], act, update)
    torch.cuda.synchronize()


def check_canaries(p, s, what):
    M, f = p["M"], p["f"]
    assert (s["c_buf"][M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    assert (s["cache_buf"][f] == SENT).all(), f"{what}: the row behind the cache's F * ldc elements was written"
    assert torch.isnan(p["a_buf"][M:].float()).all(), f"{what}: the input's slack rows changed"


# ------------------------------------------------------------------------------------------------ 1. the ungated kernel's bits
@pytest.mark.parametrize("update", [False, True], ids=["update off", "scatter"])
@pytest.mark.parametrize("M,ldc,counts", SHAPES, ids=IDS)
def test_constant_up_branch_gives_the_bits_of_the_ungated_kernel(dev, M, ldc, counts, update):
    """u is exactly 1.0 (0 * x + 1) and fma(gelu(g), 1, -c) rounds as gelu(g) - c: a condition, not a tolerance."""
    p = make_problem(dev, M, ldc, counts, seed=M)
    p["w0"], p["one"] = torch.zeros_like(p["wu"]), torch.ones_like(p["bu"])
    ref, got = fresh_state(p), fresh_state(p)
    ungated = torch.ops.chipmunk.csp_mlp_mm1_scatter if update else torch.ops.chipmunk.csp_mlp_mm1
    ungated(p["a"], p["wg"], ref["c"], p["bg"], ref["cache"], p["inds"], p["cnt"])
    glu(p, got, "gelu_tanh", update, bu="one", wu="w0")
    check_canaries(p, got, "gated")
    assert torch.equal(bits(got["c"]), bits(ref["c"])), "packed deltas differ from csp_mlp_mm1's"
    assert torch.equal(bits(got["cache"]), bits(ref["cache"])), "the cache differs from the ungated operator's"
    assert update or torch.equal(bits(got["cache"]), bits(p["cache0"]))


def make_batch(dev, B, M, ldc, counts_per_seq, seed):
    """B problems with shared weights as one batch: a [B, M, K], cache the [:, :F, :M] view of [B, F + 1, ldc] (a canary row behind every
    sequence, so the batch stride exceeds F * ldc), indices [B, G, F], counts [B, G]."""
    ps = [make_problem(dev, M, ldc, counts_per_seq[b], seed + b) for b in range(B)]
    for q in ps[1:]:
        for name in ("wg", "wu", "bg", "bu"):
            q[name] = ps[0][name]
    batch = dict(a=torch.stack([q["a"] for q in ps]), inds=torch.stack([q["inds"] for q in ps]), cnt=torch.stack([q["cnt"] for q in ps]))

    def state():
        cache_buf = torch.full((B, F + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
        cache_buf[:, F] = SENT
        for b, q in enumerate(ps):
            cache_buf[b, :F, :M] = q["cache0"]
        c_buf = torch.full((B * M + BM, F), SENT, dtype=torch.bfloat16, device=dev)
        return dict(c=c_buf[: B * M].view(B, M, F), c_buf=c_buf, cache=cache_buf[:, :F, :M], cache_buf=cache_buf)
    return ps, batch, state


def test_constant_up_branch_batch_of_two_gives_the_bits_of_the_ungated_batch(dev):
    M, ldc, counts = SHAPES[1]
    ps, batch, state = make_batch(dev, 2, M, ldc, [counts, [336, F, 0]], seed=11)
    p = ps[0]
    ref, got = state(), state()
    torch.ops.chipmunk.csp_mlp_mm1(batch["a"], p["wg"], ref["c"], p["bg"], ref["cache"], batch["inds"], batch["cnt"])
    torch.ops.chipmunk.csp_mlp_mm1_glu(batch["a"], p["wg"], torch.zeros_like(p["wu"]), got["c"], p["bg"], torch.ones_like(p["bu"]),
                                       got["cache"], batch["inds"], batch["cnt"], "gelu_tanh", False)
    torch.cuda.synchronize()
    assert torch.equal(bits(got["c_buf"]), bits(ref["c_buf"])), "packed deltas differ from csp_mlp_mm1's on the batch"
    assert torch.equal(bits(got["cache"]), bits(ref["cache"])) and (got["cache_buf"][:, F] == SENT).all()


# ------------------------------------------------------------------------------------------------ 2. fp32 torch, every group
def torch_act(act, x):
    if act == "gelu_tanh":
        return torch.nn.functional.gelu(x, approximate="tanh")
    return torch.nn.functional.silu(x) if act == "silu" else torch.nn.functional.gelu(x)


@pytest.mark.parametrize("biases", [("bg", "bu"), ("bg", None), (None, "bu"), (None, None)], ids=["both biases", "gate bias", "up bias", "no bias"])
@pytest.mark.parametrize("act", ACTS)
def test_every_group_against_fp32_torch(dev, act, biases):
    """want = act(x Wg^T + bg) * (x Wu^T + bu) - cache in fp32 under the project's bf16 GEMM1 tolerance (assert_close_bf16 defaults, as
    tests/test_gpu_mlp_ragged.py): the roundings are the fp32 accumulation order and one bf16 rounding of the result."""
    bg, bu = biases
    for (M, ldc, counts), sid in zip(SHAPES, IDS):
        p = make_problem(dev, M, ldc, counts, seed=M + 1)
        cache0 = p["cache0"]
        hg = p["a"].float() @ p["wg"].float().T + (p[bg].float() if bg else 0)
        hu = p["a"].float() @ p["wu"].float().T + (p[bu].float() if bu else 0)
        h = torch_act(act, hg) * hu                                   # [M, F], every column: shared by both update settings
        for update in (False, True):
            s = fresh_state(p)
            glu(p, s, act, update, bg=bg, bu=bu)
            what = f"{act}, {sid}, update {update}"
            check_canaries(p, s, what)
            for g in range(p["G"]):
                rows, n = slice(g * BM, min(M, (g + 1) * BM)), counts[g]
                cols, rest = p["inds"][g, :n].long(), p["inds"][g, n:].long()
                assert (s["c"][rows, n:] == SENT).all(), f"{what}: group {g}: packed columns past the count written"
                if n:
                    want = h[rows][:, cols] - cache0[cols][:, rows].float().T
                    assert_close_bf16(s["c"][rows, :n], want, what=f"{what}: group {g} vs fp32 torch")
                if update:
                    new = (cache0[cols][:, rows].float() + s["c"][rows, :n].float().T).to(torch.bfloat16)
                    assert torch.equal(s["cache"][cols][:, rows], new), f"{what}: group {g}: cache != bf16(cache + delta)"
                    assert torch.equal(s["cache"][rest][:, rows], cache0[rest][:, rows]), f"{what}: group {g}: unselected cache columns changed"
            if not update:
                assert torch.equal(bits(s["cache"]), bits(cache0)), f"{what}: the cache was written"


def gelu_projection(got, want_tanh, want_erf):
    """sum((got - want_tanh) * d) / sum(d * d) with d = want_erf - want_tanh: 0 for a tanh-GELU result and 1 for an exact-GELU one, up to
    the bf16 rounding of `got`, which averages out over the elements (170 000 here, zero cache: +- 0.06 on the CPU mirror over three
    seeds; the test allows 0.25, half the way to the point 0.5 where the two could no longer be told apart)"""
    d = (want_erf - want_tanh).double()
    return float(((got.double() - want_tanh.double()) * d).sum() / (d * d).sum())


def test_exact_gelu_and_tanh_gelu_are_told_apart(dev):
    """The two differ by 5e-4 at most, far inside the tolerance above: a "gelu" that ran the tanh code (or the reverse) would pass there.
    Projected on the difference of the two fp32 references, each kernel's output lies at its own end."""
    M, ldc, _ = SHAPES[1]
    p = make_problem(dev, M, ldc, [F, F, F], seed=9)
    p["cache0"] = torch.zeros_like(p["cache0"])          # the result is the product itself: less rounding noise under the projection
    hg = p["a"].float() @ p["wg"].float().T + p["bg"].float()
    hu = p["a"].float() @ p["wu"].float().T + p["bu"].float()
    want = {act: torch_act(act, hg) * hu - p["cache0"].float().T for act in ("gelu_tanh", "gelu")}
    unperm = torch.stack([torch.argsort(p["inds"][g].long()) for g in range(p["G"])])     # packed position of every column
    rows_g = torch.arange(M, device=dev) // BM
    got = {}
    for act in ("gelu_tanh", "gelu"):
        s = fresh_state(p)
        glu(p, s, act, False)
        got[act] = torch.gather(s["c"].float(), 1, unperm[rows_g])                         # [M, F] in column order
    assert not torch.equal(got["gelu"], got["gelu_tanh"]), "exact GELU and tanh-GELU gave the same bits"
    at_tanh, at_erf = (gelu_projection(got[act], want["gelu_tanh"], want["gelu"]) for act in ("gelu_tanh", "gelu"))
    print(f"projection on (exact - tanh): tanh-GELU kernel {at_tanh:.3f}, exact-GELU kernel {at_erf:.3f}")
    assert abs(at_tanh) < 0.25 and abs(at_erf - 1.0) < 0.25


# ------------------------------------------------------------------------------------------------ 3. - 5.
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,ldc,counts", SHAPES, ids=IDS)
def test_fused_scatter_equals_the_unfused_sequence(dev, M, ldc, counts, act):
    p = make_problem(dev, M, ldc, counts, seed=M + 2)
    fused, two = fresh_state(p), fresh_state(p)
    glu(p, fused, act, True)
    glu(p, two, act, False)
    torch.ops.chipmunk.csp_scatter_add(two["c"].unsqueeze(0), two["cache"].unsqueeze(0), p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0), 6)
    torch.cuda.synchronize()
    assert torch.equal(bits(fused["c"]), bits(two["c"])), "packed deltas differ"
    assert torch.equal(bits(fused["cache"]), bits(two["cache"])), "the cache differs from update off + csp_scatter_add"


@pytest.mark.parametrize("update", [False, True], ids=["update off", "scatter"])
def test_batch_of_three_equals_its_slices(dev, update):
    M, ldc, _ = SHAPES[1]
    ps, batch, state = make_batch(dev, 3, M, ldc, [[F, 0, 336], [0, 0, 0], [64, 272, F]], seed=21)
    p = ps[0]
    got, ref = state(), state()
    assert got["cache"].stride(0) > F * ldc
    torch.ops.chipmunk.csp_mlp_mm1_glu(batch["a"], p["wg"], p["wu"], got["c"], p["bg"], None, got["cache"], batch["inds"], batch["cnt"],
                                       "silu", update)
    for b in range(3):
        torch.ops.chipmunk.csp_mlp_mm1_glu(batch["a"][b], p["wg"], p["wu"], ref["c"][b], p["bg"], None, ref["cache"][b], batch["inds"][b],
                                           batch["cnt"][b], "silu", update)
    torch.cuda.synchronize()
    assert torch.equal(bits(got["c_buf"]), bits(ref["c_buf"])), "packed deltas of the batch differ from the per-sequence launches'"
    assert torch.equal(bits(got["cache"]), bits(ref["cache"])), "the cache of the batch differs from the per-sequence launches'"
    assert (got["cache_buf"][:, F] == SENT).all() and (got["c"][1] == SENT).all(), "a canary row or the all-zero sequence was written"
    assert not (got["c"][2][:BM, :64] == SENT).any()


@pytest.mark.parametrize("act", ACTS)
def test_three_launches_from_the_same_state_give_the_same_bits(dev, act):
    M, ldc, counts = SHAPES[2]
    p = make_problem(dev, M, ldc, counts, seed=5)
    runs = []
    for _ in range(3):
        s = fresh_state(p)
        glu(p, s, act, True)
        runs.append((bits(s["c_buf"]), bits(s["cache"])))
    assert all(torch.equal(x, y) for r in runs[1:] for x, y in zip(r, runs[0]))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_problem_and_write_nothing(dev):
    M, ldc, counts = SHAPES[1]
    p = make_problem(dev, M, ldc, counts, seed=3)
    s = fresh_state(p)
    op = torch.ops.chipmunk.csp_mlp_mm1_glu
    f8 = torch.float8_e4m3fn
    with pytest.raises(RuntimeError, match="bfloat16"):      # fp8 operands: there is no fp8 gated form
        op(p["a"].to(f8), p["wg"].to(f8), p["wu"].to(f8), s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], "silu", False)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        op(p["a"][:, :96].contiguous(), p["wg"][:, :96].contiguous(), p["wu"][:, :96].contiguous(), s["c"], p["bg"], p["bu"], s["cache"],
           p["inds"], p["cnt"], "silu", False)
    with pytest.raises(RuntimeError, match="unknown activation"):
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], s["cache"], p["inds"], p["cnt"], "relu", False)
    contiguous = p["cache0"].contiguous()                    # [F, 333]: columns 666 bytes apart
    with pytest.raises(RuntimeError, match="pitch"):
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"], contiguous, p["inds"], p["cnt"], "silu", True)
    assert torch.equal(bits(contiguous), bits(p["cache0"]))
    ps, batch, state = make_batch(dev, 3, M, ldc, [counts] * 3, seed=4)
    sb = state()
    with pytest.raises(RuntimeError, match="batch size"):
        op(batch["a"][:2], p["wg"], p["wu"], sb["c"][:2], p["bg"], p["bu"], sb["cache"], batch["inds"][:2], batch["cnt"][:2], "silu", True)
    with pytest.raises(RuntimeError, match="batch size"):
        op(batch["a"], p["wg"], p["wu"], sb["c"], p["bg"], p["bu"], sb["cache"], batch["inds"][:2], batch["cnt"][:2], "silu", True)
    with pytest.raises(RuntimeError, match="bias_up must have F entries"):
        op(p["a"], p["wg"], p["wu"], s["c"], p["bg"], p["bu"][: F // 2], s["cache"], p["inds"], p["cnt"], "silu", True)
    with pytest.raises(RuntimeError, match="bias_gate must have F entries"):
        op(p["a"], p["wg"], p["wu"], s["c"], torch.cat([p["bg"], p["bg"]]), None, s["cache"], p["inds"], p["cnt"], "silu", True)
    torch.cuda.synchronize()
    assert (s["c_buf"] == SENT).all() and (sb["c_buf"] == SENT).all(), "a refused call wrote packed deltas"
    assert torch.equal(bits(s["cache"]), bits(p["cache0"])) and (s["cache_buf"][F] == SENT).all(), "a refused call wrote the cache"
    from chipmunk_amd import ops
    with pytest.raises(ValueError, match="bf16 operands only"):
        ops.mm1_glu(p["a"].to(f8), p["wg"].to(f8), p["wu"].to(f8), s["c"], None, None, "silu", s["cache"], p["inds"], p["cnt"])
