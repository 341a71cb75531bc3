"""The weight-only fp8 GEMM2 ``chipmunk::csp_mlp_mm2_w8``: for bf16 packed deltas a, e4m3 rows of fc2^T and the weight's reciprocal scale s
c[m, :] = bf16(bf16((sum_{j < counts[g]} a[m, j] f(W[idx[g, j], :])) s) + c[m, :]) ("fp8 fc2").  F = 1024.

1. bits: with s a power of two the result IS ``csp_mlp_mm2`` on ``W.to(bf16) * s`` from the same c -- f is exact, the k placement is
   mm2_kernel's, and a power of two commutes with every rounding.  A condition, not a tolerance; the weights are random bytes in which
   every finite e4m3 value occurs among the gathered rows, so a wrong lane, column or byte order of the transpose path cannot hide;
2. masking: NaN in the packed columns at and past the counts, count-0 groups, a canary behind row M;
3. a general scale (an F8Linear-made weight) against fp64 under two bf16 roundings plus the fp32 accumulation;
4. run to run, ``ops.run_e2e`` with the scatter fused into GEMM1 or not, refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BM = 128
F = 1024
F8 = torch.float8_e4m3fn
SENT = 7.0
# M -> N2 -> counts per group, every value of {0, 8, 72, 256, 1000, F} in use; each case gathers at least 256 rows in some group
COUNTS = {
    256: {16: [F, 0], 256: [72, 1000], 400: [256, 8]},
    200: {16: [1000, 72], 256: [0, F], 400: [8, 256]},
    129: {16: [256, 8], 256: [F, 1000], 400: [72, F]},
    1: {16: [1000], 256: [F], 400: [256]},
}
CASES = [(m, n2) for m in COUNTS for n2 in COUNTS[m]]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def finite_e4m3_bytes(dev):
    b = torch.arange(256, device=dev, dtype=torch.uint8)
    return b[(b & 0x7F) != 0x7F]          # 0x7f / 0xff are the two NaNs of float8_e4m3fn


_problems = {}


def problem(dev, M, N2, counts, seed, nan_past_counts=True, cover=True):
    """a [M, F] random bf16 with NaN in the packed columns at and past each group's count, W [F, N2] random finite e4m3 bytes,
    idx randomly permuted rows, c0 random bf16.  Shared between the tests and never written.  `cover`: every finite e4m3 byte value
    occurs among the gathered rows (asserted)."""
    key = (M, N2, tuple(counts), seed, nan_past_counts)
    if key in _problems:
        return _problems[key]
    g = torch.Generator(device=dev).manual_seed(seed)
    G = (M + BM - 1) // BM
    assert len(counts) == G
    a = torch.randn(M, F, device=dev, generator=g).to(torch.bfloat16)
    fin = finite_e4m3_bytes(dev)
    w = fin[torch.randint(0, fin.numel(), (F, N2), device=dev, generator=g)].view(F8)
    idx = torch.stack([torch.randperm(F, device=dev, generator=g) for _ in range(G)]).to(torch.int32)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    if nan_past_counts:
        for gi, n in enumerate(counts):
            a[gi * BM:(gi + 1) * BM, n:] = float("nan")
    c0 = torch.randn(M, N2, device=dev, generator=g).to(torch.bfloat16)
    gathered = torch.cat([w.view(torch.uint8)[idx[gi, :n].long()].flatten() for gi, n in enumerate(counts)])
    assert not cover or torch.unique(gathered).numel() == 254, "every finite e4m3 byte value must occur among the gathered rows"
    p = dict(M=M, N2=N2, G=G, counts=counts, a=a, w=w, idx=idx, cnt=cnt, c0=c0)
    _problems[key] = p
    return p


def fresh_c(p):
    """c0 as the [:M] view of a buffer with 128 canary rows behind it"""
    buf = torch.full((p["M"] + BM, p["N2"]), SENT, dtype=torch.bfloat16, device=p["c0"].device)
    buf[: p["M"]] = p["c0"]
    return buf, buf[: p["M"]]


def scale_t(dev, s):
    return torch.tensor([s], dtype=torch.float32, device=dev)


def w8(a, w, s, idx, cnt, c):
    torch.ops.chipmunk.csp_mlp_mm2_w8(a, w, s, idx, cnt, c)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3], ids=["scale 1", "scale 2^-3"])
@pytest.mark.parametrize("M,N2", CASES, ids=[f"M{m}-N{n}" for m, n in CASES])
def test_bits_of_the_bf16_gemm2_on_the_widened_weights(dev, M, N2, scale):
    p = problem(dev, M, N2, COUNTS[M][N2], seed=M * 1000 + N2)
    w16 = p["w"].to(torch.bfloat16) * scale
    assert w16.dtype == torch.bfloat16 and torch.equal(w16.double(), p["w"].double() * scale), "the widened, scaled weights are exact in bf16"
    ref_buf, ref = fresh_c(p)
    torch.ops.chipmunk.csp_mlp_mm2(p["a"], w16, p["idx"], p["cnt"], ref)
    got_buf, got = fresh_c(p)
    w8(p["a"], p["w"], scale_t(dev, scale), p["idx"], p["cnt"], got)
    assert (got_buf[M:] == SENT).all(), "rows at or past M were written"
    assert not torch.isnan(got.float()).any(), "a packed column at or past its group's count reached the sum"
    bad = (bits(got) != bits(ref)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ from csp_mlp_mm2 on the widened weights, the first at {bad[0].tolist()}"
    for gi, n in enumerate(p["counts"]):
        rows = slice(gi * BM, min(M, (gi + 1) * BM))
        assert (n == 0) == torch.equal(bits(got[rows]), bits(p["c0"][rows])), f"group {gi} with count {n}"


def test_batch_of_two_equals_two_calls_on_the_slices(dev):
    M, N2 = 200, 400
    ps = [problem(dev, M, N2, [8, 256], seed=200400), problem(dev, M, N2, [1000, 0], seed=77)]
    w, s = ps[0]["w"], scale_t(dev, 2.0 ** -3)
    a, idx, cnt = (torch.stack([q[k] for q in ps]) for k in ("a", "idx", "cnt"))
    c0 = torch.stack([q["c0"] for q in ps])
    buf = torch.full((2 * M + BM, N2), SENT, dtype=torch.bfloat16, device=dev)
    got = buf[: 2 * M].view(2, M, N2)
    got.copy_(c0)
    w8(a, w, s, idx, cnt, got)
    ref = c0.clone()
    for b in range(2):
        w8(a[b], w, s, idx[b], cnt[b], ref[b])
    assert torch.equal(bits(got), bits(ref)), "the batch differs from the per-sequence launches"
    assert (buf[2 * M:] == SENT).all()
    ref16 = c0.clone()
    torch.ops.chipmunk.csp_mlp_mm2(a, w.to(torch.bfloat16) * 2.0 ** -3, idx, cnt, ref16)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(ref16)), "the batch differs from the batched csp_mlp_mm2 on the widened weights"
    assert torch.equal(bits(got[1, BM:]), bits(c0[1, BM:])) and not torch.equal(bits(got[0, BM:]), bits(c0[0, BM:])), \
        "each sequence goes by its own counts"


# ------------------------------------------------------------------------------------------------ 2. masking
def test_columns_past_the_counts_count_zero_groups_and_rows_past_m(dev):
    M, N2, counts = 200, 256, [72, 0]
    p = problem(dev, M, N2, counts, seed=5, nan_past_counts=False, cover=False)        # (72 gathered rows: the byte coverage is the bits tests')
    s = scale_t(dev, 0.75)
    clean = p["a"].clone()
    clean[:BM, 72:] = 0
    clean[BM:] = 0
    nan = p["a"].clone()
    nan[:BM, 72:] = float("nan")
    nan[BM:] = float("nan")
    want_buf, want = fresh_c(p)
    w8(clean, p["w"], s, p["idx"], p["cnt"], want)
    got_buf, got = fresh_c(p)
    w8(nan, p["w"], s, p["idx"], p["cnt"], got)
    assert torch.equal(bits(got), bits(want)), "NaN in packed columns at or past the counts changed the result"
    assert torch.equal(bits(got[BM:]), bits(p["c0"][BM:])), "a count-0 group's rows of mma_c changed"
    assert not torch.equal(bits(got[:BM]), bits(p["c0"][:BM]))
    assert (got_buf[M:] == SENT).all() and (want_buf[M:] == SENT).all(), "rows past M of the larger allocation were written"


# ------------------------------------------------------------------------------------------------ 3. a general scale
def test_f8linear_weight_and_scale_against_fp64(dev):
    """t = (a @ f(W)[idx]) * s in fp64; |got - (t + c)| <= 2^-8 (|t| + |t + c|) + 2^-20 s sum|a w|: the two bf16 roundings at twice
    their half-ulp (2^-9 relative each) and the fp32 accumulation of 1024 products."""
    from chipmunk_amd.modules.mlp_fp8 import F8Linear
    M, N2, counts = 200, 400, [1000, 72]
    g = torch.Generator(device=dev).manual_seed(11)
    lin = torch.nn.Linear(F, N2, bias=False, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N2, F, device=dev, generator=g) * 0.03)
    f8 = F8Linear.from_linear(lin, input_float8_dtype=F8)
    assert f8.weight.dtype == F8
    wT, s = f8.weight.data.T.contiguous(), f8.scale_reciprocal.reshape(1).float()
    a = torch.randn(M, F, device=dev, generator=g).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(F, device=dev, generator=g) for _ in range(2)]).to(torch.int32)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    c0 = torch.randn(M, N2, device=dev, generator=g).to(torch.bfloat16)
    got = c0.clone()
    w8(a, wT, s, idx, cnt, got)
    worst = 0.0
    for gi, n in enumerate(counts):
        rows = slice(gi * BM, min(M, (gi + 1) * BM))
        ad, wd = a[rows, :n].double(), wT.double()[idx[gi, :n].long()]
        t = (ad @ wd) * s.double()
        bound = 2.0 ** -8 * (t.abs() + (t + c0[rows].double()).abs()) + 2.0 ** -20 * s.double() * (ad.abs() @ wd.abs())
        err = (got[rows].double() - (t + c0[rows].double())).abs()
        worst = max(worst, float((err / bound).max()))
        print(f"group {gi}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), f"group {gi}: {int((err > bound).sum())} elements outside the bound, worst {float((err / bound).max()):.3f} x"
    assert worst > 0.0


# ------------------------------------------------------------------------------------------------ 4. other conditions
def test_two_launches_give_identical_bits(dev):
    M, N2 = 256, 400
    p = problem(dev, M, N2, COUNTS[M][N2], seed=M * 1000 + N2)
    outs = []
    for _ in range(2):
        _, c = fresh_c(p)
        w8(p["a"], p["w"], scale_t(dev, 0.3), p["idx"], p["cnt"], c)
        outs.append(bits(c))
    assert torch.equal(outs[0], outs[1])


def test_run_e2e_with_the_scatter_fused_or_not_gives_identical_bits(dev, fresh_config):
    from chipmunk_amd.ops.mlp import run_e2e
    M, K1, N2, counts = 200, 256, 400, [256, 1000]
    p = problem(dev, M, N2, counts, seed=31)
    g = torch.Generator(device=dev).manual_seed(32)
    x = torch.randn(M, K1, device=dev, generator=g).to(torch.bfloat16)
    fc1w = (torch.randn(F, K1, device=dev, generator=g) * 0.06).to(torch.bfloat16)
    fc1b = (torch.randn(F, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    cache0 = (torch.randn(F, M, device=dev, generator=g) * 0.3).to(torch.bfloat16)
    s = scale_t(dev, 0.01)
    res = []
    for fused in (True, False):
        fresh_config["mlp"]["fused_scatter"] = fused
        cache, (_, out) = cache0.clone(), fresh_c(p)
        run_e2e(x, fc1w, fc1b, p["w"], p["idx"], p["cnt"], cache, out, 6, fc2_scale=s)
        torch.cuda.synchronize()
        res.append((bits(out), bits(cache)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], bits(p["c0"])) and not torch.equal(res[0][1], bits(cache0))
    with pytest.raises(ValueError, match="fc2_scale"):
        run_e2e(x, fc1w, fc1b, p["w"], p["idx"], p["cnt"], cache0.clone(), fresh_c(p)[1], 6)


def test_refusals_name_the_problem_and_write_nothing(dev):
    from chipmunk_amd.ops.mlp import csp_mlp_mm2
    M, N2 = 200, 400
    p = problem(dev, M, N2, COUNTS[M][N2], seed=M * 1000 + N2)
    buf, c = fresh_c(p)
    op, s = torch.ops.chipmunk.csp_mlp_mm2_w8, scale_t(dev, 0.5)
    with pytest.raises(RuntimeError, match="mma_b must be float8_e4m3fn"):
        op(p["a"], p["w"].to(torch.bfloat16), s, p["idx"], p["cnt"], c)
    with pytest.raises(RuntimeError, match="mma_b must be float8_e4m3fn"):
        op(p["a"], p["w"].view(torch.float8_e5m2), s, p["idx"], p["cnt"], c)
    for bad in (s.cpu(), s.double(), torch.ones(2, device=dev)):
        with pytest.raises(RuntimeError, match="scale_b must be a one-element float32 tensor on the GPU"):
            op(p["a"], p["w"], bad, p["idx"], p["cnt"], c)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        op(p["a"], p["w"][:512].contiguous(), s, p["idx"], p["cnt"], c)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        op(p["a"], p["w"], s, p["idx"], p["cnt"], c[:, :256].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 16"):
        op(p["a"], p["w"][:, :24].contiguous(), s, p["idx"], p["cnt"], c[:, :24].contiguous())
    a2, c2 = torch.stack([p["a"], p["a"]]), torch.stack([c, c])
    with pytest.raises(RuntimeError, match="batch size of mma_a"):      # index lists of one sequence for a batch of two
        op(a2, p["w"], s, p["idx"], p["cnt"], c2)
    with pytest.raises(RuntimeError, match="2D .* or 3D"):
        op(a2, p["w"], s, p["idx"], p["cnt"], c)
    with pytest.raises(ValueError, match="fc2_scale"):
        csp_mlp_mm2(p["a"], p["w"], p["idx"], p["cnt"], c)
    torch.cuda.synchronize()
    assert torch.equal(bits(c), bits(p["c0"])) and (buf[M:] == SENT).all(), "a refused call wrote mma_c"
