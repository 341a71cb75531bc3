"""The sparse-MLP operators at token counts that are not a multiple of 128 ("Ragged M"): G = ceil(M / 128) groups, the last one
short; row-major tensors hold exactly M rows, the column-major activation cache is [F, ldc] with ldc >= M, ldc % 8 == 0.

Two references, both independent of the ragged code path:
  * today's operator on the ZERO-PADDED problem (M rounded up to whole groups, a contiguous [F, Mp] cache), sliced back to M rows: the
    ragged launch must give the same BITS on every row < M and every cache element [:, :M];
  * fp32 torch on the last group, under the tolerances the existing tests use for the same operator (tests/test_gpu_mlp.py,
    tests/test_gpu_mlp_bench_shape.py): defaults for bf16 GEMM1 and GEMM2, atol = rtol = 3e-2 for fp8.
Canaries: the row-major outputs are [:M] views of buffers with 128 sentinel rows behind them, the cache is the [:F] view of an
[F + 1, ldc] buffer (its last row must not change), the slack rows behind a / packed / mma_a hold NaN and the cache padding [M, ldc) holds
NaN as well: nothing of that may reach a valid output.  Every operator is launched ten times from the same state: same bits each time."""
import pytest
import torch

from helpers import assert_close_bf16

pytestmark = pytest.mark.gpu

BM = 128
K, F, N2 = 256, 512, 256
SENT = 7.0
# (M, ldc, counts per group): last groups of 1, 72, 40, 104 and 77 rows; ldc == M where M % 8 == 0, a pitch elsewhere (one of them wider
# than ceil8(M)); counts ragged per group with a 0 and a full F in every list
SHAPES = [
    (129, 144, [0, F]),
    (200, 200, [F, 208]),
    (296, 296, [208, 0, F]),
    (1000, 1000, [F, 0, 208, 16, 336, 512, 64, 272]),
    (333, 336, [F, 0, 336]),
]
OPS = ["mm1", "mm1_scatter", "fp8_upd0", "fp8_upd1", "fp8_scatter", "scatter_add", "mm2", "mm2_and_scatter_add"]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int8)


def with_slack(rows, fill):
    """[M, C] tensor -> its copy as the [:M] view of a [M + 128, C] buffer whose slack rows hold `fill` (returns buffer, view)."""
    buf = torch.full((rows.shape[0] + BM, rows.shape[1]), fill, dtype=torch.float32, device=rows.device).to(rows.dtype)
    buf[: rows.shape[0]] = rows
    return buf, buf[: rows.shape[0]]


def make_problem(dev, M, ldc, counts, fp8, seed, k=K, f=F, n2=N2):
    """The ragged problem (views with canaries / NaN slack) and its zero-padded twin (plain contiguous tensors)."""
    G = (M + BM - 1) // BM
    Mp = G * BM
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, k, device=dev, generator=g) * 0.5
    w = torch.randn(f, k, device=dev, generator=g) * 0.06
    p = {"M": M, "Mp": Mp, "G": G, "ldc": ldc, "counts": counts, "fp8": fp8, "f": f}
    if fp8:
        sa, sb = 448.0 / x.abs().max(), 448.0 / w.abs().max()
        a, p["w1"] = (x * sa).to(torch.float8_e4m3fn), (w * sb).to(torch.float8_e4m3fn)
        p["ra"], p["rb"] = (1.0 / sa).reshape(1).float(), (1.0 / sb).reshape(1).float()
    else:
        a, p["w1"] = x.to(torch.bfloat16), w.to(torch.bfloat16)
    p["bias"] = (torch.randn(f, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    cache = (torch.randn(f, M, device=dev, generator=g) * 0.3).to(torch.bfloat16)
    packed = (torch.randn(M, f, device=dev, generator=g) * 0.2).to(torch.bfloat16)       # input of scatter-add / GEMM2
    p["w2T"] = (torch.randn(f, n2, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    out = (torch.randn(M, n2, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    p["inds"] = torch.stack([torch.randperm(f, device=dev, generator=g) for _ in range(G)]).to(torch.int32)
    p["cnt"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    p["a_buf"], p["a"] = with_slack(a, float("nan"))
    p["packed_buf"], p["packed"] = with_slack(packed, float("nan"))
    p["cache0"], p["out0"] = cache, out
    # padded twin
    p["a_pad"] = torch.zeros(Mp, k, dtype=a.dtype, device=dev)
    p["a_pad"][:M] = a
    p["packed_pad"] = torch.zeros(Mp, f, dtype=torch.bfloat16, device=dev)
    p["packed_pad"][:M] = packed
    return p


def fresh_state(p, padded):
    """Mutable tensors of one launch: c (packed deltas out), cache, mma_c."""
    dev, M, Mp, f = p["cache0"].device, p["M"], p["Mp"], p["f"]
    if padded:
        cache = torch.zeros(f, Mp, dtype=torch.bfloat16, device=dev)
        cache[:, :M] = p["cache0"]
        out = torch.zeros(Mp, p["out0"].shape[1], dtype=torch.bfloat16, device=dev)
        out[:M] = p["out0"]
        return dict(c=torch.full((Mp, f), SENT, dtype=torch.bfloat16, device=dev), cache=cache, out=out)
    ldc = p["ldc"]
    cache_buf = torch.full((f + 1, ldc), float("nan"), dtype=torch.bfloat16, device=dev)      # padding [M, ldc) = NaN
    cache_buf[f] = SENT                                                                           # the canary row
    cache_buf[:f, :M] = p["cache0"]
    c_buf, c = with_slack(torch.full((M, f), SENT, dtype=torch.bfloat16, device=dev), SENT)
    out_buf, out = with_slack(p["out0"].clone(), SENT)
    return dict(c=c, c_buf=c_buf, cache=cache_buf[:f, :M], cache_buf=cache_buf, out=out, out_buf=out_buf)


def launch(op, p, s, padded):
    ops = torch.ops.chipmunk
    a = p["a_pad"] if padded else p["a"]
    packed = p["packed_pad"] if padded else p["packed"]
    inds, cnt = p["inds"], p["cnt"]
    if op == "mm1":
        ops.csp_mlp_mm1(a, p["w1"], s["c"], p["bias"], s["cache"], inds, cnt)
    elif op == "mm1_scatter":
        ops.csp_mlp_mm1_scatter(a, p["w1"], s["c"], p["bias"], s["cache"], inds, cnt)
    elif op in ("fp8_upd0", "fp8_upd1"):
        ops.csp_mlp_mm1_fp8(a, p["w1"], s["c"], p["bias"], s["cache"], inds, cnt, p["ra"], p["rb"], op == "fp8_upd1")
    elif op == "fp8_scatter":
        ops.csp_mlp_mm1_fp8_scatter(a, p["w1"], s["c"], p["bias"], s["cache"], inds, cnt, p["ra"], p["rb"])
    elif op == "scatter_add":
        ops.csp_scatter_add(packed.unsqueeze(0), s["cache"].unsqueeze(0), inds.unsqueeze(0), cnt.unsqueeze(0), 6)
    elif op == "mm2":
        ops.csp_mlp_mm2(packed, p["w2T"], inds, cnt, s["out"])
    elif op == "mm2_and_scatter_add":
        ops.csp_mlp_mm2_and_scatter_add(packed.unsqueeze(0), s["cache"].unsqueeze(0), inds.unsqueeze(0), cnt.unsqueeze(0),
                                        packed.unsqueeze(0), p["w2T"].unsqueeze(0), s["out"].unsqueeze(0), 6, 0)
    else:
        raise ValueError(op)
    torch.cuda.synchronize()


def check_canaries(p, s, what):
    M, f = p["M"], p["f"]
    assert (s["c_buf"][M:] == SENT).all(), f"{what}: rows at or past M of the packed deltas were written"
    assert (s["out_buf"][M:] == SENT).all(), f"{what}: rows at or past M of mma_c were written"
    assert (s["cache_buf"][f] == SENT).all(), f"{what}: the row behind the cache's F * ldc elements was written"
    assert torch.isnan(p["a_buf"][M:].float()).all() and torch.isnan(p["packed_buf"][M:].float()).all(), f"{what}: an input's slack rows changed"


def last_group_vs_torch(op, p, s, what):
    """fp32 torch on the last group (its rows, its index list)."""
    M, G, f = p["M"], p["G"], p["f"]
    g = G - 1
    rows = slice(g * BM, M)
    n = p["counts"][g]
    cols, rest = p["inds"][g, :n].long(), p["inds"][g, n:].long()
    cache0 = p["cache0"]
    if op in ("mm1", "mm1_scatter", "fp8_upd0", "fp8_upd1", "fp8_scatter"):
        assert (s["c"][rows, n:] == SENT).all(), f"{what}: packed columns past the count written"
        if p["fp8"]:
            acc = (p["a"][rows].float() @ p["w1"][cols].float().T) * p["ra"] * p["rb"] + p["bias"][cols].float()
            act = torch.nn.functional.gelu(acc, approximate="tanh").to(torch.bfloat16)
            want = (act.float() - cache0[cols][:, rows].float().T).to(torch.bfloat16)
            tol = dict(atol=3e-2, rtol=3e-2)
        else:
            act = torch.nn.functional.gelu(p["a"][rows].float() @ p["w1"][cols].float().T + p["bias"][cols].float(), approximate="tanh")
            want = act - cache0[cols][:, rows].float().T
            tol = {}
        if n:
            assert_close_bf16(s["c"][rows, :n], want, what=f"{what}: last group's deltas vs fp32 torch", **tol)
        if op in ("mm1", "fp8_upd0"):
            assert torch.equal(bits(s["cache"]), bits(cache0)), f"{what}: the cache was written"
        elif op == "fp8_upd1":
            if n:
                assert_close_bf16(s["cache"][cols][:, rows], act.T, what=f"{what}: last group's cache = new activation", **tol)
        else:
            new = (cache0[cols][:, rows].float() + s["c"][rows, :n].float().T).to(torch.bfloat16)
            assert torch.equal(s["cache"][cols][:, rows], new), f"{what}: last group's cache != bf16(cache + delta)"
        if op != "mm1" and op != "fp8_upd0":
            assert torch.equal(s["cache"][rest][:, rows], cache0[rest][:, rows]), f"{what}: unselected cache columns changed"
    if op in ("scatter_add", "mm2_and_scatter_add"):
        new = (cache0[cols][:, rows].float() + p["packed"][rows, :n].float().T).to(torch.bfloat16)
        assert torch.equal(s["cache"][cols][:, rows], new), f"{what}: last group's cache != bf16(cache + packed)"
        assert torch.equal(s["cache"][rest][:, rows], cache0[rest][:, rows]), f"{what}: unselected cache columns changed"
    if op in ("mm2", "mm2_and_scatter_add"):
        prod = (p["packed"][rows, :n].float() @ p["w2T"][cols].float()).to(torch.bfloat16)
        assert_close_bf16(s["out"][rows], prod.float() + p["out0"][rows].float(), what=f"{what}: last group's mma_c vs fp32 torch")


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("M,ldc,counts", SHAPES, ids=[f"M{m}-ld{l}" for m, l, _ in SHAPES])
def test_ragged_operator_equals_padded_run_and_torch(dev, M, ldc, counts, op):
    fp8 = op.startswith("fp8")
    p = make_problem(dev, M, ldc, counts, fp8, seed=M)
    ref = fresh_state(p, padded=True)
    launch(op, p, ref, padded=True)
    first = None
    for rep in range(10):
        s = fresh_state(p, padded=False)
        launch(op, p, s, padded=False)
        what = f"{op} M={M} ldc={ldc} launch {rep}"
        check_canaries(p, s, what)
        got = (bits(s["c"]), bits(s["cache"]), bits(s["out"]))
        if first is None:
            first = got
            assert torch.equal(got[0], bits(ref["c"][:M])), f"{what}: packed deltas differ from the padded run's rows < M"
            assert torch.equal(got[1], bits(ref["cache"][:, :M])), f"{what}: cache[:, :M] differs from the padded run's"
            assert torch.equal(got[2], bits(ref["out"][:M])), f"{what}: mma_c differs from the padded run's rows < M"
            last_group_vs_torch(op, p, s, what)
        else:
            assert all(torch.equal(x, y) for x, y in zip(got, first)), f"{what}: not the bits of the first launch"


def test_contiguous_cache_with_m_not_a_multiple_of_8_is_refused(dev):
    p = make_problem(dev, 333, 336, [F, 0, 336], False, seed=1)
    cache = p["cache0"].contiguous()                     # [F, 333]: columns 666 bytes apart
    c = torch.zeros(333, F, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="pitch"):
        torch.ops.chipmunk.csp_mlp_mm1(p["a"], p["w1"], c, p["bias"], cache, p["inds"], p["cnt"])
    with pytest.raises(RuntimeError, match="pitch"):
        torch.ops.chipmunk.csp_scatter_add(p["packed"].unsqueeze(0), cache.unsqueeze(0), p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0), 6)


@pytest.mark.parametrize("fp8", [False, True])
def test_ragged_last_group_through_the_tail_split(dev, fp8):
    """GEMM1's tail split hands an XCD's leftover tiles out as 64 x 64 sub-tiles that carry a row offset (m_off = 0 / 64).  Shape chosen so
    that the leftover tiles of the launch are column tiles of the LAST, ragged group (M = 1000: 104 rows, the m_off = 64 sub-tiles hold 40):
    8 groups x NT live column tiles with NT = slots per XCD + 2 -> every XCD keeps 2 leftover tiles = 8 sub-tiles, and XCD 7's are the last
    group's last two column tiles.  `mm1_probe = 3` makes the kernel skip exactly its sub-tiles (tests/test_gpu_mlp_bench_shape.py): the
    sentinel they leave shows the split was taken where this test needs it."""
    from chipmunk_amd import _native
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = 2 * cus // 8
    nt = slots + 2
    f, M, k = nt * 128, 1000, 256
    counts = [2048, 0, 1024, 3072, 512, 256, 4096, f]          # the maximum (= F) sets the live column tiles; the last group keeps every column
    p = make_problem(dev, M, M, counts, fp8, seed=5, k=k, f=f)
    ref = fresh_state(p, padded=True)
    op = "fp8_scatter" if fp8 else "mm1_scatter"
    launch(op, p, ref, padded=True)
    s = fresh_state(p, padded=False)
    launch(op, p, s, padded=False)
    check_canaries(p, s, op)
    assert torch.equal(bits(s["c"]), bits(ref["c"][:M])) and torch.equal(bits(s["cache"]), bits(ref["cache"][:, :M]))
    last_group_vs_torch(op, p, s, f"{op} through the tail split")
    # the split was taken, on the last group: without its sub-tiles the last two column tiles of group 7 stay untouched, all 104 rows of them
    probe = fresh_state(p, padded=False)
    _native.set_option("mm1_probe", 3)
    try:
        launch(op, p, probe, padded=False)
    finally:
        _native.set_option("mm1_probe", 0)
    nr = nt % 4 or 4                 # column tiles in the map's last block (NR = 4): the launch's last min(2, nr) tiles are the last group's
    tail = min(2, nr) * 128
    assert (probe["c"][7 * BM:, f - tail:] == SENT).all(), "the last group's last column tiles were not computed by sub-tiles"
    assert not (s["c"][7 * BM:, f - tail:] == SENT).any()


@pytest.mark.parametrize("mbm", [128, 192])
def test_block_mean_ragged(dev, mbm):
    n, c = 1000, 512
    x = (torch.randn(1, n, c, device=dev) * 2).to(torch.bfloat16)
    got = torch.ops.chipmunk.block_mean(x, mbm)
    blocks = (n + mbm - 1) // mbm
    assert got.shape == (1, blocks, c)
    for b in range(blocks):
        want = x[0, b * mbm:(b + 1) * mbm].float().mean(dim=0)      # the rows present: fp32 sum, one rounding
        # one bf16 rounding of an fp32 mean whose summation order differs from torch's: half a bf16 ulp (2^-9 relative) plus fp32 noise
        assert_close_bf16(got[0, b], want, atol=1e-5, rtol=2.0 ** -8, what=f"block {b} of {blocks} (mbm {mbm})")
    # whole blocks: the bits of the kernel on the block alone (the ragged launch changes nothing for them)
    full = torch.ops.chipmunk.block_mean(x[:, : n // mbm * mbm].contiguous(), mbm)
    assert torch.equal(got[:, : n // mbm], full)
    from chipmunk_amd.modules.mlp import block_mean
    assert torch.equal(block_mean(x, mbm), got)
