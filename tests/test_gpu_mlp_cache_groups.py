"""Group-major activation cache of the sparse MLP ("Group-major cache") on the GPU.

The arithmetic of the two layouts is the same, so every GEMM1 family and the scatter-add are held to BIT equality with their column-major
call on the same values -- the operators the fp64 and oracle tests already hold -- with the layouts converted by torch pad / reshape /
permute.  Two cases go straight against fp64 under the existing MLP_SEG_BOUND.

Shapes, the smallest at which the route can go wrong: M = 293 (three groups: a wrong group stride shows; the last has 37 rows, so a
16-byte piece straddles M), K = 128, F = 256, counts [136, 0, 256] and [72, 200, 8] (a tile plus 8 columns, an empty group, every column),
M = 384 once (whole groups), B = 2 with a batch stride of G * F * 128 + 1024.  A sentinel bit pattern fills the tail rows of the last
group, the columns a group does not keep, the slack between the sequences and the packed columns past a count; whole buffers are compared,
so all of them must survive every launch."""
import functools

import pytest
import torch

from helpers import (MLP_SEG_BOUND, MLP_SEG_W1, assert_segs_close, mlp_exact_args, mlp_group_cols, mlp_problem, mm1_exact, seg_term)

pytestmark = pytest.mark.gpu

K, F, N2 = 128, 256, 64
COUNTS = {293: ([136, 0, 256], [72, 200, 8]), 384: ([136, 0, 256], [72, 200, 8])}
SLACK = 1024
SENT_BITS = 0x7FC1      # a quiet NaN no kernel produces
E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    from chipmunk_amd import _native
    _native.set_option("mm1_variant", 0)         # shipped forms only
    _native.set_option("mm2_variant", 0)
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def sentinel(shape, dev):
    return torch.full(shape, SENT_BITS, dtype=torch.int16, device=dev).view(torch.bfloat16)


def is_sentinel(t):
    return (bits(t) == SENT_BITS).all()


def to_groups(cm, fill_bits=SENT_BITS):
    """column-major [F, M] -> group-major [G, F, 128], the tail rows of the last group `fill_bits` (plain torch)"""
    f, m = cm.shape
    g = (m + 127) // 128
    out = torch.full((f, g * 128), fill_bits, dtype=torch.int16, device=cm.device)
    out[:, :m] = bits(cm)
    return out.view(f, g, 128).permute(1, 0, 2).contiguous().view(torch.bfloat16)


def from_groups(gm, m):
    """group-major [G, F, 128] -> column-major [F, M] (plain torch)"""
    g, f, _ = gm.shape
    return gm.permute(1, 0, 2).reshape(f, g * 128)[:, :m].contiguous()


@functools.lru_cache(maxsize=None)
def problem(M, seq, fp8=False, gated=False):
    """sequence `seq` of the test's batch on the device; the cache columns a group does not keep hold the sentinel in that group's rows"""
    dev = torch.device("cuda:0")
    p = mlp_problem(M, K, F, seed=4100 + 10 * seq + M, fp8=fp8, gated=gated, counts=list(COUNTS[M][seq]))
    p = {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in p.items()}
    cache = bits(p["cache0"]).clone()
    for g, n in enumerate(p["counts"]):
        unkept = p["inds"][g, n:].long()
        cache[unkept, g * 128: min(M, (g + 1) * 128)] = SENT_BITS
    p["cache0"] = cache.view(torch.bfloat16)
    g = torch.Generator().manual_seed(77 + seq)
    p["bu2"] = (torch.randn(F, generator=g) * 0.1).to(torch.bfloat16).to(dev)      # an up bias for the gated forms
    if fp8:      # one reciprocal scale per token row / per fc1 column around the scalar ones
        p["ra_rows"] = (p["ra"] * (0.5 + torch.rand(M, generator=g).to(dev))).float().contiguous()
        p["rb_cols"] = (p["rb"] * (0.5 + torch.rand(F, generator=g).to(dev))).float().contiguous()
    return p


def batch_of(M, B, fp8=False, gated=False):
    """the operands of a launch over B sequences: (problems, stacked or 2-D tensors by name)"""
    ps = [problem(M, b, fp8, gated) for b in range(B)]
    # weights and biases are shared by the sequences of a batch: those of sequence 0
    def stack(k):      # (e4m3 tensors are stacked as bytes)
        if B == 1:
            return ps[0][k]
        if ps[0][k].dtype == E4M3:
            return torch.stack([p[k].view(torch.uint8) for p in ps]).view(E4M3)
        return torch.stack([p[k] for p in ps])
    t = {k: stack(k) for k in ("a", "inds", "cnt")}
    if fp8:
        t["ra_rows"] = torch.stack([p["ra_rows"] for p in ps]) if B > 1 else ps[0]["ra_rows"]
    return ps, t


def column_cache(ps, M):
    """the column-major cache of the launch: the [..., :M] view of a pitched [B, F, ceil8(M)] buffer with sentinel padding"""
    B, ld = len(ps), (M + 7) // 8 * 8
    buf = sentinel((B, F, ld), ps[0]["a"].device)
    for b, p in enumerate(ps):
        buf[b, :, :M] = p["cache0"]
    return buf, (buf[..., :M] if B > 1 else buf[0][:, :M])


def group_cache(ps, M):
    """the group-major cache of the launch inside a flat sentinel buffer: B blocks [G, F, 128], G * F * 128 + SLACK elements apart"""
    B, G = len(ps), (M + 127) // 128
    stride = G * F * 128 + SLACK
    flat = sentinel((B * stride,), ps[0]["a"].device)
    view = flat.as_strided((B, G, F, 128), (stride, F * 128, 128, 1))
    for b, p in enumerate(ps):
        view[b] = to_groups(p["cache0"])
    return flat, (view if B > 1 else view[0])


def expected_flat(flat0, col_buf, M):
    """what the flat group-major buffer must hold after a launch whose column-major twin left `col_buf`: the live rows converted, every
    other element -- tail rows, slack -- as it was"""
    B, G = col_buf.shape[0], (M + 127) // 128
    stride = G * F * 128 + SLACK
    want = flat0.clone()
    view = want.as_strided((B, G, F, 128), (stride, F * 128, 128, 1))
    for b in range(B):
        view[b] = to_groups(col_buf[b, :, :M])
    return want


def run_both(M, B, fp8, gated, call):
    """`call(t, ps, packed, cache)` launches one operator; run it on the column-major and on the group-major cache of the same values and
    assert bit equality of the packed deltas and of the whole cache buffers.  Returns (packed, group-major view, problems)."""
    ps, t = batch_of(M, B, fp8, gated)
    dev = ps[0]["a"].device
    shape = (B, M, F) if B > 1 else (M, F)
    col_buf, col = column_cache(ps, M)
    c_col = sentinel(shape, dev)
    call(t, ps, c_col, col)
    flat, gm = group_cache(ps, M)
    flat0 = flat.clone()
    c_gm = sentinel(shape, dev)
    call(t, ps, c_gm, gm)
    torch.cuda.synchronize()
    assert torch.equal(bits(c_gm), bits(c_col)), "packed deltas differ from the column-major call's"
    want = expected_flat(flat0, col_buf, M)
    assert torch.equal(bits(flat), bits(want)), "the group-major cache differs from the converted column-major cache"
    for b in range(B):      # ... and converted back
        back = from_groups(flat.as_strided((B, (M + 127) // 128, F, 128), ((M + 127) // 128 * F * 128 + SLACK, F * 128, 128, 1))[b], M)
        assert torch.equal(bits(back), bits(col_buf[b, :, :M])), "the group-major cache converted back differs from the column-major cache"
    # the three places by name (the whole-buffer comparison above covers them; this says which one broke)
    G, stride = (M + 127) // 128, (M + 127) // 128 * F * 128 + SLACK
    view = flat.as_strided((B, G, F, 128), (stride, F * 128, 128, 1))
    if M % 128:
        assert is_sentinel(view[:, -1, :, M % 128:]), "tail rows of the last group were written"
    assert is_sentinel(flat.view(B, stride)[:, G * F * 128:]), "the slack between the sequences was written"
    for b, p in enumerate(ps):
        for g, n in enumerate(p["counts"]):
            rows = min(128, M - g * 128)
            assert is_sentinel(view[b, g, p["inds"][g, n:].long(), :rows]), "a column the group does not keep was written"
    cols = torch.stack([mlp_group_cols(p["cnt"], M) for p in ps])
    past = torch.arange(F, device=dev) >= cols[..., None]
    assert is_sentinel(c_gm.reshape(B, M, F)[past]), "packed columns at or past a count were written"
    return c_gm, gm, ps


# ------------------------------------------------------------------------------------------------ the full step's kernel
@pytest.mark.parametrize("B,R,C", [(1, 128, 64), (1, 293, 256), (2, 37, 64), (1, 1, 64)])
def test_transpose_to_groups_is_bit_equal_to_torch(dev, B, R, C):
    x = torch.randn(B, R, C, device=dev).to(torch.bfloat16)
    out = torch.ops.chipmunk.transpose_to_groups(x)
    G = (R + 127) // 128
    assert out.shape == (B, G, C, 128) and out.is_contiguous() and out.dtype == torch.bfloat16
    want = torch.stack([to_groups(x[b].T.contiguous(), fill_bits=0) for b in range(B)])
    assert torch.equal(bits(out), bits(want))
    back = out.permute(0, 1, 3, 2).reshape(B, G * 128, C)
    assert torch.equal(bits(back[:, :R]), bits(x)) and (bits(back[:, R:]) == 0).all()
    assert torch.equal(bits(torch.ops.chipmunk.transpose_to_groups(x[0])), bits(want[0]))      # 2-D input: [G, C, 128]


# ------------------------------------------------------------------------------------------------ GEMM1, each family
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("update", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act", ["gelu_tanh", "silu", "gelu"])
def test_bf16_gemm1_matches_the_column_major_call(dev, act, bias, update, B):
    def call(t, ps, c, cache):
        torch.ops.chipmunk.csp_mlp_mm1_act(t["a"], ps[0]["w"], c, ps[0]["bias"] if bias else None, cache, t["inds"], t["cnt"], act, update)
    run_both(293, B, False, False, call)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("update", [0, 1, 2])        # 1: the literal store form, 2: the scatter-add
@pytest.mark.parametrize("rs", [False, True])
def test_fp8_gemm1_matches_the_column_major_call(dev, rs, update, B):
    def call(t, ps, c, cache):
        p = ps[0]
        if rs:
            torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs(t["a"], p["w"], c, p["bias"], cache, t["inds"], t["cnt"], t["ra_rows"], p["rb_cols"], "silu", update)
        else:
            torch.ops.chipmunk.csp_mlp_mm1_fp8_act(t["a"], p["w"], c, p["bias"], cache, t["inds"], t["cnt"], p["ra"], p["rb"], "gelu_tanh", update)
    run_both(293, B, True, False, call)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("update", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
def test_gated_gemm1_matches_the_column_major_call(dev, fp8, update, B):
    def call(t, ps, c, cache):
        p = ps[0]
        if fp8:
            torch.ops.chipmunk.csp_mlp_mm1_glu_fp8(t["a"], p["w"], p["wu"], c, p["bias"], p["bu2"], cache, t["inds"], t["cnt"], p["ra"], p["rb"],
                                                   p["rbu"], "silu", update)
        else:
            torch.ops.chipmunk.csp_mlp_mm1_glu(t["a"], p["w"], p["wu"], c, p["bias"], p["bu2"], cache, t["inds"], t["cnt"], "gelu", update)
    run_both(293, B, fp8, True, call)


@pytest.mark.parametrize("B", [1, 2])
def test_whole_groups_match_the_column_major_call(dev, B):
    """M = 384: no short group, and the group-major block has the element count of the column-major one"""
    def bf16(t, ps, c, cache):
        torch.ops.chipmunk.csp_mlp_mm1_act(t["a"], ps[0]["w"], c, ps[0]["bias"], cache, t["inds"], t["cnt"], "gelu_tanh", True)

    def fp8(t, ps, c, cache):
        p = ps[0]
        torch.ops.chipmunk.csp_mlp_mm1_fp8_act(t["a"], p["w"], c, p["bias"], cache, t["inds"], t["cnt"], p["ra"], p["rb"], "gelu_tanh", 2)
    run_both(384, B, False, False, bf16)
    run_both(384, B, True, False, fp8)


# ------------------------------------------------------------------------------------------------ scatter-add
@pytest.mark.parametrize("M", [293, 384])
@pytest.mark.parametrize("B", [1, 2])
def test_scatter_add_gm_matches_csp_scatter_add(dev, B, M):
    ps, _ = batch_of(M, B)
    g = torch.Generator().manual_seed(5)
    packed = (torch.randn(B, M, F, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    inds, cnt = torch.stack([p["inds"] for p in ps]), torch.stack([p["cnt"] for p in ps])
    col_buf, _ = column_cache(ps, M)
    torch.ops.chipmunk.csp_scatter_add(packed, col_buf[..., :M], inds, cnt, 0)
    flat, _ = group_cache(ps, M)
    flat0 = flat.clone()
    G, stride = (M + 127) // 128, (M + 127) // 128 * F * 128 + SLACK
    torch.ops.chipmunk.csp_scatter_add_gm(packed, flat.as_strided((B, G, F, 128), (stride, F * 128, 128, 1)), inds, cnt)
    torch.cuda.synchronize()
    assert not torch.equal(bits(flat), bits(flat0))
    assert torch.equal(bits(flat), bits(expected_flat(flat0, col_buf, M)))


# ------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("fp8", [False, True])
def test_group_major_gemm1_against_fp64(dev, fp8):
    """the packed deltas of a group-major launch under the existing bound (fp8: with the documented term of the bf16-rounded activation,
    as tests/test_gpu_mlp_accuracy.py); the sentinel columns of the cache are not kept, so the exact reference never reads them"""
    M = 293
    p = problem(M, 0, fp8)
    exact, fresh = mm1_exact(p["a"], p["w"], p["bias"], p["cache0"], p["inds"], p["cnt"], **mlp_exact_args(p))
    cols = mlp_group_cols(p["cnt"], M)
    _, gm = group_cache([p], M)
    c = sentinel((M, F), dev)
    if fp8:
        torch.ops.chipmunk.csp_mlp_mm1_fp8_act(p["a"], p["w"], c, p["bias"], gm, p["inds"], p["cnt"], p["ra"], p["rb"], "gelu_tanh", 0)
        term = seg_term(fresh, exact, MLP_SEG_W1, cols)
    else:
        torch.ops.chipmunk.csp_mlp_mm1_act(p["a"], p["w"], c, p["bias"], gm, p["inds"], p["cnt"], "gelu_tanh", False)
        term = None
    c = torch.where(torch.arange(F, device=dev) < cols[:, None], c, torch.zeros_like(c))      # (the sentinel past the counts is no result)
    assert_segs_close(c, exact, MLP_SEG_BOUND, f"group-major GEMM1, {'fp8' if fp8 else 'bf16'} | packed deltas", extra=term, cols=cols)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    M, ops = 293, torch.ops.chipmunk
    p = problem(M, 0)
    p8 = problem(M, 0, True)
    c = sentinel((M, F), dev)
    good = torch.zeros(3, F, 128, dtype=torch.bfloat16, device=dev)

    def act(cache, a=p["a"], cc=c):
        ops.csp_mlp_mm1_act(a, p["w"], cc, p["bias"], cache, p["inds"], p["cnt"], "gelu_tanh", False)
    act(good)                                                            # (the shape that is accepted)
    for bad, text in ((torch.zeros(3, F, 64, dtype=torch.bfloat16, device=dev), "group-major"),              # wrong last dimension
                      (torch.zeros(2, F, 128, dtype=torch.bfloat16, device=dev), "group-major"),             # wrong G
                      (torch.zeros(3, F // 2, 128, dtype=torch.bfloat16, device=dev), "group-major"),        # wrong F
                      (torch.zeros(3, F, 256, dtype=torch.bfloat16, device=dev)[..., ::2], "contiguous"),    # pieces not contiguous
                      (torch.zeros(3, 2 * F, 128, dtype=torch.bfloat16, device=dev)[:, ::2], "contiguous"),  # columns not 128 apart
                      (torch.zeros(6, F, 128, dtype=torch.bfloat16, device=dev)[::2], "contiguous"),         # groups not F * 128 apart
                      (torch.zeros(3, F, 128, dtype=torch.float16, device=dev), "bfloat16|BFloat16|bf16")):
        with pytest.raises(RuntimeError, match=text):
            act(bad)
    # a batch: the batch size and the batch stride
    a2, c2 = torch.stack([p["a"], p["a"]]), sentinel((2, M, F), dev)
    inds2, cnt2 = torch.stack([p["inds"]] * 2), torch.stack([p["cnt"]] * 2)

    def act2(cache):
        ops.csp_mlp_mm1_act(a2, p["w"], c2, p["bias"], cache, inds2, cnt2, "gelu_tanh", False)
    act2(torch.zeros(2, 3, F, 128, dtype=torch.bfloat16, device=dev))
    with pytest.raises(RuntimeError, match="group-major"):
        act2(torch.zeros(3, 3, F, 128, dtype=torch.bfloat16, device=dev))
    with pytest.raises(RuntimeError, match="batch stride"):
        act2(torch.zeros(2 * 3 * F * 128 + 4, dtype=torch.bfloat16, device=dev).as_strided((2, 3, F, 128), (3 * F * 128 + 4, F * 128, 128, 1)))
    with pytest.raises(RuntimeError, match="batch stride"):
        act2(torch.zeros(1, 3, F, 128, dtype=torch.bfloat16, device=dev).expand(2, 3, F, 128))
    # the other families take the same checks
    with pytest.raises(RuntimeError, match="group-major"):
        ops.csp_mlp_mm1_fp8_act(p8["a"], p8["w"], c, p8["bias"], good[:2], p8["inds"], p8["cnt"], p8["ra"], p8["rb"], "gelu_tanh", 0)
    with pytest.raises(RuntimeError, match="group-major"):
        ops.csp_mlp_mm1_glu(p["a"], p["w"], p["w"], c, None, None, good[:2], p["inds"], p["cnt"], "silu", False)
    packed = torch.zeros(1, M, F, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="unpacked_groups must be"):
        ops.csp_scatter_add_gm(packed, good[:2].unsqueeze(0), p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.csp_scatter_add_gm(packed, torch.zeros(1, 3, F, 256, dtype=torch.bfloat16, device=dev)[..., ::2], p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0))
    with pytest.raises(RuntimeError, match="16-bit"):
        ops.transpose_to_groups(torch.zeros(4, 4, device=dev))


def test_reference_schema_operators_refuse_a_group_major_cache(dev):
    """handed a group-major tensor they must raise, not compute: at M = 384 its element count is that of the column-major cache"""
    ops = torch.ops.chipmunk
    for M in (293, 384):
        p, p8 = problem(M, 0), problem(M, 0, True)
        G = (M + 127) // 128
        gm = torch.zeros(G, F, 128, dtype=torch.bfloat16, device=dev)
        before = gm.clone()
        c = sentinel((M, F), dev)
        out = torch.zeros(M, N2, dtype=torch.bfloat16, device=dev)
        w2 = torch.zeros(F, N2, dtype=torch.bfloat16, device=dev)
        calls = {
            "csp_mlp_mm1": lambda: ops.csp_mlp_mm1(p["a"], p["w"], c, p["bias"], gm, p["inds"], p["cnt"]),
            "csp_mlp_mm1_scatter": lambda: ops.csp_mlp_mm1_scatter(p["a"], p["w"], c, p["bias"], gm, p["inds"], p["cnt"]),
            "csp_mlp_mm1_fp8": lambda: ops.csp_mlp_mm1_fp8(p8["a"], p8["w"], c, p8["bias"], gm, p8["inds"], p8["cnt"], p8["ra"], p8["rb"], False),
            "csp_scatter_add": lambda: ops.csp_scatter_add(c.unsqueeze(0), gm.unsqueeze(0), p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0), 0),
            "csp_scatter_add, 3-D": lambda: ops.csp_scatter_add(c.unsqueeze(0), gm, p["inds"].unsqueeze(0), p["cnt"].unsqueeze(0), 0),
            "csp_mlp_mm2_and_scatter_add": lambda: ops.csp_mlp_mm2_and_scatter_add(c.unsqueeze(0), gm.unsqueeze(0), p["inds"].unsqueeze(0),
                                                                                   p["cnt"].unsqueeze(0), c.unsqueeze(0), w2.unsqueeze(0),
                                                                                   out.unsqueeze(0), 0, 0),
        }
        for name, call in calls.items():
            with pytest.raises(RuntimeError):
                call()
            torch.cuda.synchronize()
            assert torch.equal(gm, before) and is_sentinel(c) and not out.any(), f"{name} computed on a group-major cache (M = {M})"
