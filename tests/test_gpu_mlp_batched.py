"""The sparse-MLP operators over B > 1 sequences in one launch ("Batches"): a [B, M, K], c / packed [B, M, F], mma_c [B, M, N2], the
cache [B, F, ldc] with a batch stride of its own, indices [B, G, F], counts [B, G]; weights and bias shared.

The reference is today's single-sequence operator: the batched launch must give, BIT FOR BIT, what B launches of the 2-D operator on the
sequences' slices give -- in the packed deltas, the cache and mma_c.  That is a condition, not a tolerance.  One sequence other than the
first is also checked against fp32 torch under tests/test_gpu_mlp_ragged.py's tolerances (problem generator, canaries and tolerances are
that file's).  Canaries: one sentinel row behind every sequence's F * ldc cache elements (batch stride (F + 1) * ldc), 128 sentinel rows
behind the last sequence of c and mma_c, NaN in every sequence's cache padding [M, ldc), NaN slack rows behind a and packed.  Every operator
is launched ten times from the same state: same bits each time."""
import pytest
import torch

import test_gpu_mlp_ragged as R
from test_gpu_mlp_ragged import BM, F, K, N2, SENT, bits

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def seq_counts(counts, b):
    """The count list of sequence b: the shape's list rotated by b, so the lists differ between sequences; each holds a 0 and a full F."""
    n = len(counts)
    out = [counts[(i + b) % n] for i in range(n)]
    if 0 not in out:
        out[next(i for i, c in enumerate(out) if c != max(out))] = 0
    assert 0 in out and max(out) == max(counts)
    return out


def make_batch(dev, B, M, ldc, counts, fp8, seed, k=K, f=F, n2=N2, count_lists=None):
    """B problems of tests/test_gpu_mlp_ragged.py with shared weights, bias and scales, and their operands as one batch."""
    ps = []
    for b in range(B):
        cl = count_lists[b] if count_lists else seq_counts(counts, b)
        p = R.make_problem(dev, M, ldc, cl, fp8, seed=seed * 10 + b, k=k, f=f, n2=n2)
        if b:
            for name in ("w1", "bias", "w2T") + (("ra", "rb") if fp8 else ()):
                p[name] = ps[0][name]
        ps.append(p)
    a = torch.full((B * M + BM, k), NAN, device=dev).to(ps[0]["a"].dtype)          # NaN slack rows behind the last sequence
    packed = torch.full((B * M + BM, f), NAN, dtype=torch.bfloat16, device=dev)
    for b, p in enumerate(ps):
        a[b * M:(b + 1) * M] = p["a"]
        packed[b * M:(b + 1) * M] = p["packed"]
    batch = dict(B=B, M=M, ldc=ldc, f=f, ps=ps, a_buf=a, a=a[:B * M].view(B, M, k), packed_buf=packed, packed=packed[:B * M].view(B, M, f),
                 inds=torch.stack([p["inds"] for p in ps]), cnt=torch.stack([p["cnt"] for p in ps]))
    assert len({tuple(p["counts"]) for p in ps}) > 1 or B == 1, "the count lists must differ between sequences"
    return batch


def fresh_batch_state(bt):
    """Mutable tensors of one launch, as whole buffers (with their canaries) and as the views the operators get."""
    B, M, f, ldc, ps = bt["B"], bt["M"], bt["f"], bt["ldc"], bt["ps"]
    dev = bt["a"].device
    cache_buf = torch.full((B, f + 1, ldc), NAN, dtype=torch.bfloat16, device=dev)    # padding [M, ldc) = NaN
    cache_buf[:, f] = SENT                                                             # one canary row behind every sequence
    c_buf = torch.full((B * M + BM, f), SENT, dtype=torch.bfloat16, device=dev)
    out_buf = torch.full((B * M + BM, ps[0]["out0"].shape[1]), SENT, dtype=torch.bfloat16, device=dev)
    for b, p in enumerate(ps):
        cache_buf[b, :f, :M] = p["cache0"]
        out_buf[b * M:(b + 1) * M] = p["out0"]
    return views(bt, dict(c_buf=c_buf, cache_buf=cache_buf, out_buf=out_buf))


def views(bt, s):
    B, M, f = bt["B"], bt["M"], bt["f"]
    s["c"] = s["c_buf"][:B * M].view(B, M, f)
    s["cache"] = s["cache_buf"][:, :f, :M]               # [B, F, M], strides ((F + 1) * ldc, ldc, 1)
    s["out"] = s["out_buf"][:B * M].view(B, M, -1)
    return s


def clone_state(bt, s):
    return views(bt, {k: s[k].clone() for k in ("c_buf", "cache_buf", "out_buf")})


def launch_batched(op, bt, s):
    ops, p0 = torch.ops.chipmunk, bt["ps"][0]
    a, packed, inds, cnt = bt["a"], bt["packed"], bt["inds"], bt["cnt"]
    if op == "mm1":
        ops.csp_mlp_mm1(a, p0["w1"], s["c"], p0["bias"], s["cache"], inds, cnt)
    elif op == "mm1_scatter":
        ops.csp_mlp_mm1_scatter(a, p0["w1"], s["c"], p0["bias"], s["cache"], inds, cnt)
    elif op in ("fp8_upd0", "fp8_upd1"):
        ops.csp_mlp_mm1_fp8(a, p0["w1"], s["c"], p0["bias"], s["cache"], inds, cnt, p0["ra"], p0["rb"], op == "fp8_upd1")
    elif op == "fp8_scatter":
        ops.csp_mlp_mm1_fp8_scatter(a, p0["w1"], s["c"], p0["bias"], s["cache"], inds, cnt, p0["ra"], p0["rb"])
    elif op == "scatter_add":
        ops.csp_scatter_add(packed, s["cache"], inds, cnt, 6)
    elif op == "mm2":
        ops.csp_mlp_mm2(packed, p0["w2T"], inds, cnt, s["out"])
    elif op == "mm2_and_scatter_add":
        ops.csp_mlp_mm2_and_scatter_add(packed, s["cache"], inds, cnt, packed, p0["w2T"].unsqueeze(0), s["out"], 6, 0)
    else:
        raise ValueError(op)
    torch.cuda.synchronize()


def launch_per_sequence(op, bt, s):
    """B launches of today's 2-D operator on the sequences' slices of the same kind of buffers."""
    for b, p in enumerate(bt["ps"]):
        pb = dict(p, a=bt["a"][b], packed=bt["packed"][b], inds=bt["inds"][b], cnt=bt["cnt"][b])
        R.launch(op, pb, dict(c=s["c"][b], cache=s["cache"][b], out=s["out"][b]), padded=False)


def check_canaries(bt, s, what):
    B, M, f = bt["B"], bt["M"], bt["f"]
    assert (s["c_buf"][B * M:] == SENT).all(), f"{what}: rows behind the last sequence of the packed deltas were written"
    assert (s["out_buf"][B * M:] == SENT).all(), f"{what}: rows behind the last sequence of mma_c were written"
    assert (s["cache_buf"][:, f] == SENT).all(), f"{what}: the row behind a sequence's F * ldc cache elements was written"
    assert torch.isnan(bt["a_buf"][B * M:].float()).all() and torch.isnan(bt["packed_buf"][B * M:].float()).all(), f"{what}: an input's slack rows changed"
    assert not torch.isnan(s["c"].float()).any() and not torch.isnan(s["out"].float()).any() and not torch.isnan(s["cache"].float()).any(), \
        f"{what}: a NaN of the padding or the slack rows reached an output"


def state_bits(s):
    return tuple(bits(s[k]) for k in ("c_buf", "cache_buf", "out_buf"))


def assert_same_bits(got, ref, what):
    for name, x, y in zip(("packed deltas", "cache", "mma_c"), got, ref):
        assert torch.equal(x, y), f"{what}: {name} differ from the per-sequence launches ({int((x != y).sum())} of {x.numel()} elements)"


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("M,ldc,counts", R.SHAPES + [(256, 256, [F, 0]), (1024, 1024, [F, 0, 208, 16, 336, 512, 64, 272])],
                         ids=[f"M{m}-ld{l}" for m, l, _ in R.SHAPES] + ["M256-ld256", "M1024-ld1024"])
def test_batched_launch_gives_the_bits_of_separate_launches(dev, M, ldc, counts, B, op):
    fp8 = op.startswith("fp8")
    bt = make_batch(dev, B, M, ldc, counts, fp8, seed=M + B)
    start = fresh_batch_state(bt)
    ref = clone_state(bt, start)
    launch_per_sequence(op, bt, ref)
    ref_bits = state_bits(ref)
    for rep in range(10):
        s = clone_state(bt, start)
        launch_batched(op, bt, s)
        what = f"{op} B={B} M={M} ldc={ldc} launch {rep}"
        check_canaries(bt, s, what)
        assert_same_bits(state_bits(s), ref_bits, what)       # every launch: the first against the reference, the others thereby against the first
        if rep == 0:
            b = B - 1                                         # a sequence other than the first against fp32 torch
            R.last_group_vs_torch(op, bt["ps"][b], dict(c=s["c"][b], cache=s["cache"][b], out=s["out"][b]), f"{what}, sequence {b}")


@pytest.mark.parametrize("fp8", [False, True])
def test_tail_split_across_a_batch_boundary(dev, fp8):
    """B = 2, M = 1000: 16 groups.  With slots / 2 + 1 live column tiles (slots = resident workgroups per XCD) every XCD has 2 * slots + 2
    tiles and keeps two leftover tiles, which GEMM1 hands out as 64 x 64 sub-tiles; XCD 7's are the last column tile of the last two groups,
    i.e. of the SECOND sequence.  `mm1_probe = 3` makes the kernel skip exactly its sub-tiles: the sentinels they leave show where the split
    was taken."""
    from chipmunk_amd import _native
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = 2 * cus // 8
    nt = slots // 2 + 1
    f, M, k, B = nt * 128, 1000, 256, 2
    lists = [[2048, 0, 1024, 3072, 512, 256, 4096, f], [256, f, 0, 1024, 2048, 512, f, f]]
    bt = make_batch(dev, B, M, M, None, fp8, seed=5, k=k, f=f, count_lists=lists)
    op = "fp8_scatter" if fp8 else "mm1_scatter"
    start = fresh_batch_state(bt)
    ref = clone_state(bt, start)
    launch_per_sequence(op, bt, ref)
    s = clone_state(bt, start)
    launch_batched(op, bt, s)
    check_canaries(bt, s, op)
    assert_same_bits(state_bits(s), state_bits(ref), f"{op} through the tail split")
    R.last_group_vs_torch(op, bt["ps"][1], dict(c=s["c"][1], cache=s["cache"][1], out=s["out"][1]), f"{op} through the tail split, sequence 1")
    probe = clone_state(bt, start)
    _native.set_option("mm1_probe", 3)
    try:
        launch_batched(op, bt, probe)
    finally:
        _native.set_option("mm1_probe", 0)
    live = torch.zeros(B, M, f, dtype=torch.bool, device=dev)        # where a launch writes packed deltas
    for b in range(B):
        for g, n in enumerate(lists[b]):
            live[b, g * BM:(g + 1) * BM, :n] = True
    left = (probe["c"] == SENT) & live                               # ... and the sub-tiles did not
    assert not ((s["c"] == SENT) & live).any()
    assert left.any(), "no sub-tile was skipped: the tail split was not taken"
    assert left[1].any(), "no sub-tile of the second sequence"
    assert left[1, 7 * BM:, (nt - 1) * 128:].all(), "the last group's last column tile was not computed by sub-tiles"


def _small(dev, B=2, M=333, ldc=336):
    bt = make_batch(dev, B, M, ldc, [F, 0, 336], False, seed=1)
    return bt, fresh_batch_state(bt)


def test_bad_batch_stride_is_refused(dev):
    bt, s = _small(dev)
    p0, f, M, ldc = bt["ps"][0], bt["f"], bt["M"], bt["ldc"]
    flat = torch.zeros(4 * (f + 1) * ldc, dtype=torch.bfloat16, device=dev)
    for stride in (f * ldc - 8, f * ldc + 4):                 # below F * ldc; not a multiple of 8
        cache = flat.as_strided((2, f, M), (stride, ldc, 1))
        with pytest.raises(RuntimeError, match="batch stride"):
            torch.ops.chipmunk.csp_mlp_mm1(bt["a"], p0["w1"], s["c"], p0["bias"], cache, bt["inds"], bt["cnt"])
        with pytest.raises(RuntimeError, match="batch stride"):
            torch.ops.chipmunk.csp_mlp_mm1_scatter(bt["a"], p0["w1"], s["c"], p0["bias"], cache, bt["inds"], bt["cnt"])
        with pytest.raises(RuntimeError, match="batch stride"):
            torch.ops.chipmunk.csp_scatter_add(bt["packed"], cache, bt["inds"], bt["cnt"], 6)
        with pytest.raises(RuntimeError, match="batch stride"):
            torch.ops.chipmunk.csp_mlp_mm2_and_scatter_add(bt["packed"], cache, bt["inds"], bt["cnt"], bt["packed"], p0["w2T"].unsqueeze(0), s["out"], 6, 0)


def test_mismatched_batch_sizes_are_refused(dev):
    bt, s = _small(dev)
    bt3, s3 = _small(dev, B=3)
    p0 = bt["ps"][0]
    ops = torch.ops.chipmunk
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_mlp_mm1(bt["a"], p0["w1"], s3["c"], p0["bias"], s["cache"], bt["inds"], bt["cnt"])
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_mlp_mm1(bt["a"], p0["w1"], s["c"], p0["bias"], s3["cache"], bt["inds"], bt["cnt"])
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_mlp_mm1_scatter(bt["a"], p0["w1"], s["c"], p0["bias"], s["cache"], bt3["inds"], bt3["cnt"])
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_mlp_mm1(bt["a"], p0["w1"], s["c"], p0["bias"], s["cache"][0], bt["inds"], bt["cnt"])
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_scatter_add(bt["packed"], s3["cache"], bt["inds"], bt["cnt"], 6)
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_mlp_mm2(bt["packed"], p0["w2T"], bt3["inds"], bt3["cnt"], s["out"])
    with pytest.raises(RuntimeError, match="batch size"):
        ops.csp_mlp_mm2_and_scatter_add(bt["packed"], s["cache"], bt["inds"], bt["cnt"], bt["packed"], p0["w2T"].unsqueeze(0), s3["out"], 6, 0)


def test_too_many_groups_are_refused(dev):
    B, M, k, f = 65536, 1, 64, 64                 # one group per sequence: 65 536 groups
    a = torch.zeros(B, M, k, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(f, k, dtype=torch.bfloat16, device=dev)
    c = torch.zeros(B, M, f, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(B, M, k, dtype=torch.bfloat16, device=dev)
    cache = torch.zeros(B, f, 8, dtype=torch.bfloat16, device=dev)[..., :M]
    inds = torch.zeros(B, 1, f, dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, 1, dtype=torch.int32, device=dev)
    bias = torch.zeros(f, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="65535"):
        torch.ops.chipmunk.csp_mlp_mm1(a, w, c, bias, cache, inds, cnt)
    with pytest.raises(RuntimeError, match="65535"):
        torch.ops.chipmunk.csp_scatter_add(c, cache, inds, cnt, 6)
    with pytest.raises(RuntimeError, match="65535"):
        torch.ops.chipmunk.csp_mlp_mm2(c, w.T.contiguous(), inds, cnt, out)


@pytest.mark.parametrize("op", ["mm1_scatter", "fp8_scatter", "mm2_and_scatter_add", "mm2"])
def test_leading_one_gives_the_bits_of_the_2d_call(dev, op):
    """B == 1 as a 3-D operand takes the entry the 2-D call takes."""
    bt = make_batch(dev, 1, 333, 336, [F, 0, 336], op.startswith("fp8"), seed=3)
    start = fresh_batch_state(bt)
    ref = clone_state(bt, start)
    launch_per_sequence(op, bt, ref)
    s = clone_state(bt, start)
    launch_batched(op, bt, s)
    check_canaries(bt, s, op)
    assert_same_bits(state_bits(s), state_bits(ref), f"{op} with a leading 1")
