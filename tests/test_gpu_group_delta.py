"""``topk_group_delta_indices[_p]`` on the device: exact comparisons (indices, counts, cache bits) against

* the unfused GPU chain ``sub / abs / reshape / sum`` + ``topk_indices`` + ``copy_indices`` at two rows per group, where one fp32 add and
  one rounding leave no room for a different result;
* the CPU model of tests/group_delta_model.py (explicit ascending fp32 loop) at 1, 3, 4 and 6 rows per group, with a short last group,
  past the 16 384 columns the registers hold, and in three dtypes;
* the plain ``topk_delta_indices`` at one row per group.
"""
import functools

import pytest
import torch

import group_delta_model as gdm
import mlp_top_p_model as tp

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TRIPLES = [(0.7, 256, 0.0), (0.85, 112, 0.0), (0.7, 256, 0.05)]
P_TRIPLES = [(1 - tp.EXACT_TOP_KEYS, top_p, min_keys) for top_p, min_keys in tp.EXACT_PARAMS]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


@functools.lru_cache(maxsize=None)
def operands(kind, b, rows, f, dtype, seed=7):
    """(activation, cache) on the CPU; the kinds of test_topk_delta_threshold_shortcut_is_bit_identical (never modified: callers clone)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(b, rows, f, generator=g)
    if kind == "ties":
        d = torch.randint(0, 4, (b, rows, f), generator=g).float() * 0.25
    elif kind == "tiny":
        d = torch.randn(b, rows, f, generator=g) * 1e-7
    elif kind == "zeros":
        d = torch.zeros(b, rows, f)
        d[..., f // 2:] = torch.randn(b, rows, f - f // 2, generator=g)
    else:
        d = torch.randn(b, rows, f, generator=g) * 0.3
    a = a.to(dtype)
    return a, (a.float() + d).to(dtype)


def outputs(dev, b, groups, f, fill=-9):
    """(indices [B, G, F] filled with `fill`, counts [B, G]).  The index rows are the head of a longer zeroed buffer: a count rounded up
    past F (every column kept and F no multiple of multiple_of) makes copy_indices read that many entries, the last row's past its end."""
    buf = torch.zeros(b * groups * f + 1024, dtype=torch.int32, device=dev)
    inds = buf[: b * groups * f].view(b, groups, f)
    inds.fill_(fill)
    return inds, torch.full((b, groups), -7, dtype=torch.int32, device=dev)


def fused(dev, a, cache, r, sparsity, multiple_of, rk=0.0, p=None, fill=-9):
    from chipmunk_amd import ops
    b, rows, f = a.shape
    inds, counts = outputs(dev, b, gdm.groups_of(rows, r), f, fill)
    a, cache = a.to(dev), cache.clone().to(dev)
    if p is None:
        ops.topk_group_delta_indices(a, cache, inds, counts, r, sparsity, multiple_of, rk)
    else:
        ops.topk_group_delta_indices_p(a, cache, inds, counts, r, sparsity, p[0], p[1], multiple_of, rk)
    torch.cuda.synchronize()
    return inds.cpu(), counts.cpu(), cache.cpu()


def unfused(dev, a, cache, r, sparsity, multiple_of, rk=0.0, p=None, fill=-9):
    """the modules' torch sequence with its temporaries"""
    from chipmunk_amd import ops
    b, rows, f = a.shape
    assert rows % r == 0
    a, cache = a.to(dev), cache.clone().to(dev)
    mdiff = (a - cache).abs().reshape(b, -1, r, f).sum(dim=2)
    inds, counts = outputs(dev, b, rows // r, f, fill)
    if p is None:
        ops.topk_indices(mdiff, inds, counts, sparsity, multiple_of, rk)
    else:
        ops.topk_indices_p(mdiff, inds, counts, sparsity, p[0], p[1], multiple_of, rk)
    ops.copy_indices(a, cache, inds, counts)
    torch.cuda.synchronize()
    return inds.cpu(), counts.cpu(), cache.cpu()


def assert_same(got, want, what):
    assert torch.equal(got[1], want[1]), f"{what}: counts {got[1].tolist()} vs {want[1].tolist()}"
    assert torch.equal(got[0], want[0]), f"{what}: indices"
    assert torch.equal(bits(got[2]), bits(want[2])), f"{what}: cache bits"


# ------------------------------------------------------------------------------------------------------------------ R = 2: the GPU chain
@pytest.mark.parametrize("kind", ["normal", "ties", "tiny", "zeros"])
@pytest.mark.parametrize("sparsity,multiple_of,rk", TRIPLES)
@pytest.mark.parametrize("f", [1024, 4096, 12288])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_rows_per_group_equal_the_unfused_chain(dev, dtype, f, sparsity, multiple_of, rk, kind):
    from chipmunk_amd import ops
    a, cache = operands(kind, 2, 6, f, DTYPES[dtype])
    ops.manual_seed(99)      # random keys: the same seed and launch order give the same set
    want = unfused(dev, a, cache, 2, sparsity, multiple_of, rk)
    ops.manual_seed(99)
    got = fused(dev, a, cache, 2, sparsity, multiple_of, rk)
    assert_same(got, want, f"{dtype} F {f} {kind} {(sparsity, multiple_of, rk)}")
    assert int(got[1].min()) > 0


# ------------------------------------------------------------------------------------------------------------------ R = 1, 3, 4, 6: the model
@functools.lru_cache(maxsize=None)
def model(kind, b, rows, f, dtype, r, sparsity, multiple_of):
    a, cache = operands(kind, b, rows, f, dtype)
    return gdm.run(a, cache, r, sparsity, multiple_of)


@pytest.mark.parametrize("f", [1024, 17384])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("r", [1, 3, 4, 6])
def test_rows_per_group_equal_the_model(dev, r, dtype, f):
    a, cache = operands("normal", 2, 2 * r, f, DTYPES[dtype])
    got = fused(dev, a, cache, r, 0.7, 256)
    assert_same(got, model("normal", 2, 2 * r, f, DTYPES[dtype], r, 0.7, 256), f"R {r} {dtype} F {f}")
    if r == 1:      # ... and the kernel this one generalises
        inds, counts = outputs(dev, 2, 2, f)
        c1 = cache.clone().to(dev)
        torch.ops.chipmunk.topk_delta_indices(a.to(dev), c1, inds, counts, 0.7, 256, 0.0)
        assert_same(got, (inds.cpu(), counts.cpu(), c1.cpu()), f"R 1 {dtype} F {f} against topk_delta_indices")


@pytest.mark.parametrize("f", [1024, 17384])
@pytest.mark.parametrize("rows", [3 * 4 - 1, 2 * 4 + 1], ids=["last group lacks a row", "last group has one row"])
def test_short_last_group(dev, rows, f):
    """G = 3, R = 4: the last group sums and refreshes the rows it has; the whole cache is compared, so the rows of the other groups and
    of the other sequence keep their bits"""
    a, cache = operands("normal", 2, rows, f, torch.bfloat16)
    got = fused(dev, a, cache, 4, 0.7, 256)
    want = model("normal", 2, rows, f, torch.bfloat16, 4, 0.7, 256)
    assert got[0].shape == (2, 3, f)
    assert_same(got, want, f"rows {rows} F {f}")
    # (activation and cache differ in nearly every column, so a row that was refreshed at all shows it)
    assert bool((bits(got[2]) != bits(cache)).any(-1).all()), "every row of every group has some listed column refreshed"


# ------------------------------------------------------------------------------------------------------------------ edges and errors
def test_sparsity_zero_lists_and_copies_everything(dev):
    a, cache = operands("normal", 2, 7, 1500, torch.bfloat16)       # R = 4: a short last group
    inds, counts, out = fused(dev, a, cache, 4, 0.0, 256)
    assert torch.equal(counts, torch.full((2, 2), 1500, dtype=torch.int32))
    assert torch.equal(inds, torch.arange(1500, dtype=torch.int32).expand(2, 2, 1500))
    assert torch.equal(bits(out), bits(a))


def test_sparsity_one_lists_nothing(dev):
    a, cache = operands("normal", 2, 7, 1500, torch.bfloat16)
    inds, counts, out = fused(dev, a, cache, 4, 1.0, 256)
    assert int(counts.abs().max()) == 0 and bool((inds == -1).all())
    assert torch.equal(bits(out), bits(cache))


def test_bad_arguments_raise(dev):
    from chipmunk_amd import ops

    def call(a, cache, inds, counts, r):
        ops.topk_group_delta_indices(a, cache, inds, counts, r, 0.7, 256, 0.0)

    def tensors(f=1024, rows=4, groups=2, dtype=torch.bfloat16, cache_dtype=torch.bfloat16):
        return (torch.zeros(1, rows, f, dtype=dtype, device=dev), torch.zeros(1, rows, f, dtype=cache_dtype, device=dev),
                torch.zeros(1, groups, f, dtype=torch.int32, device=dev), torch.zeros(1, groups, dtype=torch.int32, device=dev))

    with pytest.raises(RuntimeError, match="1024"):
        call(*tensors(f=512), 2)
    with pytest.raises(RuntimeError, match="rows_per_group"):
        call(*tensors(), 0)
    with pytest.raises(RuntimeError, match="rows_per_group"):
        call(*tensors(rows=130, groups=2), 65)
    with pytest.raises(RuntimeError, match="indices must be"):
        call(*tensors(groups=3), 2)
    with pytest.raises(RuntimeError, match="same dtype"):
        call(*tensors(cache_dtype=torch.float16), 2)
    with pytest.raises(ValueError, match="top_p"):
        ops.topk_group_delta_indices_p(*tensors(), 2, 0.7, 0.0, 0.0, 256, 0.0)
    call(*tensors(), 2)     # (the good call goes through)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the _p form
@pytest.mark.parametrize("sparsity,top_p,min_keys", P_TRIPLES)
@pytest.mark.parametrize("f", [1024, 12288])
def test_p_form_two_rows_per_group_equal_the_unfused_chain(dev, f, sparsity, top_p, min_keys):
    a, cache = operands("normal", 2, 6, f, torch.bfloat16)
    want = unfused(dev, a, cache, 2, sparsity, 256, p=(top_p, min_keys))
    got = fused(dev, a, cache, 2, sparsity, 256, p=(top_p, min_keys))
    assert_same(got, want, f"_p F {f} {(sparsity, top_p, min_keys)}")
    assert int(got[1].min()) > 0


def exact_operands(f, r, dtype, seed=11):
    """[2, 3 r, F] operands whose scores are tp.exact_rows(f)[:6] exactly: every value an integer <= 255 split into r integer terms,
    cache in {0, 1}, activation = cache +- term -- every partial sum in any order is exact in fp32 (and in T), so the fp64 rule holds"""
    vals = tp.exact_rows(f)[:6].view(2, 3, 1, f)
    part = torch.floor(vals / r).expand(2, 3, r, f).clone()
    part[:, :, r - 1] = vals[:, :, 0] - (r - 1) * part[:, :, 0]
    part = part.reshape(2, 3 * r, f)
    g = torch.Generator().manual_seed(seed)
    cache = torch.randint(0, 2, part.shape, generator=g).float()
    sign = torch.where((torch.rand(part.shape, generator=g) < 0.5) & (part < 255), -1.0, 1.0)
    a = cache + sign * part
    assert float(a.abs().max()) <= 256 and torch.equal(gdm.scores(a, cache, r).view(6, f), tp.exact_rows(f)[:6])
    return a.to(dtype), cache.to(dtype)


@pytest.mark.parametrize("sparsity,top_p,min_keys", P_TRIPLES)
@pytest.mark.parametrize("f", [1500, 17024])
def test_p_form_three_rows_per_group_equal_the_model(dev, f, sparsity, top_p, min_keys):
    a, cache = exact_operands(f, 3, torch.bfloat16)
    want = gdm.run_p(a, cache, 3, sparsity, top_p, min_keys, 256)
    got = fused(dev, a, cache, 3, sparsity, 256, p=(top_p, min_keys), fill=-1)
    assert_same(got, want, f"_p R 3 F {f} {(sparsity, top_p, min_keys)}")
    assert len(set(want[1].flatten().tolist())) > 1, "the groups keep different counts"


# ------------------------------------------------------------------------------------------------------------------ hipGraph
def test_one_call_is_graph_capturable(dev):
    from chipmunk_amd import ops
    a, cache0 = operands("normal", 2, 8, 4096, torch.bfloat16)
    want = fused(dev, a, cache0, 4, 0.7, 256)
    a, cache0 = a.to(dev), cache0.to(dev)
    cache = cache0.clone()
    inds, counts = outputs(dev, 2, 2, 4096)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):     # eager warm-up on the capture stream
        ops.topk_group_delta_indices(a, cache, inds, counts, 4, 0.7, 256, 0.0)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.topk_group_delta_indices(a, cache, inds, counts, 4, 0.7, 256, 0.0)
    cache.copy_(cache0)
    inds.fill_(-9)
    counts.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert_same((inds.cpu(), counts.cpu(), cache.cpu()), want, "graph replay")


def test_chipmunk_alias_has_the_operators():
    import chipmunk
    import chipmunk_amd
    assert chipmunk.ops.topk_group_delta_indices is chipmunk_amd.ops.topk_group_delta_indices
    assert chipmunk.ops.topk_group_delta_indices_p is chipmunk_amd.ops.topk_group_delta_indices_p
