"""Top-p key selection under the top-k cap on the GPU (``chipmunk_topk_mask_p``): every kernel form against the
written-down rule (tests/topk_mask_p_model.py) on rows whose sums are exact in fp32 -- bit-equal masks, ties included --, the rule's
property on random rows, the random part, the fused mask step, the untouched ``topk_mask`` and ``SparseDiffAttn`` with ``attn.top_p``.
Six rows per launch and one reference per case, shared by the variants of the case."""
import math

import pytest
import torch

import helpers
from helpers import randn_bf16
from topk_mask_model import bf16_keys, topk_mask_model
from topk_mask_p_model import exact_rows, row_order, topk_mask_p_model

pytestmark = pytest.mark.gpu

K_MIN = 64
SHAPE = (1, 2, 3)                       # rows are [1, 2, 3, n]
# (n, option topk_mask_stream, form)
FORMS = [(1001, 0, "generic, unaligned"), (4100, 0, "KPT 16, two 4096-column steps"), (20000, 0, "KPT 48"), (60000, 0, "KPT 120"),
         (4100, 1, "streaming form at a small size"), (131072, 0, "streaming by size")]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class stream_option:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from chipmunk_amd import _native
        if self.on:
            _native.set_option("topk_mask_stream", 1)

    def __exit__(self, *exc):
        from chipmunk_amd import _native
        if self.on:
            torch.cuda.synchronize()
            _native.set_option("topk_mask_stream", 0)
        return False


def _exact_case(n, hot):
    return exact_rows(6, n, hot, seed=n + hot).view(*SHAPE, n)


def _extras(n):
    g = torch.Generator().manual_seed(n)
    static = torch.rand(*SHAPE, n, generator=g) < 0.02
    groups = torch.tensor([True, True, False, True, True, True]).view(*SHAPE, 1)        # one inactive row
    return groups, static


@pytest.mark.parametrize("n,stream,form", FORMS, ids=[f"{n}{'-stream' if s else ''}" for n, s, _ in FORMS])
def test_exact_rows_equal_the_model_in_every_bit(dev, n, stream, form):
    """Integer column sums (background {0, 1, 2}, ``hot`` columns at 2^3 .. 2^7): every value, every partial sum in any order and
    ``top_p * total`` are exact in fp32 for top_p in {0.5, 0.75}, so the kernel must equal the fp64 rule bit for bit -- the count per
    row, the threshold, the ties in ((c % 4096) // 4, c) order.  With and without a static mask and an inactive row."""
    from chipmunk_amd import ops
    k = n // 4
    groups, static = _extras(n)
    regimes = set()
    for hot in (4, n // 64, n // 8):
        cs = _exact_case(n, hot)
        cs_d = cs.to(dev)
        for top_p in (0.5, 0.75):
            want, counts = topk_mask_p_model(cs, k, top_p, K_MIN)
            with stream_option(stream):
                got = ops.topk_mask_p(cs_d, k, top_p, K_MIN, 0.0, None, None)
                got_x = ops.topk_mask_p(cs_d, k, top_p, K_MIN, 0.0, groups.to(dev), static.to(dev))
                got, got_x = got.cpu(), got_x.cpu()
            s_got = got.sum(-1).view(-1)
            print(f"n {n} ({form}) hot {hot} top_p {top_p}: s {s_got.tolist()} model (s, k_p) {counts.tolist()}")
            assert got.dtype == torch.bool and got.shape == cs.shape
            assert torch.equal(s_got, counts[:, 0]), (n, hot, top_p)
            assert torch.equal(got, want), (n, hot, top_p, int((got != want).sum()))
            assert torch.equal(got_x, (want & groups) | static), (n, hot, top_p)
            assert torch.equal(got_x[0, 0, 2], static[0, 0, 2]), "the inactive row is its static part"
            for s, k_p in counts.tolist():
                regimes.add("k_min" if k_p < K_MIN else ("top_p" if k_p < k else "cap"))
            if (n, hot, top_p) == (1001, 125, 0.5):
                assert (counts[:, 1] < K_MIN).all() and (s_got == K_MIN).all(), "n = 1001, hot = 125, top_p = 0.5 is a k_min row"
    print(f"n {n}: regimes seen {sorted(regimes)}")
    assert {"top_p", "cap"} <= regimes


@pytest.mark.parametrize("n,stream,form", FORMS, ids=[f"{n}{'-stream' if s else ''}" for n, s, _ in FORMS])
def test_plain_topk_mask_is_unchanged_on_the_exact_rows(dev, n, stream, form):
    """The existing operator (the kernels' MASS = false instantiations) still equals its own model, on the same rows."""
    from chipmunk_amd import ops
    cs = _exact_case(n, n // 64)
    groups, static = _extras(n)
    k = n // 4
    want = topk_mask_model(cs, k, groups, static)
    with stream_option(stream):
        got = ops.topk_mask(cs.to(dev), k, 0.0, groups.to(dev), static.to(dev)).cpu()
    assert torch.equal(got, want), (n, int((got != want).sum()))


@pytest.mark.parametrize("n", [4100, 60000])
def test_random_rows_have_the_property(dev, n):
    """cs = bf16(192 softmax(3 randn)): the kept set is a top set of the order, min(k, k_min) <= s <= k, and in fp64, with
    eps = n 2^-24 (the bound of any-order fp32 summation of n non-negative terms): mass(S) >= top_p total (1 - 2 eps) unless s = k,
    mass(S minus its last column) < top_p total (1 + 2 eps) unless s = k_min.  Two launches give the same bits."""
    from chipmunk_amd import ops
    rows = 4
    g = torch.Generator().manual_seed(n)
    cs = (192.0 * torch.softmax(3.0 * torch.randn(rows, n, generator=g, dtype=torch.float64), dim=-1)).to(torch.bfloat16).view(1, 1, rows, n)
    cs_d = cs.to(dev)
    eps = n * 2.0 ** -24
    orders = [row_order(bf16_keys(cs[0, 0, r])) for r in range(rows)]
    for top_p in (0.9, 0.99):
        for k in (n, n // 8):
            a = ops.topk_mask_p(cs_d, k, top_p, K_MIN, 0.0, None, None)
            b = ops.topk_mask_p(cs_d, k, top_p, K_MIN, 0.0, None, None)
            assert torch.equal(a, b), "two launches, the same bits"
            got = a.cpu()
            for r in range(rows):
                keep, order = got[0, 0, r], orders[r]
                s = int(keep.sum())
                assert min(k, K_MIN) <= s <= k, (n, top_p, k, r, s)
                assert bool(keep[order[:s]].all()), "the kept set is a top set of the order"
                mass = cs[0, 0, r].double().clamp(min=0)[order]
                total, target = float(mass.sum()), top_p * float(mass.sum())
                m_s, m_less = float(mass[:s].sum()), float(mass[:s - 1].sum())
                print(f"n {n} top_p {top_p} k {k} row {r}: s {s}, mass(S) / target - 1 = {m_s / target - 1:+.3e}, "
                      f"mass(S - last) / target - 1 = {m_less / target - 1:+.3e}, 2 eps = {2 * eps:.3e}")
                if s != k:
                    assert m_s >= target * (1 - 2 * eps), (n, top_p, k, r, s, m_s, target)
                if s != K_MIN:
                    assert m_less < target * (1 + 2 * eps), (n, top_p, k, r, s, m_less, target)


def test_random_part_only_adds(dev):
    from chipmunk_amd import ops
    n = 4100
    cs = _exact_case(n, n // 64).to(dev)
    groups, static = _extras(n)
    plain = ops.topk_mask_p(cs, n // 4, 0.75, K_MIN, 0.0, groups.to(dev), None)
    ops.manual_seed(5)
    rnd = ops.topk_mask_p(cs, n // 4, 0.75, K_MIN, 0.05, groups.to(dev), None)
    assert (rnd | ~plain).all(), "the mask contains the random_amount = 0 mask"
    extra = (rnd & ~plain).sum(-1).view(-1)
    act = groups.view(-1).to(dev)
    free = (n - plain.sum(-1).view(-1)).float()
    print("extra columns per row:", extra.tolist(), "expected about", (0.05 * free).tolist())
    assert (extra[~act] == 0).all()
    # Binomial(free, 0.05): mean 0.05 free, sigma <= sqrt(0.05 * 0.95 * 4100) = 14; 6 sigma = 84
    assert ((extra[act].float() - 0.05 * free[act]).abs() <= 84).all(), extra.tolist()


@pytest.mark.parametrize("n,nk,heads", [(1536, 1536, 4), (1000, 1000, 3), (2304, 2304, 2), (960, 2304, 2)])
def test_fused_mask_step_equals_colsum_then_topk_mask_p(dev, n, nk, heads):
    """chipmunk.dense_colsum_topk_mask_p against dense_colsum_attn followed by topk_mask_p: o, l and the mask bit for bit (the shapes
    and the one-pass forcing of tests/test_gpu_attn64.py::test_fused_mask_step_equals_colsum_then_topk_mask), with the cap out of
    reach (k_top = nk) and binding (k_top = 128)."""
    from chipmunk_amd import _native, ops
    G = math.ceil(n / 192)
    q = randn_bf16(1, heads, n, 128, seed=n + 1).to(dev)
    k = randn_bf16(1, heads, nk, 128, seed=nk + 2).to(dev)
    v = randn_bf16(1, heads, nk, 128, seed=nk + 3).to(dev)
    gen = torch.Generator().manual_seed(7)
    static = (torch.rand(1, heads, G, nk, generator=gen) < 0.02).to(dev)
    groups = (torch.rand(1, heads, G, 1, generator=gen) < 0.8).to(dev)
    for opt in ("attn_dense64", "attn_colsum64"):
        _native.set_option(opt, 1)
    try:
        _, l0 = ops.dense_attn(q, k, v)
        o_a, cs, l_a = ops.dense_colsum_attn(q, k, v, l0)
        cs = cs[..., :G, :nk]
        res = []
        for ktop, top_p in ((nk, 0.5), (nk, 0.9), (128, 0.9)):
            m_a = ops.topk_mask_p(cs, ktop, top_p, K_MIN, 0.0, groups, static)
            o_b, m_b, l_b = ops.dense_colsum_topk_mask_p(q, k, v, l0, ktop, top_p, K_MIN, 0.0, groups, static)
            res.append((ktop, top_p, m_a, o_b, m_b, l_b))
        torch.cuda.synchronize()
    finally:
        for opt in ("attn_dense64", "attn_colsum64"):
            _native.set_option(opt, 0)
    counts = []
    for ktop, top_p, m_a, o_b, m_b, l_b in res:
        assert torch.equal(o_a, o_b) and torch.equal(l_a, l_b)
        assert m_b.shape == (1, heads, G, nk) and torch.equal(m_a, m_b), (ktop, top_p, int((m_a != m_b).sum()))
        own = (m_b & ~static).sum(-1)[groups[..., 0]]
        counts.append(own)
        assert (own <= ktop).all()
    print("kept keys per active group, top_p 0.5 / 0.9 without cap:", counts[0].tolist(), counts[1].tolist())
    assert (counts[0] <= counts[1]).all() and (counts[0] < counts[1]).any()


def test_module_with_top_p(fresh_config):
    """SparseDiffAttn with attn.top_p = 0.9, compressed indices, H = 2, N = 818 (four full groups and one of 50 rows), structured
    inputs, steps 0, 1, 2: the stored mask's rows do not all hold the same number of keys, and the sparse step's output is within
    ROW_ERR_BOUND of cache + exact fp64 attention over the stored mask.  The keys of a group are the mask's row, its count rounded
    up to counts_multiple_of with the first columns that are not in it -- the method's own rounding (tests/method_model.py
    ``kept_from_mask``), which the top-p count does not change."""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.modules import attn as attn_mod
    from chipmunk_amd.util.layer_counter import LayerCounter
    from method_model import kept_from_mask
    dev = torch.device("cuda:0")
    cfg = fresh_config
    cfg["steps"] = 50
    cfg["offloading"]["global_disable_offloading"] = True
    H, vid, txt = 2, (4, 12, 16), 50
    N = vid[0] * vid[1] * vid[2] + txt
    assert N == 818
    cfg["attn"].update(dict(top_keys=0.3, random_keys=0.0, local_voxels=0, first_n_dense_layers=0, recompute_mask=True,
                            should_compress_indices=True, counts_multiple_of=128, pad_qkv_before_kernel=True,
                            full_step_schedule={0, 1}, top_p=0.9, top_p_min_keys=0.0))
    layer = SparseDiffAttn(0, LayerCounter(1, 1))
    torch.manual_seed(5)
    layer.initialize_static_mask(vid, txt, H, dev)
    calls = {"p": 0}
    real = ops.dense_colsum_topk_mask_p, ops.topk_mask_p

    def spy(fn):
        def inner(*a, **kw):
            calls["p"] += 1
            return fn(*a, **kw)
        return inner

    ops.dense_colsum_topk_mask_p, ops.topk_mask_p = spy(real[0]), spy(real[1])
    try:
        for step in range(3):
            q, k, v, _ = helpers.structured_qkv(H, N, 24, step, 0)
            q, k, v = q.to(dev), k.to(dev), v.to(dev)
            out = layer(q, k, v).clone()
            if step == 1:
                cache = layer.storage.get_out_cache().clone()
                mask = ops.bitunpack(layer.storage.get_indices(), layer.mask_shape[0]).clone()
        torch.cuda.synchronize()
    finally:
        ops.dense_colsum_topk_mask_p, ops.topk_mask_p = real
        layer.release_kept_indices()
    assert calls["p"] == 1, "the mask step of step 1 went through a top-p operator"
    sparse = attn_mod.singleton_video_query_groups.expand(1, H, -1, 1)[..., 0]
    per_row = mask.sum(-1)
    print("kept keys per (head, group):", per_row.tolist(), "sparse groups:", sparse.tolist())
    assert sparse.any() and len(set(per_row[sparse].tolist())) > 1, "the stored mask's row counts are not all equal"
    # the 24 hot keys of structured_qkv carry 24 e^6 / (24 e^6 + 794 e^0.03) = 0.92 of every row's mass: k_p <= 24 where top_keys
    # alone keeps 256, and the random 1 % adds Binomial(818, 0.01): 8 + 6 sigma = 25
    own = (mask & ~attn_mod.singleton_static_mask).sum(-1)[sparse]
    print("of them outside the static mask:", own.tolist())
    assert (own <= 24 + 25).all(), own.tolist()
    assert torch.equal(layer.storage.get_out_cache(), cache), "a sparse step leaves the cache alone"
    inds, counts = kept_from_mask(mask, 128)
    G = mask.shape[2]
    exact = torch.zeros(1, H, N, 128, dtype=torch.float64, device=dev)
    for g in range(G):
        keep = torch.zeros(1, H, N, dtype=torch.bool, device=dev)
        for h in range(H):
            keep[0, h, inds[0, h, g, : int(counts[0, h, g])].long()] = True
        assert (keep | ~mask[:, :, g]).all()
        r0, r1 = g * 192, min(N, (g + 1) * 192)
        exact[:, :, r0:r1] = helpers.attn_exact(q, k, v, rows=(r0, r1), keep=keep)
    helpers.assert_delta_rows_close(out, cache, exact, what="SparseDiffAttn top_p = 0.9, sparse step")
