"""The mask step past 122 880 tokens: the streaming form of the top-k mask kernel (topk_mask_stream_kernel) against the written-down
rule (tests/topk_mask_model.py), against the register form where both apply, inside the fused mask step and inside SparseDiffAttn.
Few rows and at most two heads everywhere: these tests ride along with a long suite."""
import math
import os

import pytest
import torch

from helpers import randn_bf16
from topk_mask_model import topk_mask_model

pytestmark = pytest.mark.gpu

REG_MAX_N = 1024 * 120     # longest row of the register form


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(kind, rows, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        x = torch.randn(1, 1, rows, n, generator=g)
    else:                                                # heavy ties: 40 distinct values
        x = torch.randint(0, 40, (1, 1, rows, n), generator=g).float() / 8
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("extras", [True, False], ids=["groups_static", "plain"])
@pytest.mark.parametrize("kind", ["random", "tied"])
@pytest.mark.parametrize("n,rows", [(122884, 3), (131072, 4), (200002, 3), (522240, 2)])
def test_long_rows_equal_the_model(dev, n, rows, kind, extras):
    """Rows longer than the register form takes, random part off: every mask bit is the model's -- threshold, everything above
    it, ties in ((c % 4096) // 4, c) order, group flags, static mask.  200 002 columns take the generic (unaligned) kernel."""
    cs = _rows(kind, rows, n, seed=n + rows)
    groups = static = None
    if extras:
        g = torch.Generator().manual_seed(n)
        groups = torch.tensor([True, False, True, True][:rows]).view(1, 1, rows, 1)
        static = torch.rand(1, 1, rows, n, generator=g) < 0.02
    cs_d = cs.to(dev)
    groups_d = None if groups is None else groups.to(dev)
    static_d = None if static is None else static.to(dev)
    for k in (0, 1, n, round(0.07 * n)):
        out = torch.ops.chipmunk.topk_mask(cs_d, k, 0.0, groups_d, static_d)
        assert out.dtype == torch.bool and out.shape == (1, 1, rows, n)
        ref = topk_mask_model(cs, k, groups, static)
        got = out.cpu()
        assert torch.equal(got, ref), (n, kind, extras, k, int((got != ref).sum()))


def test_rows_past_the_ceiling_are_refused_with_the_number(dev):
    from chipmunk_amd import ops
    cs = torch.zeros(1, 1, 1, ops.TOPK_MASK_MAX_N + 4, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match=str(ops.TOPK_MASK_MAX_N)):
        torch.ops.chipmunk.topk_mask(cs, 16, 0.0, None, None)


@pytest.mark.parametrize("kind", ["random", "tied"])
@pytest.mark.parametrize("n", [4352, 10003, 20000, 119056])
def test_streaming_form_equals_register_form(dev, n, kind):
    """Option topk_mask_stream = 1 sends every row to the streaming kernel: bit-identical to the default dispatch (the register
    form at these lengths), ties and the random part included -- same seed before each call, so both draw the same salt."""
    from chipmunk_amd import _native, ops
    rows = 3
    cs = _rows(kind, rows, n, seed=n).to(dev)
    g = torch.Generator().manual_seed(n + 1)
    static = (torch.rand(1, 1, rows, n, generator=g) < 0.02).to(dev)
    groups = torch.tensor([True, False, True]).view(1, 1, rows, 1).to(dev)
    cases = [(k, ra, gr, st) for k in (0, 1, n, round(0.07 * n)) for ra in (0.0, 0.01) for gr, st in ((groups, static), (None, None))]
    base = []
    for i, (k, ra, gr, st) in enumerate(cases):
        ops.manual_seed(100 + i)
        base.append(torch.ops.chipmunk.topk_mask(cs, k, ra, gr, st))
    _native.set_option("topk_mask_stream", 1)
    try:
        for i, (k, ra, gr, st) in enumerate(cases):
            ops.manual_seed(100 + i)
            got = torch.ops.chipmunk.topk_mask(cs, k, ra, gr, st)
            assert torch.equal(got, base[i]), (n, kind, k, ra, gr is not None, int((got != base[i]).sum()))
        torch.cuda.synchronize()
    finally:
        _native.set_option("topk_mask_stream", 0)
    # the model agrees with both where the random part is off
    k = round(0.07 * n)
    got = torch.ops.chipmunk.topk_mask(cs, k, 0.0, groups, static)
    assert torch.equal(got.cpu(), topk_mask_model(cs.cpu(), k, groups.cpu(), static.cpu()))


def test_random_part_at_long_rows(dev):
    """n = 131 072, k = 8192, random_amount = 0.01: the extra columns of an active row are Binomial(122 880, 0.01) = 1229 +- 6 sigma
    (sigma = 34.9, 6 sigma = 210); inactive rows get none; the random part only adds."""
    from chipmunk_amd import ops
    n, k, rows = 131072, 8192, 4
    cs = _rows("random", rows, n, seed=77).to(dev)
    groups = torch.tensor([True, False, True, True]).view(1, 1, rows, 1).to(dev)
    plain = torch.ops.chipmunk.topk_mask(cs, k, 0.0, groups, None)
    ops.manual_seed(5)
    out = torch.ops.chipmunk.topk_mask(cs, k, 0.01, groups, None)
    act = groups.view(-1)
    assert (plain.sum(-1).view(-1)[act] == k).all() and (plain.sum(-1).view(-1)[~act] == 0).all()
    extra = (out.sum(-1) - plain.sum(-1)).view(-1)
    print("extra columns per row:", extra.tolist())
    assert (extra[~act] == 0).all()
    assert ((extra[act] >= 1229 - 210) & (extra[act] <= 1229 + 210)).all(), extra.tolist()
    assert (out | ~plain).all(), "the random part only adds"


@pytest.mark.parametrize("n,nk,heads", [(1536, 131072, 2), (123008, 123008, 1)])
def test_fused_mask_step_equals_colsum_then_topk_mask_past_122880_keys(dev, n, nk, heads):
    """chipmunk.dense_colsum_topk_mask (the mask kernel combines a group's partial column-sum rows itself, once, and streams the
    keys) against dense_colsum_attn followed by topk_mask: o, l and the mask bit for bit."""
    from chipmunk_amd import _native, ops
    G = math.ceil(n / 192)
    q = randn_bf16(1, heads, n, 128, seed=n + 1).to(dev)
    k = randn_bf16(1, heads, nk, 128, seed=nk + 2).to(dev)
    v = randn_bf16(1, heads, nk, 128, seed=nk + 3).to(dev)
    gen = torch.Generator().manual_seed(7)
    static = (torch.rand(1, heads, G, nk, generator=gen) < 0.02).to(dev)
    groups = (torch.rand(1, heads, G, 1, generator=gen) < 0.8).to(dev)
    ktop = 128
    for opt in ("attn_dense64", "attn_colsum64"):
        _native.set_option(opt, 1)
    try:
        _, l0 = ops.dense_attn(q, k, v)
        o_a, cs, l_a = ops.dense_colsum_attn(q, k, v, l0)
        cs = cs[..., :G, :nk]
        m_a = ops.topk_mask(cs, ktop, 0.0, groups, static)
        o_b, m_b, l_b = ops.dense_colsum_topk_mask(q, k, v, l0, ktop, 0.0, groups, static)
        torch.cuda.synchronize()
    finally:
        for opt in ("attn_dense64", "attn_colsum64"):
            _native.set_option(opt, 0)
    assert torch.equal(o_a, o_b) and torch.equal(l_a, l_b)
    assert m_b.shape == (1, heads, G, nk) and torch.equal(m_a, m_b)
    assert (m_b.sum(-1)[groups[..., 0]] >= ktop).all()


@pytest.mark.parametrize("n,nk,heads", [(1536, 1536, 2), (1000, 1000, 2), (960, 2304, 2)])
def test_fused_mask_step_streaming_form_equals_register_form(dev, n, nk, heads):
    """The PARTS shape of the streaming kernel at lengths the register form takes too: same o, l and mask from the fused mask step
    with topk_mask_stream = 1 as without, random part on (same seed)."""
    from chipmunk_amd import _native, ops
    G = math.ceil(n / 192)
    q = randn_bf16(1, heads, n, 128, seed=n + 1).to(dev)
    k = randn_bf16(1, heads, nk, 128, seed=nk + 2).to(dev)
    v = randn_bf16(1, heads, nk, 128, seed=nk + 3).to(dev)
    gen = torch.Generator().manual_seed(7)
    static = (torch.rand(1, heads, G, nk, generator=gen) < 0.02).to(dev)
    groups = (torch.rand(1, heads, G, 1, generator=gen) < 0.8).to(dev)
    opts = ("attn_dense64", "attn_colsum64")
    for opt in opts:
        _native.set_option(opt, 1)
    try:
        _, l0 = ops.dense_attn(q, k, v)
        res = []
        for stream in (0, 1):
            _native.set_option("topk_mask_stream", stream)
            for ra in (0.0, 0.01):
                ops.manual_seed(9)
                res.append(ops.dense_colsum_topk_mask(q, k, v, l0, 128, ra, groups, static))
        torch.cuda.synchronize()
    finally:
        for opt in opts + ("topk_mask_stream",):
            _native.set_option(opt, 0)
    for a, b in zip(res[:2], res[2:]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_module_takes_the_hip_mask_step_past_122880_tokens(fresh_config, monkeypatch):
    """SparseDiffAttn at N = 123 136 with the shipped HunyuanVideo configuration: the mask step of step 1 goes through
    ops.dense_colsum_topk_mask, not through the torch chain (torch.randint + topk + scatter_), and unchanged q, k, v reproduce the
    dense output through steps 0, 1 and a sparse step (2e-2 for full steps, 6e-2 for the sparse one)."""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.util import config as cfgmod
    from chipmunk_amd.util.layer_counter import LayerCounter
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfgmod.load_from_file(os.path.join(root, "configs", "hunyuan_c3.yml"))
    cfg = fresh_config
    cfg["steps"] = 50
    dev = torch.device("cuda:0")
    H, vid, txt = 2, (40, 48, 64), 256
    N = vid[0] * vid[1] * vid[2] + txt
    assert N == 123136 and N > REG_MAX_N
    L = cfg["attn"]["first_n_dense_layers"] + 1          # the dense layers of the configuration and one sparse layer
    g = torch.Generator().manual_seed(11)
    q, k, v = [torch.randn(1, H, N, 128, generator=g).to(torch.bfloat16).to(dev) for _ in range(3)]
    layers = []
    for _ in range(L):
        layer_num, counter = LayerCounter.build_for_layer(is_attn_sparse=True)
        layers.append(SparseDiffAttn(layer_num, counter))
    layers[0].initialize_static_mask(vid, txt, H, dev)
    calls = {"fused": 0, "randint": 0}
    real_fused, real_randint = ops.dense_colsum_topk_mask, torch.randint

    def spy_fused(*a, **kw):
        calls["fused"] += 1
        return real_fused(*a, **kw)

    def spy_randint(*a, **kw):
        calls["randint"] += 1
        return real_randint(*a, **kw)

    monkeypatch.setattr(ops, "dense_colsum_topk_mask", spy_fused)
    monkeypatch.setattr(torch, "randint", spy_randint)
    dense = torch.ops.chipmunk.dense_attn(q, k, v)[0]
    invocations = cfg["num_model_invocations_per_inference_step"]
    try:
        for step in range(3):
            full = step < 2
            for _ in range(invocations):
                for li, layer in enumerate(layers):
                    assert counter.cur_inference_step == step and counter.should_do_full_attn_step() == full
                    if step > 0 or li > 0:
                        layer.storage.load_async_wait()
                    layers[(li + 1) % L].storage.load_async()
                    out = layer(q, k, v)
                    err = (out.float() - dense.float()).abs().max().item()
                    print(f"step {step} layer {li}: max |o - dense| = {err:.4g}")
                    assert err < (2e-2 if full or li < L - 1 else 6e-2), (step, li, err)
            if step == 1:
                assert calls["fused"] == invocations, calls
        torch.cuda.synchronize()
    finally:
        for layer in layers:
            layer.release_kept_indices()
    assert calls["fused"] == invocations and calls["randint"] == 0, calls
