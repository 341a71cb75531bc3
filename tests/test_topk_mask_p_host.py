"""Top-p key selection under the top-k cap (``chipmunk_topk_mask_p``) without a GPU: the written-down rule
(tests/topk_mask_p_model.py) against brute force, the CPU path of ``ops.topk_mask_p`` against the rule, the reach of the GPU test's
exact-row generator, and ``SparseDiffAttn`` on CPU tensors with ``attn.top_p`` on and off."""
import pytest
import torch

from topk_mask_model import topk_mask_model
from topk_mask_p_model import brute_force_row, exact_rows, regime, threshold_inside_tie_class, topk_mask_p_model, topp_row

# the exact-row cases of tests/test_gpu_topk_mask_p.py: (n, hot) per kernel form, k = n // 4, k_min = 64
EXACT_N = (1001, 4100, 20000, 60000, 131072)
EXACT_TOP_P = (0.5, 0.75)
K_MIN = 64


def exact_hots(n):
    return (4, n // 64, n // 8)


def _short_row(n, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 12, (n,), generator=g).float() / 8        # heavy ties, sums exact in any float format
    if special:
        x[torch.randperm(n, generator=g)[:3]] = torch.tensor([-1.0, float("nan"), -0.0])
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("special", [False, True], ids=["plain", "negative_nan"])
def test_model_equals_brute_force_on_short_rows(special):
    seen = set()
    for seed in range(40):
        n = (5, 17, 64, 200, 4099 + 9)[seed % 5]
        row = _short_row(n, seed, special)
        for top_p in (0.25, 0.5, 0.9, 1.0):
            for k, k_min in ((n, 0), (n // 3, 0), (n // 2, n // 8), (3, 5), (0, 0)):
                keep, s, k_p = topp_row(row, k, top_p, k_min)
                want, ws, wk = brute_force_row(row, k, top_p, k_min)
                assert (s, k_p) == (ws, wk), (seed, n, top_p, k, k_min)
                assert set(torch.nonzero(keep).flatten().tolist()) == want and int(keep.sum()) == s
                seen.add(regime((s, k_p), min(k, n), k_min))
    assert seen == {"k_min", "top_p", "cap"}


def test_model_edge_rows():
    zero = torch.zeros(40, dtype=torch.bfloat16)
    assert topp_row(zero, 10, 0.9, 0)[1:] == (0, 0) and topp_row(zero, 10, 0.9, 4)[1:] == (4, 0)
    neg = torch.full((40,), -1.0, dtype=torch.bfloat16)                 # no mass at all: as the all-zero row
    assert topp_row(neg, 10, 0.9, 0)[1:] == (0, 0)
    one = torch.zeros(40, dtype=torch.bfloat16)
    one[7] = 3.0
    keep, s, k_p = topp_row(one, 10, 1.0, 0)
    assert (s, k_p) == (1, 1) and bool(keep[7])
    flat = torch.ones(4100, dtype=torch.bfloat16)                        # one tie class: the first s columns of the thread order
    keep, s, k_p = topp_row(flat, 4100, 0.5, 0)
    assert (s, k_p) == (2050, 2050)
    cols = torch.nonzero(keep).flatten()
    assert bool(keep[4096:4100].all()) and int(cols[cols < 4096].max()) == 2045      # thread 0 owns columns 0..3 and 4096..4099


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "groups_static"])
def test_cpu_path_of_the_operator_equals_the_model(extras):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    for n, hot, seed in ((1001, 125, 1), (4100, 64, 2), (300, 4, 3)):
        cs = exact_rows(3, n, hot, seed)
        cs[0, 0, 1, :5] = torch.tensor([-2.0, float("nan"), -0.0, 0.0, 1.0]).to(torch.bfloat16)
        groups = static = None
        if extras:
            groups = torch.tensor([True, False, True]).view(1, 1, 3, 1)
            static = torch.rand(1, 1, 3, n, generator=torch.Generator().manual_seed(n)) < 0.02
        for top_p in (0.5, 0.75, 0.93, 1.0):
            for k, k_min in ((n // 4, K_MIN), (n, 0), (0, 0), (7, 9)):
                want, counts = topk_mask_p_model(cs, k, top_p, k_min, groups, static)
                got = ops.topk_mask_p(cs, k, top_p, k_min, 0.0, groups, static)
                assert got.dtype == torch.bool and torch.equal(got, want), (n, top_p, k, k_min)
                if not extras:
                    assert torch.equal(got.sum(-1).view(-1), counts[:, 0])
    # the random part only adds, and only to active rows
    cs = exact_rows(2, 4100, 64, 9)
    groups = torch.tensor([True, False]).view(1, 1, 2, 1)
    plain = ops.topk_mask_p(cs, 1000, 0.75, K_MIN, 0.0, groups, None)
    torch.manual_seed(3)
    rnd = ops.topk_mask_p(cs, 1000, 0.75, K_MIN, 0.05, groups, None)
    assert (rnd | ~plain).all() and int(rnd[0, 0, 1].sum()) == 0 and int(rnd[0, 0, 0].sum()) > int(plain[0, 0, 0].sum())
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(k_min=-1)):
        with pytest.raises(ValueError):
            ops.topk_mask_p(cs, 10, **{"top_p": 0.5, "k_min": 0, **bad})


def test_top_p_one_with_no_cap_keeps_every_column_with_mass_and_cap_alone_is_topk():
    """Two anchors to the existing rule: with ``top_p`` reaching past the cap the kept set is ``topk_mask_model``'s for k, and with
    k_min >= k likewise."""
    cs = exact_rows(2, 4100, 64, 4)
    k = 200
    want = topk_mask_model(cs, k)
    got, counts = topk_mask_p_model(cs, k, 1.0, 0)
    assert torch.equal(got, want) and (counts[:, 0] == k).all() and (counts[:, 1] > k).all()
    got, _ = topk_mask_p_model(cs, k, 0.5, k)
    assert torch.equal(got, want)


def test_exact_row_generator_reaches_the_three_regimes_inside_tie_classes():
    """Over the GPU test's own cases (same generator, same seeds: ``seed = n + hot``) every regime -- k_p < k_min, k_min <= k_p < k,
    k_p >= k -- occurs with the end of the kept set inside a class of equal keys, and n = 1001, hot = 125, top_p = 0.5 is a k_min row."""
    inside = set()
    for n in EXACT_N[:4]:                                   # (131 072 columns use the same generator; the sort is what takes the time here)
        for hot in exact_hots(n):
            cs = exact_rows(6, n, hot, seed=n + hot)
            for top_p in EXACT_TOP_P:
                _, counts = topk_mask_p_model(cs, n // 4, top_p, K_MIN)
                for r in range(6):
                    reg = regime(counts[r], n // 4, K_MIN)
                    if threshold_inside_tie_class(cs[0, 0, r], int(counts[r, 0])):
                        inside.add(reg)
                    if (n, hot, top_p) == (1001, 125, 0.5):
                        assert reg == "k_min", counts[r].tolist()
    assert inside == {"k_min", "top_p", "cap"}, inside


# ------------------------------------------------------------------------------------------------------------------ module
@pytest.fixture()
def cpu_chipmunk(fresh_config):
    import cpu_ops
    cpu_ops.register()
    fresh_config["offloading"]["global_disable_offloading"] = True
    fresh_config["steps"] = 50
    return fresh_config


H, VID, TXT = 2, (4, 12, 16), 50
N = VID[0] * VID[1] * VID[2] + TXT          # 818: four full groups and one of 50 rows


def _run_module(cfg, top_p, min_keys=0.0, steps=3, compressed=True, set_keys=True):
    """Steps 0, 1 (mask), 2 (sparse) of one sparse layer on CPU tensors; returns (outputs, stored bool mask).  ``set_keys`` off: the
    two keys are absent from the live configuration, as in a section copied from the reference."""
    from chipmunk_amd import ops
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.util.layer_counter import LayerCounter
    from helpers import structured_qkv
    cfg["attn"].update(dict(top_keys=0.3, random_keys=0.0, local_voxels=0, first_n_dense_layers=0, recompute_mask=True,
                            should_compress_indices=compressed, counts_multiple_of=128, pad_qkv_before_kernel=True,
                            full_step_schedule={0, 1}))
    for key, val in (("top_p", top_p), ("top_p_min_keys", min_keys)):
        if set_keys:
            cfg["attn"][key] = val
        else:
            cfg["attn"].pop(key, None)
    counter = LayerCounter(1, 1)
    layer = SparseDiffAttn(0, counter)
    torch.manual_seed(5)
    layer.initialize_static_mask(VID, TXT, H, torch.device("cpu"))
    outs = []
    for step in range(steps):
        q, k, v, _ = structured_qkv(H, N, 24, step, 0)
        torch.manual_seed(100 + step)                   # (the torch chain of top_p = 0 draws its 1 % from torch's generator)
        outs.append(layer(q, k, v).clone())
    mask = ops.bitunpack(layer.storage.get_indices(), layer.mask_shape[0]) if compressed and steps > 1 else None
    return outs, mask


def test_module_top_p_zero_is_todays_module(cpu_chipmunk, monkeypatch):
    """``attn.top_p = 0``: the operators of the per-group count are never called and the masks and outputs are bit for bit those of a
    configuration that does not know the keys at all."""
    from chipmunk_amd import ops
    from chipmunk_amd.util import config as cfgmod
    from chipmunk_amd.util import layer_counter as lc

    def boom(*a, **kw):
        raise AssertionError("a top-p operator was called with attn.top_p = 0")

    monkeypatch.setattr(ops, "topk_mask_p", boom)
    monkeypatch.setattr(ops, "dense_colsum_topk_mask_p", boom)
    outs0, mask0 = _run_module(cpu_chipmunk, 0.0)
    cfgmod.reset_to_base()
    lc.singleton.__init__(0, 0)
    cfg = cfgmod.GLOBAL_CONFIG
    cfg["offloading"]["global_disable_offloading"] = True
    outs1, mask1 = _run_module(cfg, 0.0, set_keys=False)          # amd_key() supplies the default
    assert "top_p" not in cfg["attn"]
    assert torch.equal(mask0, mask1)
    for a, b in zip(outs0, outs1):
        assert torch.equal(a, b)


def test_module_with_top_p_keeps_a_count_per_group(cpu_chipmunk):
    outs_k, mask_k = _run_module(cpu_chipmunk, 0.0)
    from chipmunk_amd.util import layer_counter as lc
    lc.singleton.__init__(0, 0)
    outs_p, mask_p = _run_module(cpu_chipmunk, 0.9, min_keys=0.0)
    from chipmunk_amd.modules import attn as attn_mod
    sparse = attn_mod.singleton_video_query_groups.expand(1, H, -1, 1)[..., 0]
    static = attn_mod.singleton_static_mask
    tk = int(128 * round(0.3 * N / 128))
    # top_p = 0: every sparse group keeps tk keys + 1 % random + static; top_p = 0.9 under the same cap: fewer, and not the same number everywhere
    own_k = (mask_k & ~static).sum(-1)[sparse]
    own_p = (mask_p & ~static).sum(-1)[sparse]
    print("kept keys per sparse group, top_keys alone:", own_k.tolist(), " with top_p = 0.9:", own_p.tolist())
    assert (own_k >= tk - static.sum(-1)[sparse]).all()
    assert (own_p <= tk + 0.05 * N).all() and len(set(own_p.tolist())) > 1, own_p.tolist()
    assert int(own_p.sum()) < int(own_k.sum())
    assert torch.equal(mask_p[~sparse], static.expand_as(mask_p)[~sparse])          # a group flagged non-sparse keeps its static mask
    # full steps are dense attention either way; the sparse step differs because the kept sets do
    assert torch.equal(outs_k[0], outs_p[0]) and torch.equal(outs_k[1], outs_p[1])
    assert outs_p[2].shape == outs_k[2].shape and torch.isfinite(outs_p[2].float()).all()


def test_top_p_is_refused_for_fixed_width_indices(cpu_chipmunk):
    with pytest.raises(ValueError, match="attn.top_p") as e:
        _run_module(cpu_chipmunk, 0.9, compressed=False, steps=2)
    assert "attn.should_compress_indices" in str(e.value)


def test_new_keys_are_extra_keys_with_the_feature_off():
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["attn.top_p"] == 0.0 and cfg.AMD_EXTRA_KEYS["attn.top_p_min_keys"] == 0.0
    assert cfg.BASE_CONFIG["attn"]["top_p"] == 0.0 and cfg.BASE_CONFIG["attn"]["top_p_min_keys"] == 0.0


def test_fake_kernels_and_aliases():
    import chipmunk  # noqa: F401
    import chipmunk_amd
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert chipmunk.ops.topk_mask_p is chipmunk_amd.ops.topk_mask_p
    assert chipmunk.ops.dense_colsum_topk_mask_p is chipmunk_amd.ops.dense_colsum_topk_mask_p
    with FakeTensorMode():
        cs = torch.empty(1, 2, 3, 400, dtype=torch.bfloat16)
        m = torch.ops.chipmunk.topk_mask_p(cs, 100, 0.9, 8, 0.0, None, None)
        assert m.shape == cs.shape and m.dtype == torch.bool
        q = torch.empty(1, 2, 400, 128, dtype=torch.bfloat16)
        p = torch.empty(1, 2, 400, 1)
        o, m, l = torch.ops.chipmunk.dense_colsum_topk_mask_p(q, q, q, p, 100, 0.9, 8, 0.0, None, None)
        assert o.shape == q.shape and m.shape == (1, 2, 3, 400) and m.dtype == torch.bool and l.shape == (1, 2, 400, 1)
