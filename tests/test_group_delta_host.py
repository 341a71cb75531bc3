"""``topk_group_delta_indices[_p]`` without a GPU: schemas, exported symbols, argument errors as codes with messages, the config key, the
CPU model against the plain torch chain, and the modules' unchanged op sequence with the key off."""
import ctypes
import os
import re

import pytest
import torch

import group_delta_model as gdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMAS = {
    "topk_group_delta_indices": "chipmunk::topk_group_delta_indices(Tensor activation, Tensor(cache!) cache, Tensor(indices!) indices, "
                                "Tensor(counts!) counts, int rows_per_group, float sparsity_amount, int multiple_of, float random_amount) -> ()",
    "topk_group_delta_indices_p": "chipmunk::topk_group_delta_indices_p(Tensor activation, Tensor(cache!) cache, Tensor(indices!) indices, "
                                  "Tensor(counts!) counts, int rows_per_group, float sparsity_amount, float top_p, float min_keys, "
                                  "int multiple_of, float random_amount) -> ()",
}


def _reset():
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_registered_schema(name):
    import chipmunk_amd  # noqa: F401
    assert str(getattr(torch.ops.chipmunk, name).default._schema) == SCHEMAS[name]


def test_symbols_are_declared_exported_and_listed():
    from chipmunk_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(chipmunk_[a-z0-9_]+)\s*\(", text))
    lib = _native.lib()
    for name in ("chipmunk_topk_group_delta_indices", "chipmunk_topk_group_delta_indices_p"):
        assert name in declared and name in _native.SYMBOLS and hasattr(lib, name)


def test_python_wrappers_and_alias():
    import chipmunk
    import chipmunk_amd
    for name in SCHEMAS:
        assert name in chipmunk_amd.ops.__all__
        assert getattr(chipmunk.ops, name) is getattr(chipmunk_amd.ops, name)
    with pytest.raises(ValueError, match="top_p"):      # the _p wrapper checks its parameters before the operator is reached
        t = torch.zeros(1, 2, 1024)
        chipmunk_amd.ops.topk_group_delta_indices_p(t, t, t, t, 2, 0.7, 1.5, 0.0, 256, 0.0)


def test_fake_kernels_check_the_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        act = torch.empty(2, 7, 1024, dtype=torch.bfloat16)
        inds, counts = torch.empty(2, 2, 1024, dtype=torch.int32), torch.empty(2, 2, dtype=torch.int32)
        assert torch.ops.chipmunk.topk_group_delta_indices(act, act.clone(), inds, counts, 4, 0.7, 256, 0.0) is None
        assert torch.ops.chipmunk.topk_group_delta_indices_p(act, act.clone(), inds, counts, 4, 0.7, 0.5, 0.1, 256, 0.0) is None
        with pytest.raises(RuntimeError, match="indices must be"):
            torch.ops.chipmunk.topk_group_delta_indices(act, act.clone(), inds, counts, 2, 0.7, 256, 0.0)


def test_invalid_arguments_return_codes_with_messages():
    from chipmunk_amd import _native
    lib = _native.lib()
    p, null, d = ctypes.c_void_p(16), ctypes.c_void_p(0), ctypes.c_double

    def plain(act=p, cache=p, inds=p, counts=p, b=1, rows=4, r=2, cols=1024, sparsity=0.5, multiple_of=256):
        return lib.chipmunk_topk_group_delta_indices(act, cache, 0, inds, counts, b, rows, r, cols, d(sparsity), multiple_of, d(0.0), null)

    def mass(cache=p, r=2, cols=1024, top_p=0.5):
        return lib.chipmunk_topk_group_delta_indices_p(p, cache, 0, p, p, 1, 4, r, cols, d(0.5), d(top_p), d(0.0), 256, d(0.0), null)

    for call, word in ((lambda: plain(cols=512), "1024"), (lambda: plain(r=0), "rows_per_group"), (lambda: plain(r=65), "rows_per_group"),
                       (lambda: plain(cache=null), "null"), (lambda: plain(rows=0), "rows >= 1"), (lambda: plain(multiple_of=0), "multiple_of"),
                       (lambda: plain(b=1 << 30, rows=4, r=1), "too many groups"), (lambda: plain(sparsity=1.5), "sparsity_amount"),
                       (lambda: mass(cols=512), "1024"), (lambda: mass(r=0), "rows_per_group"), (lambda: mass(cache=null), "null"),
                       (lambda: mass(top_p=0.0), "top_p")):
        assert call() == 1 and word in _native.last_error(), _native.last_error()
    assert "topk_group_delta_indices_p" in _native.last_error()
    assert plain(b=0) == 0      # nothing to do, nothing launched


def test_config_key_is_an_extra_key_and_off():
    from chipmunk_amd.util import config as cfg
    _reset()
    try:
        assert cfg.AMD_EXTRA_KEYS["mlp.fused_group_topk_delta"] is False
        assert cfg.BASE_CONFIG["mlp"]["fused_group_topk_delta"] is False
        assert cfg.amd_key("mlp", "fused_group_topk_delta") is False
        cfg.GLOBAL_CONFIG["mlp"]["fused_group_topk_delta"] = True
        assert cfg.amd_key("mlp", "fused_group_topk_delta") is True
        del cfg.GLOBAL_CONFIG["mlp"]["fused_group_topk_delta"]        # a section copied from the reference does not carry the key
        assert cfg.amd_key("mlp", "fused_group_topk_delta") is False
    finally:
        _reset()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_model_equals_the_torch_chain_at_two_rows_per_group(dtype):
    """one fp32 add, one rounding: the explicit loop and torch's reduction cannot differ; then topk_indices and copy_indices as the
    modules run them"""
    import oracle
    g = torch.Generator().manual_seed(3)
    b = torch.randn(2, 6, 1500, generator=g).to(dtype)
    cache = (b.float() + 0.3 * torch.randn(2, 6, 1500, generator=g)).to(dtype)
    mdiff = (b - cache).abs().reshape(2, 3, 2, 1500).sum(dim=2)
    assert mdiff.dtype == dtype
    view = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(gdm.scores(b, cache, 2).view(view), mdiff.view(view))
    inds = torch.full((2, 3, 1500), -9, dtype=torch.int32)
    counts = torch.zeros(2, 3, dtype=torch.int32)
    oracle.topk_indices(mdiff, inds, counts, 0.7, 256, 0.0)
    want = cache.clone()
    oracle.copy_indices(b, want, inds, counts)
    got = gdm.run(b, cache, 2, 0.7, 256)
    assert torch.equal(got[0], inds) and torch.equal(got[1], counts) and torch.equal(got[2].view(view), want.view(view))
    assert 0 < int(counts.min()) and int(counts.max()) < 1500


def test_model_sums_a_short_last_group_and_leaves_other_rows_alone():
    g = torch.Generator().manual_seed(4)
    b = torch.randn(1, 5, 1024, generator=g).to(torch.bfloat16)
    cache = (b.float() + 0.3 * torch.randn(1, 5, 1024, generator=g)).to(torch.bfloat16)
    sc = gdm.scores(b, cache, 4)
    assert sc.shape == (1, 2, 1024)
    assert torch.equal(sc[0, 1].view(torch.int16), (b[0, 4] - cache[0, 4]).abs().view(torch.int16))
    inds, counts, out = gdm.run(b, cache, 4, 0.7, 256)
    listed = torch.zeros(1024, dtype=torch.bool)
    listed[inds[0, 1, : int(counts[0, 1])].long()] = True
    assert torch.equal(out[0, 4].view(torch.int16), torch.where(listed, b[0, 4], cache[0, 4]).view(torch.int16))


@pytest.mark.parametrize("key", ["off", "absent", "on"])
def test_cpu_gated_step_runs_the_unfused_chain(monkeypatch, key):
    """With the key off (or missing from the section) a SparseDiffGatedMlp selection is today's op sequence and never reaches the new
    operators; on CPU tensors that also holds with the key on (the operators take GPU tensors only)."""
    import cpu_ops
    from chipmunk_amd import ops
    from chipmunk_amd.modules import SparseDiffGatedMlp
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    from chipmunk_amd.util.layer_counter import LayerCounter
    import method_model as mm

    def boom(*a, **kw):
        raise AssertionError("the fused group operator was reached")

    cpu_ops.register()
    _reset()
    monkeypatch.setattr(ops, "topk_group_delta_indices", boom)
    monkeypatch.setattr(ops, "topk_group_delta_indices_p", boom)
    monkeypatch.setattr(ops, "mlp_glu", lambda **kw: None)       # (the gated GEMMs have no CPU stand-in; the selection is what is looked at)
    try:
        GLOBAL_CONFIG["num_model_invocations_per_inference_step"] = 1
        GLOBAL_CONFIG["steps"] = 50
        GLOBAL_CONFIG["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=10, block_mask_cache=2, first_n_dense_layers=0,
                                         counts_multiple_of=256))
        GLOBAL_CONFIG["offloading"].update({"global_disable_offloading": True})
        if key == "absent":
            del GLOBAL_CONFIG["mlp"]["fused_group_topk_delta"]
        else:
            GLOBAL_CONFIG["mlp"]["fused_group_topk_delta"] = key == "on"
        lin = lambda i, o: cpu_ops.ExactLinear(i, o).bfloat16()      # noqa: E731
        mod = SparseDiffGatedMlp(0, LayerCounter(1, 1), lin(64, 1024), lin(64, 1024), torch.nn.SiLU(), lin(1024, 64))
        with torch.no_grad():
            mod(mm.mlp_input(0, 0, 0, 300, 64))
            with cpu_ops.recording() as calls:
                mod(mm.mlp_input(1, 0, 0, 300, 64))
                names = [name for name, _ in calls]
        assert names == ["topk_indices", "copy_indices"]
        assert mod.storage.get_indices().shape == (1, 3, 1024) and int(mod.storage.get_counts().min()) > 0
    finally:
        _reset()
