"""MXFP4 fc2 without a GPU: the key, ``W4LinearT``, the C entry's and the wrapper's refusals, the fake kernel, ``check_fc2``, the swap."""
import ctypes

import pytest
import torch

BF16, U8 = torch.bfloat16, torch.uint8
P, NULL = ctypes.c_void_p(256), ctypes.c_void_p(0)      # (no launch happens: every call is refused)


def lin(i, o):
    return torch.nn.Linear(i, o).bfloat16()


def test_w4lineart_is_w4linear_of_the_transposed_layer_and_from_mx_t_shares_storage():
    from chipmunk_amd.modules.mlp_fp8 import W4Linear, W4LinearT
    layer, transposed = lin(96, 160), torch.nn.Linear(160, 96, bias=False).bfloat16()
    transposed.weight = torch.nn.Parameter(layer.weight.data.t().contiguous())
    t, ref = W4LinearT.from_linear(layer), W4Linear.from_linear(transposed)
    assert tuple(t.weight_t.shape) == (96, 80) and tuple(t.block_scale_t.shape) == (96, 5) and t.weight_format == "mxfp4_t" and t.weight_only
    w = t.widened()
    assert w.dtype == BF16 and torch.equal(w.view(torch.int16), ref.widened().t().contiguous().view(torch.int16))
    x = torch.randn(3, 96).to(BF16)
    assert torch.equal(t(x), torch.nn.functional.linear(x, w, layer.bias))
    shared = W4LinearT.from_mx_t(t.weight_t.data, t.block_scale_t, t.bias.data)
    assert shared.weight_t.data_ptr() == t.weight_t.data_ptr() and shared.block_scale_t.data_ptr() == t.block_scale_t.data_ptr()


@pytest.mark.parametrize("kw,text", [
    (dict(a=NULL), "mma_a is null"), (dict(b=NULL), "mma_b is null"), (dict(s=NULL), "scale_b is null"), (dict(c=NULL), "mma_c is null"),
    (dict(inds=NULL), "indices / counts"), (dict(M=0), "M must be positive"), (dict(F=96), "multiple of 64"),
    (dict(N2=0), "multiple of 128"), (dict(N2=64), "multiple of 128"), (dict(N2=192), "multiple of 128"),
    (dict(b=ctypes.c_void_p(264)), "16-byte aligned"), (dict(s=ctypes.c_void_p(258)), "4-byte aligned"),
    (dict(M=1 << 20, F=2048), "32-bit offsets"), (dict(F=1 << 16, N2=1 << 15), "32-bit offsets"), (dict(M=1 << 16, N2=1 << 15), "32-bit offsets"),
    (dict(B=0), "batch size"), (dict(B=65536), "65535"), (dict(B=2, N2=64), "multiple of 128"), (dict(B=2, s=NULL), "scale_b is null")])
def test_the_c_entry_refuses_before_any_launch(kw, text):
    from chipmunk_amd import _native
    lib = _native.lib()
    assert {"chipmunk_csp_mlp_mm2_w4", "chipmunk_csp_mlp_mm2_w4_batched"} <= set(_native.SYMBOLS) and lib.chipmunk_abi_version() == 1
    v = dict(dict(a=P, b=P, s=P, c=P, inds=P, cnt=P, M=100, F=256, N2=128, B=None), **kw)
    args = (v["a"], v["b"], v["s"], v["c"], v["inds"], v["cnt"], v["M"], v["F"], v["N2"])
    rc = lib.chipmunk_csp_mlp_mm2_w4(*args, NULL) if v["B"] is None else lib.chipmunk_csp_mlp_mm2_w4_batched(*args, v["B"], NULL)
    assert rc == 1 and text in _native.last_error(), (kw, rc, _native.last_error())


def test_the_wrapper_names_the_argument_and_the_fake_kernel_checks_shapes():
    from chipmunk_amd.ops.mlp import csp_mlp_mm2
    from torch._subclasses.fake_tensor import FakeTensorMode
    a, c = torch.zeros(128, 64, dtype=BF16), torch.zeros(128, 128, dtype=BF16)
    w, s, inds, cnt = torch.zeros(64, 64, dtype=U8), torch.zeros(64, 4, dtype=U8), torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for args, scale, text in (((a, w, c), None, "needs fc2_scale"), ((a, w, c), s.float(), "fc2_scale .* uint8 or float8_e8m0fnu"),
                              ((a, w, c), s[:, :2], r"fc2_scale must be \[F, N / 32\]"), ((a, w[:, :32], c), s, r"fc2wT must be \[F, N / 2\]"),
                              ((a.float(), w, c), s, "sparse_act_packed and cached_out must be bfloat16"),
                              ((a, w[:, :32], c[:, :64]), s[:, :2], "cached_out must have N % 128 == 0")):
        with pytest.raises(ValueError, match=text):
            csp_mlp_mm2(args[0], args[1], inds, cnt, args[2], fc2_scale=scale)
    with FakeTensorMode():
        a, c, w, s = torch.empty(2, 333, 512, dtype=BF16), torch.empty(2, 333, 256, dtype=BF16), torch.empty(512, 128, dtype=U8), torch.empty(512, 8, dtype=U8)
        inds, counts = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        op = torch.ops.chipmunk.csp_mlp_mm2_w4
        assert op(a, w, s, inds, counts, c) is None and op(a[0], w, s, inds[0], counts[0], c[0]) is None
        for bad, text in (((a, w.to(BF16), s, inds, counts, c), "uint8"), ((a, w, s[:, :4], inds, counts, c), r"scale_b must be \[F, N2 / 32\]"),
                          ((a, w, s, inds, counts, c[0]), "shape mismatch")):
            with pytest.raises(RuntimeError, match=text):
                op(*bad)


def test_check_fc2_with_the_key_on_and_off(fresh_config):
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.modules.mlp import fc2_scale_of
    from chipmunk_amd.modules.mlp_fp8 import W4Linear, W4LinearT
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util.layer_counter import LayerCounter
    assert cfg.AMD_EXTRA_KEYS["mlp.mxfp4_fc2"] is False and cfg.amd_key("mlp", "mxfp4_fc2") is False, "the key defaults to off"
    counter, fc2 = LayerCounter(1, 1), W4LinearT.from_linear(lin(256, 128))
    makes = (lambda f: SparseDiffMlp(0, counter, lin(128, 256), torch.nn.GELU(approximate="tanh"), f),
             lambda f: SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), torch.nn.SiLU(), f))
    for make in makes:
        with pytest.raises(ValueError, match="mlp.mxfp4_fc2"):
            make(fc2)
    fresh_config["mlp"]["mxfp4_fc2"] = True
    for make in makes:
        m = make(fc2)
        wT = m.fc2w_T[0] if isinstance(m, SparseDiffMlp) else m.fc2w_T
        assert wT.data_ptr() == fc2.weight_t.data_ptr() and fc2_scale_of(fc2) is fc2.block_scale_t, "no transposed copy"
        with pytest.raises(ValueError, match="out_features % 128"):
            make(W4LinearT.from_linear(lin(256, 96)))
    with pytest.raises(ValueError, match="W4Linear fc2 .* W4LinearT"):      # blocks along in_features: still refused, and told where to go
        makes[0](W4Linear.from_linear(lin(256, 128)))


def test_the_swap_builds_w4lineart_for_fc2_of_a_sparse_image_mlp_only(fresh_config):
    from chipmunk_amd.modules.mlp_fp8 import W4LinearT, W8Linear, recursive_swap_linears

    def swapped(out=128, **keys):
        fresh_config["mlp"].update(keys)
        blk = torch.nn.Module()
        blk.img_mlp = torch.nn.Sequential(lin(128, 256), torch.nn.GELU(approximate="tanh"), lin(256, out))
        blk.txt_mlp = torch.nn.Sequential(lin(128, 256), torch.nn.GELU(approximate="tanh"), lin(256, out))
        recursive_swap_linears(blk)
        return blk
    assert fresh_config["mlp"]["is_enabled"] and type(swapped(fp8_weight_only=True).img_mlp[2]) is torch.nn.Linear
    on = swapped(mxfp4_fc2=True)
    assert isinstance(on.img_mlp[2], W4LinearT) and tuple(on.img_mlp[2].weight_t.shape) == (256, 64)
    assert all(isinstance(m, W8Linear) for m in (on.img_mlp[0], on.txt_mlp[0], on.txt_mlp[2]))
    assert type(swapped(out=96).img_mlp[2]) is torch.nn.Linear, "out_features % 128 != 0: what it gets without the key"
    assert type(swapped(fp8_weight_only=False).img_mlp[2]) is torch.nn.Linear, "without mlp.fp8_weight_only the key builds nothing"
