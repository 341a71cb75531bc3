"""MXFP4 fc1 without a GPU ("MXFP4 fc1"): W4Linear, the argument rules of ops.mlp, the fake kernel, the layer swap, the modules."""
from types import SimpleNamespace as Layer      # what from_linear reads of an nn.Linear: weight, bias

import pytest
import torch

from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp, W4Linear, W8Linear, recursive_swap_linears
from chipmunk_amd.modules.mlp_fp8 import E2M1_VALUES, F8Linear
from chipmunk_amd.util.layer_counter import LayerCounter

BF16, U8 = torch.bfloat16, torch.uint8
GRID = list(E2M1_VALUES) + [-v for v in E2M1_VALUES]          # the 16 nibbles' values, both zeros.  BLOCKS: (a block's values, widened, e8m0 byte)
BLOCKS = [([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -2.5], [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -2.0], 127),    # every midpoint: ties to even
          ([7.0, 7.9, -7.5, 0.26], [6.0, 6.0, -6.0, 0.5], 127),                                   # past 6 saturates
          ([3.9999, 0.7, -0.3], [3.0, 0.75, -0.25], 126),                                         # amax just under 4: floor(log2) = 1
          ([], [], 127), ([2.0 ** -140], [0.0], 0)]                                               # a zero block; the exponent clamps at -127
BLOCKS += [([v * 2.0 ** e for v in GRID], [v * 2.0 ** e for v in GRID], e + 127) for e in (-126, -12, -1, 0, 3, 120)]      # representable: reproduced


@pytest.mark.parametrize("values,want,byte", BLOCKS)
def test_quantiser_block(values, want, byte):
    w = torch.nn.functional.pad(torch.tensor([values], dtype=torch.float32), (32, 32 - len(values)))       # the second block of two
    q = W4Linear.from_linear(Layer(weight=w, bias=None))
    assert q.block_scale.tolist() == [[127, byte]] and (q.weight[0, :16] == 0).all() and q.widened().dtype == BF16
    assert q.widened()[0, 32:32 + len(values)].double().tolist() == want


def test_nibble_order_from_mx_and_forward():
    assert W4Linear.from_linear(Layer(weight=torch.tensor([[1.0, -2.0] + [0.0] * 30]), bias=None)).weight[0, 0] == 0x4 | 0xE << 4       # e = -1: codes 4 and 8 | 6; element 0 low
    g = torch.Generator().manual_seed(0)
    w, s = torch.randint(0, 256, (8, 64), generator=g, dtype=U8), torch.randint(100, 140, (8, 4), generator=g, dtype=U8)
    bias, x = torch.randn(8, generator=g).to(BF16), torch.randn(5, 128, generator=g).to(BF16)
    a, b = W4Linear.from_mx(w, s, bias), W4Linear.from_mx(w.view(torch.float4_e2m1fn_x2), s.view(torch.float8_e8m0fnu), bias)
    assert (a.in_features, a.out_features, a.weight_only, a.weight_format, a.weight.shape) == (128, 8, True, "mxfp4", (8, 64))
    assert torch.equal(a.weight, b.weight) and torch.equal(a.block_scale, b.block_scale) and b.weight.dtype == b.block_scale.dtype == U8
    assert torch.equal(a(x), torch.nn.functional.linear(x, a.widened(), bias)) and torch.equal(a(x), b(x)) and a.widened() is not a.widened()
    with pytest.raises(ValueError, match="scales"):
        W4Linear.from_mx(w, s[:, :3])


X, W, S = torch.zeros(128, 128, dtype=BF16), torch.zeros(64, 64, dtype=U8), torch.zeros(64, 4, dtype=U8)
TAIL = (torch.zeros(128, 64, dtype=BF16), None, torch.zeros(64, 128, dtype=BF16), torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
E2E, ONE = (None, torch.zeros(64, 32, dtype=BF16), TAIL[3], TAIL[4], TAIL[2], torch.zeros(128, 32, dtype=BF16), 0), torch.ones(())


@pytest.mark.parametrize("fn,args,kw,error,message", [
    ("mm1_w4", (X, W, S) + TAIL, dict(act="relu"), ValueError, "unknown activation"),
    ("mm1_w4", (X, W.to(BF16), S) + TAIL, {}, ValueError, "mm1_w4: fc1w must be uint8 or float4_e2m1fn_x2"),
    ("mm1", (X, W.view(torch.float4_e2m1fn_x2)) + TAIL, dict(fc1_scale=ONE), ValueError, "mm1: fc1_scale .* e8m0"),
    ("mm1_scatter", (X.float(), W) + TAIL, dict(fc1_scale=S), ValueError, "mm1_scatter: .* x must be bfloat16"),
    ("run_e2e", (X, W) + E2E, dict(mm1_scale_b=ONE, fc1_scale=S.view(torch.float8_e8m0fnu)), ValueError, "run_e2e: mm1_scale_b must be None"),
    ("mm1", (X[:, :64].contiguous(), W[:, :32].contiguous()) + TAIL, dict(fc1_scale=S[:, :2].contiguous()), ValueError, "K % 128"),
    ("mm1_scatter", (X, W) + TAIL, dict(fc1_scale=S[:, :2].contiguous()), ValueError, r"fc1_scale must be \[F, K / 32\]"),
    ("run_e2e", (X, W) + E2E, {}, AssertionError, "K1 must match")])      # (without fc1_scale a uint8 fc1w is no format: refused as it always was)
def test_ops_argument_rules(fn, args, kw, error, message):
    import importlib
    with pytest.raises(error, match=message):
        getattr(importlib.import_module("chipmunk_amd.ops.mlp"), fn)(*args, **kw)


def test_fake_kernel_shapes_and_dtypes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a, c, w, s = torch.empty(2, 333, 256, dtype=BF16), torch.empty(2, 333, 512, dtype=BF16), torch.empty(512, 128, dtype=U8), torch.empty(512, 8, dtype=U8)
        rest = (torch.empty(512, dtype=BF16), torch.empty(2, 512, 333, dtype=BF16), torch.empty(2, 3, 512, dtype=torch.int32),
                torch.empty(2, 3, dtype=torch.int32), "silu", True)
        op = torch.ops.chipmunk.csp_mlp_mm1_w4
        assert op(a, w, s, c, *rest) is None and op(a, w, s, c, None, *rest[1:]) is None
        for bad in ((a, w, s[:, :4], c), (a, w[:, :64], s, c), (a, w.to(BF16), s, c), (a[..., :192], w[:, :96], s[:, :6], c), (a, w, s, c[..., :256])):
            with pytest.raises(RuntimeError):
                op(*bad, *rest)


@pytest.mark.parametrize("key,weight_only,enabled,k,want", [(True, True, True, 128, W4Linear), (False, True, True, 128, W8Linear),
                                                           (True, False, True, 128, F8Linear), (True, True, False, 128, W8Linear),
                                                           (True, True, True, 64, W8Linear)])
def test_recursive_swap_linears_builds_the_named_layer_only(fresh_config, key, weight_only, enabled, k, want):
    assert fresh_config["mlp"]["mxfp4_fc1"] is False
    fresh_config["mlp"].update(mxfp4_fc1=key, fp8_weight_only=weight_only, is_enabled=enabled)
    mlp = lambda: torch.nn.Sequential(torch.nn.Linear(k, 64), torch.nn.GELU(approximate="tanh"), torch.nn.Linear(64, k))      # noqa: E731
    block = torch.nn.ModuleDict(dict(img_mlp=mlp(), txt_mlp=mlp(), proj=torch.nn.Linear(k, k))).bfloat16()
    recursive_swap_linears(block)
    other = W8Linear if weight_only else F8Linear
    assert type(block["img_mlp"][0]) is want and type(block["img_mlp"][2]) is (torch.nn.Linear if enabled else other)
    assert type(block["txt_mlp"][0]) is other and type(block["txt_mlp"][2]) is other and type(block["proj"]) is other


def test_modules_accept_and_refuse(fresh_config):
    gelu, counter = torch.nn.GELU(approximate="tanh"), LayerCounter(1, 1)
    q128, q64 = (W4Linear.from_linear(torch.nn.Linear(k, 64).bfloat16()) for k in (128, 64))
    fc2, x = torch.nn.Linear(64, 128).bfloat16(), torch.randn(1, 8, 128).to(BF16)
    m = SparseDiffMlp(0, counter, q128, gelu, fc2)          # (mlp.is_enabled off: the dense route)
    assert torch.equal(m(x), fc2(gelu(torch.nn.functional.linear(x, q128.widened(), q128.bias))))
    fresh_config["mlp"]["w8_gated"] = True
    for message, build in (("in_features % 128", lambda: SparseDiffMlp(0, counter, q64, gelu, torch.nn.Linear(64, 64).bfloat16())),
                           ("W4Linear fc2", lambda: SparseDiffMlp(0, counter, torch.nn.Linear(64, 64).bfloat16(), gelu, q64)),
                           ("W4Linear projection", lambda: SparseDiffGatedMlp(0, counter, q128, q128, torch.nn.SiLU(), fc2))):
        with pytest.raises(ValueError, match=message):
            build()
