"""e4m3 activations x MXFP4 fc1 without a GPU: symbols, config key, ops.mlp's argument rules, the fake kernel, quantize_input_rowwise"""
import importlib
import os

import pytest
import torch

from chipmunk_amd.modules import W4Linear
from chipmunk_amd.modules.mlp_fp8 import quantize_rowwise_torch

BF16, U8, E4M3 = torch.bfloat16, torch.uint8, torch.float8_e4m3fn


def test_symbols_are_declared_and_exported_and_the_key_is_off(fresh_config):
    from chipmunk_amd import _native
    from chipmunk_amd.util.config import AMD_EXTRA_KEYS
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "chipmunk_hip.h")).read()
    assert all(f"int chipmunk_csp_mlp_mm1_fp8_w4{e}(" in header and f"chipmunk_csp_mlp_mm1_fp8_w4{e}" in _native.SYMBOLS for e in ("", "_batched", "_gm"))
    assert fresh_config["mlp"]["mxfp4_fp8_act"] is False and AMD_EXTRA_KEYS["mlp.mxfp4_fp8_act"] is False


XQ, X, W, S = torch.zeros(128, 128, dtype=E4M3), torch.zeros(128, 128, dtype=BF16), torch.zeros(64, 64, dtype=U8), torch.zeros(64, 4, dtype=U8)
TAIL = (torch.zeros(128, 64, dtype=BF16), None, torch.zeros(64, 128, dtype=BF16), torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
E2E, ONE, ROWS = (None, torch.zeros(64, 32, dtype=BF16), TAIL[3], TAIL[4], TAIL[2], torch.zeros(128, 32, dtype=BF16), 0), torch.ones(()), torch.ones(128)


@pytest.mark.parametrize("fn,args,kw,message", [
    ("mm1", (XQ, W) + TAIL, dict(fc1_scale=S), "mm1: a float8_e4m3fn x with an MXFP4 fc1w needs scale_a"),
    ("mm1", (XQ, W) + TAIL, dict(fc1_scale=S, scale_a=ROWS, scale_b=ONE), "mm1: scale_b must be None"),
    ("run_e2e", (XQ, W) + E2E, dict(fc1_scale=S), "run_e2e: .* needs mm1_scale_a"),
    ("run_e2e", (X, W) + E2E, dict(fc1_scale=S, mm1_scale_a=ONE), "run_e2e: mm1_scale_a must be None"),      # a bf16 x with a scale_a: still refused
    ("mm1_scatter", (X.float(), W) + TAIL, dict(fc1_scale=S), "mm1_scatter: .* x must be bfloat16"),
    ("mm1", (XQ[:, :64].contiguous(), W[:, :32].contiguous()) + TAIL, dict(fc1_scale=S[:, :2].contiguous(), scale_a=ONE), "K % 128"),
    ("mm1", (XQ, W) + TAIL, dict(fc1_scale=S[:, :2].contiguous(), scale_a=ONE), r"fc1_scale must be \[F, K / 32\]"),
    ("mm1_fp8_scatter", (XQ, W) + TAIL + (ROWS, ONE), dict(fc1_scale=S), "mm1_fp8_scatter: scale_b must be None")])
def test_ops_argument_rules(fn, args, kw, message):
    with pytest.raises(ValueError, match=message):
        getattr(importlib.import_module("chipmunk_amd.ops.mlp"), fn)(*args, **kw)


def test_fake_kernel_shapes_and_dtypes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a, c, w, s = torch.empty(2, 333, 256, dtype=E4M3), torch.empty(2, 333, 512, dtype=BF16), torch.empty(512, 128, dtype=U8), torch.empty(512, 8, dtype=U8)
        rest = (torch.empty(512, dtype=BF16), torch.empty(2, 512, 333, dtype=BF16), torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32))
        sa, op = torch.empty(2, 333), torch.ops.chipmunk.csp_mlp_mm1_fp8_w4
        assert op(a, w, s, c, *rest, sa, "silu", 1) is None and op(a, w, s, c, None, *rest[1:], torch.empty(1), "gelu", 0) is None
        for bad, scale, upd in (((a, w, s[:, :4], c), sa, 1), ((a.to(BF16), w, s, c), sa, 1), ((a, w, s, c[..., :256]), sa, 1), ((a[..., :192], w[:, :96], s[:, :6], c), sa, 1),
                                ((a, w, s, c), sa[:, :332], 1), ((a, w, s, c), sa.double(), 1), ((a, w, s, c), sa, 2)):
            with pytest.raises(RuntimeError):
                op(*bad, *rest, scale, "silu", upd)


def test_quantize_input_rowwise_is_the_torch_chain_off_the_gpu():
    q = W4Linear.from_linear(torch.nn.Linear(128, 64).bfloat16())
    x = (torch.randn(2, 37, 128, generator=torch.Generator().manual_seed(3)) * torch.logspace(-2, 2, 37)[:, None]).to(BF16)
    (xq, recip), (wq, wrecip) = q.quantize_input_rowwise(x), quantize_rowwise_torch(x, 448.0)
    assert xq.dtype == E4M3 and recip.dtype == torch.float32 and recip.shape == (2, 37)
    assert torch.equal(xq.view(U8), wq.view(U8)) and torch.equal(recip, wrecip)
