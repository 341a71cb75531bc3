"""The MXFP4 linear layer for few rows without a GPU ("MXFP4 forward for few rows"): the key ``mlp.w4_stream_rows`` defaults to 0;
``chipmunk_w4_linear`` refuses bad arguments with a code and a message before any launch; the wrapper refuses by ``ValueError``; the fake
kernel checks shapes; the CPU path is fp32 ``F.linear`` over ``widened()`` rounded once and meets the GPU test's bound against fp64 with room."""
import ctypes

import pytest
import torch

from helpers import MLP_SEG_BOUND, seg_rel_err

VP = ctypes.c_void_p
REFUSALS = ((dict(x=VP(0)), "null"), (dict(w=VP(0)), "null"), (dict(s=VP(0)), "null"), (dict(y=VP(0)), "null"),
            (dict(M=0), "M >= 1"), (dict(K=64, ldx=64), "K >= 128"), (dict(K=192, ldx=192), "multiple of 128"), (dict(F=4), "F >= 8"),
            (dict(F=252), "multiple of 8"), (dict(M=(1 << 20) + 1), "above the grid"), (dict(s=VP(258)), "4-byte aligned"),
            (dict(x=VP(264)), "16-byte aligned"), (dict(w=VP(264)), "16-byte aligned"), (dict(y=VP(264)), "16-byte aligned"),
            (dict(bias=VP(264)), "16-byte aligned"), (dict(ldx=132), "multiples of 8"), (dict(ldy=260), "multiples of 8"),
            (dict(ldx=120), "ldx >= K"), (dict(ldy=248), "ldy >= F"))


def test_the_key_defaults_to_zero_and_the_entry_refuses_bad_arguments_before_any_launch(fresh_config):
    from chipmunk_amd import _native
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.w4_stream_rows"] == 0 and cfg.BASE_CONFIG["mlp"]["w4_stream_rows"] == 0
    assert type(cfg.AMD_EXTRA_KEYS["mlp.w4_stream_rows"]) is int and cfg.amd_key("mlp", "w4_stream_rows") == 0
    lib, i, i64 = _native.lib(), ctypes.c_int, ctypes.c_int64
    assert "chipmunk_w4_linear" in _native.SYMBOLS
    lib.chipmunk_w4_linear.argtypes = [VP, i64, VP, VP, VP, VP, i64, i, i, i, VP]
    for kw, text in REFUSALS:
        v = dict(dict(x=VP(256), ldx=128, w=VP(256), s=VP(256), bias=VP(0), y=VP(256), ldy=256, M=34, K=128, F=256), **kw)
        rc = lib.chipmunk_w4_linear(v["x"], v["ldx"], v["w"], v["s"], v["bias"], v["y"], v["ldy"], v["M"], v["K"], v["F"], VP(0))
        msg = _native.last_error()
        assert rc == 1 and text in msg and msg.startswith("w4_linear:"), (kw, rc, msg)


def test_wrapper_refusals_and_the_cpu_definition():
    from chipmunk_amd import ops
    from chipmunk_amd.modules import W4Linear
    g = torch.Generator().manual_seed(0)
    w = torch.randint(0, 256, (136, 192), generator=g, dtype=torch.uint8)
    w.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    s, b = torch.randint(119, 136, (136, 12), generator=g, dtype=torch.uint8), (8 * torch.randn(136, generator=g)).bfloat16()
    x, q = torch.randn(34, 384, generator=g).bfloat16(), W4Linear.from_mx(w, s, b)
    for bad, match in (((x, w.float(), s), "weight must be a uint8"), ((x, w[0], s), "weight must be a uint8"), ((x.float(), w, s), "x must be bfloat16"),
                       ((x[:, :128], w, s), r"x must be \[..., K\] with K = 384"), ((x, w, s.float()), "block_scale must be uint8"),
                       ((x, w, s[:, :4]), "block_scale must be uint8"), ((x, w, s, b[:8]), "bias must be bfloat16 with F = 136"),
                       ((x, w, s, b.float()), "bias must be bfloat16")):
        with pytest.raises(ValueError, match=match):
            ops.w4_linear(*bad)
    assert "w4_linear" in ops.__all__
    for bias in (None, b):
        got = ops.w4_linear(x.view(2, 17, 384), w, s, bias)
        want = torch.nn.functional.linear(x.float(), q.widened().float(), None if bias is None else bias.float()).to(torch.bfloat16)
        assert got.shape == (2, 17, 136) and got.dtype == torch.bfloat16 and torch.equal(got.view(34, 136), want)
        exact = x.double() @ q.widened().double().T + (0.0 if bias is None else bias.double())
        assert float(seg_rel_err(got.view(34, 136), exact, 64).max()) <= MLP_SEG_BOUND / 2, "the definition meets the GPU test's bound with room"


def test_fake_kernel_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16, u8 = torch.bfloat16, torch.uint8
        x, w, s, y = torch.empty(34, 128, dtype=bf16), torch.empty(512, 64, dtype=u8), torch.empty(512, 4, dtype=u8), torch.empty(34, 512, dtype=bf16)
        op = torch.ops.chipmunk.w4_linear
        assert op(x, w, s, torch.empty(512, dtype=bf16), y) is None and op(x, w, s, None, y) is None
        with pytest.raises(RuntimeError, match=r"y \[M, F\]"):
            op(x, w, s, None, y[:, :8])
