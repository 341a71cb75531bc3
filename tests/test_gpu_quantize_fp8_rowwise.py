"""chipmunk_quantize_fp8_rowwise on the device: bytes and reciprocal scales bit-identical to its chain evaluated by torch on the CPU
(tests/mlp_rowscale_model.quantize_chain: fp32, IEEE division, one rounding into e4m3), rows 1 / 3 / 257 x K 16 / 128 / 1552 / 13 824
(one to 27 16-byte vectors per lane, a last vector that is partly or wholly past the row; more rows than one workgroup takes).  Inputs
(mlp_rowscale_model.quantizer_rows): rows spanning 1e-3 .. 1e3, an all-zero row, a row of e4m3 rounding ties, a maximum in the last
element.  Sentinels behind both outputs, two launches, and F8Linear.quantize_input_rowwise = the kernel."""
import ctypes
import functools

import pytest
import torch

import mlp_rowscale_model as rm
from helpers import F8

pytestmark = pytest.mark.gpu

ROWS, KS = (1, 3, 257), (16, 128, 1552, 13824)
SENT_BYTE, SENT_F32 = 0xA5, 7.0


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(rows, K):
    """(x bf16 on the CPU, the chain's bytes, the chain's reciprocal scales), computed once"""
    x = rm.quantizer_rows(rows, K, 1000 + rows + K)
    out, recip = rm.quantize_chain(x)
    return x, out.view(torch.uint8), recip


def launch(x, dev):
    """the C entry on buffers of the test's own: returns (out bytes [rows, K], recip [rows], the two whole buffers)"""
    from chipmunk_amd import _native
    rows, K = x.shape
    xd = x.to(dev).contiguous()
    out_buf = torch.full((rows * K + 256,), SENT_BYTE, dtype=torch.uint8, device=dev)
    recip_buf = torch.full((rows + 64,), SENT_F32, dtype=torch.float32, device=dev)
    rc = _native.lib().chipmunk_quantize_fp8_rowwise(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(out_buf.data_ptr()),
                                                     ctypes.c_void_p(recip_buf.data_ptr()), ctypes.c_int64(rows), ctypes.c_int(K),
                                                     ctypes.c_float(448.0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "chipmunk_quantize_fp8_rowwise")
    torch.cuda.synchronize()
    return out_buf[: rows * K].view(rows, K), recip_buf[:rows], out_buf, recip_buf


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_bytes_and_scales_are_those_of_the_chain_on_the_cpu(dev, rows, K):
    x, want, want_recip = case(rows, K)
    out, recip, out_buf, recip_buf = launch(x, dev)
    assert (out_buf[rows * K:] == SENT_BYTE).all(), "bytes behind out were written"
    assert (recip_buf[rows:] == SENT_F32).all(), "floats behind scale_recip were written"
    bad = recip.cpu().view(torch.int32) != want_recip.view(torch.int32)
    assert not bad.any(), f"{int(bad.sum())} of {rows} reciprocal scales differ, first at row {int(bad.nonzero()[0])}"
    diff = out.cpu() != want
    assert not diff.any(), f"{int(diff.sum())} of {rows * K} bytes differ, first at {diff.nonzero()[0].tolist()}"
    if rows >= 2:
        assert (out[rows // 2] == 0).all() and recip[rows // 2].item() == want_recip[rows // 2].item()      # the all-zero row
    out2, recip2, _, _ = launch(x, dev)
    assert torch.equal(out, out2) and torch.equal(recip.view(torch.int32), recip2.view(torch.int32)), "two launches, different bits"


def test_the_entry_refuses_a_row_it_does_not_take(dev):
    x = torch.zeros(2, 16400, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="16384"):
        torch.ops.chipmunk.quantize_fp8_rowwise(x, 448.0)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        torch.ops.chipmunk.quantize_fp8_rowwise(x[:, :24], 448.0)
    with pytest.raises(RuntimeError, match="bfloat16"):
        torch.ops.chipmunk.quantize_fp8_rowwise(x[:, :32].float(), 448.0)


def test_f8linear_quantize_input_rowwise_returns_what_the_kernel_returns(dev):
    from chipmunk_amd.modules import F8Linear
    x, want, want_recip = case(257, 128)
    layer = F8Linear.from_linear(torch.nn.Linear(128, 64).bfloat16().to(dev), input_float8_dtype=F8, scaling="row")
    xd = torch.stack([x, x.flip(0)]).to(dev)                                      # [2, 257, 128]
    xq, recip = layer.quantize_input_rowwise(xd)
    assert xq.dtype == F8 and xq.shape == xd.shape and recip.shape == (2, 257) and recip.dtype == torch.float32
    out, r, _, _ = launch(x, dev)
    assert torch.equal(xq[0].view(torch.uint8), out) and torch.equal(recip[0].view(torch.int32), r.view(torch.int32))
    assert torch.equal(xq[1].view(torch.uint8), out.flip(0)) and torch.equal(recip[1].view(torch.int32), r.flip(0).view(torch.int32))
    assert torch.equal(xq[0].cpu().view(torch.uint8), want)
    # a row longer than the kernel takes: the torch chain, the same definition
    long = torch.randn(3, 16400, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    wide = F8Linear.from_linear(torch.nn.Linear(16400, 16).bfloat16().to(dev), input_float8_dtype=F8, scaling="row")
    xq, recip = wide.quantize_input_rowwise(long.to(dev))
    w_out, w_recip = rm.quantize_chain(long)
    assert xq.shape == (3, 16400) and torch.allclose(recip.cpu(), w_recip, rtol=1e-6, atol=0)
    assert (xq.cpu().float() - w_out.float()).abs().max() <= 32.0                 # (the device's division may differ in the last bit: one e4m3 step)
