"""The gated MXFP4 GEMM1 ("Gated MXFP4 GEMM1") without a GPU: ``mlp.mxfp4_gated`` switches what ``SparseDiffGatedMlp`` accepts, a
fused ``W4Linear`` is split into views, ``ops.mlp.mm1_glu_w4`` names the argument it refuses, and the fake operator checks shapes."""
import pytest
import torch

BF16 = torch.bfloat16


def _makers():
    from chipmunk_amd.modules import SparseDiffGatedMlp, W4Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    plain = lambda i, o: torch.nn.Linear(i, o).bfloat16()      # noqa: E731
    w4 = lambda i, o: W4Linear.from_linear(plain(i, o))      # noqa: E731
    counter, silu = LayerCounter(1, 1), torch.nn.SiLU()
    two = lambda k=128: SparseDiffGatedMlp(0, counter, w4(k, 256), w4(k, 256), silu, plain(256, 128))      # noqa: E731
    mixed = lambda: SparseDiffGatedMlp(0, counter, w4(128, 256), plain(128, 256), silu, plain(256, 128))      # noqa: E731
    fused = lambda gate_first=True: SparseDiffGatedMlp.from_fused(0, counter, w4(128, 512), silu, plain(256, 128), gate_first=gate_first)      # noqa: E731
    return two, mixed, fused


def test_key_off_refuses_key_on_accepts_and_a_fused_layer_is_split_into_views(fresh_config):
    from chipmunk_amd.util import config as cfg
    two, mixed, fused = _makers()
    assert cfg.AMD_EXTRA_KEYS["mlp.mxfp4_gated"] is False and not cfg.amd_key("mlp", "mxfp4_gated")
    for key in (False, True):
        fresh_config["mlp"]["mxfp4_gated"] = key
        with pytest.raises(ValueError, match="mixed pair"):
            mixed()
        for make in (two, fused):
            if key:
                m = make()
                assert m.w4 and not m.w8 and not m.fp8 and m.gate[0].dtype == torch.uint8 and tuple(m.up[0].shape) == (256, 64)
            else:
                with pytest.raises(ValueError, match="W4Linear projection.*mlp.mxfp4_gated"):
                    make()
    with pytest.raises(ValueError, match="in_features % 128"):
        two(k=64)
    for gate_first in (True, False):      # a fused layer's weight, block_scale and bias are split into views of the right halves
        m = fused(gate_first)
        fc1 = m.projs[0]
        for (gate, up), whole in (((m.gate[0], m.up[0]), fc1.weight.data), (m.w4_scales, fc1.block_scale), ((m.gate[1], m.up[1]), fc1.bias.data)):
            for got, second in ((gate, not gate_first), (up, gate_first)):      # the up half is the second one when the gate comes first
                assert got.shape[0] == 256 and got.is_contiguous()
                assert got.data_ptr() == whole.data_ptr() + second * 256 * whole.stride(0) * whole.element_size(), "a view, not a copy"


def test_wrapper_refusals_name_the_argument():
    from chipmunk_amd import ops
    from chipmunk_amd.ops.mlp import mm1_glu_w4, run_e2e_glu_w4
    assert ops.mlp_glu_w4 is run_e2e_glu_w4 and ops.mm1_glu_w4 is mm1_glu_w4 and "mlp_glu_w4" in ops.__all__
    x, w, s = torch.zeros(128, 128, dtype=BF16), torch.zeros(64, 64, dtype=torch.uint8), torch.zeros(64, 4, dtype=torch.uint8)
    tail = (torch.zeros(128, 64, dtype=BF16), None, None, "silu", torch.zeros(64, 128, dtype=BF16), torch.zeros(1, 64, dtype=torch.int32),
            torch.zeros(1, dtype=torch.int32))
    for message, args in (("w_gate must be uint8", (x, w.to(BF16), w, s, s)), ("w_up must be uint8", (x, w, w.to(BF16), s, s)),
                          ("x must be bfloat16", (x.float(), w, w, s, s)), ("K % 128", (x[:, :64], w[:, :32], w[:, :32], s[:, :2], s[:, :2])),
                          (r"w_up must be \[F, K / 2\]", (x, w, w[:32], s, s)), ("scale_gate must be e8m0", (x, w, w, s.float(), s)),
                          (r"scale_up must be \[F, K / 32\]", (x, w, w, s, s[:, :3]))):
        with pytest.raises(ValueError, match=message):
            mm1_glu_w4(*args, *tail)
    with pytest.raises(ValueError, match="unknown activation"):
        mm1_glu_w4(x, w, w, s, s, *tail[:3], "relu", *tail[4:])


def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a, c = torch.empty(2, 333, 128, dtype=BF16), torch.empty(2, 333, 512, dtype=BF16)
        fused, scales = torch.empty(1024, 64, dtype=torch.uint8), torch.empty(1024, 4, dtype=torch.uint8)
        (wg, wu), (sg, su) = (fused[:512], fused[512:]), (scales[:512], scales[512:])
        cache, bias = torch.empty(2, 512, 333, dtype=BF16), torch.empty(512, dtype=BF16)
        inds, counts = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        op = torch.ops.chipmunk.csp_mlp_mm1_glu_w4
        assert op(a, wg, wu, sg, su, c, bias, None, cache, inds, counts, "silu", True) is None
        assert op(a[0], wu, wg, su, sg, c[0], None, bias, cache[0], inds[0], counts[0], "gelu", False) is None
        for message, args in (("uint8", (a, wg.to(BF16), wu, sg, su, c)), (r"\[F, K / 32\]", (a, wg, wu, sg, su[:, :3], c)),
                              ("c must be", (a, wg, wu, sg, su, c[0]))):
            with pytest.raises(RuntimeError, match=message):
                op(*args, bias, None, cache, inds, counts, "silu", True)
