"""The gated fp8 feed-forward path without a GPU (tests/glu_fp8_method_model.py):

* the plain-torch mirror of the operator's formula passes the bound tests/test_gpu_mlp_glu_fp8.py asserts (fp32 torch from the quantised
  operands, atol = rtol = 3e-2), and every mutant lies at least 2 x outside it on the same inputs (gate and up scales swapped, scale_a
  dropped, bias added before the scaling, halves swapped, activation applied to the product);
* (the gated fp8 GEMM1 kernels compile for gfx950 without spills or scratch and within 64 KiB of LDS: tests/test_mlp_mm1_form_audit.py;)
* the fake kernel traces without a GPU, the C ABI lists the two new entries and refuses bad arguments, the module refuses at construction
  what the sparse steps could not honour."""
import os
import re

import pytest
import torch

import glu_fp8_method_model as gfp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ operator mirror
@pytest.mark.parametrize("act", ["gelu_tanh", "silu", "gelu"])
def test_operator_mirror_passes_the_operator_bound_and_every_mutant_is_twice_outside(act):
    """the second shape of the GPU operator test (M = 333, counts F / 0 / 336) on the CPU, both biases"""
    p = gfp.fp8_problem(torch.device("cpu"), 333, [512, 0, 336], seed=334)
    assert float(p["rbu"] / p["rbg"]) >= 2.0
    args = (p["a"], p["wg"], p["wu"], p["bg"], p["bu"], act, p["cache0"], p["inds"], p["cnt"], p["ra"], p["rbg"], p["rbu"])
    h = gfp.want_fp32(p, act, "bg", "bu")
    good = max(gfp.group_ratios(p, gfp.mm1_glu_fp8_mirror(*args), h))
    print(f"{act}: mirror {good:.3f} x the tolerance")
    assert good <= 1.0
    for defect in gfp.OP_DEFECTS:
        bad = max(gfp.group_ratios(p, gfp.mm1_glu_fp8_mirror(*args, defect=defect), h))
        print(f"{act}: mutant {defect} {bad:.1f} x the tolerance")
        assert bad >= 2.0, f"{defect} is not twice outside the operator bound: {bad:.3f} x"


def test_swapped_scales_put_a_large_share_of_the_elements_outside_the_bound():
    """not a lucky element: with weight scales 2.5 x apart the mutant misses the tolerance on about half of the kept elements (a third is asserted)"""
    p = gfp.fp8_problem(torch.device("cpu"), 333, [512, 0, 336], seed=334)
    args = (p["a"], p["wg"], p["wu"], p["bg"], p["bu"], "silu", p["cache0"], p["inds"], p["cnt"], p["ra"], p["rbg"], p["rbu"])
    c = gfp.mm1_glu_fp8_mirror(*args, defect="scales_swapped")
    h = gfp.want_fp32(p, "silu", "bg", "bu")
    cols = p["inds"][0].long()
    want = h[:128][:, cols] - p["cache0"][cols][:, :128].float().T
    off = ((c[:128].float() - want).abs() > 3e-2 + 3e-2 * want.abs()).float().mean()
    print(f"swapped scales: {float(off):.2f} of the elements outside atol = rtol = 3e-2")
    assert off > 1 / 3


# ------------------------------------------------------------------------------------------------------------------ plumbing
def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16, f8 = torch.bfloat16, torch.float8_e4m3fn
        a, w, c = torch.empty(2, 333, 256, dtype=f8), torch.empty(512, 256, dtype=f8), torch.empty(2, 333, 512, dtype=bf16)
        cache = torch.empty(2, 512, 336, dtype=bf16)[..., :333]
        inds, counts = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        s, bias = torch.empty(1), torch.empty(512, dtype=bf16)
        op = torch.ops.chipmunk.csp_mlp_mm1_glu_fp8
        assert op(a, w, w, c, None, None, cache, inds, counts, s, s, s, "silu", True) is None
        assert op(a[0], w, w, c[0], bias, None, cache[0], inds[0], counts[0], s, s, s, "gelu", False) is None
        with pytest.raises(RuntimeError, match="c must be"):
            op(a, w, w, c[0], None, None, cache, inds, counts, s, s, s, "silu", True)
        with pytest.raises(RuntimeError, match="unknown activation"):
            op(a, w, w, c, None, None, cache, inds, counts, s, s, s, "relu", True)
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            op(c, w, w, c, None, None, cache, inds, counts, s, s, s, "silu", True)
        with pytest.raises(RuntimeError, match="one-element float32"):
            op(a, w, w, c, None, None, cache, inds, counts, s, torch.empty(2), s, "silu", True)


def test_abi_lists_the_gated_fp8_entries_and_refuses_bad_arguments():
    import ctypes
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    for name in ("chipmunk_csp_mlp_mm1_glu_fp8", "chipmunk_csp_mlp_mm1_glu_fp8_batched"):
        assert name in _native.SYMBOLS and re.search(rf"\b{name}\s*\(", header)
    lib, p, null = _native.lib(), ctypes.c_void_p(16), ctypes.c_void_p(0)      # (no launch happens: every call below is refused)

    def call(a=p, sa=p, sbu=p, M=128, K=128, F=256, ldc=128, act=1, upd=0):
        return lib.chipmunk_csp_mlp_mm1_glu_fp8(a, p, p, p, null, null, p, p, p, sa, p, sbu, M, K, F, ldc, act, upd, null), _native.last_error()
    for kw, text in ((dict(a=null), "null"), (dict(sa=null), "null"), (dict(sbu=null), "null"), (dict(act=3), "unknown activation"),
                     (dict(upd=2), "update_cache"), (dict(K=192), "multiple of 128"), (dict(K=64), "multiple of 128"),
                     (dict(M=100, ldc=100), "pitch"), (dict(ldc=120), "pitch"),
                     (dict(M=65536, K=32768, ldc=65536), "32-bit offsets")):      # M * K = 2^31 one-byte elements
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    batched = lib.chipmunk_csp_mlp_mm1_glu_fp8_batched
    rc = batched(p, p, p, p, null, null, p, p, p, p, p, p, 100, 128, 256, 104, 1, 0, 2, ctypes.c_int64(100), null)
    assert rc == 1 and "batch stride" in _native.last_error()
    rc = batched(p, p, p, p, null, null, p, p, p, p, p, p, 100, 128, 256, 104, 1, 0, 0, ctypes.c_int64(256 * 104), null)
    assert rc == 1 and "batch size" in _native.last_error()


def test_module_refuses_what_the_fp8_sparse_steps_cannot_honour():
    """construction only: no operator runs"""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.modules import F8Linear, SparseDiffGatedMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    e4m3, e5m2 = torch.float8_e4m3fn, torch.float8_e5m2
    lin = lambda i, o: torch.nn.Linear(i, o).bfloat16()      # noqa: E731
    f8 = lambda i, o, **kw: F8Linear.from_linear(lin(i, o), **kw)      # noqa: E731
    counter, silu = LayerCounter(1, 1), torch.nn.SiLU()
    m = SparseDiffGatedMlp(0, counter, f8(128, 256, input_float8_dtype=e4m3), f8(128, 256, input_float8_dtype=e4m3), silu, lin(256, 128))
    assert m.fp8 and m.gate[0].dtype == e4m3 and m.up[0].shape == (256, 128)
    fc1 = f8(128, 512, input_float8_dtype=e4m3)
    m = SparseDiffGatedMlp.from_fused(0, counter, fc1, silu, lin(256, 128), gate_first=False)
    assert m.fp8 and m.gate[0].data_ptr() == fc1.weight.data[256:].data_ptr() and m.projs[0] is m.projs[-1]
    assert not SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), silu, lin(256, 128)).fp8
    with pytest.raises(ValueError, match="mixed pair"):
        SparseDiffGatedMlp(0, counter, f8(128, 256, input_float8_dtype=e4m3), lin(128, 256), silu, lin(256, 128))
    with pytest.raises(ValueError, match="mixed pair"):
        SparseDiffGatedMlp(0, counter, lin(128, 256), f8(128, 256, input_float8_dtype=e4m3), silu, lin(256, 128))
    with pytest.raises(ValueError, match="float8_e4m3fn weights and inputs only"):      # from_linear's default input dtype is e5m2
        SparseDiffGatedMlp(0, counter, f8(128, 256), f8(128, 256), silu, lin(256, 128))
    with pytest.raises(ValueError, match="float8_e4m3fn weights and inputs only"):
        SparseDiffGatedMlp.from_fused(0, counter, f8(128, 512, input_float8_dtype=e5m2), silu, lin(256, 128))
    with pytest.raises(ValueError, match="float8_e4m3fn weights and inputs only"):      # e5m2 weights
        SparseDiffGatedMlp(0, counter, f8(128, 256, float8_dtype=e5m2, input_float8_dtype=e4m3),
                           f8(128, 256, float8_dtype=e5m2, input_float8_dtype=e4m3), silu, lin(256, 128))
    with pytest.raises(ValueError, match="fc2 must stay bf16"):
        SparseDiffGatedMlp(0, counter, f8(128, 256, input_float8_dtype=e4m3), f8(128, 256, input_float8_dtype=e4m3), silu,
                           f8(256, 128, input_float8_dtype=e4m3))
    with pytest.raises(ValueError, match="fc2 must stay bf16"):      # ... also under bf16 projections
        SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), silu, f8(256, 128, input_float8_dtype=e4m3))
