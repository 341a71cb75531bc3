"""``csp_mlp_mm1_glu_w4`` ("Gated MXFP4 GEMM1") on the GPU: the bits of ``csp_mlp_mm1_glu`` on the two ``W4Linear.widened()`` weights
(random bytes, every widened value a normal bf16 or zero), of ``csp_mlp_mm1_w4`` under a unit up branch; fp64 segments under the bf16 form's bound."""
import functools

import pytest
import torch

import test_gpu_mlp_glu_w8 as w8
from helpers import MLP_ACTS as ACTS, MLP_SEG_BOUND, MLP_SEG_W1, assert_segs_close, mm1_exact
from test_gpu_mlp_glu_w8 import F, assert_same, check_untouched, dev, fresh_state, operands  # noqa: F401  (dev: the device fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def problem(M, K, B, quantised=False):
    """tests/test_gpu_mlp_glu_w8.py's inputs (a, cache, biases, index lists, counts) with two MXFP4 weights: random bytes and scale bytes, or --
    `quantised` -- W4Linear.from_linear of randn * 0.06 (the OCP rule)"""
    from chipmunk_amd.modules import W4Linear
    p, g, dev = dict(w8.problem(M, K, B)), torch.Generator().manual_seed(1000 * M + K), torch.device("cuda:0")
    for name in "gu":      # gate and up: different bytes, different scales
        if quantised:
            lin = torch.nn.Linear(K, F, bias=False)
            lin.weight.data = torch.randn(F, K, generator=g) * 0.06
            layer = W4Linear.from_linear(lin).to(dev)
        else:
            layer = W4Linear.from_mx(torch.randint(0, 256, (F, K // 2), generator=g, dtype=torch.uint8),
                                     torch.randint(127 - 12, 127 + 5, (F, K // 32), generator=g, dtype=torch.uint8)).to(dev)
        p["w" + name], p["s" + name], p["wide_" + name] = layer.weight.data, layer.block_scale, layer.widened()
        assert ((p["wide_" + name] == 0) | (p["wide_" + name].abs() >= 2.0 ** -126)).all(), "every widened value is a normal bf16 or zero"
    return p


def run_w4(p, s, biases, act, upd, w_up=None):
    a, c, cache, inds, cnt = operands(p, s)
    torch.ops.chipmunk.csp_mlp_mm1_glu_w4(a, p["wg"], p["wu"] if w_up is None else w_up, p["sg"], p["su"], c, *biases, cache, inds, cnt, act, upd)


BIT_CASES = ([(1003, 1536, 1, "column", act, upd) for act in ACTS for upd in (False, True)] +
             [(40, 128, 1, "column", "gelu_tanh", True), (40, 128, 1, "group", "silu", False), (128, 256, 1, "column", "gelu", True),
              (1003, 384, 1, "column", "silu", True), (1003, 384, 2, "column", "gelu_tanh", True), (1003, 384, 1, "group", "gelu", True)])


@pytest.mark.parametrize("M,K,B,layout,act,upd", BIT_CASES)
def test_bits_of_the_bf16_gated_form_on_the_widened_weights(dev, M, K, B, layout, act, upd):
    p = problem(M, K, B)
    assert len(p["wg"].unique()) == len(p["wu"].unique()) == 256 and not torch.equal(p["wg"], p["wu"]) and not torch.equal(p["sg"], p["su"])
    for biases in ((None, None), (p["bg"], p["bu"])):
        s, ref = fresh_state(p, layout), fresh_state(p, layout)
        run_w4(p, s, biases, act, upd)
        a, c, cache, inds, cnt = operands(p, ref)
        torch.ops.chipmunk.csp_mlp_mm1_glu(a, p["wide_g"], p["wide_u"], c, *biases, cache, inds, cnt, act, upd)
        what = f"M {M} K {K} B {B} {layout} {act} update {upd} biases {biases[0] is not None}"
        check_untouched(p, s, what, cache_written=upd)
        assert_same(s, ref, what)


def test_a_unit_up_branch_gives_the_bits_of_the_ungated_mxfp4_kernel(dev, act="gelu_tanh"):
    p = problem(1003, 384, 1)
    s, ref = fresh_state(p, "column"), fresh_state(p, "column")
    run_w4(p, s, (p["bg"], torch.ones(F, dtype=torch.bfloat16, device=dev)), act, True, w_up=torch.zeros_like(p["wu"]))
    a, c, cache, inds, cnt = operands(p, ref)
    torch.ops.chipmunk.csp_mlp_mm1_w4(a, p["wg"], p["sg"], c, p["bg"], cache, inds, cnt, act, True)
    check_untouched(p, s, "unit up branch", cache_written=True)
    assert_same(s, ref, "unit up branch", other="csp_mlp_mm1_w4 with the gate's weight, scales and bias")


@pytest.mark.parametrize("act", ACTS)
def test_segments_against_the_fp64_definition(dev, act):
    p = problem(1003, 384, 1, quantised=True)
    exact, _ = mm1_exact(p["a"][0], p["wide_g"], p["bg"], p["cache0"][0], p["inds"][0], p["cnt"][0], act, w_up=p["wide_u"], bias_up=p["bu"])
    s = fresh_state(p, "column")
    run_w4(p, s, (p["bg"], p["bu"]), act, True)
    check_untouched(p, s, f"definition {act}", cache_written=True)
    worst = assert_segs_close(s["c"][0], exact, MLP_SEG_BOUND, f"csp_mlp_mm1_glu_w4 {act}: packed deltas", width=MLP_SEG_W1, cols=p["cols"][0])
    print(f"csp_mlp_mm1_glu_w4 {act}: worst {MLP_SEG_W1}-column segment error {worst:.5f} (bound {MLP_SEG_BOUND})")


def test_the_operator_refuses_what_the_kernel_does_not_take(dev):
    p = problem(128, 256, 1)
    s = fresh_state(p, "column")
    a, c, cache, inds, cnt = operands(p, s)
    op, tail = torch.ops.chipmunk.csp_mlp_mm1_glu_w4, (c, None, None, cache, inds, cnt, "gelu_tanh", False)
    half = lambda t, n: t[:, :n].contiguous()      # noqa: E731
    for message, args in (("multiple of 128", (half(a, 64), half(p["wg"], 32), half(p["wu"], 32), half(p["sg"], 2), half(p["su"], 2))),
                          ("b_gate and b_up", (a, p["wide_g"], p["wu"], p["sg"], p["su"])),
                          ("scale_gate and scale_up", (a, p["wg"], p["wu"], p["sg"], half(p["su"], 7)))):
        with pytest.raises(RuntimeError, match=message):
            op(*args, *tail)
    check_untouched(p, s, "refused calls", cache_written=False)
    assert (s["c"] == 7.0).all()
