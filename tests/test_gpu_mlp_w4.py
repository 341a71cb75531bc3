"""``csp_mlp_mm1_w4`` ("MXFP4 fc1") on the GPU.  (a) Bits: packed deltas and cache are ``csp_mlp_mm1_act``'s on ``W4Linear.widened()``,
with and without a bias, sentinels included (random bytes: all 16 nibbles; block exponents in [-12, 4]: every widened value a normal bf16 or
zero).  (b) Definition: 64-column segments against helpers.mm1_exact in fp64 under helpers.MLP_SEG_BOUND, the bf16 form's own bound.
(c) Known answer: a = rows of the identity, c[m, j] = bf16(act(W[indices[j], m])) exactly."""
import functools

import pytest
import torch

import test_gpu_mlp_w8 as w8
from helpers import MLP_ACTS as ACTS, MLP_COUNTS, MLP_SEG_BOUND, MLP_SEG_W1, assert_segs_close, mm1_exact
from test_gpu_mlp_w8 import dev  # noqa: F401  (the device fixture)

pytestmark = pytest.mark.gpu

F = 512
COUNTS = {40: (tuple(MLP_COUNTS[333][2:]),), 128: (tuple(MLP_COUNTS[333][1:2]),), 1003: (tuple(MLP_COUNTS[1000]), tuple(MLP_COUNTS[1000][::-1]))}


@functools.lru_cache(maxsize=None)
def problem(M, K, B, f=F, seed=0, counts=None, layer=None):
    """tests/test_gpu_mlp_w8.py's inputs (a, cache, bias, index lists) with an MXFP4 weight: random, or `layer`'s (a W4Linear)"""
    from chipmunk_amd.modules import W4Linear
    p = dict(w8.problem(M, K, B, f=f, seed=seed, counts=counts or COUNTS[M][:B]))
    g = torch.Generator().manual_seed(M + K + seed)
    layer = layer or W4Linear.from_mx(torch.randint(0, 256, (f, K // 2), generator=g, dtype=torch.uint8),
                                      torch.randint(127 - 12, 127 + 5, (f, K // 32), generator=g, dtype=torch.uint8))
    layer = layer.to(p["a"].device)
    p["w4"], p["sc"], p["wide"] = layer.weight.data, layer.block_scale, layer.widened()
    assert ((p["wide"] == 0) | (p["wide"].abs() >= 2.0 ** -126)).all(), "every widened value is a normal bf16 or zero"
    return p


def run_both(p, layout, bias, act, upd, what):      # both forms from equal states: untouched sentinels, equal bits
    s, ref = w8.fresh_state(p, layout), w8.fresh_state(p, layout)
    a, c, cache, inds, cnt = w8.operands(p, s)
    torch.ops.chipmunk.csp_mlp_mm1_w4(a, p["w4"], p["sc"], c, bias, cache, inds, cnt, act, upd)
    a, c, cache, inds, cnt = w8.operands(p, ref)
    torch.ops.chipmunk.csp_mlp_mm1_act(a, p["wide"], c, bias, cache, inds, cnt, act, upd)
    w8.check_untouched(p, s, what, cache_written=upd)
    w8.assert_same(p, s, ref, what)
    return s


BIT_CASES = ([(1003, 1536, 1, "column", act, upd) for act in ACTS for upd in (False, True)] +
             [(40, 128, 1, "column", "gelu_tanh", True), (40, 256, 1, "group", "silu", False), (128, 384, 1, "column", "gelu", True), (128, 128, 1, "group", "gelu_tanh", True),
              (1003, 256, 2, "column", "gelu_tanh", True), (1003, 384, 2, "group", "silu", True), (1003, 128, 2, "column", "gelu", False),
              (1003, 1536, 1, "group", "gelu_tanh", True), (1003, 384, 1, "group", "gelu", False)])


@pytest.mark.parametrize("M,K,B,layout,act,upd", BIT_CASES)
def test_bits_of_the_bf16_form_on_the_widened_weight(dev, M, K, B, layout, act, upd):
    p = problem(M, K, B)
    assert len(p["w4"].unique()) == 256
    for bias in (None, p["bias"]):
        run_both(p, layout, bias, act, upd, f"M {M} K {K} B {B} {layout} {act} update {upd} bias {bias is not None}")


@pytest.mark.parametrize("layout", ["column", "group"])
def test_bits_through_the_tail_split(dev, layout):
    # every XCD keeps leftover tiles and hands them out as 64 x 64 sub-tiles (tests/test_gpu_mlp_w8.py's launch shape); a remainder of 40 columns
    f = ((2 * torch.cuda.get_device_properties(0).multi_processor_count // 8) // 2 + 1) * 128
    lists = ((2048, 0, 1024, 3072, 512, 256, 4096, f), (256, f, 0, 1024, 2048, 552, f, f))
    p = problem(1003, 256, 2, f=f, seed=7, counts=tuple(tuple(min(c, f) for c in row) for row in lists))
    run_both(p, layout, p["bias"], "gelu_tanh", True, f"tail split {layout}")


@pytest.mark.parametrize("act", ACTS)
def test_segments_against_the_fp64_definition(dev, act):
    from chipmunk_amd.modules import W4Linear
    lin = torch.nn.Linear(384, F, bias=False)
    lin.weight.data = torch.randn(F, 384, generator=torch.Generator().manual_seed(77)) * 0.06      # quantised by the OCP rule
    p = problem(1003, 384, 1, seed=3, layer=W4Linear.from_linear(lin))
    exact, _ = mm1_exact(p["a"][0], p["wide"], p["bias"], p["cache0"][0], p["inds"][0], p["cnt"][0], act)
    s = run_both(p, "column", p["bias"], act, True, f"definition {act}")
    worst = assert_segs_close(s["c"][0], exact, MLP_SEG_BOUND, f"csp_mlp_mm1_w4 {act}: packed deltas", width=MLP_SEG_W1, cols=p["cols"][0])
    print(f"csp_mlp_mm1_w4 {act}: worst {MLP_SEG_W1}-column segment error {worst:.5f} (bound {MLP_SEG_BOUND})")


@pytest.mark.parametrize("act", ACTS)
def test_known_answer_from_identity_rows(dev, act):
    """act is the kernels' fp32 one (299 of 26 624 gelu_tanh values a bf16 step off fp64's): its table comes from the bf16 form run without a gather"""
    p = dict(problem(128, 128, 1))
    p["a"], p["cache0"] = torch.eye(128, dtype=torch.bfloat16, device=dev)[None], torch.zeros_like(p["cache0"])
    s = run_both(p, "column", None, act, False, f"identity rows {act}")
    table, n = torch.zeros(128, F, dtype=torch.bfloat16, device=dev), int(p["cnt"][0, 0])
    torch.ops.chipmunk.csp_mlp_mm1_act(p["a"][0], p["wide"], table, None, p["cache0"][0].clone(), torch.arange(F, dtype=torch.int32, device=dev)[None],
                                       torch.tensor([F], dtype=torch.int32, device=dev), act, False)
    off = s["c"][0][:, :n] != table[:, p["inds"][0, 0, :n].long()]
    assert not off.any(), f"{act}: {int(off.sum())} elements are not act(W[indices[j], m]), first at (m, j) = {off.nonzero()[0].tolist()}"
