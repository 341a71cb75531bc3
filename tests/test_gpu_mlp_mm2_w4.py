"""``chipmunk::csp_mlp_mm2_w4`` ("MXFP4 fc2"), F = 1024; N2 = 128 is a partial column tile, 256 a whole one, 384 both.  Bits: the
result IS ``csp_mlp_mm2`` on ``widened()^T`` from the same c, a condition, not a tolerance -- on uniform weight bytes and independent scale
bytes; NaN in the packed columns at and past the counts, canary rows behind M, count-0 groups, a repeat launch.  Then the fp64 definition
under the segment bound tests/test_gpu_mlp_accuracy.py holds ``csp_mlp_mm2`` to, and a batch of two against two calls."""
import functools

import pytest
import torch

from helpers import MLP_SEG_BOUND, MLP_SEG_W2, assert_segs_close, mm2_exact
from test_gpu_mlp_mm2_w8 import BM, F, SENT, bits, dev, fresh_c  # noqa: F401  (F = 1024; c0 with 128 canary rows behind it)

pytestmark = pytest.mark.gpu
# M -> N2 -> counts per group, every value of {0, 8, 72, 256, 1000, F} in use
COUNTS = {
    256: {128: (F, 0), 256: (72, 1000), 384: (256, 8)},
    200: {128: (1000, 72), 256: (0, F), 384: (8, 256)},
    129: {128: (256, 8), 256: (F, 1000), 384: (72, F)},
    1: {128: (1000,), 256: (F,), 384: (256,)},
}
CASES = [(m, n2) for m in COUNTS for n2 in COUNTS[m]]


@functools.lru_cache(maxsize=None)
def problem(dev, M, N2, counts, seed):
    """NaN in the packed columns at and past each group's count; uniform weight bytes, scale bytes in 119 .. 135.  Shared, never written."""
    from chipmunk_amd.modules.mlp_fp8 import W4LinearT
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, F, device=dev, generator=g).to(torch.bfloat16)
    w = torch.randint(0, 256, (F, N2 // 2), device=dev, generator=g, dtype=torch.uint8)
    s = torch.randint(119, 136, (F, N2 // 32), device=dev, generator=g, dtype=torch.uint8)
    idx = torch.stack([torch.randperm(F, device=dev, generator=g) for _ in counts]).to(torch.int32)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    for gi, n in enumerate(counts):
        a[gi * BM:(gi + 1) * BM, n:] = float("nan")
    c0 = torch.randn(M, N2, device=dev, generator=g).to(torch.bfloat16)
    gathered = torch.cat([w[idx[gi, :n].long()].flatten() for gi, n in enumerate(counts)])
    assert torch.unique(gathered).numel() == 256, "all 256 byte values must occur among the gathered rows"
    assert (s[1:] != s[:-1]).float().mean() > 0.9 and (s[:, 1:] != s[:, :-1]).float().mean() > 0.9, "neighbouring rows and blocks must differ"
    w16T = W4LinearT.from_mx_t(w, s).widened().t().contiguous()
    assert w16T.dtype == torch.bfloat16 and torch.isfinite(w16T.float()).all()
    return dict(M=M, N2=N2, counts=counts, a=a, w=w, s=s, w16T=w16T, idx=idx, cnt=cnt, c0=c0)


def w4(a, w, s, idx, cnt, c):
    torch.ops.chipmunk.csp_mlp_mm2_w4(a, w, s, idx, cnt, c)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N2", CASES, ids=[f"M{m}-N{n}" for m, n in CASES])
def test_bits_of_the_bf16_gemm2_on_the_widened_weight(dev, M, N2):
    p = problem(dev, M, N2, COUNTS[M][N2], seed=M * 1000 + N2)
    ref_buf, ref = fresh_c(p)
    torch.ops.chipmunk.csp_mlp_mm2(p["a"], p["w16T"], p["idx"], p["cnt"], ref)
    got_buf, got = fresh_c(p)
    w4(p["a"], p["w"], p["s"], p["idx"], p["cnt"], got)
    assert (got_buf[M:] == SENT).all(), "rows at or past M were written"
    assert not torch.isnan(got.float()).any(), "a packed column at or past its group's count reached the sum"
    bad = (bits(got) != bits(ref)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ from csp_mlp_mm2 on the widened weight, the first at {bad[0].tolist()}"
    for gi, n in enumerate(p["counts"]):
        rows = slice(gi * BM, min(M, (gi + 1) * BM))
        assert (n == 0) == torch.equal(bits(got[rows]), bits(p["c0"][rows])), f"group {gi} with count {n}"
    again = fresh_c(p)[1]
    w4(p["a"], p["w"], p["s"], p["idx"], p["cnt"], again)
    assert torch.equal(bits(again), bits(got)), "a repeat launch gives other bits"


@pytest.mark.parametrize("M,N2", [(200, 128), (129, 256), (256, 384)], ids=["M200-N128", "M129-N256", "M256-N384"])
def test_fp64_definition_under_the_segment_bound_of_gemm2(dev, M, N2):
    p = problem(dev, M, N2, COUNTS[M][N2], seed=M * 1000 + N2)
    out = torch.zeros(M, N2, dtype=torch.bfloat16, device=dev)      # the zero base: a plain output, one rounding, no term
    w4(p["a"], p["w"], p["s"], p["idx"], p["cnt"], out)
    assert_segs_close(out, mm2_exact(p["a"], p["w16T"], p["idx"], p["cnt"]), MLP_SEG_BOUND, f"csp_mlp_mm2_w4 M{M} N{N2}", width=MLP_SEG_W2)      # (prints the worst segment)


def test_batch_of_two_equals_two_calls_on_the_slices(dev):
    M, N2 = 200, 384
    ps = [problem(dev, M, N2, (8, 256), seed=200384), problem(dev, M, N2, (1000, 0), seed=77)]
    (w, s), (a, idx, cnt, c0) = (ps[0]["w"], ps[0]["s"]), (torch.stack([q[k] for q in ps]) for k in ("a", "idx", "cnt", "c0"))
    got, ref = c0.clone(), c0.clone()
    w4(a, w, s, idx, cnt, got)
    for b in range(2):
        w4(a[b], w, s, idx[b], cnt[b], ref[b])
    assert torch.equal(bits(got), bits(ref)), "the batch differs from the per-sequence launches"
