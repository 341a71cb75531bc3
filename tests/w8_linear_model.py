"""The weight-only fp8 linear layer for few rows (``chipmunk_w8_linear`` / ``ops.w8_linear``; DESIGN 4.2, "Weight-only forward for few rows")
by its definition in fp64, the definition with its roundings in torch, and mutants of it -- for tests/test_w8_linear_host.py,
tests/test_gpu_w8_linear.py and tests/test_gpu_w8_linear_e2e.py.

    y[m, i] = (sum_k x[m, k] * f(w[i, k])) * s[i] + b[i]

x bf16 ``[M, K]``, w e4m3 ``[F, K]`` with f the exact widening, s fp32 (one number or ``[F]``), b bf16 ``[F]`` or None (zero)."""
import functools

import torch

from mlp_w8_model import E4M3, every_byte_weight

SHAPES_HOST = ((1, 64, 1024), (34, 192, 1032), (129, 3072, 1024), (257, 1536, 2048))     # (M, K, F)
SHAPES_GPU = ((1, 64, 8), (34, 192, 1032), (129, 3072, 1024), (257, 1536, 2048), (128, 64, 16),
              (96, 64, 16), (97, 128, 24), (385, 128, 136))      # the 96-row block exactly full / one row over; a fourth 128-row block of one row
SEG_WIDTH = 64
# the worst 64-column segment of the torch definition path (fp32 matmul, bf16(S s), bf16(. + b)) against the fp64 model over SHAPES_HOST,
# both scale kinds, with and without a bias, on the inputs of `case`, rounded up: two bf16 roundings of independent elements (per shape
# 0.0028, 0.0046, 0.0038, 0.0051).  tests/test_w8_linear_host.py pins it (test_floor_constant_is_tight); the bound of every comparison
# stays the sparse MLP's MLP_SEG_BOUND.
FLOOR_W8_LINEAR = 0.0052


def exact(x, w8, scale, bias):
    """-> ``[M, F]`` fp64"""
    s = scale.double().reshape(-1)
    y = (x.double() @ w8.double().T) * (s if s.numel() > 1 else s[0])
    return y if bias is None else y + bias.double()


def definition(x, w8, scale, bias, mutant=None):
    """The definition with its roundings: fp32 sums, ``bf16(bf16(S s) + b)``; ``mutant`` names one of MUTANTS."""
    xf, wf = x.float(), w8.float()
    s = scale.float().reshape(-1)
    s = s if s.numel() > 1 else s[0]
    b = None if bias is None else bias.float()
    K = xf.shape[1]
    if mutant == "last_k_block_dropped":
        xf, wf = xf[:, : K - 64], wf[:, : K - 64]
    elif mutant == "k_halves_of_a_16_byte_piece_swapped":          # on the weight only: k <-> k ^ 8
        wf = wf[:, torch.arange(K) ^ 8]
    elif mutant == "scale_of_row_i_plus_1" and s.dim() == 1:
        s = s.roll(-1)
    elif mutant == "bias_of_row_i_plus_1" and b is not None:
        b = b.roll(-1)
    elif mutant == "input_row_m_plus_1":
        xf = xf.roll(-1, dims=0)
    elif mutant == "subnormals_read_as_zero":
        wf = torch.where((w8.view(torch.uint8) & 0x78) == 0, torch.zeros_like(wf), wf)
    S = xf @ wf.T
    if mutant == "bias_before_scale" and b is not None:
        return ((S + b) * s).to(torch.bfloat16)
    t = (S * s).to(torch.bfloat16)
    return t if b is None else (t.float() + b).to(torch.bfloat16)


MUTANTS = ("last_k_block_dropped", "k_halves_of_a_16_byte_piece_swapped", "scale_of_row_i_plus_1", "bias_of_row_i_plus_1",
           "bias_before_scale", "input_row_m_plus_1", "subnormals_read_as_zero")


@functools.lru_cache(maxsize=None)
def case(M, K, F):
    """The inputs of a shape, built once and shared: x = randn bf16, w with every finite e4m3 byte, one scale and a vector of scales
    uniform in [0.001, 0.011], bias 2 randn bf16 -- and the fp64 results by (vector scale?, bias?).  Treat as read-only."""
    g = torch.Generator().manual_seed(1000 * M + K + F)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w8 = every_byte_weight(F, K, seed=M + K + F)
    sv = (0.001 + 0.01 * torch.rand(F, generator=g)).float()
    s1 = sv[:1].clone()
    bias = (2 * torch.randn(F, generator=g)).to(torch.bfloat16)
    ref = {(vec, hb): exact(x, w8, sv if vec else s1, bias if hb else None) for vec in (False, True) for hb in (False, True)}
    return dict(x=x, w=w8, s1=s1, sv=sv, bias=bias, exact=ref)


@functools.lru_cache(maxsize=None)
def integer_case(M, K, F):
    """Known answers: x integers in [-4, 4], weight VALUES integers in [-8, 8], a power-of-two scale: every partial sum is exact in fp32
    (|S| <= 32 K < 2^24), so without a bias the result is the ONE rounding of the exact value -- ``exact(...).to(bf16)``.  With a bias
    the inner rounding has to be exact as well: ``x_sparse`` has at most 6 nonzero entries per row (|S| <= 192), so under the scale 1/2
    and an integer bias in [-16, 16] every intermediate is a multiple of 1/2 below 128 -- a bf16 value."""
    g = torch.Generator().manual_seed(7 * M + K + F)
    x = torch.randint(-4, 5, (M, K), generator=g).float()
    xs = torch.zeros(M, K)
    for m in range(M):
        cols = torch.randperm(K, generator=g)[:6]
        xs[m, cols] = x[m, cols]
    w = torch.randint(-8, 9, (F, K), generator=g).float()
    bias = torch.randint(-16, 17, (F,), generator=g).float()
    return dict(x=x.to(torch.bfloat16), x_sparse=xs.to(torch.bfloat16), w=w.to(E4M3), bias=bias.to(torch.bfloat16))
