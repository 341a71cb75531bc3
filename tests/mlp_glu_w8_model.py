"""The gated weight-only fp8 GEMM1 (``csp_mlp_mm1_glu_w8``; DESIGN 4.2, "Gated weight-only GEMM1") by its definition, in fp64 -- for
tests/test_mlp_glu_w8_host.py, tests/test_gpu_mlp_glu_w8.py and tests/test_gpu_mlp_glu_w8_e2e.py.  With i = idx[g, j]:

    g = (sum_k A[m, k] * f(Wg[i, k])) * sg[i] + bg[i]
    u = (sum_k A[m, k] * f(Wu[i, k])) * su[i] + bu[i]
    C[m, j] = act(g) * u - cache[i, m]

A bf16 ``[M, K]``, Wg / Wu e4m3 ``[F, K]`` with f the exact widening, sg / su one fp32 number each or one per weight row, bg / bu bf16
``[F]`` or None (zero).  The packed layout of ``mlp_w8_model.mm1_w8_exact``."""
import torch

from helpers import MLP_BM, mlp_act64


def _per_row(scale, F):
    sd = scale.double().reshape(-1)
    return sd.expand(F) if sd.numel() == 1 else sd


def mm1_glu_w8_exact(a, w_gate, w_up, scale_gate, scale_up, bias_gate, bias_up, cache, inds, counts, act="silu"):
    """-> (delta, fresh) ``[M, F]`` fp64 in the packed layout, 0 at and past the counts."""
    M, F = a.shape[0], w_gate.shape[0]
    delta = torch.zeros(M, F, dtype=torch.float64, device=a.device)
    fresh = torch.zeros_like(delta)
    ad, gd, ud = a.double(), w_gate.double(), w_up.double()                 # (e4m3 -> fp64 is exact)
    sg, su = _per_row(scale_gate, F), _per_row(scale_up, F)
    for g in range(inds.shape[0]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(counts[g])
        if n == 0:
            continue
        col = inds[g, :n].long()
        hg = (ad[rows] @ gd[col].T) * sg[col]
        hu = (ad[rows] @ ud[col].T) * su[col]
        if bias_gate is not None:
            hg = hg + bias_gate[col].double()
        if bias_up is not None:
            hu = hu + bias_up[col].double()
        f = mlp_act64(act, hg) * hu
        fresh[rows, :n] = f
        delta[rows, :n] = f - cache[col][:, rows].double().T
    return delta, fresh
