"""The weight-only fp8 GEMM1 (``csp_mlp_mm1_w8``; DESIGN 4.2, "Weight-only fc1") by its definition, in fp64, and ``W8Linear``'s quantiser
written out on its own -- for tests/test_mlp_w8_host.py, tests/test_gpu_mlp_w8.py and tests/test_gpu_mlp_w8_e2e.py.

    C[m, j] = act((sum_k A[m, k] * f(W[idx[g, j], k])) * s[idx[g, j]] + bias[idx[g, j]]) - cache[idx[g, j], m]

A bf16 ``[M, K]``, W e4m3 ``[F, K]`` with f the exact widening, s one fp32 number or one per row of W, bias bf16 ``[F]`` or None (zero)."""
import torch

from helpers import MLP_BM, mlp_act64

E4M3 = torch.float8_e4m3fn


def mm1_w8_exact(a, w8, scale, bias, cache, inds, counts, act="gelu_tanh"):
    """-> (delta, fresh) ``[M, F]`` fp64 in the packed layout, 0 at and past the counts (the layout of helpers.mm1_exact)."""
    M, F = a.shape[0], w8.shape[0]
    delta = torch.zeros(M, F, dtype=torch.float64, device=a.device)
    fresh = torch.zeros_like(delta)
    ad, wd = a.double(), w8.double()                                        # (e4m3 -> fp64 is exact)
    sd = scale.double().reshape(-1)
    sd = sd.expand(F) if sd.numel() == 1 else sd
    for g in range(inds.shape[0]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(counts[g])
        if n == 0:
            continue
        col = inds[g, :n].long()
        h = (ad[rows] @ wd[col].T) * sd[col]
        if bias is not None:
            h = h + bias[col].double()
        f = mlp_act64(act, h)
        fresh[rows, :n] = f
        delta[rows, :n] = f - cache[col][:, rows].double().T
    return delta, fresh


def pow2_quantize(w, scaling):
    """W8Linear's quantiser by its definition: per tensor or per output feature (row of ``w [out, in]``) the smallest power of two ``2^e``
    with ``amax / 2^e <= 448``, found by exact comparisons in fp64; -> (e4m3 weight, reciprocal scale fp32 ``[]`` or ``[out]``)."""
    wd = w.double()
    amax = wd.abs().amax(dim=1) if scaling == "row" else wd.abs().amax().reshape(1)
    recip = torch.ones_like(amax)
    for i, v in enumerate(amax.tolist()):
        e = 0
        if v > 0:
            while v > 448.0 * 2.0 ** e:
                e += 1
            while v <= 448.0 * 2.0 ** (e - 1):
                e -= 1
        recip[i] = 2.0 ** e
    q = (wd / (recip[:, None] if scaling == "row" else recip)).float().to(E4M3)
    return q, (recip if scaling == "row" else recip.reshape(())).float()


def every_byte_weight(F, K, seed):
    """An e4m3 ``[F, K]`` weight in which every finite byte occurs (254 of them: 0x7f / 0xff are NaN), in every row when K >= 254:
    each row is a random draw of finite bytes whose first min(K, 254) entries are a permutation of all of them."""
    g = torch.Generator().manual_seed(seed)
    finite = torch.tensor([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=torch.uint8)
    rows = []
    for _ in range(F):
        perm = finite[torch.randperm(254, generator=g)]
        if K <= 254:
            rows.append(perm[:K])
        else:
            rows.append(torch.cat([perm, finite[torch.randint(0, 254, (K - 254,), generator=g)]]))
    w = torch.stack(rows)
    if K < 254:      # short rows: the bytes are spread over the rows instead
        flat = w.flatten()
        flat[:254] = finite
        w = flat.reshape(F, K)
    return w.view(E4M3)
