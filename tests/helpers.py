"""Shared helpers for the parity tests: seeded synthetic inputs in the reference's shapes, index generators."""
import torch


def randn_bf16(*shape, seed=0, device="cpu", scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(device)


def random_index_sets(B, H, G, n_keys, count, width, seed=0, multiple_of=1):
    """Per (b,h,g) a random sorted subset of `count` distinct columns of range(n_keys); rows padded to `width` with -1."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    inds = torch.full((B, H, G, width), -1, dtype=torch.int32)
    counts = torch.full((B, H, G), count, dtype=torch.int32)
    for b in range(B):
        for h in range(H):
            for q in range(G):
                perm = torch.randperm(n_keys, generator=g)[:count].sort().values
                inds[b, h, q, :count] = perm.to(torch.int32)
    assert count % multiple_of == 0
    return inds, counts


def assert_close_bf16(a, b, atol=2e-2, rtol=2e-2, what=""):
    a32, b32 = a.float().cpu(), b.float().cpu()
    diff = (a32 - b32).abs()
    tol = atol + rtol * b32.abs()
    bad = ~(diff <= tol)   # (not `diff > tol`: a NaN on either side must count as a mismatch)
    assert not bad.any(), (f"{what}: {int(bad.sum())} / {bad.numel()} elements off ({int(torch.isnan(a32).sum())} NaN), "
                           f"max abs diff {torch.nan_to_num(diff, nan=float('inf')).max().item():.4g}")


def structured_qkv(H, N, n_hot, step, layer, seed=31337, gain=6.0):
    """Attention inputs with planted structure for module-level parity tests: per head a fixed hot set of `n_hot` keys
    whose scores sit `gain` above the noise floor for every query (q and the hot keys share a direction), fresh noise per
    (step, layer).  The top-k of the column sums is then the hot set plus noise-floor filler whose choice cannot move the
    output: implementations that break ties / round column sums differently still agree to bf16 precision.
    Returns q, k, v ``[1, H, N, 128]`` bf16 and hot ``[H, n_hot]`` (sorted)."""
    g0 = torch.Generator().manual_seed(seed)
    hot = torch.stack([torch.randperm(N, generator=g0)[:n_hot].sort().values for _ in range(H)])
    u = torch.randn(H, 128, generator=g0)
    u = u / u.norm(dim=-1, keepdim=True)
    g = torch.Generator().manual_seed(seed + 1000 * step + 10 * layer + 1)
    q = 0.3 * torch.randn(1, H, N, 128, generator=g)
    k = 0.3 * torch.randn(1, H, N, 128, generator=g)
    v = torch.randn(1, H, N, 128, generator=g)
    amp = (gain * 128 ** 0.5) ** 0.5            # (amp * u) . (amp * u) / sqrt(128) = gain
    q = q + amp * u[None, :, None, :]
    for h in range(H):
        k[0, h, hot[h]] += amp * u[h]
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), hot


# --------------------------------------------------------------------------- attention accuracy: exact reference + row metric
# The attention outputs shrink like sqrt(e / n_keys) with randn inputs, so an absolute tolerance stops seeing defects from a
# few thousand keys on.  The row-relative error against exact fp64 attention does not: docs/TEST_SENSITIVITY.md.
#
# ORACLE_ROW_ERR: the largest row error of the CPU oracle (the reference's roundings: bf16 P, bf16 output) against
# attn_exact over the case list of tests/test_attn_metric_cpu.py (accumulate form included), rounded up to two digits; that
# file pins it.
# ROW_ERR_MARGIN: what a correct kernel may do differently (summation order, tile size, reference point of the
# exponentials, hardware exp2).  tests/test_attn_metric_cpu.py caps margin * floor at half the weakest mutant's error.
ORACLE_ROW_ERR = 0.0029
ROW_ERR_MARGIN = 2.0
ROW_ERR_BOUND = ROW_ERR_MARGIN * ORACLE_ROW_ERR
BF16_EPS = 2.0 ** -8          # round-to-nearest bf16 (8 significant bits): relative error of one rounding, per element
GROUP_ROWS = 192              # query rows that share one index list
SCALE_LOG2E = 1.4426950408889634 / 128 ** 0.5     # the kernels' constant c: scores in exp2 units are q.k * c


def _row_range(rows, n):
    if rows is None:
        return 0, n
    if isinstance(rows, slice):
        start, stop, step = rows.indices(n)
        assert step == 1
        return start, stop
    return int(rows[0]), int(rows[1])


def attn_exact(q, k, v, inds=None, counts=None, rows=None, keep=None, scale_mul=1.0, chunk_bytes=1 << 28, with_top=False):
    """fp64 ``softmax(q k^T / sqrt(D)) v`` with plain torch on the inputs' device: ``[B, H, rows, D]`` float64.

    inds / counts ``[B, H, G, width]`` / ``[B, H, G]``: per (head, 192-row group) the keys are ``inds[..., :count]`` (count
    clamped to the key count, as the kernels do), duplicates counted as often as listed.  A group with count 0 has no
    attention output: its rows are 0 (what every form adds for it) and `row_rel_err` wants them reproduced exactly.
    rows: ``slice`` or ``(start, stop)`` of query rows.  keep: bool key mask broadcastable to ``[B, H, Nk]`` (dense form) and
    scale_mul (multiplies the 1/sqrt(D) scale): the defects of tests/test_attn_metric_cpu.py.
    with_top: also return ``[B, H, rows]`` ``max_j w_ij * ||v_j||`` of the row's heaviest key (w the softmax weights), the
    ingredient of `top_key_term`."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    r0, r1 = _row_range(rows, Nq)
    scale = scale_mul / (D ** 0.5)
    out = torch.zeros(B, H, r1 - r0, D, dtype=torch.float64, device=q.device)
    tops = torch.zeros(B, H, r1 - r0, dtype=torch.float64, device=q.device)
    if keep is not None:
        keep = keep.to(q.device).expand(B, H, Nk)

    def block(qb, kb, vb, mask, top=None):
        # qb [R, D], kb / vb [n, D] float64; chunked over rows so that the score block stays under chunk_bytes
        res = torch.empty(qb.shape[0], D, dtype=torch.float64, device=qb.device)
        step = max(1, chunk_bytes // (8 * max(1, kb.shape[0])))
        for a in range(0, qb.shape[0], step):
            s = (qb[a:a + step] @ kb.T) * scale
            if mask is not None:
                s = s.masked_fill(~mask[None, :], float("-inf"))
            w = torch.softmax(s, dim=-1)
            res[a:a + step] = w @ vb
            if top is not None:
                wmax, jmax = w.max(-1)
                top[a:a + step] = wmax * vb[jmax].norm(dim=-1)
        return res

    for b in range(B):
        for h in range(H):
            qd = q[b, h, r0:r1].double()
            kd, vd = k[b, h].double(), v[b, h].double()
            top = tops[b, h] if with_top else None
            if inds is None:
                out[b, h] = block(qd, kd, vd, None if keep is None else keep[b, h], top)
                continue
            assert keep is None, "defects of a gathered launch are made by editing the index list"
            for g in range(r0 // GROUP_ROWS, (r1 + GROUP_ROWS - 1) // GROUP_ROWS):
                a, e = max(r0, g * GROUP_ROWS), min(r1, (g + 1) * GROUP_ROWS)
                c = min(int(counts[b, h, g]), Nk)
                if c <= 0 or a >= e:
                    continue
                idx = inds[b, h, g, :c].to(q.device).long()
                out[b, h, a - r0:e - r0] = block(qd[a - r0:e - r0], kd[idx], vd[idx], None, None if top is None else top[a - r0:e - r0])
    return (out, tops) if with_top else out


# --------------------------------------------------------------------------- computed allowance for one documented design rounding
# Every kernel rounds P to bf16 for the PV product and sums the unrounded p into the normaliser, as the reference (and the
# oracle) does.  With a running maximum the heaviest key of a row has p = 1 exactly; its rounding is the one rounding the
# oracle's floor does not contain.  Two kernels take the exponentials against another point when they can prove the scores
# bounded -- attn64.hip's dense kernel ("Fixed reference point", `nomax`: M_i = |q_i| max|k|) and attn96.hip (`nomax`: no
# reference point, c folded into Q) -- so there that p is not 1 and its bf16 rounding, up to 2^-8, scales its key's whole
# contribution: at most 2^-8 w_max ||v_jmax|| / ||x_i|| of row error (w_max the largest softmax weight of the row).  On
# diffuse rows over thousands of keys that is a tenth of the bound, over a few hundred keys a quarter, on a one-hot row
# 0.0039; measured: 0.0055 - 0.0058 on the spike / aligned inputs against the oracle's 0.0001.  The term is a function of the inputs alone; it is added to the bound for
# the rows of the waves that take those paths, and for no other kernel.
def top_key_term(exact, top):
    den = exact.norm(dim=-1)
    return torch.where(den > 0, BF16_EPS * top / den, torch.zeros_like(den))


def _wave_all(ok, wave):
    """ok [B, H, Nq] bool -> the same shape, True where every row of the row's `wave`-row wave is ok (rows past Nq are)"""
    n = ok.shape[-1]
    pad = (-n) % wave
    w = torch.nn.functional.pad(ok, (0, pad), value=True).view(*ok.shape[:-1], -1, wave).all(-1)
    return w.repeat_interleave(wave, dim=-1)[..., :n]


def _score_bound(q, k):
    """|q_i| max_j |k_j| c per row, exp2 units, fp64 (max over ALL keys of the head, as knorm_max_kernel takes it)"""
    kmax = k.double().norm(dim=-1).max(-1).values
    return q.double().norm(dim=-1) * kmax[..., None] * SCALE_LOG2E


def attn_exact_dense64(q, k, v, rows=None, running_max=False):
    """(exact, extra) for attn64.hip's dense kernel: plain exact attention, and per row the `top_key_term` where the row's 64-row
    wave takes the fixed reference point (2 |q_i| max|k| c <= 64 for all its queries; never with option attn_nomax = 2:
    running_max), 0 elsewhere.  assert_rows_close takes the pair as its `exact`."""
    exact, top = attn_exact(q, k, v, rows=rows, with_top=True)
    r0, r1 = _row_range(rows, q.shape[2])
    fixed = _wave_all(2.0 * _score_bound(q, k) <= 64.0, 64) & (not running_max) & (q.shape[0] * q.shape[1] * 4 <= (32 << 10))
    return exact, torch.where(fixed[..., r0:r1], top_key_term(exact, top), torch.zeros_like(top))


def attn_exact_csp96(q, k, v, inds, counts, rows=None, running_max=False):
    """(exact, extra) for attn96.hip.  A 96-row wave whose queries all have |q_i| max|k| c <= 55 drops the reference point and
    folds c into the bf16 Q fragments (load_q: `pack_bf16x2(lo * SCALE_LOG2E, hi * SCALE_LOG2E)`): for its rows `exact` is
    attention over bf16(q c) with the rest of the scale in fp64 -- the exact effect of that documented rounding -- and
    `extra` the `top_key_term`; other waves (and option attn_nomax = 2: running_max): plain exact attention, 0."""
    plain = attn_exact(q, k, v, inds, counts, rows=rows)
    r0, r1 = _row_range(rows, q.shape[2])
    folds = (_wave_all(_score_bound(q, k) <= 55.0, 96) & (not running_max) & (q.shape[0] * q.shape[1] * 4 <= (32 << 10)))[..., r0:r1]
    if not folds.any():
        return plain, torch.zeros_like(plain[..., 0])
    c32 = torch.tensor(0.08838834764, dtype=torch.float32) * torch.tensor(1.44269504089, dtype=torch.float32)   # as compiled
    qf = (q.float() * c32.to(q.device)).to(torch.bfloat16)
    folded, top = attn_exact(qf, k, v, inds, counts, rows=rows, scale_mul=0.6931471805599453 * 128 ** 0.5, with_top=True)
    folds = folds.to(plain.device)
    return torch.where(folds[..., None], folded, plain), torch.where(folds, top_key_term(folded, top), torch.zeros_like(top))


def row_rel_err(o, exact):
    """Per query row ``||o_i - x_i||_2 / ||x_i||_2`` in fp64, shape ``o.shape[:-1]``.  A NaN / Inf anywhere in ``o_i`` is an
    infinite error; a row whose exact value is 0 (group without keys) has error 0 if reproduced exactly, else infinite."""
    o = o.to(exact.device).double()
    num = (o - exact).norm(dim=-1)
    den = exact.norm(dim=-1)
    err = num / den
    err = torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))), err)
    return torch.where(torch.isfinite(o).all(dim=-1) & ~torch.isnan(err), err, torch.full_like(err, float("inf")))


def _record_row_err(what, worst, bound):
    import os
    path = os.environ.get("CHIPMUNK_ROW_ERR_LOG")      # (how the per-path table of docs/TEST_SENSITIVITY.md is collected)
    print(f"row error {what}: worst {worst:.5f} (bound {bound:.5f}, {worst / ORACLE_ROW_ERR:.2f} x oracle floor)")
    if path:
        with open(path, "a") as f:
            f.write(f"{what}\t{worst:.6f}\t{bound:.6f}\n")


def assert_rows_close(o, exact, bound=ROW_ERR_BOUND, what="", row0=0, extra=None):
    """Every row of ``o`` ``[B, H, R, D]`` within `bound` (row-relative, see `row_rel_err`) of ``exact``; ``row0`` is the index
    of the first row in the full launch (for the group / row named in the message); ``extra`` ``[B, H, R]`` widens the bound
    per row by a derived term.  Returns the worst ``error - extra``."""
    if isinstance(exact, tuple):           # (exact, per-row term of a design rounding: attn_exact_dense64 / attn_exact_csp96)
        exact, term = exact
        extra = term if extra is None else extra.to(term.device) + term
    assert o.shape == exact.shape, (o.shape, exact.shape)
    err = row_rel_err(o, exact)
    if extra is not None:
        err = err - extra.to(err.device)
    worst = float(err.max()) if err.numel() else 0.0
    _record_row_err(what, worst, bound)
    bad = ~(err <= bound)
    if bad.any():
        flat = int(torch.nan_to_num(err, nan=float("inf")).argmax())
        R = err.shape[2]
        b, h, r = flat // (err.shape[1] * R), (flat // R) % err.shape[1], flat % R
        raise AssertionError(
            f"{what}: row error {worst:.4g} > {bound:.4g} at batch {b} head {h} group {(row0 + r) // GROUP_ROWS} "
            f"row {row0 + r} (row {(row0 + r) % GROUP_ROWS} of its group); {int(bad.sum())} / {bad.numel()} rows over the "
            f"bound, {int((~torch.isfinite(o.float())).sum())} non-finite elements")
    return worst


def assert_delta_rows_close(result, base, exact, o_scale=1, bound=ROW_ERR_BOUND, what="", row0=0):
    """Accumulate forms (``result = base + o_scale * attention``): the error is taken on ``result - base`` against
    ``o_scale * exact``.  The stored sum is rounded to bf16 once more than a plain output, which moves element e of the
    difference by at most 2^-8 |result_e| (half of the 2^-7 spacing of 8 significant bits): per row the bound is widened by
    ``2^-8 ||result_i|| / ||exact_i||``.  Derived, not tuned; with a unit-size base this term is several times the bound
    itself, which is why the accumulate tests also run on a base of the delta's magnitude."""
    term = None
    if isinstance(exact, tuple):
        exact, term = exact
    dev = exact.device
    res, b0 = result.to(dev).double(), base.to(dev).double()
    den = exact.norm(dim=-1)
    extra = torch.where(den > 0, BF16_EPS * res.norm(dim=-1) / den, torch.zeros_like(den))
    delta = torch.where(torch.isfinite(res), res - b0, res)
    extra = torch.nan_to_num(extra, nan=0.0, posinf=0.0)
    return assert_rows_close(delta, o_scale * exact, bound, what, row0, extra=extra if term is None else extra + term)


# |sum_d o[i, d] - 1| of the oracle with an indicator V (every row of a non-empty group is a probability vector), measured
# by tests/test_attn_metric_cpu.py::test_indicator_v_row_sums_of_the_oracle on the GPU test's inputs, rounded up
ORACLE_ROWSUM_ERR = 0.0024


def indicator_v(n, kind, device="cpu"):
    """``v[j, d] = 1 if class(j) == d else 0``, bf16 ``[n, 128]``: o[i, d] is then the softmax mass of class d.
    kind "key": class(j) = j mod 128; "tile": (j // 32) mod 128 -- a 32-key tile that is skipped, read twice or taken
    from elsewhere moves ONE column by its whole value, and the column names the tile."""
    j = torch.arange(n, device=device)
    cls = j % 128 if kind == "key" else (j // 32) % 128
    return torch.nn.functional.one_hot(cls, 128).to(torch.bfloat16)


# --------------------------------------------------------------------------- inputs shared by test_gpu_attn_accuracy.py and the CPU
# test that measures the oracle on them (tests/test_attn_metric_cpu.py); all CPU tensors


def gathered_matrix_inputs():
    """3 heads, 4 100 query rows (22 groups, the last of 68 rows), 8 448 keys; per (head, group) a random key order of which a
    ragged count is kept (0, 7, 33, every key, tails that are no multiple of 16 / 32 / 64); `shared`: one key order per
    head for all its groups, so that the position in the list is a property of the key and an indicator V can mark it
    (`v_pos`: class = 32-key tile of the list, mod 128)."""
    H, nq, nk = 3, 4100, 8448
    G = (nq + GROUP_ROWS - 1) // GROUP_ROWS
    q, k, v = [randn_bf16(1, H, n, 128, seed=s) for n, s in ((nq, 211), (nk, 212), (nk, 213))]
    gen = torch.Generator().manual_seed(214)
    inds = torch.stack([torch.randperm(nk, generator=gen) for _ in range(H * G)]).view(1, H, G, nk).to(torch.int32)
    inds[0, 2, 3] = torch.arange(nk, dtype=torch.int32)
    counts = torch.full((1, H, G), 1100, dtype=torch.int32)          # 1100 = 17 x 64 + 12: a masked tail everywhere
    counts[0, 0, 1], counts[0, 1, 2], counts[0, 2, 3] = 0, 7, nk      # no key, fewer than a tile, every key (sliced by the plan)
    counts[0, 0, 5], counts[0, 1, 7], counts[0, 2, 9] = 1093, 2050, 33
    counts[0, 0, G - 1], counts[0, H - 1, G - 1] = 1055, 4129         # the ragged last group
    shared = inds[:, :, :1].expand(1, H, G, nk).contiguous()
    pos = torch.empty(1, H, nk, dtype=torch.long)
    for h in range(H):
        pos[0, h, shared[0, h, 0].long()] = torch.arange(nk)
    v_pos = torch.nn.functional.one_hot((pos // 32) % 128, 128).to(torch.bfloat16)
    return dict(q=q, k=k, v=v, inds=inds, counts=counts, shared=shared, v_pos=v_pos)


STRADDLE_PATTERNS = {"all rows at 0.9": (0.9, None), "all rows at 0.99": (0.99, None), "all rows at 1.01": (1.01, None),
                     "all rows at 1.1": (1.1, None), "one row per other wave at 1.1, the rest at 0.9": (0.9, 1.1)}


def straddle_inputs(align, pattern, threshold, mult, period, nq, nk, seed, planted=False):
    """q, k, v bf16 ``[1, 2, n, 128]`` with |q_i| set so that mult * |q_i| * max_j |k_j| * c = f_i * threshold, f from the pattern
    (row 5 of every `period` rows gets the second value); the bound is evaluated in fp64 on the bf16 inputs and returned
    per row in units of the threshold.
    align: "random"; "along": every query close to the direction of the largest-norm key (scores at the top of the proven
    range); "against": all keys share a direction and the queries point the other way (scores near -M: the exponentials at
    the bottom of the range).  planted: key 0 gets 1.5 x the largest norm (the caller keeps it out of the index lists)."""
    H = 2
    g = torch.Generator().manual_seed(seed)
    q, k, v = [torch.randn(1, H, n, 128, generator=g) for n in (nq, nk, nk)]
    u = torch.randn(H, 1, 128, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    if align == "against":
        k = 0.5 * k + 128 ** 0.5 * u
    if planted:
        k[0, :, 0] *= 1.5 * k.norm(dim=-1).max() / k[0, :, 0].norm(dim=-1, keepdim=True)
    k = k.to(torch.bfloat16)
    kmax, jmax = k.double().norm(dim=-1).max(-1)                    # [1, H]
    if align == "along":
        d = torch.stack([k[0, h, jmax[0, h]].float() / float(kmax[0, h]) for h in range(H)])[:, None]
        q = d + 0.02 * q
    elif align == "against":
        q = -u + 0.02 * q
    f_lo, f_hi = STRADDLE_PATTERNS[pattern]
    f = torch.full((nq,), f_lo, dtype=torch.float64)
    if f_hi is not None:
        f[5::period] = f_hi
    target = f[None, None, :] * threshold / (mult * kmax[..., None] * SCALE_LOG2E)
    q = (q.double() / q.double().norm(dim=-1, keepdim=True) * target[..., None]).to(torch.bfloat16)
    bound = mult * q.double().norm(dim=-1) * kmax[..., None] * SCALE_LOG2E / threshold
    assert ((bound - f).abs() < 2e-3).all()
    return q, k, v.to(torch.bfloat16), bound


# --------------------------------------------------------------------------- sparse-MLP kernels: exact references + segment metric
# The GEMM1 operators write packed deltas act(h) - cache, the GEMM2 operators add packed x fc2^T[kept] to a base.  Both shrink
# with the regime (a cache that holds the previous step's activations leaves deltas a tenth of the activations), so an
# absolute tolerance sees no 1 % defect there.  The error is taken per row and per SEGMENT of W columns against plain fp64:
# docs/TEST_SENSITIVITY.md, "Sparse MLP kernels".
#
# ORACLE_MLP_SEG_ERR: the largest segment error of the CPU references (the oracle where it has the operator, the plain-torch
# mirrors elsewhere) against the exact references below over the case list of tests/test_mlp_metric_cpu.py, derived terms
# taken off, rounded up to two digits; that file pins it.
# MLP_SEG_MARGIN: what a correct kernel may do differently (summation order, MFMA accumulation, hardware exp / tanh).
# tests/test_mlp_metric_cpu.py caps margin * floor at half the weakest counted mutant's error.
MLP_BM = 128                  # token rows that share one index list
MLP_SEG_W1 = 64               # GEMM1's packed deltas and cache columns: the kernel's column sub-tile
MLP_SEG_W2 = 256              # GEMM2's output: GEMM2_BN
ORACLE_MLP_SEG_ERR = 0.0035
MLP_SEG_MARGIN = 2.0
MLP_SEG_BOUND = MLP_SEG_MARGIN * ORACLE_MLP_SEG_ERR
MLP_ACTS = ("gelu_tanh", "silu", "gelu")
MLP_COUNTS = {333: [512, 208, 40], 1000: [512, 0, 208, 16, 40, 512, 64, 272]}      # M -> kept columns per 128-row group
F8 = torch.float8_e4m3fn


def _segments(t, width):
    pad = (-t.shape[-1]) % width
    return torch.nn.functional.pad(t, (0, pad)).unflatten(-1, (-1, width))


def seg_rel_err(got, exact, width, cols=None):
    """Per row i and segment s of `width` columns ``||got[i, seg] - exact[i, seg]||_2 / ||exact[i, seg]||_2`` in fp64:
    ``[..., rows, n] -> [..., rows, ceil(n / width)]``, the last segment short.  cols ``[..., rows]``: the row's live column
    count (its group's kept columns); the columns at or past it are no part of the result and of no segment.  As `row_rel_err`:
    a NaN / Inf in a live ``got`` element is an infinite error, a segment whose exact value is 0 (a group without kept
    columns, a segment past the count) has error 0 if reproduced exactly, else infinite."""
    exact = exact.double()
    got = got.to(exact.device).double()
    if cols is not None:
        live = torch.arange(exact.shape[-1], device=exact.device) < cols.to(exact.device)[..., None]
        got, exact = torch.where(live, got, torch.zeros_like(got)), torch.where(live, exact, torch.zeros_like(exact))
    g, x = _segments(got, width), _segments(exact, width)
    num, den = (g - x).norm(dim=-1), x.norm(dim=-1)
    err = num / den
    err = torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))), err)
    return torch.where(torch.isfinite(g).all(dim=-1) & ~torch.isnan(err), err, torch.full_like(err, float("inf")))


def seg_term(result, exact, width, cols=None):
    """``2^-8 ||result[i, seg]|| / ||exact[i, seg]||``, the shape of `seg_rel_err`: what one more bf16 rounding of a stored
    ``result`` (8 significant bits: element e moves by at most 2^-8 |result_e|) can add to the segment error against
    ``exact``; 0 where the segment's exact value is 0."""
    exact = exact.double()
    result = torch.nan_to_num(result.to(exact.device).double(), nan=0.0, posinf=0.0, neginf=0.0)
    if cols is not None:
        live = torch.arange(exact.shape[-1], device=exact.device) < cols.to(exact.device)[..., None]
        result, exact = torch.where(live, result, torch.zeros_like(result)), torch.where(live, exact, torch.zeros_like(exact))
    num, den = _segments(result, width).norm(dim=-1), _segments(exact, width).norm(dim=-1)
    return torch.where(den > 0, BF16_EPS * num / den, torch.zeros_like(den))


def refreshed_cache_term(result, fresh, delta, bound, width, cols=None, act_rounded=False):
    """The per-segment allowance, beyond `bound`, of a cache column refreshed as ``bf16(cache + delta^)`` and held against the
    fresh fp64 activation: the packed delta is within ``bound ||delta_seg||`` of exact (asserted on its own), the stored sum is
    rounded once more (2^-8 ||result_seg||, `assert_delta_rows_close`'s term), and a route that rounds the activation to bf16
    before it subtracts (ungated fp8, `act_rounded`) adds 2^-8 ||fresh_seg||.  Relative to ||fresh_seg||:
    ``error <= bound rho + 2^-8 ||result_seg|| / ||fresh_seg|| (+ 2^-8)`` with ``rho = ||delta_seg|| / ||fresh_seg||``; returned is that
    minus `bound`.  With the previous step's activations in the cache rho is 0.1 - 0.2 and the allowance is the one rounding of
    the stored sum: a refreshed column is one rounding from fresh.  With a random cache rho is 1.4 - 4."""
    rho = seg_term(delta, fresh, width, cols) / BF16_EPS
    term = bound * (rho - 1.0) + seg_term(result, fresh, width, cols) + (BF16_EPS if act_rounded else 0.0)
    return torch.where(rho > 0, term, torch.zeros_like(term))          # (no allowance where nothing is refreshed: those segments are exact)


def assert_segs_close(got, exact, bound, what, extra=None, width=MLP_SEG_W1, cols=None):
    """Every segment of every row of ``got`` ``[rows, n]`` (or ``[B, rows, n]``) within `bound` of ``exact`` (see `seg_rel_err`;
    rows in groups of 128); ``extra``, the shape of the error, widens the bound per segment by a derived term.  Returns the
    worst ``error - extra``."""
    assert got.shape == exact.shape, (got.shape, exact.shape)
    err = seg_rel_err(got, exact, width, cols)
    if extra is not None:
        err = err - extra.to(err.device)
    worst = float(err.max()) if err.numel() else 0.0
    bad = ~(err <= bound)
    shown = err[(err != 0) | bad]          # (the record: segments with a result; those of empty groups and past the counts are exact or bad)
    _record_row_err(what, float(shown.max()) if shown.numel() else worst, bound)
    if bad.any():
        flat = int(torch.nan_to_num(err, nan=float("inf")).argmax())
        R, S = err.shape[-2], err.shape[-1]
        b, r, s = flat // (R * S), (flat // S) % R, flat % S
        live = got.to(exact.device) if cols is None else got.to(exact.device)[torch.arange(exact.shape[-1], device=exact.device) < cols.to(exact.device)[..., None]]
        raise AssertionError(
            f"{what}: segment error {worst:.4g} > {bound:.4g} at batch {b} group {r // MLP_BM} row {r} (row {r % MLP_BM} of its "
            f"group) segment {s} (columns {s * width} to {min(exact.shape[-1], (s + 1) * width) - 1}); {int(bad.sum())} / "
            f"{bad.numel()} segments over the bound, {int((~torch.isfinite(live.float())).sum())} non-finite elements")
    return worst


def assert_rowwise_close(got, exact, bound, what, width=None, copy_of=None):
    """The four assertions of every row-wise norm case (docs/TEST_SENSITIVITY.md, "Row-wise norm kernels"; tests/rowwise_model.py has the
    bounds): ``got`` is finite; where ``copy_of`` is given it is that tensor bit for bit; every segment whose exact value is all zero
    (an all-zero input row of an RMSNorm part) is exactly zero; every segment is within `bound` -- a number, or a tensor of the
    error's shape: the class of each segment -- of ``exact``.  A segment is a row of the last dimension (``[B, H, n, 128]``:
    `row_rel_err`) or, with `width`, that many consecutive columns of it (``xm [rows, C]``: `seg_rel_err`, the last segment short).  No
    segment is left out.  Appends ``rowwise <what> <tab> worst <tab> its bound <tab> worst error / bound`` to CHIPMUNK_ROW_ERR_LOG.
    Returns the worst error."""
    assert got.shape == exact.shape, (got.shape, exact.shape)
    g = got.to(exact.device)
    nonfinite = int((~torch.isfinite(g.float())).sum())
    assert nonfinite == 0, f"{what}: {nonfinite} non-finite elements of {g.numel()}"
    if copy_of is not None:
        c = copy_of.to(exact.device)
        assert g.dtype == c.dtype and torch.equal(g.view(torch.int16), c.view(torch.int16)), f"{what}: a copied part must be a bit copy"
    w = exact.shape[-1] if width is None else width
    zero = _segments(exact.double(), w).abs().amax(-1) == 0
    dirty = (_segments(g.double(), w) != 0).any(-1) & zero
    assert not dirty.any(), f"{what}: {int(dirty.sum())} of {int(zero.sum())} segments whose exact value is 0 are not exactly zero"
    err = seg_rel_err(g, exact, w)
    if width is None:
        err = err[..., 0]
    b = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    flat = int(torch.nan_to_num(ratio, nan=float("inf")).argmax()) if err.numel() else 0
    worst, at, share = (float(err.max()), float(b.flatten()[flat]), float(ratio.flatten()[flat])) if err.numel() else (0.0, 0.0, 0.0)
    import os
    path = os.environ.get("CHIPMUNK_ROW_ERR_LOG")
    print(f"rowwise {what}: worst segment {worst:.5f}, {share:.2f} of its bound")
    if path:
        with open(path, "a") as f:
            f.write(f"rowwise {what}\t{worst:.6f}\t{at:.6f}\t{share:.4f}\n")
    bad = ~(ratio <= 1.0)
    if bad.any():
        idx = []
        for s in reversed(err.shape):
            idx.append(flat % s)
            flat //= s
        raise AssertionError(f"{what}: segment error {float(err[tuple(reversed(idx))]):.4g} > {at:.4g} at index {tuple(reversed(idx))} of {tuple(err.shape)} "
                             f"(segments of {w} columns); {int(bad.sum())} / {bad.numel()} segments over the bound")
    return worst


def mlp_act64(act, x):
    """the activations of DESIGN "Gated MLPs" in the precision of ``x``"""
    if act == "gelu_tanh":
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    if act == "silu":
        return x * torch.sigmoid(x)
    assert act == "gelu", act
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def mlp_group_cols(counts, M):
    """[M] long: the kept-column count of every token row's 128-row group"""
    return counts.long().repeat_interleave(MLP_BM)[:M]


def mm1_exact(a, w, bias, cache, inds, counts, act="gelu_tanh", w_up=None, bias_up=None, scales=None, pre_mul=1.0):
    """GEMM1 by its definition (ops/mlp.py, DESIGN "Gated MLPs"), fp64, plain torch on the inputs' device: per 128-row group g
    and packed column j < counts[g], with col = inds[g, j],
    ``fresh[m, j] = act(a[m] . w[col] * s + bias[col]) (* (a[m] . w_up[col] * s_up + bias_up[col]))`` and
    ``delta[m, j] = fresh[m, j] - cache[col, m]``.  a ``[M, K]``, w / w_up ``[F, K]``, bias / bias_up ``[F]`` or None, cache
    ``[F, M]``.  e4m3 operands are widened exactly; scales = (scale_a, scale_b[, scale_b_up]), the RECIPROCAL quantisation
    scales as the fp32 numbers the operator receives.  pre_mul multiplies the (gate's) pre-activation: a defect of
    tests/test_mlp_metric_cpu.py.  Returns (delta, fresh) ``[M, F]`` in the packed layout, 0 at and past the counts."""
    M, F = a.shape[0], w.shape[0]
    s = [1.0, 1.0]
    if scales is not None:
        ra = float(scales[0].double())
        s = [ra * float(scales[1].double()), ra * float(scales[2 if len(scales) > 2 else 1].double())]
    delta = torch.zeros(M, F, dtype=torch.float64, device=a.device)
    fresh = torch.zeros_like(delta)
    ad, wd, ud = a.double(), w.double(), None if w_up is None else w_up.double()      # (e4m3 -> fp64 is exact)
    for g in range(inds.shape[0]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(counts[g])
        if n == 0:
            continue
        col = inds[g, :n].long()
        h = (ad[rows] @ wd[col].T) * s[0]
        if bias is not None:
            h = h + bias[col].double()
        f = mlp_act64(act, h * pre_mul)
        if w_up is not None:
            u = (ad[rows] @ ud[col].T) * s[1]
            f = f * (u if bias_up is None else u + bias_up[col].double())
        fresh[rows, :n] = f
        delta[rows, :n] = f - cache[col][:, rows].double().T
    return delta, fresh


def mm2_exact(packed, w2T, inds, counts, scale=None):
    """GEMM2's product by its definition, fp64: ``prod[m] = sum_{j < counts[g]} packed[m, j] * w2T[inds[g, j]]`` (``* scale``, the
    reciprocal quantisation scale of an e4m3 ``w2T`` as the fp32 number the operator receives); the packed columns at and past
    the counts are not read.  ``[M, N2]``, 0 for the rows of a group without kept columns."""
    M = packed.shape[0]
    out = torch.zeros(M, w2T.shape[1], dtype=torch.float64, device=packed.device)
    wd = w2T.double()                                                                 # (e4m3 -> fp64 is exact)
    for g in range(inds.shape[0]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(counts[g])
        if n:
            out[rows] = packed[rows, :n].double() @ wd[inds[g, :n].long()]
    return out if scale is None else out * float(scale.double())


def gathered_cache(cache, inds, counts):
    """the cache ``[F, M]`` in the packed layout of the deltas: ``[M, F]`` with ``[m, j] = cache[inds[g, j], m]``, 0 at and past the counts"""
    F, M = cache.shape
    out = torch.zeros(M, F, dtype=cache.dtype, device=cache.device)
    for g in range(inds.shape[0]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(counts[g])
        out[rows, :n] = cache[inds[g, :n].long()][:, rows].T
    return out


def quantize_e4m3(t):
    """(e4m3 tensor, reciprocal scale [1] fp32) with scale = 448 / amax: no power of two on random data"""
    s = 448.0 / t.abs().max()
    return (t * s).clamp(-448.0, 448.0).to(F8), (1.0 / s).reshape(1).float()


# --------------------------------------------------------------------------- inputs shared by test_gpu_mlp_accuracy.py and the CPU
# test that measures the references on them (tests/test_mlp_metric_cpu.py); all CPU tensors, at the data scales of the
# existing MLP tests: a 0.5, weights 0.06, biases 0.1


def mlp_problem(M, K, F, seed, regime="random", act="gelu_tanh", fp8=False, gated=False, biases=True, counts=None):
    """One GEMM1 problem.  regime "random": the cache is 0.3 randn.  "previous step": the cache holds bf16 of the activations
    of x0 and the operator sees x = x0 + 0.05 randn, the regime the method runs in (deltas small against the activations).
    fp8: a / w / wu are e4m3 with reciprocal scales ra / rb / rbu (the up weight is twice the gate's size, so the two weight
    scales differ by about 2 x); x0 is quantised with x's scale."""
    counts = MLP_COUNTS[M] if counts is None else counts
    G = (M + MLP_BM - 1) // MLP_BM
    assert len(counts) == G
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape, scale: torch.randn(*shape, generator=g) * scale      # noqa: E731
    x0, w, wu = rnd(M, K, scale=0.5), rnd(F, K, scale=0.06), rnd(F, K, scale=0.12 if fp8 else 0.06)
    bias, bu = rnd(F, scale=0.1).to(torch.bfloat16), rnd(F, scale=0.1).to(torch.bfloat16)
    cache = rnd(F, M, scale=0.3).to(torch.bfloat16)
    inds = torch.stack([torch.randperm(F, generator=g) for _ in range(G)]).to(torch.int32)
    step = rnd(M, K, scale=0.05)
    p = dict(M=M, K=K, F=F, G=G, counts=list(counts), regime=regime, act=act, fp8=fp8, gated=gated, inds=inds,
             cnt=torch.tensor(counts, dtype=torch.int32), bias=bias if biases else None, bu=bu if biases and gated else None)
    x = x0 if regime == "random" else x0.to(torch.bfloat16).float() + step
    if fp8:
        p["a"], p["ra"] = quantize_e4m3(x)
        a0 = (x0 / p["ra"]).clamp(-448.0, 448.0).to(F8)
        p["w"], p["rb"] = quantize_e4m3(w)
        p["wu"], p["rbu"] = quantize_e4m3(wu)
        if not gated:
            del p["wu"], p["rbu"]
    else:
        p["a"], a0, p["w"] = x.to(torch.bfloat16), x0.to(torch.bfloat16), w.to(torch.bfloat16)
        if gated:
            p["wu"] = wu.to(torch.bfloat16)
    if regime != "random":
        assert regime == "previous step", regime
        every = torch.arange(F, dtype=torch.int32).expand(G, F)
        fresh0 = mm1_exact(a0, p["w"], p["bias"], torch.zeros(F, M), every, [F] * G, **mlp_exact_args(p))[1]
        cache = fresh0.T.to(torch.bfloat16).contiguous()
    p["cache0"] = cache
    return p


def mlp_exact_args(p):
    """the keyword arguments of `mm1_exact` that state the operator of problem `p`"""
    kw = dict(act=p["act"])
    if p["gated"]:
        kw.update(w_up=p["wu"], bias_up=p["bu"])
    if p["fp8"]:
        kw["scales"] = (p["ra"], p["rb"], p["rbu"]) if p["gated"] else (p["ra"], p["rb"])
    return kw


def mlp2_problem(M, F, N2, seed, counts=None):
    """One GEMM2 problem: packed ``[M, F]`` 0.2 randn with NaN at and past each group's count, w2T ``[F, N2]`` 0.05 randn (bf16,
    and as e4m3 `w8` with its reciprocal scale `r8`), one index permutation per group."""
    counts = MLP_COUNTS[M] if counts is None else counts
    G = (M + MLP_BM - 1) // MLP_BM
    g = torch.Generator().manual_seed(seed)
    packed = (torch.randn(M, F, generator=g) * 0.2).to(torch.bfloat16)
    w = torch.randn(F, N2, generator=g) * 0.05
    inds = torch.stack([torch.randperm(F, generator=g) for _ in range(G)]).to(torch.int32)
    for gi, n in enumerate(counts):
        packed[gi * MLP_BM:(gi + 1) * MLP_BM, n:] = float("nan")
    w8, r8 = quantize_e4m3(w)
    return dict(M=M, F=F, N2=N2, G=G, counts=list(counts), packed=packed, w2T=w.to(torch.bfloat16), w8=w8, r8=r8, inds=inds,
                cnt=torch.tensor(counts, dtype=torch.int32), seed=seed)


def mlp1_cases():
    """name -> `mlp_problem` arguments: the GEMM1 case list of both MLP accuracy files.  M = 333 (three groups, the last of 77 rows)
    and 1000 (eight groups, one empty); K = 320 / 256 for bf16 operands (five / four 64-wide k steps), 384 for e4m3 (three 128-wide
    steps); every operator in both cache regimes; the gated operators with the three activations and, at M = 333, without biases."""
    out = {}
    for M in (333, 1000):
        for regime in ("random", "previous step"):
            for kind in ("bf16", "fp8", "glu", "glu fp8"):
                fp8, gated = "fp8" in kind, "glu" in kind
                K = 384 if fp8 else 320 if M == 333 else 256
                for act in (MLP_ACTS if gated else ("gelu_tanh",)):
                    for biases in ((True, False) if gated and M == 333 else (True,)):
                        name = f"{kind} {act}{'' if biases else ' no bias'} M{M} K{K}, {regime} cache"
                        out[name] = dict(M=M, K=K, F=512, seed=100 + len(out), regime=regime, act=act, fp8=fp8, gated=gated, biases=biases)
    return out


def mlp2_cases():
    """name -> `mlp2_problem` arguments: N2 = 384 (one full and one half 256-column tile) and 512 (two full tiles)"""
    return {f"M{M} N{N2}": dict(M=M, F=512, N2=N2, seed=300 + M + N2) for M in (333, 1000) for N2 in (384, 512)}


def mlp2_base(p, kind, exact):
    """the tensor GEMM2 accumulates into: "zero", "product" (randn of the exact product's rms: the accumulate term stays below
    the bound) or "unit" (randn: shows that the base survives and the product is added once, and little else)"""
    g = torch.Generator().manual_seed(p["seed"] + 7)
    scale = {"zero": 0.0, "product": float(exact.pow(2).mean().sqrt()), "unit": 1.0}[kind]
    return (torch.randn(p["M"], p["N2"], generator=g) * scale).to(torch.bfloat16)


# --------------------------------------------------------------------------- column sums: exact reference + element metric
# cs[b, h, g, j] = sum_{i in group g} exp(s_ij) p_i is a sum of positive terms: no cancellation, so EVERY element carries a small
# relative error, and the number of bf16 roundings on its path can be read from the source.  A column sum over n keys is about
# 192 / n, so the absolute tolerance the suite used (2e-3 + 3e-2 |x|) is 7 % of the signal at 4 160 keys and larger than it at the
# HunyuanVideo size.  The guard is the relative error per element against plain fp64 (docs/TEST_SENSITIVITY.md, "Column sums";
# the bound's numbers live in tests/colsum_model.py and are pinned by tests/test_colsum_metric_cpu.py).
COLSUM_SEG_W = 64             # the segment metric's width: the 64-row kernels' key tile


def colsum_exact(q, k, p, k_lens=None, scale_mul=1.0, chunk_bytes=1 << 28):
    """fp64 ``cs[b, h, g, j] = sum_{i in group g} exp(q_i . k_j / sqrt(D)) p_i`` with plain torch on the operands' device:
    ``[B, H, ceil(Nq / 192), Nk]`` float64.  p ``[B, H, >= Nq, 1]`` or ``[B, H, >= Nq]`` (the padded ``l`` of a previous call is
    taken up to ``Nq``).  Group rows past ``Nq`` add nothing; columns at and past ``k_lens[b]`` are 0.  scale_mul multiplies the
    ``1 / sqrt(D)`` scale (a defect of tests/test_colsum_metric_cpu.py, and the rest of a scale that was folded into q)."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    G = (Nq + GROUP_ROWS - 1) // GROUP_ROWS
    scale = scale_mul / (D ** 0.5)
    pd = p.to(q.device).double().reshape(B, H, -1)[..., :Nq]
    out = torch.zeros(B, H, G, Nk, dtype=torch.float64, device=q.device)
    rows_per = max(1, chunk_bytes // (8 * Nk * GROUP_ROWS)) * GROUP_ROWS
    for b in range(B):
        L = Nk if k_lens is None else max(1, min(Nk, int(k_lens[b])))
        for h in range(H):
            kd = k[b, h, :L].double()
            for a in range(0, Nq, rows_per):
                e = min(Nq, a + rows_per)
                w = torch.exp((q[b, h, a:e].double() @ kd.T) * scale) * pd[b, h, a:e, None]
                g0, ng = a // GROUP_ROWS, (e - a + GROUP_ROWS - 1) // GROUP_ROWS
                w = torch.nn.functional.pad(w, (0, 0, 0, ng * GROUP_ROWS - (e - a)))
                out[b, h, g0:g0 + ng, :L] = w.view(ng, GROUP_ROWS, L).sum(1)
    return out


def colsum_elem_err(cs, exact):
    """Per element ``|cs - x| / max(x, 2^-60 max_j x[g, :])`` in fp64, the shape of ``exact``.  A non-finite result is an infinite
    error.  The clamp only gives a definition to a column whose exact sum is (nearly) 0 -- a spike pattern, a column past
    ``k_lens`` (where a value of the signal's size is then an error of 2^60; the tests assert an exact 0 there on their own); on
    `randn` inputs no element is clamped."""
    x = exact.double()
    c = cs.to(x.device).double()
    den = torch.maximum(x, 2.0 ** -60 * x.max(dim=-1, keepdim=True).values)
    err = (c - x).abs() / den
    err = torch.where(den == 0, torch.where(c == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))), err)
    return torch.where(torch.isfinite(c) & ~torch.isnan(err), err, torch.full_like(err, float("inf")))


def colsum_seg_err(cs, exact, width=COLSUM_SEG_W):
    """Per (group, `width`-key tile) ``||cs[g, seg] - x[g, seg]||_2 / ||x[g, seg]||_2`` (`seg_rel_err` with the groups as rows):
    ``[B, H, G, ceil(Nk / width)]``."""
    return seg_rel_err(cs, exact, width)


def assert_colsums_close(cs, exact, rounds, extra=None, what="", fp32_term=0.0, seg_bound=None):
    """Every element of ``cs`` ``[B, H, G, Nk]`` within ``rounds[g] * 2^-8 + fp32_term + extra`` (relative, `colsum_elem_err`) of
    ``exact``.  rounds: per group the bf16 roundings on the element's path (a list / tensor ``[G]``, or one number); extra: a
    derived term of one route (a number or broadcastable to ``exact``); seg_bound (per group like rounds, or a number): also hold
    the segment metric `colsum_seg_err` under it.  Appends ``what <tab> worst element <tab> bound <tab> worst segment`` to
    CHIPMUNK_ROW_ERR_LOG as `assert_rows_close` does.  Returns (worst element error / its bound, worst segment error)."""
    assert cs.shape == exact.shape, (cs.shape, exact.shape)
    dev = exact.device
    G = exact.shape[2]
    per_group = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev).expand(G).view(1, 1, G, 1)      # noqa: E731
    bound = per_group(rounds) * BF16_EPS + fp32_term
    if extra is not None:
        bound = bound + torch.as_tensor(extra, dtype=torch.float64, device=dev)
    err = colsum_elem_err(cs, exact)
    ratio = err / bound
    worst, worst_ratio = (float(err.max()), float(ratio.max())) if err.numel() else (0.0, 0.0)
    seg = colsum_seg_err(cs, exact)
    worst_seg = float(seg.max()) if seg.numel() else 0.0
    import os
    path = os.environ.get("CHIPMUNK_ROW_ERR_LOG")
    print(f"column sums {what}: worst element {worst:.5f} ({worst_ratio:.2f} of its bound), worst segment {worst_seg:.5f}")
    if path:
        with open(path, "a") as f:
            f.write(f"colsum {what}\t{worst:.6f}\t{float(bound.max()):.6f}\t{worst_seg:.6f}\t{worst_ratio:.4f}\n")
    bad = ~(ratio <= 1.0)
    if bad.any():
        flat = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        Nk = exact.shape[3]
        b, h, g, j = flat // (exact.shape[1] * G * Nk), (flat // (G * Nk)) % exact.shape[1], (flat // Nk) % G, flat % Nk
        raise AssertionError(
            f"{what}: column-sum element error {float(err[b, h, g, j]):.4g} > {float(bound.expand_as(err)[b, h, g, j]):.4g} at batch {b} "
            f"head {h} group {g} column {j} (column {j % COLSUM_SEG_W} of key tile {j // COLSUM_SEG_W}): got {float(cs[b, h, g, j]):.6g}, exact "
            f"{float(exact[b, h, g, j]):.6g}; {int(bad.sum())} / {bad.numel()} elements over the bound, "
            f"{int((~torch.isfinite(cs.float())).sum())} non-finite")
    if seg_bound is not None:
        sb = per_group(seg_bound)
        sbad = ~(seg <= sb)
        if sbad.any():
            flat = int(torch.nan_to_num(seg / sb, nan=float("inf")).argmax())
            S = seg.shape[3]
            b, h, g, s = flat // (seg.shape[1] * G * S), (flat // (G * S)) % seg.shape[1], (flat // S) % G, flat % S
            raise AssertionError(f"{what}: column-sum segment error {float(seg[b, h, g, s]):.4g} > {float(sb.expand_as(seg)[b, h, g, s]):.4g} at "
                                 f"batch {b} head {h} group {g} key tile {s}; {int(sbad.sum())} / {sbad.numel()} segments over the bound")
    return worst_ratio, worst_seg
