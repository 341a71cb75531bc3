"""Per-sequence key lengths (``k_lens``) on the GPU, operator by operator: for sequence ``b`` the keys ``j >= k_lens[b]``
do not exist -- ``o``, ``l`` and the column sums are those of K / V cropped to ``k_lens[b]`` rows, the column sums and the mask are 0
past them, and no K / V row past them is read (the padding holds NaN in those cases).

References are computed here, once per (shape, lengths), in fp64: ``helpers.attn_exact(keep=)`` for the general kernel,
``helpers.attn_exact_dense64`` on the cropped K / V for the 64-row kernels (it adds the term of their fixed reference point, whose
``max |k|`` runs over the valid rows), ``l = 1 / sum_j exp(s_ij)`` and ``cs[g, j] = sum_{i in group g} exp(s_ij) p_i`` over the valid
keys.  Bounds are the project's: ``ROW_ERR_BOUND`` per row of ``o``, ``l`` at rtol 1e-3, ``cs`` at rtol 3e-2 + atol 2e-3.

The 64-row kernels fetch rows 0..63 of a sequence shorter than one 64-key tile (include/chipmunk_hip.h: the first 64 rows of K and V
must be finite), so the sub-tile lengths of case 2 run with finite padding; every other case also runs with NaN padding."""
import functools
import math

import pytest
import torch

from helpers import assert_rows_close, attn_exact, attn_exact_dense64, colsum_exact, randn_bf16

pytestmark = pytest.mark.gpu

B, H, D = 3, 2, 128
GENERAL = {"n": 416, "opts": {"attn_dense64": 2, "attn_colsum64": 2}, "lens": ([416, 33, 1], [32, 97, 415])}
WAVE64 = {"n": 448, "opts": {"attn_dense64": 1, "attn_colsum64": 1}, "lens": ([448, 65, 64], [129, 63, 1])}


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class forced:
    """library options for the length of a with-block (routes are a host decision on Nk: the tests force them)"""

    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from chipmunk_amd import _native
        for k, v in self.opts.items():
            _native.set_option(k, v)

    def __exit__(self, *exc):
        from chipmunk_amd import _native
        for k in self.opts:
            _native.set_option(k, 0)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    return tuple(randn_bf16(B, H, n, D, seed=n + s) for s in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def _reference(n, lens, dense64):
    """(exact o -- what assert_rows_close takes --, l [B,H,n,1] fp32, cs [B,H,G,n] fp32 with zeros past the lengths), on the GPU"""
    dev = torch.device("cuda:0")
    q, k, v = [t.to(dev) for t in _inputs(n)]
    G = math.ceil(n / 192)
    if dense64:
        parts = [attn_exact_dense64(q[b:b + 1], k[b:b + 1, :, :L].contiguous(), v[b:b + 1, :, :L].contiguous()) for b, L in enumerate(lens)]
        exact = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    else:
        keep = torch.arange(n, device=dev)[None, None, :] < torch.tensor(lens, device=dev)[:, None, None]
        exact = attn_exact(q, k, v, keep=keep)
    l = torch.zeros(B, H, n, 1, dtype=torch.float64, device=dev)
    for b, L in enumerate(lens):
        e = torch.exp((q[b].double() @ k[b, :, :L].double().transpose(-1, -2)) / math.sqrt(D))      # [H, n, L]
        l[b] = 1.0 / e.sum(-1, keepdim=True)
    cs = colsum_exact(q, k, l, lens)
    assert cs.shape == (B, H, G, n)
    return exact, l.float(), cs.float()


def _operands(dev, n, lens, nan_padding):
    q, k, v = [t.to(dev) for t in _inputs(n)]
    if nan_padding:
        k, v = k.clone(), v.clone()
        for b, L in enumerate(lens):
            k[b, :, L:] = float("nan")
            v[b, :, L:] = float("nan")
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=dev)


def _check(o, l, cs, ref, lens, what):
    exact, l_ref, cs_ref = ref
    n = o.shape[2]
    assert torch.isfinite(o.float()).all() and torch.isfinite(l).all(), f"{what}: non-finite o / l"
    assert_rows_close(o, exact, what=what)
    torch.testing.assert_close(l[..., :n, :], l_ref, rtol=1e-3, atol=0)
    assert float(l[..., n:, :].abs().sum()) == 0
    if cs is not None:
        assert cs.shape == cs_ref.shape and cs.dtype == torch.bfloat16
        assert torch.isfinite(cs.float()).all(), f"{what}: non-finite column sums"
        for b, L in enumerate(lens):
            assert not cs[b, :, :, L:].float().any(), f"{what}: column sums past k_lens[{b}] = {L} are not exactly 0"
        print(f"{what}: cs worst abs diff {float((cs.float() - cs_ref).abs().max()):.4g}")
        torch.testing.assert_close(cs.float(), cs_ref, rtol=3e-2, atol=2e-3)


def _run_case(dev, case, lens, nan_padding, token_major, fused_colsum=0):
    from chipmunk_amd import ops
    n = case["n"]
    dense64 = case["opts"]["attn_dense64"] == 1
    ref = _reference(n, tuple(lens), dense64)
    q, k, v, kl = _operands(dev, n, lens, nan_padding)
    with forced(attn_fused_colsum=fused_colsum, **case["opts"]):
        o, l = ops.dense_attn(q, k, v, token_major, kl)
        o2, cs, l2 = ops.dense_colsum_attn(q, k, v, ref[1].to(dev), token_major, kl)
        torch.cuda.synchronize()
    tag = f"k_lens {lens}, n {n}, dense64 {dense64}, fused_colsum {fused_colsum}, nan {nan_padding}, token-major {token_major}"
    if token_major:
        assert o.stride(1) == D and o2.stride(1) == D          # the [B, H, N, D] view of [B, N, H, D] storage
    _check(o, l, None, ref, lens, "dense_attn, " + tag)
    _check(o2, l2, cs, ref, lens, "dense_colsum_attn, " + tag)


# ---- 1: the general kernel (13 tiles of 32 keys, a ragged last 192-row group): one tile, tile +- 1, a single key, full ----
@pytest.mark.parametrize("token_major", [False, True])
@pytest.mark.parametrize("nan_padding", [False, True])     # 3: no padding row is read, at any length
@pytest.mark.parametrize("lens", GENERAL["lens"])
def test_general_kernel(dev, lens, nan_padding, token_major):
    _run_case(dev, GENERAL, lens, nan_padding, token_major)


# ---- 2: the 64-row kernels; fused_colsum 0 = column sums inside the dense kernel, 2 = two passes, 3 = weighted sums ----
@pytest.mark.parametrize("fused_colsum", [0, 2, 3])
@pytest.mark.parametrize("lens,nan_padding", [(WAVE64["lens"][0], False), (WAVE64["lens"][0], True),    # 3: lengths >= 64: NaN padding
                                              (WAVE64["lens"][1], False)])                             # sub-tile lengths: finite padding
def test_wave64_kernels(dev, lens, nan_padding, fused_colsum):
    _run_case(dev, WAVE64, lens, nan_padding, False, fused_colsum)


def test_wave64_kernels_token_major(dev):
    _run_case(dev, WAVE64, WAVE64["lens"][0], True, True)


# ---- 4: k_lens = [Nk] * B is the call without it, bit for bit ----
@pytest.mark.parametrize("case,fused_colsum", [(GENERAL, 0), (WAVE64, 0), (WAVE64, 2), (WAVE64, 3)], ids=["general", "fused", "two_pass", "weighted"])
def test_full_lengths_are_the_plain_operators(dev, case, fused_colsum):
    from chipmunk_amd import ops
    n = case["n"]
    q, k, v, kl = _operands(dev, n, [n] * B, False)
    G = math.ceil(n / 192)
    gen = torch.Generator().manual_seed(11)
    static = (torch.rand(1, H, G, n, generator=gen) < 0.02).to(dev)
    groups = (torch.rand(1, H, G, 1, generator=gen) < 0.8).to(dev)
    with forced(attn_fused_colsum=fused_colsum, **case["opts"]):
        o0, l0 = ops.dense_attn(q, k, v)
        o1, l1 = ops.dense_attn(q, k, v, False, kl)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
        a = ops.dense_colsum_attn(q, k, v, l0)
        b = ops.dense_colsum_attn(q, k, v, l0, False, kl)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        for mass in (False, True):
            outs = []
            for lengths in (None, kl):
                ops.manual_seed(5)          # the random part draws one salt per launch
                if mass:
                    outs.append(ops.dense_colsum_topk_mask_p(q, k, v, l0, 96, 0.9, 8, 0.01, groups, static, False, lengths))
                else:
                    outs.append(ops.dense_colsum_topk_mask(q, k, v, l0, 96, 0.01, groups, static, False, lengths))
            for x, y in zip(*outs):
                assert torch.equal(x, y)
        cs = a[1][..., :G, :n].contiguous()
        for stream in (0, 1):
            with forced(topk_mask_stream=stream):
                ops.manual_seed(6)
                m0 = ops.topk_mask(cs, 96, 0.01, groups, static)
                ops.manual_seed(6)
                m1 = ops.topk_mask(cs, 96, 0.01, groups, static, kl)
                assert torch.equal(m0, m1)
                assert torch.equal(ops.topk_mask_p(cs, 96, 0.9, 8, 0.0, groups, static), ops.topk_mask_p(cs, 96, 0.9, 8, 0.0, groups, static, kl))


# ---- 5: the mask kernels on a column-sum tensor made here ----
MB, MG, MN, MLENS = 2, 3, 448, [448, 130]        # 130 is no multiple of 4: one 4-column step of the aligned forms straddles it


@functools.lru_cache(maxsize=None)
def _mask_problem():
    gen = torch.Generator().manual_seed(23)
    # 512 distinct positive bf16 values (4 binades x 128 mantissas); every row a different 448 of them in a different order: no ties
    pool = torch.tensor([2.0 ** e * (1 + m / 128) for e in range(-3, 1) for m in range(128)])
    cs = torch.stack([pool[torch.randperm(512, generator=gen)[:MN]] for _ in range(MB * H * MG)]).view(MB, H, MG, MN)
    cs[1, 0, 1] = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (MN,), generator=gen)]      # a row of ties and zeros
    cs[0, 1, 0] = cs[1, 0, 1]
    static = torch.rand(1, H, MG, MN, generator=gen) < 0.03
    static[:, :, MG - 1] = True                   # the "text group": keeps every key ...
    groups = torch.ones(1, H, MG, 1, dtype=torch.bool)
    groups[:, :, MG - 1] = False                  # ... and takes no part in the selection
    return cs.to(torch.bfloat16), static, groups


def _select(ops, cs, k, mass, random_amount, groups, static, kl=None):
    if mass:
        return ops.topk_mask_p(cs, k, 0.9, 8, random_amount, groups, static, kl)
    return ops.topk_mask(cs, k, random_amount, groups, static, kl)


@pytest.mark.parametrize("stream", [0, 1], ids=["register_form", "streaming_form"])
@pytest.mark.parametrize("k,mass", [(0, False), (48, False), (200, False), (200, True)])
def test_mask_kernels_select_among_the_valid_columns(dev, k, mass, stream):
    from chipmunk_amd import ops
    cs, static, groups = [t.to(dev) for t in _mask_problem()]
    kl = torch.tensor(MLENS, dtype=torch.int32, device=dev)
    with forced(topk_mask_stream=stream):
        got = _select(ops, cs, k, mass, 0.0, groups, static, kl)
        for b, L in enumerate(MLENS):
            want = _select(ops, cs[b:b + 1, ..., :L].contiguous(), min(k, L), mass, 0.0, groups, static[..., :L].contiguous())
            assert torch.equal(got[b:b + 1, ..., :L], want), f"sequence {b}: not the mask of the cropped column sums"
            assert not got[b, ..., L:].any(), f"sequence {b}: a bit at or past k_lens = {L} (the all-True static group included)"
        ops.manual_seed(3)
        rnd = _select(ops, cs, k, mass, 0.01, groups, static, kl)
    for b, L in enumerate(MLENS):
        assert not rnd[b, ..., L:].any()
        if not mass:
            assert (rnd[b, :, :MG - 1, :L].sum(-1) >= min(k, L)).all()      # the active rows keep their top-k under the random part


# ... and at the row lengths real launches have: a sequence end past the first 4096-column step (the register forms of 16, 48 and 120
# keys per thread, whose cut sits in step j >= 1; the streaming form's cut at j > 0), and a row whose width is no multiple of 4 (the
# generic form, element by element).  Two rows per sequence; k straddles the number of columns of the last, partial step.
@pytest.mark.parametrize("stream", [0, 1], ids=["register_form", "streaming_form"])
@pytest.mark.parametrize("n,L", [(8192, 4099), (20480, 12290), (53248, 49155), (8190, 4101)])
def test_mask_kernels_cut_past_the_first_step(dev, n, L, stream):
    from chipmunk_amd import ops
    gen = torch.Generator().manual_seed(n)
    cs = (torch.rand(2, 1, 2, n, generator=gen) + 0.01).to(torch.bfloat16).to(dev)      # bf16 of 53 248 draws: ties at every threshold
    static = (torch.rand(1, 1, 2, n, generator=gen) < 0.01).to(dev)
    groups = torch.tensor([True, False]).view(1, 1, 2, 1).to(dev)
    static[:, :, 1] = True
    kl = torch.tensor([n, L], dtype=torch.int32, device=dev)
    with forced(topk_mask_stream=stream):
        for k, mass in ((300, False), (L - 2, False), (4000, True)):
            got = _select(ops, cs, k, mass, 0.0, groups, static, kl)
            for b, Lb in enumerate((n, L)):
                want = _select(ops, cs[b:b + 1, ..., :Lb].contiguous(), min(k, Lb), mass, 0.0, groups, static[..., :Lb].contiguous())
                assert torch.equal(got[b:b + 1, ..., :Lb], want), f"sequence {b}, k {k}: not the mask of the cropped column sums"
                assert not got[b, ..., Lb:].any()
        ops.manual_seed(4)
        assert not _select(ops, cs, 300, False, 0.01, groups, static, kl)[1, ..., L:].any()


# ---- 6, 7: the fused mask step with lengths = the two operators with lengths; the gathered step over such a mask ----
@functools.lru_cache(maxsize=None)
def _mask_step(fused):
    from chipmunk_amd import ops
    dev = torch.device("cuda:0")
    n, lens = WAVE64["n"], [448, 132, 65]
    q, k, v, kl = _operands(dev, n, lens, False)
    G = math.ceil(n / 192)
    gen = torch.Generator().manual_seed(7)
    static = (torch.rand(1, H, G, n, generator=gen) < 0.02).to(dev)
    static[:, :, G - 1] = True
    groups = (torch.rand(1, H, G, 1, generator=gen) < 0.8).to(dev)
    groups[:, :, G - 1] = False
    with forced(**WAVE64["opts"]):
        _, l0 = ops.dense_attn(q, k, v, False, kl)
        if fused:
            o, mask, l = ops.dense_colsum_topk_mask(q, k, v, l0, 64, 0.0, groups, static, False, kl)
        else:
            o, cs, l = ops.dense_colsum_attn(q, k, v, l0, False, kl)
            mask = ops.topk_mask(cs[..., :G, :n], 64, 0.0, groups, static, kl)
        torch.cuda.synchronize()
    return o, mask, l, lens


def test_fused_mask_step_equals_the_two_operators_with_lengths(dev):
    o_a, m_a, l_a, lens = _mask_step(False)
    o_b, m_b, l_b, _ = _mask_step(True)
    assert torch.equal(o_a, o_b) and torch.equal(l_a, l_b) and torch.equal(m_a, m_b)
    for b, L in enumerate(lens):
        assert not m_b[b, ..., L:].any()
        assert m_b[b, :, -1, :L].all()            # the group that keeps every key keeps every VALID key


def test_gathered_step_over_a_mask_made_with_lengths(dev):
    from chipmunk_amd import ops
    _, mask, _, lens = _mask_step(True)
    n = WAVE64["n"]
    q, k, v, _ = _operands(dev, n, lens, True)        # NaN padding: a listed padding key would show
    packed, shape = ops.bitpack(mask)
    flat, offsets, counts = ops.mask_to_ragged_indices(packed, shape, 1, 192, True)
    G = mask.shape[2]
    inds = torch.zeros(B, H, G, n, dtype=torch.int32, device=dev)
    past = 0
    for r in range(B * H * G):
        b, c = r // (H * G), int(counts.view(-1)[r])
        row = flat[int(offsets[r]):int(offsets[r]) + c]
        past += int((row >= lens[b]).sum())
        inds.view(-1, n)[r, :c] = row
    assert past == 0, f"{past} listed keys at or past their sequence's k_lens"
    base = torch.zeros_like(q)
    o = ops.csp_attn_out_ragged(q, k, v, base, flat, offsets, counts, 1)
    qc, kc, vc = [t.to(dev) for t in _inputs(n)]
    assert_rows_close(o, attn_exact(qc, kc, vc, inds, counts), what="gathered step over a k_lens mask")


# ---- 8: the lengths are read on the device: a captured graph replays with whatever the tensor holds then ----
def test_graph_replays_with_other_lengths(dev):
    from chipmunk_amd import ops
    n = WAVE64["n"]
    q, k, v, kl = _operands(dev, n, [448, 200, 64], False)
    G = math.ceil(n / 192)
    static = (torch.rand(1, H, G, n, generator=torch.Generator().manual_seed(9)) < 0.02).to(dev)
    with forced(**WAVE64["opts"]):
        _, l0 = ops.dense_attn(q, k, v)

        def step():
            return ops.dense_colsum_topk_mask(q, k, v, l0, 64, 0.0, None, static, False, kl)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                       # scratch of the capture stream reaches its size
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            captured = step()
        kl.copy_(torch.tensor([100, 448, 301], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        eager = step()
        torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    assert not captured[1][0, ..., 100:].any() and not captured[1][2, ..., 301:].any() and captured[1][2, ..., 64:301].any()
