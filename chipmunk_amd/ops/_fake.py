"""Shape/dtype-only implementations of the returning ops for FakeTensor / torch.compile tracing.

The reference registers none, so every op is a graph break under ``torch.compile`` ("adding fake impls is
a free win").  The in-place ops need nothing (they return ``()``)."""
import torch


def _o_like(q, token_major):
    B, H, N, D = q.shape
    return q.new_empty((B, N, H, D)).permute(0, 2, 1, 3) if token_major else q.new_empty((B, H, N, D))


def _register():
    lib = torch.library

    @lib.register_fake("chipmunk::csp_128_attn")
    def _(q, k, v, indices, indices_counts):
        return torch.empty_like(q)

    @lib.register_fake("chipmunk::csp_attn_out")
    def _(q, k, v, o_in, indices, indices_counts, o_scale):
        return torch.empty_like(o_in)

    @lib.register_fake("chipmunk::residual_ln_modulate")
    def _(x, y, gate, shift, scale, eps):
        return [torch.empty_like(x), torch.empty_like(x)] if y is not None else [torch.empty_like(x)]

    @lib.register_fake("chipmunk::residual_ln_modulate_f32")
    def _(x, y, gate, shift, scale, weight, bias, eps):
        xm = torch.empty_like(x, dtype=torch.bfloat16)
        return [torch.empty_like(x, dtype=torch.float32), xm] if y is not None else [xm]

    @lib.register_fake("chipmunk::csp_attn_out_ragged")
    def _(q, k, v, o_in, indices, offsets, indices_counts, o_scale):
        return torch.empty_like(o_in)

    @lib.register_fake("chipmunk::dense_attn")
    def _(q, k, v):
        return [_o_like(q, False), q.new_empty((q.shape[0], q.shape[1], q.shape[2], 1), dtype=torch.float32)]

    @lib.register_fake("chipmunk::dense_attn_layout")
    def _(q, k, v, token_major_o):
        return [_o_like(q, token_major_o), q.new_empty((q.shape[0], q.shape[1], q.shape[2], 1), dtype=torch.float32)]

    @lib.register_fake("chipmunk::dense_colsum_attn_layout")
    def _(q, k, v, p, token_major_o):
        groups = (q.shape[2] + 191) // 192
        return [_o_like(q, token_major_o),
                q.new_empty((q.shape[0], q.shape[1], groups, max(q.shape[2], k.shape[2]))),
                q.new_empty((q.shape[0], q.shape[1], q.shape[2], 1), dtype=torch.float32)]

    @lib.register_fake("chipmunk::dense_colsum_attn")
    def _(q, k, v, p):
        groups = (q.shape[2] + 191) // 192
        return [_o_like(q, False),
                q.new_empty((q.shape[0], q.shape[1], groups, max(q.shape[2], k.shape[2]))),
                q.new_empty((q.shape[0], q.shape[1], q.shape[2], 1), dtype=torch.float32)]

    @lib.register_fake("chipmunk::mask_to_indices")
    def _(mask, multiple_of, pad_to_multiple_of):
        b, h, m, n = mask.shape
        pad_n = (n + pad_to_multiple_of - 1) // pad_to_multiple_of * pad_to_multiple_of
        return [mask.new_empty((b, h, m, pad_n), dtype=torch.int32), mask.new_empty((b, h, m), dtype=torch.int32)]

    @lib.register_fake("chipmunk::packed_mask_to_indices")
    def _(packed, shape, multiple_of, pad_to_multiple_of):
        b, h, m, n = shape
        pad_n = (n + pad_to_multiple_of - 1) // pad_to_multiple_of * pad_to_multiple_of
        return [packed.new_empty((b, h, m, pad_n), dtype=torch.int32), packed.new_empty((b, h, m), dtype=torch.int32)]

    @lib.register_fake("chipmunk::topk_mask")
    def _(cs, k, random_amount, groups, static_mask):
        return cs.new_empty(cs.shape, dtype=torch.bool)

    @lib.register_fake("chipmunk::block_mean")
    def _(x, mbm):
        return x.new_empty((x.shape[0], (x.shape[1] + mbm - 1) // mbm, x.shape[2]))   # a ragged last block counts

    @lib.register_fake("chipmunk::transpose_last2")
    def _(x):
        return x.new_empty(x.shape[:-2] + (x.shape[-1], x.shape[-2]))

    @lib.register_fake("chipmunk::transpose_last2_pitched")
    def _(x, ld):
        return x.new_empty(x.shape[:-2] + (x.shape[-1], ld))

    @lib.register_fake("chipmunk::transpose_to_groups")
    def _(x):
        torch._check(x.ndim >= 2 and x.element_size() == 2, lambda: "transpose_to_groups: need a >=2-D tensor of a 16-bit dtype")
        return x.new_empty(x.shape[:-2] + ((x.shape[-2] + 127) // 128, x.shape[-1], 128))   # the last group may be short: zero rows

    @lib.register_fake("chipmunk::csp_scatter_add_gm")
    def _(packed, unpacked_groups, sp_inds, sp_counts):
        # accumulates into unpacked_groups in place and returns nothing
        torch._check(packed.ndim == 3 and unpacked_groups.ndim == 4, lambda: "packed must be [B, M, F], unpacked_groups [B, G, F, 128]")
        b, m, f = packed.shape
        g = (m + 127) // 128
        torch._check(unpacked_groups.shape == (b, g, f, 128), lambda: "unpacked_groups must be [B, ceil(M/128), F, 128]")
        torch._check(sp_inds.shape == (b, g, f) and sp_counts.shape == (b, g), lambda: "sp_inds must be [B, ceil(M/128), F], sp_counts [B, ceil(M/128)]")
        return None

    @lib.register_fake("chipmunk::quantize_fp8")
    def _(x, scale, max_value):
        return x.new_empty(x.shape, dtype=torch.float8_e4m3fn)

    @lib.register_fake("chipmunk::bitpack")
    def _(mask):
        return mask.new_empty(((mask.numel() + 7) // 8,), dtype=torch.uint8)

    @lib.register_fake("chipmunk::bitunpack")
    def _(packed, shape):
        return packed.new_empty(tuple(shape), dtype=torch.bool)

    @lib.register_fake("chipmunk::gather_rows")
    def _(src, map):
        shape = list(src.shape)
        shape[-2] = map.shape[0]
        return src.new_empty(shape)

    @lib.register_fake("chipmunk::dense_colsum_topk_mask")
    def _(q, k, v, p, k_top, random_amount, groups, static_mask, token_major_o=False):
        B, H, Nq, D = q.shape
        G = (Nq + 191) // 192
        return [_o_like(q, token_major_o), q.new_empty((B, H, G, k.shape[2]), dtype=torch.bool),
                q.new_empty((B, H, Nq, 1), dtype=torch.float32)]

    @lib.register_fake("chipmunk::topk_mask_p")
    def _(cs, k, top_p, k_min, random_amount, groups, static_mask):
        return cs.new_empty(cs.shape, dtype=torch.bool)

    @lib.register_fake("chipmunk::dense_colsum_topk_mask_p")
    def _(q, k, v, p, k_top, top_p, k_min, random_amount, groups, static_mask, token_major_o=False):
        B, H, Nq, D = q.shape
        G = (Nq + 191) // 192
        return [_o_like(q, token_major_o), q.new_empty((B, H, G, k.shape[2]), dtype=torch.bool),
                q.new_empty((B, H, Nq, 1), dtype=torch.float32)]

    # padded batches (k_lens): the shapes and dtypes of the operators without it
    def _dense_out(q):
        return q.new_empty((q.shape[0], q.shape[1], q.shape[2], 1), dtype=torch.float32)

    @lib.register_fake("chipmunk::dense_attn_varlen")
    def _(q, k, v, k_lens, token_major_o=False):
        return [_o_like(q, token_major_o), _dense_out(q)]

    @lib.register_fake("chipmunk::dense_colsum_attn_varlen")
    def _(q, k, v, p, k_lens, token_major_o=False):
        groups = (q.shape[2] + 191) // 192
        return [_o_like(q, token_major_o), q.new_empty((q.shape[0], q.shape[1], groups, max(q.shape[2], k.shape[2]))), _dense_out(q)]

    @lib.register_fake("chipmunk::topk_mask_varlen")
    def _(cs, k_lens, k, random_amount, groups, static_mask):
        return cs.new_empty(cs.shape, dtype=torch.bool)

    @lib.register_fake("chipmunk::topk_mask_p_varlen")
    def _(cs, k_lens, k, top_p, k_min, random_amount, groups, static_mask):
        return cs.new_empty(cs.shape, dtype=torch.bool)

    @lib.register_fake("chipmunk::dense_colsum_topk_mask_varlen")
    def _(q, k, v, p, k_lens, k_top, random_amount, groups, static_mask, token_major_o=False):
        G = (q.shape[2] + 191) // 192
        return [_o_like(q, token_major_o), q.new_empty((q.shape[0], q.shape[1], G, k.shape[2]), dtype=torch.bool), _dense_out(q)]

    @lib.register_fake("chipmunk::dense_colsum_topk_mask_p_varlen")
    def _(q, k, v, p, k_lens, k_top, top_p, k_min, random_amount, groups, static_mask, token_major_o=False):
        G = (q.shape[2] + 191) // 192
        return [_o_like(q, token_major_o), q.new_empty((q.shape[0], q.shape[1], G, k.shape[2]), dtype=torch.bool), _dense_out(q)]

    @lib.register_fake("chipmunk::topk_indices_p")
    def _(activation, indices, counts, sparsity_amount, top_p, min_keys, multiple_of, random_amount):
        # writes indices and counts in place and returns nothing: the shapes are checked, so that a trace fails where the operator would
        torch._check(activation.ndim == 3 and activation.shape[-1] >= 1024, lambda: "activation must be [batch, rows, cols] with cols >= 1024")
        torch._check(indices.shape == activation.shape and counts.numel() == activation.shape[0] * activation.shape[1],
                     lambda: "indices must have the shape of activation, counts must be [batch, rows]")
        return None

    @lib.register_fake("chipmunk::topk_delta_indices_p")
    def _(activation, cache, indices, counts, sparsity_amount, top_p, min_keys, multiple_of, random_amount):
        # as topk_indices_p; also copies the listed columns into cache in place
        torch._check(activation.ndim == 3 and activation.shape[-1] >= 1024, lambda: "activation must be [batch, rows, cols] with cols >= 1024")
        torch._check(cache.shape == activation.shape and cache.dtype == activation.dtype, lambda: "cache must have the shape and dtype of activation")
        torch._check(indices.shape == activation.shape and counts.numel() == activation.shape[0] * activation.shape[1],
                     lambda: "indices must have the shape of activation, counts must be [batch, rows]")
        return None

    def _check_group_delta(activation, cache, indices, counts, rows_per_group):
        torch._check(activation.ndim == 3 and activation.shape[-1] >= 1024, lambda: "activation must be [batch, rows, cols] with cols >= 1024")
        torch._check(cache.shape == activation.shape and cache.dtype == activation.dtype, lambda: "cache must have the shape and dtype of activation")
        torch._check(1 <= rows_per_group <= 64, lambda: "rows_per_group must be in [1, 64]")
        groups = (activation.shape[1] + rows_per_group - 1) // rows_per_group
        torch._check(tuple(indices.shape) == (activation.shape[0], groups, activation.shape[2]) and tuple(counts.shape) == (activation.shape[0], groups),
                     lambda: "indices must be [batch, ceil(rows / rows_per_group), cols], counts [batch, ceil(rows / rows_per_group)]")

    @lib.register_fake("chipmunk::topk_group_delta_indices")
    def _(activation, cache, indices, counts, rows_per_group, sparsity_amount, multiple_of, random_amount):
        # writes indices, counts and the listed columns of cache in place and returns nothing
        _check_group_delta(activation, cache, indices, counts, rows_per_group)
        return None

    @lib.register_fake("chipmunk::topk_group_delta_indices_p")
    def _(activation, cache, indices, counts, rows_per_group, sparsity_amount, top_p, min_keys, multiple_of, random_amount):
        _check_group_delta(activation, cache, indices, counts, rows_per_group)
        return None

    @lib.register_fake("chipmunk::qkv_split_norm")
    def _(qkv, q_weight, k_weight, heads, eps, freqs_cos=None, freqs_sin=None):
        out = qkv.new_empty((3, 1, heads, qkv.shape[0], 128))
        return [out[0], out[1], out[2]]

    @lib.register_fake("chipmunk::split_heads_rownorm")
    def _(x, heads, parts, w0, w1, w2, norm_mask, rope_mask, eps, freqs_cos=None, freqs_sin=None):
        out = x.new_empty((parts, x.shape[0] if x.dim() == 3 else 1, heads, x.shape[-2], 128))
        return [out[p] for p in range(parts)]

    @lib.register_fake("chipmunk::csp_mlp_mm1_glu")
    def _(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache_colmajor, indices, indices_counts, act, update_cache):
        # writes c (and the cache) in place and returns nothing: the shapes are checked, so that a trace fails where the operator would
        torch._check(a.shape[-1] == b_gate.shape[1] and b_gate.shape == b_up.shape, lambda: "a, b_gate and b_up must share K; b_up the shape of b_gate")
        torch._check(c.shape == a.shape[:-1] + (b_gate.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_glu: unknown activation '{act}'")
        return None

    @lib.register_fake("chipmunk::csp_mlp_mm1_glu_fp8")
    def _(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache_colmajor, indices, indices_counts, scale_a, scale_b_gate, scale_b_up, act,
          update_cache):
        # as csp_mlp_mm1_glu, with e4m3 a / weights and three one-element float32 scales
        f8 = torch.float8_e4m3fn
        torch._check(a.dtype == f8 and b_gate.dtype == f8 and b_up.dtype == f8, lambda: "a, b_gate and b_up must be float8_e4m3fn")
        torch._check(c.dtype == torch.bfloat16 and pa_cache_colmajor.dtype == torch.bfloat16, lambda: "c and pa_cache_colmajor must be bfloat16")
        torch._check(a.shape[-1] == b_gate.shape[1] and b_gate.shape == b_up.shape, lambda: "a, b_gate and b_up must share K; b_up the shape of b_gate")
        torch._check(c.shape == a.shape[:-1] + (b_gate.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        for s in (scale_a, scale_b_gate, scale_b_up):
            torch._check(s.dtype == torch.float32 and s.numel() == 1, lambda: "scale_a, scale_b_gate and scale_b_up must be one-element float32 tensors")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_glu_fp8: unknown activation '{act}'")
        return None

    @lib.register_fake("chipmunk::csp_mlp_mm1_act")
    def _(a, b, c, bias, pa_cache, indices, counts, act, update_cache):
        # writes c (and the cache) in place and returns nothing: the shapes are checked, so that a trace fails where the operator would
        torch._check(a.shape[-1] == b.shape[1], lambda: "a and b must share the K dimension")
        torch._check(c.shape == a.shape[:-1] + (b.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        torch._check(bias is None or bias.numel() == b.shape[0], lambda: "bias must have F entries")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_act: unknown activation '{act}'")
        return None

    @lib.register_fake("chipmunk::csp_mlp_mm1_fp8_act")
    def _(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, act, update_cache):
        # as csp_mlp_mm1_act, with e4m3 a / b and two one-element float32 scales; update_cache 0 / 1 / 2
        f8 = torch.float8_e4m3fn
        torch._check(a.dtype == f8 and b.dtype == f8, lambda: "a and b must be float8_e4m3fn")
        torch._check(c.dtype == torch.bfloat16 and pa_cache.dtype == torch.bfloat16, lambda: "c and pa_cache must be bfloat16")
        torch._check(a.shape[-1] == b.shape[1], lambda: "a and b must share the K dimension")
        torch._check(c.shape == a.shape[:-1] + (b.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        torch._check(bias is None or bias.numel() == b.shape[0], lambda: "bias must have F entries")
        for s in (scale_a, scale_b):
            torch._check(s.dtype == torch.float32 and s.numel() == 1, lambda: "scale_a and scale_b must be one-element float32 tensors")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_fp8_act: unknown activation '{act}'")
        torch._check(update_cache in (0, 1, 2), lambda: "csp_mlp_mm1_fp8_act: update_cache must be 0, 1 or 2")
        return None

    @lib.register_fake("chipmunk::csp_mlp_mm1_fp8_act_rs")
    def _(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, act, update_cache):
        # as csp_mlp_mm1_fp8_act, with scale_a float32 [M] ([B, M] for a batched a) and scale_b float32 [F]
        f8 = torch.float8_e4m3fn
        torch._check(a.dtype == f8 and b.dtype == f8, lambda: "a and b must be float8_e4m3fn")
        torch._check(c.dtype == torch.bfloat16 and pa_cache.dtype == torch.bfloat16, lambda: "c and pa_cache must be bfloat16")
        torch._check(a.ndim in (2, 3) and b.ndim == 2 and a.shape[-1] == b.shape[1], lambda: "a and b must share the K dimension")
        torch._check(c.shape == a.shape[:-1] + (b.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        torch._check(bias is None or bias.numel() == b.shape[0], lambda: "bias must have F entries")
        torch._check(scale_a.dtype == torch.float32 and scale_b.dtype == torch.float32, lambda: "scale_a and scale_b must be float32")
        torch._check(scale_a.shape == a.shape[:-1] and scale_a.is_contiguous(), lambda: "scale_a must be [M] ([B, M] for a batched a), contiguous")
        torch._check(scale_b.shape == (b.shape[0],) and scale_b.is_contiguous(), lambda: "scale_b must be [F], contiguous")
        torch._check(scale_a.device == a.device and scale_b.device == a.device, lambda: "scale_a and scale_b must be on the device of a")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_fp8_act_rs: unknown activation '{act}'")
        torch._check(update_cache in (0, 1, 2), lambda: "csp_mlp_mm1_fp8_act_rs: update_cache must be 0, 1 or 2")
        return None

    @lib.register_fake("chipmunk::quantize_fp8_rowwise")
    def _(x, max_value):
        torch._check(x.dtype == torch.bfloat16 and x.ndim >= 1 and x.shape[-1] % 16 == 0, lambda: "x must be bfloat16 [..., K] with K % 16 == 0")
        return [x.new_empty(x.shape, dtype=torch.float8_e4m3fn), x.new_empty(x.shape[:-1], dtype=torch.float32)]

    @lib.register_fake("chipmunk::csp_mlp_mm2_w8")
    def _(mma_a, mma_b, scale_b, indices, counts, mma_c):
        # accumulates into mma_c in place and returns nothing
        torch._check(mma_b.dtype == torch.float8_e4m3fn, lambda: "mma_b must be float8_e4m3fn")
        torch._check(scale_b.dtype == torch.float32 and scale_b.numel() == 1, lambda: "scale_b must be a one-element float32 tensor on the GPU")
        torch._check(mma_b.ndim == 2 and mma_b.shape[0] == mma_a.shape[-1] and mma_c.shape == mma_a.shape[:-1] + (mma_b.shape[1],),
                     lambda: "shape mismatch (mma_b must be [F, N2], mma_c [M, N2], or [B, M, N2] with the batch size of mma_a)")
        return None

    @lib.register_fake("chipmunk::csp_mlp_mm1_w8")
    def _(a, b, scale_b, c, bias, pa_cache, indices, counts, act, update_cache):
        # as csp_mlp_mm1_act, with an e4m3 b and its float32 reciprocal scale: one element, or [F]
        torch._check(a.dtype == torch.bfloat16 and b.dtype == torch.float8_e4m3fn, lambda: "a must be bfloat16 and b float8_e4m3fn")
        torch._check(c.dtype == torch.bfloat16 and pa_cache.dtype == torch.bfloat16, lambda: "c and pa_cache must be bfloat16")
        torch._check(a.ndim in (2, 3) and b.ndim == 2 and a.shape[-1] == b.shape[1], lambda: "a and b must share the K dimension")
        torch._check(c.shape == a.shape[:-1] + (b.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        torch._check(bias is None or bias.numel() == b.shape[0], lambda: "bias must have F entries")
        torch._check(scale_b.dtype == torch.float32 and (scale_b.numel() == 1 or scale_b.shape == (b.shape[0],)),
                     lambda: "scale_b must be float32 with one element, or [F]")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_w8: unknown activation '{act}'")
        return None

    @lib.register_fake("chipmunk::csp_mlp_mm1_glu_w8")
    def _(a, b_gate, b_up, scale_gate, scale_up, c, bias_gate, bias_up, pa_cache, indices, counts, act, update_cache):
        # as csp_mlp_mm1_glu, with e4m3 b_gate / b_up and their float32 reciprocal scales: one element each, or [F]
        f8 = torch.float8_e4m3fn
        torch._check(a.dtype == torch.bfloat16 and b_gate.dtype == f8 and b_up.dtype == f8,
                     lambda: "a must be bfloat16, b_gate and b_up float8_e4m3fn")
        torch._check(c.dtype == torch.bfloat16 and pa_cache.dtype == torch.bfloat16, lambda: "c and pa_cache must be bfloat16")
        torch._check(a.ndim in (2, 3) and b_gate.ndim == 2 and a.shape[-1] == b_gate.shape[1] and b_gate.shape == b_up.shape,
                     lambda: "a, b_gate and b_up must share K; b_up the shape of b_gate")
        torch._check(c.shape == a.shape[:-1] + (b_gate.shape[0],), lambda: "c must be [M, F] ([B, M, F] with the batch size of a)")
        for bias in (bias_gate, bias_up):
            torch._check(bias is None or bias.numel() == b_gate.shape[0], lambda: "bias_gate and bias_up must have F entries")
        for s in (scale_gate, scale_up):
            torch._check(s.dtype == torch.float32 and (s.numel() == 1 or s.shape == (b_gate.shape[0],)),
                         lambda: "scale_gate and scale_up must be float32 with one element, or [F]")
        torch._check(act in ("gelu_tanh", "silu", "gelu"), lambda: f"csp_mlp_mm1_glu_w8: unknown activation '{act}'")
        return None

    @lib.register_fake("chipmunk::w8_linear")
    def _(x, w, scale_b, bias, y):
        # writes y [M, F] in place and returns nothing
        torch._check(x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and w.dtype == torch.float8_e4m3fn,
                     lambda: "x and y must be bfloat16 and w float8_e4m3fn")
        torch._check(x.ndim == 2 and w.ndim == 2 and x.shape[1] == w.shape[1] and y.shape == (x.shape[0], w.shape[0]),
                     lambda: "x must be [M, K], w [F, K] and y [M, F]")
        torch._check(bias is None or bias.numel() == w.shape[0], lambda: "bias must have F entries")
        torch._check(scale_b.dtype == torch.float32 and (scale_b.numel() == 1 or scale_b.shape == (w.shape[0],)),
                     lambda: "scale_b must be float32 with one element, or [F]")
        return None


_register()
