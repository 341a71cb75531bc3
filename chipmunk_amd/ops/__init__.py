"""Operator wrappers with the reference's names (``src/chipmunk/ops/__init__.py:1-7``)."""
from .mlp import run_e2e as mlp, GLU_ACTS
from .mlp import run_e2e_glu as mlp_glu, run_e2e_glu, mm1_glu
from .mlp import run_e2e_glu_fp8 as mlp_glu_fp8, run_e2e_glu_fp8, mm1_glu_fp8
from .mlp import run_e2e_glu_w8 as mlp_glu_w8, run_e2e_glu_w8, mm1_glu_w8
from .indexed_io import (copy_indices, topk_indices, mask_to_indices, scatter_add, packed_mask_to_indices,
                         mask_to_sorted_indices, mask_to_ragged_indices, topk_mask, topk_mask_p, topk_indices_p, topk_delta_indices_p, manual_seed,
                         topk_group_delta_indices, topk_group_delta_indices_p, TOPK_MASK_MAX_N)
from .attn import compact_indices, csp_attn, csp_attn_inplace, csp_attn_out, csp_attn_out_ragged, dense_attn, dense_colsum_attn, dense_colsum_topk_mask, dense_colsum_topk_mask_p
from .patch import patchify, unpatchify, patchify_rope
from .bitpack import bitpack, bitunpack
from . import voxel
from .w8_linear import w8_linear
from .qkv import qkv_split_norm, residual_ln_modulate, residual_ln_modulate_f32, split_heads_rownorm, wan_rope_table

__all__ = ["mlp", "copy_indices", "topk_indices", "mask_to_indices", "scatter_add", "csp_attn", "dense_attn",
           "dense_colsum_attn", "patchify", "unpatchify", "patchify_rope", "bitpack", "bitunpack",
           "packed_mask_to_indices", "mask_to_sorted_indices", "csp_attn_inplace", "csp_attn_out", "topk_mask", "TOPK_MASK_MAX_N", "voxel", "manual_seed", "qkv_split_norm", "dense_colsum_topk_mask", "compact_indices", "csp_attn_out_ragged", "residual_ln_modulate", "residual_ln_modulate_f32",
           "split_heads_rownorm", "wan_rope_table", "mask_to_ragged_indices", "mlp_glu", "run_e2e_glu", "mm1_glu",
           "mlp_glu_fp8", "run_e2e_glu_fp8", "mm1_glu_fp8", "mlp_glu_w8", "run_e2e_glu_w8", "mm1_glu_w8", "topk_mask_p", "dense_colsum_topk_mask_p",
           "topk_indices_p", "topk_delta_indices_p", "topk_group_delta_indices", "topk_group_delta_indices_p", "w8_linear"]

from . import _fake  # noqa: E402,F401  shape-only ("fake") kernels so torch.compile can trace through the ops
