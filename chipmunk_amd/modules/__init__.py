from .attn import SparseDiffAttn
from .mlp import SparseDiffMlp
from .mlp_glu import SparseDiffGatedMlp
from .mlp_fp8 import F8Linear, W8Linear, quantize_fp8, recursive_swap_linears

__all__ = ["SparseDiffAttn", "SparseDiffMlp", "SparseDiffGatedMlp", "F8Linear", "W8Linear", "quantize_fp8", "recursive_swap_linears"]
