"""fp8 linear layers for the sparse MLP (mirror of reference ``src/chipmunk/modules/mlp_fp8.py:7-400``: ``F8Linear``,
``recursive_swap_linears``, ``quantize_fp8``).

Per-tensor scaling: ``scale = clamp(fp8_max / max(amax, 1e-12), max=fp8_max)``; values are multiplied by the scale,
clamped to the fp8 range and cast; the matmul result is multiplied by the RECIPROCAL scales
(``input_scale_reciprocal``, ``scale_reciprocal``) -- the two numbers ``SparseDiffMlp`` hands to ``csp_mlp_mm1_fp8``.
The input scale is calibrated over the first ``num_scale_trials`` calls and then frozen.
gfx950 implements the OCP formats (``float8_e4m3fn`` / ``float8_e5m2``), the same dtypes the reference uses on H100.

Row scaling (``scaling="row"``, config key ``mlp.fp8_scaling``; not in the reference): one scale per output feature of the weight
(``scale`` / ``scale_reciprocal`` are ``[out, 1]``) and one DYNAMIC scale per token row of the input, computed on every call
(``quantize_input_rowwise``: no calibration trials, nothing frozen).  The product is ``bf16((sum_k xq wq) * sa[m] * sb[n] + bias[n])``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
from torch.nn import init

from ..util.config import amd_key


def amax_to_scale(amax: torch.Tensor, max_val: float) -> torch.Tensor:
    return (max_val / torch.clamp(amax, min=1e-12)).clamp(max=max_val)


def to_fp8_saturated(x: torch.Tensor, scale: torch.Tensor, max_val: float) -> torch.Tensor:
    return (x * scale).clamp(-max_val, max_val)


SCALINGS = ("tensor", "row")
ROWWISE_MAX_K = 16384      # include/chipmunk_hip.h, CHIPMUNK_QUANTIZE_ROWWISE_MAX_K


def quantize_rowwise_torch(x: torch.Tensor, max_val: float, float8_dtype=torch.float8_e4m3fn):
    """The row-wise chain in torch, over the last dimension, all in fp32: ``amax = max_k |x|``, ``scale = amax_to_scale(amax)`` per row,
    ``xq = fp8((x.float() * scale).clamp(-max, max))`` -- the product is fp32 and rounded once, into fp8.  Returns ``(xq, 1 / scale)``,
    the reciprocal scales fp32 of shape ``x.shape[:-1]``.  What ``chipmunk_quantize_fp8_rowwise`` computes, bit for bit where the
    division is IEEE's -- so the quotient is tensor / tensor here: ``amax_to_scale``'s ``number / tensor`` is torch's reciprocal-then-multiply,
    two roundings, one ulp off the correctly rounded quotient for some rows."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    scale = (torch.full_like(amax, max_val) / torch.clamp(amax, min=1e-12)).clamp(max=max_val)
    xq = (xf * scale.unsqueeze(-1)).clamp(-max_val, max_val).to(float8_dtype)
    return xq, scale.reciprocal()


_SCALED_MM_ROWWISE = {}     # device -> does torch._scaled_mm take [M, 1] / [1, N] scales there (probed once, on a tiny call)


def scaled_mm_takes_row_scales(device: torch.device) -> bool:
    key = str(device)
    if key not in _SCALED_MM_ROWWISE:
        try:
            a = torch.ones(16, 32, device=device).to(torch.float8_e4m3fn)
            b = torch.ones(16, 32, device=device).to(torch.float8_e4m3fn)
            out = torch._scaled_mm(a, b.T, scale_a=torch.full((16, 1), 0.5, device=device), scale_b=torch.full((1, 16), 2.0, device=device),
                                   out_dtype=torch.bfloat16)
            _SCALED_MM_ROWWISE[key] = bool((out.float() == 32.0).all())
        except (RuntimeError, NotImplementedError, ValueError):      # refused by this build: an answer, the fallback below computes the same formula
            _SCALED_MM_ROWWISE[key] = False
    return _SCALED_MM_ROWWISE[key]


class F8Linear(nn.Module):
    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=torch.float16,
                 float8_dtype=torch.float8_e4m3fn, float_weight: Optional[torch.Tensor] = None,
                 float_bias: Optional[torch.Tensor] = None, num_scale_trials: int = 12,
                 input_float8_dtype=torch.float8_e4m3fn, scaling: str = "tensor") -> None:
        super().__init__()
        if scaling not in SCALINGS:
            raise ValueError(f"F8Linear: unknown scaling {scaling!r} (one of {', '.join(SCALINGS)})")
        self.scaling = scaling
        self.in_features, self.out_features = in_features, out_features
        self.float8_dtype, self.input_float8_dtype = float8_dtype, input_float8_dtype
        self.max_value = torch.finfo(float8_dtype).max
        self.input_max_value = torch.finfo(input_float8_dtype).max
        self.input_scale_initialized = False
        self.weight_initialized = False
        if float_weight is None:
            self.weight = nn.Parameter(torch.empty((out_features, in_features), dtype=dtype, device=device))
        else:
            self.weight = nn.Parameter(float_weight, requires_grad=float_weight.requires_grad)
        if float_bias is not None:
            self.bias = nn.Parameter(float_bias, requires_grad=float_bias.requires_grad)
        elif bias:
            self.bias = nn.Parameter(torch.empty(out_features, dtype=dtype, device=device))
        else:
            self.register_parameter("bias", None)
        self.num_scale_trials = num_scale_trials
        self.input_amax_trials = torch.zeros(num_scale_trials, requires_grad=False, device=device, dtype=torch.float32)
        self.trial_index = 0
        for name in ("scale", "input_scale", "scale_reciprocal", "input_scale_reciprocal"):
            self.register_buffer(name, None)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Quantise on load (reference mlp_fp8.py:67-168).  Two checkpoint forms are accepted: a float ``weight`` of the
        layer's shape (quantised here), or an already quantised layer -- ``float8_data`` (the reference's buffer name) or
        an fp8 ``weight`` -- with its ``scale`` / ``scale_reciprocal`` (and optionally the frozen input scale)."""
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        shape = (self.out_features, self.in_features)
        if "weight" not in sd and "float8_data" not in sd:
            raise RuntimeError("Weight tensor not found or has incorrect shape in state dict")
        fp8 = sd.get("float8_data")
        if fp8 is None and sd["weight"].dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
            fp8 = sd["weight"]
        if "bias" in sd:
            self._parameters["bias"] = nn.Parameter(sd["bias"], requires_grad=False)
        if fp8 is None:
            if tuple(sd["weight"].shape) != shape:
                raise RuntimeError(f"Weight tensor not found or has incorrect shape in state dict: {sd.keys()}")
            self._parameters["weight"] = nn.Parameter(sd["weight"], requires_grad=False)
            self.weight_initialized = False
            self.quantize_weight()
            return
        if tuple(fp8.shape) != shape or "scale" not in sd:
            raise RuntimeError(f"Weight tensor not found or has incorrect shape in state dict: {sd.keys()}")
        self._parameters["weight"] = nn.Parameter(fp8.to(self.float8_dtype), requires_grad=False)
        self.weight_initialized = True
        # the checkpoint's granularity decides the mode: one scale per output feature = row scaling, one number = per tensor
        n_scales = sd["scale"].numel()
        if n_scales not in (1, self.out_features) or ("scale_reciprocal" in sd and sd["scale_reciprocal"].numel() != n_scales):
            raise RuntimeError(f"F8Linear: a quantised checkpoint carries one scale, or one per output feature ({self.out_features}); "
                               f"got {n_scales}")
        if self.out_features > 1:           # (a one-feature layer keeps the mode it was built with: both forms have one scale)
            self.scaling = "row" if n_scales == self.out_features else "tensor"
        shape_of = (lambda t: t.float().reshape(-1, 1)) if self.scaling == "row" else (lambda t: t.float())
        self.scale = shape_of(sd["scale"])
        self.scale_reciprocal = shape_of(sd["scale_reciprocal"]) if "scale_reciprocal" in sd else self.scale.reciprocal()
        if self.scaling == "row":           # dynamic input scales: nothing to load, nothing to calibrate
            return
        if "input_scale" in sd and "input_scale_reciprocal" in sd:
            self.input_scale = sd["input_scale"].float()
            self.input_scale_reciprocal = sd["input_scale_reciprocal"].float()
            self.input_scale_initialized = True
            self.trial_index = self.num_scale_trials
        else:                                   # calibrate the input scale again over the first calls
            self.input_scale_initialized = False
            self.trial_index = 0
            self.input_amax_trials = torch.zeros(self.num_scale_trials, requires_grad=False, dtype=torch.float32,
                                                 device=self.weight.device)

    # kept as methods too: the reference exposes them on the instance (mlp_fp8.py:191-195)
    def amax_to_scale(self, amax, max_val):
        return amax_to_scale(amax, max_val)

    def to_fp8_saturated(self, x, scale, max_val):
        return to_fp8_saturated(x, scale, max_val)

    def quantize_weight(self) -> None:
        if self.weight_initialized:
            return
        if self.scaling == "row":           # one scale per output feature: amax over the input dimension, everything in fp32
            w = self.weight.data.float()
            self.scale = amax_to_scale(w.abs().amax(dim=1, keepdim=True), self.max_value)          # [out, 1]
            self.scale_reciprocal = self.scale.reciprocal()
            fp8 = (w * self.scale).clamp(-self.max_value, self.max_value).to(self.float8_dtype)
            self.weight = nn.Parameter(fp8, requires_grad=False)
            self.weight_initialized = True
            return
        amax = self.weight.data.abs().max().float()
        self.scale = amax_to_scale(amax, self.max_value)
        self.scale_reciprocal = self.scale.reciprocal()
        fp8 = to_fp8_saturated(self.weight.data, self.scale, self.max_value).to(self.float8_dtype)
        self.weight = nn.Parameter(fp8, requires_grad=False)
        self.weight_initialized = True

    def set_weight_tensor(self, tensor: torch.Tensor) -> None:
        self.weight = nn.Parameter(tensor, requires_grad=False)
        self.weight_initialized = False
        self.quantize_weight()

    def quantize_input_rowwise(self, x: torch.Tensor):
        """Row scaling: ``x [..., K] -> (xq [..., K] fp8, scale_recip [...] fp32)``, one dynamic scale per row of the last dimension
        (``quantize_rowwise_torch``'s chain).  A bf16 GPU tensor with e4m3 inputs and ``K % 16 == 0``, ``K <= ROWWISE_MAX_K`` takes the
        one-pass kernel; everything else the torch chain."""
        if self.scaling != "row":
            raise RuntimeError("F8Linear.quantize_input_rowwise: this layer scales per tensor (scaling='tensor'): call quantize_input")
        K = x.shape[-1]
        if (x.is_cuda and x.dtype == torch.bfloat16 and self.input_float8_dtype == torch.float8_e4m3fn and K % 16 == 0
                and 0 < K <= ROWWISE_MAX_K and x.numel() > 0):
            xq, recip = torch.ops.chipmunk.quantize_fp8_rowwise(x, float(self.input_max_value))
            return xq, recip
        return quantize_rowwise_torch(x, self.input_max_value, self.input_float8_dtype)

    def quantize_input(self, x: torch.Tensor) -> torch.Tensor:
        if self.scaling == "row":
            raise RuntimeError("F8Linear.quantize_input: this layer scales per row (scaling='row'), there is no frozen input scale: call "
                               "quantize_input_rowwise, which returns (xq, scale_recip)")
        if not self.input_scale_initialized:
            if self.trial_index < self.num_scale_trials:
                self.input_amax_trials[self.trial_index] = x.abs().max().float()
                self.trial_index += 1
                amax = self.input_amax_trials[: self.trial_index].max()
            else:
                amax = self.input_amax_trials.max()
                self.input_scale_initialized = True
            self.input_scale = amax_to_scale(amax, self.input_max_value)
            self.input_scale_reciprocal = self.input_scale.reciprocal()
        if (x.is_cuda and x.dtype == torch.bfloat16 and self.input_float8_dtype == torch.float8_e4m3fn and x.numel() % 8 == 0
                and self.input_scale.dtype == torch.float32 and self.input_scale.is_cuda and self.input_scale.dim() == 0
                and amd_key("mlp", "fused_fp8_quantize")):
            # the three elementwise kernels below as one pass, bit-identical (tests/test_gpu_mlp.py::test_quantize_fp8_matches_the_torch_chain)
            # -- for a 0-dim device scale only: a shape-[1] scale makes torch's `x * scale` a single fp32 rounding, a host scale
            # cannot be read by the kernel; both take the torch chain below
            return torch.ops.chipmunk.quantize_fp8(x, self.input_scale.reshape(1), float(self.input_max_value))
        return to_fp8_saturated(x, self.input_scale, self.input_max_value).to(self.input_float8_dtype)

    def reset_parameters(self) -> None:
        if self.weight_initialized:
            self.weight = nn.Parameter(torch.empty((self.out_features, self.in_features), dtype=torch.bfloat16,
                                                   device=self.weight.device))
            self.weight_initialized = False
            self.input_scale_initialized = False
            self.trial_index = 0
            self.input_amax_trials.zero_()
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in, _ = init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
            init.uniform_(self.bias, -bound, bound)
        self.quantize_weight()

    def _forward_rowwise(self, x: torch.Tensor) -> torch.Tensor:
        """``bf16((sum_k xq wq) * sa[m] * sb[n] + bias[n])``, fp32 sums: ``torch._scaled_mm`` with ``[M, 1]`` / ``[1, N]`` scales where
        this torch build takes them on the device (probed once), otherwise the same formula as a matmul over the widened operands
        (e4m3 -> fp32 is exact)."""
        xq, sa = self.quantize_input_rowwise(x)
        lead = xq.shape[:-1]
        xq2, sa2 = xq.reshape(-1, self.in_features), sa.reshape(-1, 1)
        sb = self.scale_reciprocal.reshape(1, -1)
        if xq2.is_cuda and xq2.shape[0] > 0 and scaled_mm_takes_row_scales(xq2.device):
            out = torch._scaled_mm(xq2, self.weight.T, scale_a=sa2.contiguous(), scale_b=sb.contiguous(), bias=self.bias,
                                   out_dtype=torch.bfloat16)
        else:
            acc = (xq2.float() @ self.weight.float().T) * sa2 * sb
            out = (acc if self.bias is None else acc + self.bias.float()).to(torch.bfloat16)
        return out.view(*lead, self.out_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.scaling == "row":
            return self._forward_rowwise(x)
        xq = self.quantize_input(x)
        lead = xq.shape[:-1]
        out = torch._scaled_mm(xq.view(-1, self.in_features), self.weight.T, scale_a=self.input_scale_reciprocal,
                               scale_b=self.scale_reciprocal, bias=self.bias, out_dtype=torch.bfloat16,
                               use_fast_accum=True)
        return out.view(*lead, self.out_features)

    @classmethod
    def from_linear(cls, linear: nn.Linear, float8_dtype=torch.float8_e4m3fn,
                    input_float8_dtype=torch.float8_e5m2, scaling: str = "tensor") -> "F8Linear":
        f8 = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, device=linear.weight.device,
                 dtype=linear.weight.dtype, float8_dtype=float8_dtype, float_weight=linear.weight.data,
                 float_bias=None if linear.bias is None else linear.bias.data, input_float8_dtype=input_float8_dtype, scaling=scaling)
        f8.quantize_weight()
        return f8


def pow2_scale_reciprocal(amax: torch.Tensor, max_val: float = 448.0) -> torch.Tensor:
    """The smallest power of two ``2^e`` with ``amax / 2^e <= max_val``, fp32, elementwise (``amax == 0`` gives 1).  ``amax`` and
    ``max_val * 2^e`` are compared as they are, so the choice does not depend on how a logarithm rounds."""
    amax = amax.float()
    _, e = torch.frexp(amax / max_val)                      # amax / max_val = m * 2^e with m in [0.5, 1), up to one rounding
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    for _ in range(2):                                      # the rounding of the quotient can leave e one off, either way
        e = torch.where(amax > torch.ldexp(torch.full_like(amax, max_val), e), e + 1, e)
        e = torch.where((amax > 0) & (amax <= torch.ldexp(torch.full_like(amax, max_val), e - 1)), e - 1, e)
    return torch.ldexp(torch.ones_like(amax), e)


class W8Linear(nn.Module):
    """Weight-only fp8 linear layer (``mlp.fp8_weight_only``; not in the reference): ``weight`` ``[out, in]`` ``float8_e4m3fn``,
    ``scale_reciprocal`` fp32 -- ``[]`` (``scaling="tensor"``) or ``[out]`` (``scaling="row"``: one per output feature) --, an optional bias,
    bf16 activations.  The scales are POWERS OF TWO (``pow2_scale_reciprocal``), so ``weight.to(bf16) * scale_reciprocal`` is exact in bf16:
    the layer IS the bf16 linear layer over that widened weight, and ``forward`` computes it as such -- widening on every call, so that
    the weight costs one byte per element; no widened copy is kept.  With ``mlp.w8_stream_rows`` > 0 a bf16 GPU input of at most that many
    rows does not widen at all: ``ops.w8_linear`` streams the e4m3 weight once (``bf16(bf16(S * scale) + bias)``, fp32 sums).  As ``fc1`` of a ``SparseDiffMlp`` its sparse steps gather the e4m3
    rows themselves (``csp_mlp_mm1_w8``); as ``fc2`` under ``mlp.fp8_fc2`` (per tensor only) GEMM2 does (``csp_mlp_mm2_w8``)."""
    weight_only = True

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=torch.bfloat16,
                 scaling: str = "tensor") -> None:
        super().__init__()
        if scaling not in SCALINGS:
            raise ValueError(f"W8Linear: unknown scaling {scaling!r} (one of {', '.join(SCALINGS)})")
        self.scaling = scaling
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.zeros((out_features, in_features), dtype=torch.float8_e4m3fn, device=device), requires_grad=False)
        self.register_buffer("scale_reciprocal", torch.ones((out_features,) if scaling == "row" else (), dtype=torch.float32, device=device))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_features, dtype=dtype, device=device), requires_grad=False)
        else:
            self.register_parameter("bias", None)

    @property
    def scale(self) -> torch.Tensor:
        return self.scale_reciprocal.reciprocal()

    def widened(self) -> torch.Tensor:
        """``weight.to(bf16) * scale_reciprocal``: exact (every e4m3 value is a bf16 value, the scale a power of two).  A new tensor per call."""
        s = self.scale_reciprocal.to(torch.bfloat16)
        return self.weight.to(torch.bfloat16) * (s.unsqueeze(1) if s.dim() == 1 else s)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # few rows (mlp.w8_stream_rows): the e4m3 weight streamed once through ops.w8_linear, nothing widened in memory
        cap = int(amd_key("mlp", "w8_stream_rows"))
        if (cap > 0 and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() >= 1 and x.shape[-1] == self.in_features and x.stride(-1) == 1
                and self.in_features % 64 == 0 and self.out_features % 8 == 0 and 0 < x.numel() // self.in_features <= cap
                and (self.bias is None or self.bias.dtype == torch.bfloat16)):
            from .. import ops
            return ops.w8_linear(x, self.weight, self.scale_reciprocal, self.bias)
        w = self.widened()
        return torch.nn.functional.linear(x, w if x.dtype == w.dtype else w.to(x.dtype), self.bias)

    @classmethod
    def from_linear(cls, linear: nn.Linear, scaling: str = "tensor") -> "W8Linear":
        w = linear.weight.data
        q = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, device=w.device,
                dtype=w.dtype if linear.bias is None else linear.bias.dtype, scaling=scaling)
        wf = w.float()
        amax = wf.abs().amax(dim=1) if scaling == "row" else wf.abs().amax()
        recip = pow2_scale_reciprocal(amax, torch.finfo(torch.float8_e4m3fn).max)
        scaled = wf / (recip.unsqueeze(1) if scaling == "row" else recip)      # a division by a power of two: exact
        q.weight = nn.Parameter(scaled.to(torch.float8_e4m3fn), requires_grad=False)
        q.scale_reciprocal = recip
        if linear.bias is not None:
            q.bias = nn.Parameter(linear.bias.data, requires_grad=False)
        return q


@torch.inference_mode()
def recursive_swap_linears(model: nn.Module, float8_dtype=torch.float8_e4m3fn,
                           input_float8_dtype=torch.float8_e4m3fn, parent_name: Optional[str] = None,
                           quantize_modulation: bool = True, ignore_keys=("modulation",), scaling: Optional[str] = None) -> None:
    """Replace the ``nn.Linear`` children below ``model`` by ``F8Linear`` in place, with the reference's exclusions
    (mlp_fp8.py:295-350): children named in ``ignore_keys``, children whose name contains ``mod`` (the modulation
    layers -- skipped regardless of ``quantize_modulation``, exactly as the reference does), and ``fc2`` of a sparse
    image MLP (child ``"2"`` of an ``nn.Sequential`` named ``img_mlp``) while ``mlp.is_enabled``: the sparse step's
    GEMM2 gathers bf16 rows of ``fc2.weight.T``.  With ``mlp.fp8_fc2`` on (and e4m3 weights asked for) that ``fc2`` is swapped too:
    the sparse step's GEMM2 then gathers e4m3 rows (``csp_mlp_mm2_w8``).  ``scaling`` (default: the config key ``mlp.fp8_scaling``) is the
    layers' scale granularity; that ``fc2`` of a sparse image MLP is built per tensor whatever it says (GEMM2's gather takes one scale).
    With ``mlp.fp8_weight_only`` on, every layer that would become an ``F8Linear`` becomes a ``W8Linear`` instead (e4m3 weights with
    power-of-two scales, bf16 activations; ``input_float8_dtype`` is then not used): same exclusions, same rule for that ``fc2``."""
    from ..util.config import GLOBAL_CONFIG
    if scaling is None:
        scaling = amd_key("mlp", "fp8_scaling")
    if scaling not in SCALINGS:
        raise ValueError(f"recursive_swap_linears: mlp.fp8_scaling must be one of {', '.join(SCALINGS)} (got {scaling!r})")
    # mlp.fp8_weight_only: W8Linear in F8Linear's place -- same exclusions, same rule for fc2 of a sparse image MLP
    weight_only = bool(amd_key("mlp", "fp8_weight_only"))
    if weight_only and float8_dtype != torch.float8_e4m3fn:
        raise ValueError(f"recursive_swap_linears: mlp.fp8_weight_only builds float8_e4m3fn weights only (got float8_dtype {float8_dtype})")
    for name, child in list(model.named_children()):
        if name in ignore_keys or "mod" in name:
            continue
        sparse_fc2 = (isinstance(model, nn.Sequential) and str(name) == "2" and isinstance(child, nn.Linear)
                      and parent_name == "img_mlp" and GLOBAL_CONFIG["mlp"]["is_enabled"])
        if sparse_fc2 and not (amd_key("mlp", "fp8_fc2") and float8_dtype == torch.float8_e4m3fn):
            print("skipping fc2 of sparse img mlp")
            continue
        if isinstance(child, nn.Linear) and not isinstance(child, F8Linear):
            if weight_only:      # e4m3 weights with power-of-two scales, bf16 activations
                setattr(model, name, W8Linear.from_linear(child, scaling="tensor" if sparse_fc2 else scaling))
                continue
            setattr(model, name, F8Linear.from_linear(child, float8_dtype, input_float8_dtype,
                                                      scaling="tensor" if sparse_fc2 else scaling))
        else:
            recursive_swap_linears(child, float8_dtype, input_float8_dtype, name, quantize_modulation, ignore_keys, scaling)


@torch.inference_mode()
def quantize_fp8(flow_model: nn.Module, device=torch.device("cuda"), float8_dtype=torch.float8_e4m3fn,
                 input_float8_dtype=torch.float8_e4m3fn, quantize_modulation: bool = True, scaling: Optional[str] = None) -> nn.Module:
    """Move the transformer blocks to ``device`` one at a time and swap their linear layers to fp8 (reference
    mlp_fp8.py:352-400; called as ``quantize_fp8(model, device=device)`` by examples/flux/src/flux/util.py:350).
    The reference walks ``flow_model.double_blocks`` and ``.single_blocks``; a module without those attributes is
    treated as one block."""
    blocks = []
    for attr in ("double_blocks", "single_blocks"):
        if hasattr(flow_model, attr):
            blocks.extend(getattr(flow_model, attr))
    if not blocks:
        blocks = [flow_model]
    for module in blocks:
        module.to(device)
        module.eval()
        recursive_swap_linears(module, float8_dtype=float8_dtype, input_float8_dtype=input_float8_dtype,
                               quantize_modulation=quantize_modulation, scaling=scaling)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    return flow_model
