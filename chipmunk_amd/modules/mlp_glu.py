"""Sparse-delta layer for gated feed-forwards, ``fc2(act(gate_proj(x)) * up_proj(x))`` (SwiGLU / GEGLU; no reference counterpart: the
reference's ``SparseDiffMlp`` knows ``fc2(act(fc1(x)))`` only).  The state machine is ``SparseDeltaMlp`` of ``modules/mlp.py``; this file
holds what the gated layer adds to it.

The method carries over unchanged: a hidden column ``j`` is recomputed or kept as a whole, its activation-cache entry is the gated product,
and GEMM2 and the scatter-add see the same packed deltas as in ``SparseDiffMlp``.  Only GEMM1 differs (``csp_mlp_mm1_glu``: two gathered
weight rows per kept column) and the movement of a column is the movement of its two inputs: the block means of BOTH pre-activations are
cached as one ``[B, 2 Gm, F]`` tensor (rows ``2i`` / ``2i + 1`` = gate / up means of block ``i``) and the score of a column in a group is
the sum of ``|delta block mean|`` over the group's rows of that tensor -- ``select_columns`` with ``R = 2 bm / mbm`` rows per group.

fp8 projections (``F8Linear``: two layers, or one fused ``[2F, K]`` layer) take ``csp_mlp_mm1_glu_fp8`` on the sparse steps: ``x`` is quantised
ONCE, with the gate projection's (or the fused projection's) ``quantize_input``, and the kernel multiplies both sums by that layer's
``input_scale_reciprocal`` and each by its own layer's ``scale_reciprocal``.  Dequantising with the gate's input scale is exact arithmetic for
both products -- the e4m3 values ARE ``x * input_scale`` rounded, whichever weight they meet -- so the up layer's own input scale is used only
by its dense forward (full steps, the block means of the selection), which is also what calibrates it.

Weight-only fp8 projections (``W8Linear``: two layers, or one fused ``[2F, K]`` layer; per-tensor or per-row scales) are taken with
``mlp.w8_gated`` on and run ``csp_mlp_mm1_glu_w8`` on the sparse steps: ``x`` stays bf16, GEMM1 gathers e4m3 rows of both weights and
multiplies each branch's sum by its layer's ``scale_reciprocal`` (a fused layer's ``[2F]`` scale is split like its weight, a ``[]`` scale
serves both halves).  Dense and full steps and the block-mean probe call the layers' own forward -- the bf16 linear layer over the widened
weight, or ``ops.w8_linear`` for few rows under ``mlp.w8_stream_rows`` --, a fused layer once, its output split.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import ops
from ..util.config import amd_key
from ..util.layer_counter import LayerCounter
from ..util.storage import MlpStorage
from .mlp import _F8, SparseDeltaMlp, activation_code, check_fc2, fc2_scale_of


def _params(lin: torch.nn.Linear, rows: Optional[slice] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(weight, bias | None) of a Linear as it is NOW (``model.to(...)`` rebinds ``param.data``), optionally a slice of its output rows"""
    w, b = lin.weight.data, None if lin.bias is None else lin.bias.data
    return (w, b) if rows is None else (w[rows], None if b is None else b[rows])


class SparseDiffGatedMlp(SparseDeltaMlp):
    """``gate_proj`` / ``up_proj`` / ``fc2``: ``nn.Linear`` with or without bias, bf16 for the sparse steps; or ``gate_proj`` / ``up_proj``
    (or the fused ``fc1``) BOTH ``F8Linear`` with e4m3 weights and e4m3 inputs (``input_float8_dtype=torch.float8_e4m3fn``;
    ``F8Linear.from_linear`` defaults to e5m2, which the kernel does not read); or, with ``mlp.w8_gated`` on, BOTH ``W8Linear`` (weight-only
    e4m3, bf16 inputs; a fused ``W8Linear`` likewise).  ``fc2`` is bf16 (GEMM2 gathers bf16 rows) or, with
    ``mlp.fp8_fc2`` on, an ``F8Linear`` with e4m3 weights (GEMM2 gathers e4m3 rows, ``fc2.scale_reciprocal`` on its sums).
    Their parameters are read at every call, so the model may be moved or cast after wrapping.  The sparse steps select columns with
    ``topk_indices``, which takes rows of 1024 columns or more: the hidden width ``F`` must be at least 1024."""
    _who = "SparseDiffGatedMlp"

    def __init__(self, layer_num: int, layer_counter: LayerCounter, gate_proj: torch.nn.Linear, up_proj: torch.nn.Linear,
                 activation: torch.nn.Module, fc2: torch.nn.Linear, heuristic_sms_scatter_add: int = 6):
        self._init(layer_num, layer_counter, [gate_proj, up_proj], None, activation, fc2, heuristic_sms_scatter_add)

    @classmethod
    def from_fused(cls, layer_num: int, layer_counter: LayerCounter, fc1: torch.nn.Linear, activation: torch.nn.Module,
                   fc2: torch.nn.Linear, gate_first: bool = True, heuristic_sms_scatter_add: int = 6) -> "SparseDiffGatedMlp":
        """One ``[2F, K]`` projection whose output is split in two halves: ``gate_first`` says which half is the gate.  The halves are
        used as views of ``fc1``'s parameters, nothing is copied."""
        f2 = fc1.weight.shape[0]
        if f2 % 2:
            raise ValueError(f"SparseDiffGatedMlp.from_fused: fc1 has {f2} output features, not two halves")
        self = cls.__new__(cls)
        self._init(layer_num, layer_counter, [fc1], gate_first, activation, fc2, heuristic_sms_scatter_add)
        return self

    def _init(self, layer_num, layer_counter, projs, gate_first, activation, fc2, heuristic_sms_scatter_add):
        self.act_code = activation_code(activation)      # raises for an activation the sparse steps could not honour
        self.projs = projs              # (lists keep the Linear modules out of any parent nn.Module's parameter registry)
        self.gate_first = gate_first    # None: two projections; True / False: the halves of projs[0], and which of them is the gate
        gate, up = self.gate, self.up
        if gate[0].shape != up[0].shape or gate[0].ndim != 2:
            raise ValueError(f"SparseDiffGatedMlp: gate and up projections must have one shape [F, K] (got {tuple(gate[0].shape)} and "
                             f"{tuple(up[0].shape)})")
        if fc2.weight.shape[1] != gate[0].shape[0]:
            raise ValueError(f"SparseDiffGatedMlp: fc2 takes {fc2.weight.shape[1]} features, the projections give {gate[0].shape[0]}")
        w8 = [bool(getattr(p, "weight_only", False)) for p in projs]
        if any(w8) and not amd_key("mlp", "w8_gated"):
            raise ValueError("SparseDiffGatedMlp: a W8Linear projection (weight-only fp8, mlp.fp8_weight_only) is refused: only the ungated "
                             "GEMM1 has a weight-only form (csp_mlp_mm1_w8) unless mlp.w8_gated is on -- set it to run the gated weight-only "
                             "GEMM1 (csp_mlp_mm1_glu_w8), or keep the gate and up projections in bf16, or build them as F8Linear")
        if any(w8) != all(w8):
            raise ValueError("SparseDiffGatedMlp: a mixed pair -- one projection is a W8Linear (weight-only fp8), the other is not; the "
                             "gated weight-only GEMM1 takes both projections as W8Linear")
        self.w8 = all(w8)               # weight-only e4m3 projections: x stays bf16 (csp_mlp_mm1_glu_w8)
        for p in projs if self.w8 else ():
            if p.weight.dtype != torch.float8_e4m3fn:
                raise ValueError(f"SparseDiffGatedMlp: the gated weight-only GEMM1 reads float8_e4m3fn weights only (got {p.weight.dtype})")
        f8 = [p.weight.dtype in _F8 and not self.w8 for p in projs]
        if any(f8) != all(f8):
            raise ValueError("SparseDiffGatedMlp: a mixed pair -- one projection is fp8, the other is not; the gated GEMM1 takes both "
                             "projections in bf16 or both as F8Linear")
        self.fp8 = all(f8)
        for p in projs if self.fp8 else ():
            if p.weight.dtype != torch.float8_e4m3fn or getattr(p, "input_float8_dtype", None) != torch.float8_e4m3fn:
                raise ValueError(f"SparseDiffGatedMlp: the gated fp8 GEMM1 reads float8_e4m3fn weights and inputs only (got weight "
                                 f"{p.weight.dtype}, input_float8_dtype {getattr(p, 'input_float8_dtype', None)}); build the projection with "
                                 "F8Linear.from_linear(..., input_float8_dtype=torch.float8_e4m3fn)")
            if getattr(p, "scaling", "tensor") != "tensor":
                raise ValueError("SparseDiffGatedMlp: a row-scaled projection (F8Linear scaling='row', mlp.fp8_scaling: row) is refused: the "
                                 "gated fp8 GEMM1 takes one scale per tensor; build the gate and up projections with scaling='tensor'")
        check_fc2("SparseDiffGatedMlp", fc2)    # bf16, or an e4m3 F8Linear with mlp.fp8_fc2 on
        self.fc2 = [fc2]
        self._fc2w_T = None             # ((address, dtype, device) of the fc2.weight it was made from, its transpose)
        self.layer_counter = layer_counter
        self.activation = activation
        self.storage = MlpStorage(layer_num)
        self.num_sms_scatter_add = heuristic_sms_scatter_add

    def _half(self, which: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """which = 0: the gate projection's (weight, bias), 1: the up projection's"""
        if self.gate_first is None:
            return _params(self.projs[which])
        f = self.projs[0].weight.shape[0] // 2
        first = which == (0 if self.gate_first else 1)
        return _params(self.projs[0], slice(0, f) if first else slice(f, 2 * f))

    @property
    def gate(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        return self._half(0)

    @property
    def up(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        return self._half(1)

    @property
    def w8_scales(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(gate, up) ``scale_reciprocal`` of ``W8Linear`` projections as they are NOW: each layer's own, or -- a fused layer -- the halves
        of its ``[2F]`` scale as views, split like the weight; a ``[]`` scale serves both halves"""
        if self.gate_first is None:
            return self.projs[0].scale_reciprocal, self.projs[1].scale_reciprocal
        s = self.projs[0].scale_reciprocal
        if s.dim() == 0:
            return s, s
        f = s.shape[0] // 2
        first, second = s[:f], s[f:]
        return (first, second) if self.gate_first else (second, first)

    @property
    def fc2w_T(self) -> torch.Tensor:
        """fc2.weight^T, contiguous ``[F, C]``: made once per weight tensor (again after the module was moved or cast)"""
        w = self.fc2[0].weight.data
        key = (w.data_ptr(), w.dtype, w.device)
        if self._fc2w_T is None or self._fc2w_T[0] != key:
            self._fc2w_T = (key, w.transpose(0, 1).contiguous())
        return self._fc2w_T[1]

    def _pre(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.fp8 or self.w8:   # the projections' own forward (F8Linear: torch._scaled_mm, which also feeds their input-scale calibration)
            if self.gate_first is None:
                return self.projs[0](x), self.projs[1](x)
            first, second = self.projs[0](x).chunk(2, dim=-1)   # one call of the fused projection, its output split
            return (first, second) if self.gate_first else (second, first)
        return torch.nn.functional.linear(x, *self.gate), torch.nn.functional.linear(x, *self.up)

    @staticmethod
    def _paired_block_means(g: torch.Tensor, u: torch.Tensor, rows: int) -> torch.Tensor:
        """[B, Gm, F] gate and up block means -> [B, 2 * rows, F], rows 2i / 2i + 1 = gate / up of block i (zero rows behind the Gm blocks
        present, so that every 128-row group owns the same number of rows)."""
        pair = torch.stack([g, u], dim=2)
        if pair.shape[1] < rows:
            pair = torch.nn.functional.pad(pair, (0, 0, 0, 0, 0, rows - pair.shape[1]))
        return pair.reshape(pair.shape[0], 2 * rows, pair.shape[-1]).contiguous()

    def _act(self, g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        return self.activation(g) * u

    def _check_config(self, cfg) -> None:
        assert cfg["bm"] % cfg["mbm"] == 0, "mlp.bm must be a multiple of mlp.mbm"

    def _layout(self, means, n: int, cfg) -> Tuple[torch.Tensor, int]:
        # a column's movement is the movement of its two inputs: |delta| summed over the group's 2 r rows (gate and up means)
        bm, r = cfg["bm"], cfg["bm"] // cfg["mbm"]         # r: block means per 128-row group and branch
        return self._paired_block_means(*means, (n + bm - 1) // bm * r), 2 * r

    def _sparse(self, x, batched, indices, counts, sparse_act_T, out_cache) -> None:
        gate, up = self.gate, self.up
        if self.fp8:
            qgate, qup = self.projs[0], self.projs[-1]     # (the same layer twice for a fused projection)
            xq = qgate.quantize_input(x)                   # once, with the gate's input scale: see the module docstring
            ops.mlp_glu_fp8(x=xq if batched else xq[0], w_gate=gate[0], w_up=up[0], b_gate=gate[1], b_up=up[1],
                            act=self.act_code, fc2w_T=self.fc2w_T, indices=indices, counts=counts, sparse_act_T=sparse_act_T,
                            cached_out=out_cache, num_sms_scatter_add=self.num_sms_scatter_add,
                            scale_a=qgate.input_scale_reciprocal, scale_b_gate=qgate.scale_reciprocal, scale_b_up=qup.scale_reciprocal,
                            fc2_scale=fc2_scale_of(self.fc2[0]))
        elif self.w8:
            scale_gate, scale_up = self.w8_scales
            ops.mlp_glu_w8(x=x if batched else x[0], w_gate=gate[0], w_up=up[0], scale_gate=scale_gate, scale_up=scale_up, b_gate=gate[1],
                           b_up=up[1], act=self.act_code, fc2w_T=self.fc2w_T, indices=indices, counts=counts, sparse_act_T=sparse_act_T,
                           cached_out=out_cache, num_sms_scatter_add=self.num_sms_scatter_add, fc2_scale=fc2_scale_of(self.fc2[0]))
        else:
            ops.mlp_glu(x=x if batched else x[0], w_gate=gate[0], w_up=up[0], b_gate=gate[1], b_up=up[1],
                        act=self.act_code, fc2w_T=self.fc2w_T, indices=indices, counts=counts, sparse_act_T=sparse_act_T,
                        cached_out=out_cache, num_sms_scatter_add=self.num_sms_scatter_add, fc2_scale=fc2_scale_of(self.fc2[0]))
