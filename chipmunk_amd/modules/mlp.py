"""Sparse-delta MLP layer state machine (mirror of reference ``src/chipmunk/modules/mlp.py:11-123``): ``SparseDeltaMlp``, once, for
``SparseDiffMlp`` below and for the gated ``SparseDiffGatedMlp`` of ``modules/mlp_glu.py``, with the column selection (``select_columns``).

Full step: dense ``fc2(act(fc1(x)))``; cache the transposed activations (column-major ``[F, M]``), the output and the
128-row block means of the fc1 output.  Sparse step: pick, per 128-row group, the fc1 columns whose block mean moved
most since they were last computed (``topk_indices`` on |delta|), recompute only those columns (``csp_mlp_mm1``),
scatter the activation deltas into the cache and add ``delta @ fc2^T`` onto the cached output
(``csp_mlp_mm2_and_scatter_add``).  The fc2 bias is already inside the cached output.

An e4m3 ``fc1`` built with row scaling (``F8Linear(scaling="row")``, config key ``mlp.fp8_scaling``) quantises the sparse steps' input with
one dynamic scale per token (``fc1.quantize_input_rowwise``) and hands GEMM1 the ``[N]`` row scales with the ``[F]`` weight scales
(``csp_mlp_mm1_fp8_act_rs``); everything else on the route is unchanged.

``fc2`` is bf16, or -- with ``mlp.fp8_fc2`` on -- an ``F8Linear`` with e4m3 weights: dense and full steps call its forward as it is
(``torch._scaled_mm``), the sparse steps gather e4m3 rows of ``fc2.weight^T`` (``csp_mlp_mm2_w8``) with ``fc2.scale_reciprocal``.

A weight-only ``fc1`` (``W8Linear``, ``mlp.fp8_weight_only``: e4m3 weight, power-of-two scales, bf16 activations) keeps ``x`` in bf16: dense and
full steps and the block-mean probe call its forward (the bf16 linear layer over the widened weight), the sparse steps gather e4m3 rows of
``fc1.weight`` (``csp_mlp_mm1_w8``) with ``fc1.scale_reciprocal``.  A ``W8Linear`` ``fc2`` (per tensor) is taken under ``mlp.fp8_fc2`` like an ``F8Linear``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops
from ..util.config import GLOBAL_CONFIG, amd_key
from ..util.layer_counter import LayerCounter
from ..util.storage import MlpStorage


def block_mean(x: torch.Tensor, mbm: int) -> torch.Tensor:
    """[b, n, c] -> [b, ceil(n/mbm), c] mean over consecutive row blocks (reference modules/mlp.py:11-16).  bf16 GPU tensors take the
    one-pass kernel (``mlp.fused_block_mean``: fp32 sums, one rounding -- torch's reduction in another summation order).  A ragged last
    block (``n % mbm != 0``; the reference has none) is the mean over the rows present."""
    b, n, c = x.shape
    if (x.is_cuda and x.dtype == torch.bfloat16 and mbm % 4 == 0 and c % 8 == 0
            and b * ((n + mbm - 1) // mbm) < 65536       # the kernel's row blocks ride on grid.y
            and amd_key("mlp", "fused_block_mean")):
        return torch.ops.chipmunk.block_mean(x, mbm)
    full = n // mbm * mbm
    out = x[:, :full].reshape(b, n // mbm, mbm, c).mean(dim=2)
    if full < n:
        out = torch.cat([out, x[:, full:].mean(dim=1, keepdim=True)], dim=1)
    return out


def _ceil8(n: int) -> int:
    return (n + 7) // 8 * 8


def _transposed_pitched(x: torch.Tensor, ld: int) -> torch.Tensor:
    """[..., R, C] -> [..., C, ld] with ``[..., :R]`` the transpose and zeros behind it: the activation cache at a column pitch the
    sparse-MLP operators accept for a token count that is not a multiple of 8 (``ld >= R``, ``ld % 8 == 0``)."""
    if x.is_cuda and x.element_size() == 2:
        return torch.ops.chipmunk.transpose_last2_pitched(x, ld)
    out = x.new_zeros(x.shape[:-2] + (x.shape[-1], ld))
    out[..., : x.shape[-2]] = x.transpose(-1, -2)
    return out


def _transposed(x: torch.Tensor) -> torch.Tensor:
    """``x.transpose(-1, -2).contiguous()``; one HBM-rate kernel for 16-bit GPU tensors."""
    if x.is_cuda and x.element_size() == 2:
        return torch.ops.chipmunk.transpose_last2(x)
    return x.transpose(-1, -2).contiguous()


CACHE_LAYOUTS = ("column", "group")


def _to_groups(x: torch.Tensor) -> torch.Tensor:
    """[..., N, F] -> [..., ceil(N/128), F, 128]: element (g, f, r) is column f of token g * 128 + r, the rows of the last group at or past
    N zero -- the group-major activation cache.  One HBM-rate kernel for 16-bit GPU tensors, plain torch otherwise."""
    if x.is_cuda and x.element_size() == 2:
        return torch.ops.chipmunk.transpose_to_groups(x)
    n, f = x.shape[-2:]
    g = (n + 127) // 128
    padded = torch.nn.functional.pad(x, (0, 0, 0, g * 128 - n))
    return padded.reshape(x.shape[:-2] + (g, 128, f)).transpose(-1, -2).contiguous()


def activation_cache_of(who: str, act: torch.Tensor) -> torch.Tensor:
    """The activation cache a full step stores for ``act`` ``[B, N, F]``, in the layout ``mlp.cache_layout`` names at that moment:
    ``"column"`` -- ``[B, F, ceil8(N)]`` with zeroed padding (``[B, F, N]``, the reference's contiguous cache, for every N % 8 == 0) --
    or ``"group"`` -- ``[B, ceil(N/128), F, 128]``.  Stored (and offloaded) whole either way."""
    layout = amd_key("mlp", "cache_layout")
    if layout not in CACHE_LAYOUTS:
        raise ValueError(f"{who}: mlp.cache_layout must be one of {', '.join(CACHE_LAYOUTS)} (got {layout!r})")
    if layout == "group":
        return _to_groups(act)
    n = act.shape[1]
    return _transposed(act) if n % 8 == 0 else _transposed_pitched(act, _ceil8(n))


def activation_cache_view(stored: torch.Tensor, n: int, batched: bool) -> torch.Tensor:
    """What the sparse-MLP operators take of the stored activation cache, by its rank: a group-major ``[B, G, F, 128]`` whole (its
    ``[G, F, 128]`` block for one sequence), of a column-major ``[B, F, ld]`` the ``[F, N]`` view of the pitched columns."""
    if stored.ndim == 4:
        return stored if batched else stored[0]
    return stored[..., :n] if batched else stored[0][:, :n]


_F8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def check_fc2(who: str, fc2: torch.nn.Module) -> None:
    """An fp8 ``fc2`` is taken with ``mlp.fp8_fc2`` on, as an ``F8Linear`` with e4m3 weights: the sparse steps' GEMM2 then gathers e4m3
    rows of ``fc2.weight^T`` and multiplies its sums by ``fc2.scale_reciprocal``.  A ``W8Linear`` (weight-only, per tensor) carries the
    same attributes and is taken the same way.  Everything else raises at construction."""
    if fc2.weight.dtype not in _F8:
        return
    if not amd_key("mlp", "fp8_fc2"):
        raise ValueError(f"{who}: fc2 must stay bf16 (GEMM2 gathers bf16 rows of fc2.weight^T); an fp8 fc2 is refused unless the config "
                         "key mlp.fp8_fc2 is on")
    if fc2.weight.dtype != torch.float8_e4m3fn or getattr(fc2, "scale_reciprocal", None) is None:
        raise ValueError(f"{who}: with mlp.fp8_fc2 the fp8 fc2 must be an F8Linear with float8_e4m3fn weights and their scale_reciprocal "
                         f"(got weight {fc2.weight.dtype}); e5m2 weights are refused")
    if getattr(fc2, "scaling", "tensor") != "tensor" or fc2.scale_reciprocal.numel() != 1:
        raise ValueError(f"{who}: a row-scaled fc2 (F8Linear scaling='row': one scale per output feature) is refused: GEMM2's weight-only "
                         "gather takes one scale per tensor; build fc2 with scaling='tensor' (recursive_swap_linears does, whatever "
                         "mlp.fp8_scaling says)")


def fc2_scale_of(fc2: torch.nn.Module):
    """``fc2.scale_reciprocal`` for an e4m3 ``fc2``, ``None`` for a bf16 one"""
    return fc2.scale_reciprocal if fc2.weight.dtype == torch.float8_e4m3fn else None


def top_p_of(who: str, cfg) -> tuple:
    """(``mlp.top_p``, ``mlp.top_p_min_keys``) of a step that makes a selection; ``top_p`` 0.0 when the per-group count is off (the
    ``top_keys`` selection, untouched).  On: a 128-row group keeps the columns that carry the share ``top_p`` of its |block-mean delta|
    mass, a subset of what ``top_keys`` keeps, and at least the sampled ``top_p_min_keys`` quantile (``ops.topk_indices_p``)."""
    top_p = float(amd_key("mlp", "top_p"))
    if top_p == 0.0:
        return 0.0, 0.0
    min_keys = float(amd_key("mlp", "top_p_min_keys"))
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"{who}: mlp.top_p must be in [0, 1] (got {top_p})")
    if not 0.0 <= min_keys <= cfg["top_keys"]:
        raise ValueError(f"{who}: mlp.top_p_min_keys must be in [0, mlp.top_keys] (got {min_keys} with top_keys {cfg['top_keys']})")
    return top_p, min_keys


def activation_code(activation: torch.nn.Module, who: str = "SparseDiffGatedMlp", what: str = "the gated GEMM1") -> str:
    """The GEMM1 kernels' name for an activation module (one of ``ops.mlp.GLU_ACTS``); anything the kernels do not compute raises."""
    if isinstance(activation, torch.nn.SiLU):
        return "silu"
    if isinstance(activation, torch.nn.GELU) and activation.approximate in ("tanh", "none"):
        return "gelu_tanh" if activation.approximate == "tanh" else "gelu"
    raise ValueError(f"{who}: unsupported activation {activation!r}: {what} computes nn.SiLU(), "
                     "nn.GELU(approximate='tanh') and nn.GELU() only")


def select_route(is_cuda: bool, contiguous: bool, R: int, fused_single: bool, fused_group: bool) -> str:
    """How a sparse step selects its columns from ``R`` block-mean rows per 128-row group: ``"single"`` -- one kernel for
    ``|pre - cache|`` -> top-k indices -> copy of the selected columns into the cache (``R == 1``, ``mlp.fused_topk_delta``) -- ``"group"`` --
    the same over the ``R`` rows of a group (``R > 1``, ``mlp.fused_group_topk_delta``) -- or ``"chain"``, those steps as separate
    operators.  The kernels take contiguous GPU tensors; everything else, every CPU tensor included, is the chain."""
    if is_cuda and contiguous and (fused_single if R == 1 else fused_group):
        return "single" if R == 1 else "group"
    return "chain"


def _topk(plain, with_top_p, operands: tuple, cfg, top_p: float, min_keys: float) -> None:
    """``plain`` with the ``top_keys`` selection or, when ``mlp.top_p`` is set, its ``_p`` sibling with ``top_keys`` as the cap"""
    if top_p > 0.0:
        with_top_p(*operands, 1 - cfg["top_keys"], top_p, min_keys, cfg["counts_multiple_of"], cfg["random_keys"])
    else:
        plain(*operands, 1 - cfg["top_keys"], cfg["counts_multiple_of"], cfg["random_keys"])


def select_columns(pre: torch.Tensor, cache: torch.Tensor, R: int, cfg, top_p: float, min_keys: float) -> tuple:
    """(indices ``[B, G, F]``, counts ``[B, G]``) of the columns whose block means ``pre`` ``[B, rows, F]`` moved most against ``cache``,
    summed over the ``R`` rows of each of the ``G = ceil(rows / R)`` groups; the listed columns of ``cache`` are refreshed in place.  A
    ragged last group sums and refreshes the rows it has."""
    b, rows, f = pre.shape
    groups = (rows + R - 1) // R
    route = select_route(pre.is_cuda, pre.is_contiguous(), R, amd_key("mlp", "fused_topk_delta"), amd_key("mlp", "fused_group_topk_delta"))
    inds = torch.empty((b, groups, f), dtype=torch.int32, device=pre.device)
    counts = torch.empty((b, groups), dtype=torch.int32, device=pre.device)
    if route == "single":
        _topk(torch.ops.chipmunk.topk_delta_indices, ops.topk_delta_indices_p, (pre, cache, inds, counts), cfg, top_p, min_keys)
    elif route == "group":
        _topk(ops.topk_group_delta_indices, ops.topk_group_delta_indices_p, (pre, cache, inds, counts, R), cfg, top_p, min_keys)
    else:
        mdiff = (pre - cache).abs()
        if rows % R:   # ragged last group: it sums the blocks it has
            mdiff = torch.nn.functional.pad(mdiff, (0, 0, 0, R - rows % R))
        mdiff = mdiff.reshape(b, groups, R, f).sum(dim=2)
        _topk(ops.topk_indices, ops.topk_indices_p, (mdiff, inds, counts), cfg, top_p, min_keys)
        ops.copy_indices(pre, cache, inds, counts)       # rows [R g, R (g + 1)) take group g's list
    return inds, counts


def _host_copy_follows(holder) -> None:
    """The LOADED tensor of ``holder`` was updated in place.  When it lives in host memory (offloading on, not kept resident) the host copy
    has to follow, or the next load brings back the tensor of the last full step: the next selection is then made against stale block
    means, the next deltas are taken against activations the output cache has long moved on from."""
    if holder is not None and not holder.is_resident():
        holder.offload_cur_value()


class SparseDeltaMlp:
    """The state machine of both sparse MLP layers: dense layers, full steps, sparse steps and the cached selection.  A layer is this
    class plus what differs between ``fc2(act(fc1(x)))`` and the gated ``fc2(act(gate(x)) * up(x))``: ``_pre`` (the pre-activations of
    ``x``, a tuple), ``_act`` (the activation they become), ``_layout`` (their block means as the selection and the cache take them, and
    the rows ``R`` a 128-row group owns there), ``_sparse`` (the operator call of a sparse step) and ``_check_config``.  It reads
    ``fc2`` (a one-element list), ``layer_counter`` and ``storage`` of the layer, and ``_who``, its name in messages."""
    _who = ""

    def _check_config(self, cfg) -> None:
        """what the layer asserts of ``GLOBAL_CONFIG["mlp"]`` at every call with the method enabled (here: nothing)"""

    def _dense(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc2[0](self._act(*self._pre(x)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        cfg = GLOBAL_CONFIG["mlp"]
        if not cfg["is_enabled"]:
            return self._dense(x)

        top_p, min_keys = top_p_of(self._who, cfg)     # (0.0, 0.0) unless mlp.top_p is set: top_keys is then only the cap
        do_full = self.layer_counter.should_do_full_mlp_step()
        inference_step, layer, _submodule = self.layer_counter.increment()
        assert x.ndim == 3 and x.shape[0] >= 1, "x must be (B, N, C)"
        mbm = cfg["mbm"]
        self._check_config(cfg)

        if layer < cfg["first_n_dense_layers"]:
            return self._dense(x)

        n = x.shape[1]
        if do_full:
            pre = self._pre(x)
            act = self._act(*pre)
            out = self.fc2[0](act)
            # the module owns the activation cache: [B, F, ld] with ld = ceil8(N) and zeroed padding, stored (and offloaded) whole; the
            # operators get its [F, N] view ([B, F, N] for a batch).  ld == N for every N % 8 == 0: the contiguous cache of the reference.
            # (mlp.cache_layout "group": [B, ceil(N/128), F, 128] instead, handed to the operators whole)
            self.storage.set_sparse_act_T(activation_cache_of(self._who, act))
            self.storage.set_out_cache(out)
            self.storage.set_blockmean_mid_cache(self._layout([block_mean(p, mbm) for p in pre], n, cfg)[0])
            return out

        # the stored state (activation cache [B, F, ld], output cache [B, N, C], block means, indices [B, G, F], counts [B, G]) is per
        # sequence: a sparse step continues the B sequences of the last full step and nothing else
        stored = self.storage.get_out_cache()
        if stored is None or stored.shape[0] != x.shape[0] or stored.shape[1] != n:
            raise RuntimeError(
                f"{self._who}: a sparse step got x of shape {tuple(x.shape)} but the state of the last full step is for "
                f"{'no input at all' if stored is None else f'batch size {stored.shape[0]} with {stored.shape[1]} tokens'}: the batch size "
                "and token count may only change on a full step")

        reuse_mask = (inference_step % cfg["block_mask_cache"] != 0 and inference_step >= 10
                      and self.storage.get_indices() is not None)
        if not reuse_mask:
            pre, R = self._layout(self._pre(block_mean(x, mbm)), n, cfg)
            inds, counts = select_columns(pre, self.storage.get_blockmean_mid_cache(), R, cfg, top_p, min_keys)
            _host_copy_follows(self.storage.blockmean_mid_cache)
            self.storage.set_indices(inds)
            self.storage.set_counts(counts)
        else:
            inds, counts = self.storage.get_indices(), self.storage.get_counts()

        # (a step that made the selection uses it as it made it: read back through the storage, a selection that was just sent to the host
        # -- offloading["mlp.indices"] -- is not what the getter shows, which is the pipeline slot as last loaded)
        batched = x.shape[0] > 1     # B == 1 passes the 2-D operands it always passed
        out_cache = stored if batched else stored[0]
        # (the [F, N] view of the pitched cache, or the group-major cache whole: the stored tensor's rank decides, not the config key)
        sparse_act_T = activation_cache_view(self.storage.get_sparse_act_T(), n, batched)
        self._sparse(x, batched, inds if batched else inds[0], counts if batched else counts[0], sparse_act_T, out_cache)
        _host_copy_follows(self.storage.sparse_act_T)

        if not batched:
            out_cache = out_cache.unsqueeze(0)
        self.storage.set_out_cache(out_cache)
        return out_cache

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


class SparseDiffMlp(SparseDeltaMlp):
    """``fc2(activation(fc1(x)))``.  The sparse steps recompute ``activation`` inside GEMM1, so it has to be one the kernel knows:
    ``nn.GELU(approximate="tanh")`` (the reference's), ``nn.GELU()`` (exact, erf) or ``nn.SiLU()``, subclasses included; for any other
    callable that computes one of the three, ``act`` names it (``"gelu_tanh"``, ``"gelu"``, ``"silu"``).  Everything else raises at
    construction: its sparse steps would subtract another function from the activation cache than the full steps put there.
    ``fc1`` may have no bias (``nn.Linear(..., bias=False)``, or an e4m3 ``F8Linear`` without one)."""
    _who = "SparseDiffMlp"

    def __init__(self, layer_num: int, layer_counter: LayerCounter, fc1: torch.nn.Linear,
                 activation: torch.nn.Module, fc2: torch.nn.Linear, heuristic_sms_scatter_add: int = 6, act: Optional[str] = None):
        # lists keep the Linear modules out of any parent nn.Module's parameter registry (reference mlp.py:21-23)
        check_fc2("SparseDiffMlp", fc2)
        if act is not None:
            if act not in ops.GLU_ACTS:
                raise ValueError(f"SparseDiffMlp: unknown act {act!r} (one of {', '.join(ops.GLU_ACTS)})")
            self.act_code = act
        else:
            try:
                self.act_code = activation_code(activation, "SparseDiffMlp", "GEMM1")
            except ValueError as e:
                raise ValueError(f"{e}; for another callable that computes one of them pass act='gelu_tanh', 'gelu' or 'silu'") from None
        self.fc1 = [fc1]
        self.fc2 = [fc2]
        self.fc2w_T = [fc2.weight.data.transpose(0, 1).contiguous()]
        self.layer_counter = layer_counter
        self.activation = activation
        self.storage = MlpStorage(layer_num)
        self.num_sms_scatter_add = heuristic_sms_scatter_add

    def _pre(self, x: torch.Tensor) -> tuple:
        return (self.fc1[0](x),)

    def _act(self, mid: torch.Tensor) -> torch.Tensor:
        return self.activation(mid)

    def _layout(self, means, n: int, cfg) -> tuple:
        return means[0], cfg["bm"] // cfg["mbm"]

    def _sparse(self, x, batched, indices, counts, sparse_act_T, out_cache) -> None:
        fc1, fc2 = self.fc1[0], self.fc2[0]
        scale_a = scale_b = fc1_scale = None
        if getattr(fc1, "weight_only", False):                  # W8Linear: x stays bf16, GEMM1 gathers e4m3 rows of fc1.weight
            fc1_scale = fc1.scale_reciprocal                    # one number, or one per fc1 column: [F]
        elif fc1.weight.dtype == torch.float8_e4m3fn and getattr(fc1, "scaling", "tensor") == "row":
            x, scale_a = fc1.quantize_input_rowwise(x)          # one reciprocal scale per token: [B, N]
            scale_a = scale_a if batched else scale_a[0]
            scale_b = fc1.scale_reciprocal.view(-1)             # one per fc1 column: [F]
        elif fc1.weight.dtype == torch.float8_e4m3fn:
            x = fc1.quantize_input(x)
            scale_a, scale_b = fc1.input_scale_reciprocal, fc1.scale_reciprocal

        ops.mlp(x=x if batched else x[0], fc1w=fc1.weight.data, fc1b=None if fc1.bias is None else fc1.bias.data,
                fc2w_T=self.fc2w_T[0], indices=indices, counts=counts, sparse_act_T=sparse_act_T, cached_out=out_cache,
                num_sms_scatter_add=self.num_sms_scatter_add, mm1_scale_a=scale_a, mm1_scale_b=scale_b, fc2_scale=fc2_scale_of(fc2),
                act=self.act_code, **({} if fc1_scale is None else {"fc1_scale": fc1_scale}))
