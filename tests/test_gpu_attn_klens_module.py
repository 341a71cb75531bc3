"""``SparseDiffAttn.forward(q, k, v, k_lens)`` over a padded batch: dense step 0, mask step 1, two sparse steps with
perturbed inputs; a 4 x 6 x 8 video plus 64 text rows (two 192-row groups, the second ragged), ``k_lens = [N, N - 40]``; both index
styles (bit-packed mask / ``torch.topk`` rows), the fused paths on and off.

* K and V hold NaN at and past each sequence's length in every call (N = 256 takes the general kernels: no row there may be read),
  so a padding key in any dense pass or gathered step shows; the references are computed from the clean tensors;
* the stored mask has no bit, the stored ``torch.topk`` rows no index, at or past a sequence's length;
* every full-step output is within ``ROW_ERR_BOUND`` of fp64 attention over the valid keys;
* every sparse-step output is within the module tolerance of DESIGN 2 (6e-3 + 2e-2 |ref|) of
  ``dense(step 1) - sparse(step 1) + sparse(now)``, all three in fp64, the sparse ones over the module's own stored selection
  (its index rows, each row's count capped at the sequence's length as the module caps it);
* without ``k_lens`` the layer is the layer it was: equal bits to an instance that is never given the argument."""
import os

import pytest
import torch

from helpers import assert_rows_close, attn_exact
from method_model import AMD_ATTN_KEYS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, VID, TXT = 2, 2, (4, 6, 8), 64
N = VID[0] * VID[1] * VID[2] + TXT
LENS = [N, N - 40]
STEPS = 4


def _configure(cfg, compress, fused):
    from chipmunk_amd.util import config as cfgmod
    cfgmod.load_from_file(os.path.join(ROOT, "configs", "hunyuan_c3.yml" if compress else "flux_c2.yml"))
    cfg["steps"] = 50
    cfg["num_model_invocations_per_inference_step"] = 1
    cfg["offloading"]["global_disable_offloading"] = True
    cfg["mlp"]["is_enabled"] = False
    # tk = 128 of the 256 padded keys (compressed: counts in multiples of 128) / 112 (torch.topk rows: multiples of 112); both are
    # at most min(k_lens) = 216, the documented precondition of the fixed-width rows
    cfg["attn"].update(first_n_dense_layers=0, full_step_schedule={0, 1}, top_keys=0.5 if compress else 0.45, token_major_output=False)
    for key in AMD_ATTN_KEYS:
        cfg["attn"][key] = fused


def _inputs(dev, step):
    g = torch.Generator().manual_seed(100)
    base = [torch.randn(B, H, N, 128, generator=g) for _ in range(3)]
    g2 = torch.Generator().manual_seed(200 + step)
    out = []
    for j, t in enumerate(base):
        t = t + 0.05 * step * torch.randn(B, H, N, 128, generator=g2)
        out.append(((1.6 if j == 0 else 1.0) * t).to(torch.bfloat16).to(dev))
    return out


def _module(dev, compress):
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.util.layer_counter import LayerCounter
    mod = SparseDiffAttn(0, LayerCounter(1, 1))
    if compress:
        torch.manual_seed(5)                 # (the static mask draws its random keys from torch's generator)
        mod.initialize_static_mask(VID, TXT, H, dev)
    return mod


def _schedule(mod, dev, seed, call):
    import chipmunk_amd
    chipmunk_amd.ops.manual_seed(seed)       # the mask kernels' random 1 %
    torch.manual_seed(seed)                  # ... and the torch chain's
    outs = []
    with torch.no_grad():
        for step in range(STEPS):
            q, k, v = _inputs(dev, step)
            outs.append(call(mod, q, k, v, step).clone())
    return outs


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("compress", [True, False], ids=["packed_mask", "topk_rows"])
def test_padded_batch_through_the_layer(fresh_config, compress, fused):
    from chipmunk_amd import ops
    cfg = fresh_config
    _configure(cfg, compress, fused)
    dev = torch.device("cuda:0")
    kl = torch.tensor(LENS, dtype=torch.int32, device=dev)
    keep = torch.arange(N, device=dev)[None, None, :] < kl[:, None, None]
    multiple_of = 128 if cfg["attn"]["pad_qkv_before_kernel"] else cfg["attn"]["counts_multiple_of"]
    mod = _module(dev, compress)
    state = {}

    def call(m, q, k, v, step):
        kn, vn = k.clone(), v.clone()
        for b, L in enumerate(LENS):
            kn[b, :, L:] = float("nan")
            vn[b, :, L:] = float("nan")
        out = m(q, kn, vn, kl)
        assert torch.isfinite(out.float()).all(), f"step {step}: a padding row was read"
        what = f"step {step}, {'packed mask' if compress else 'topk rows'}, {'fused' if fused else 'unfused'}"
        if step < 2:
            assert_rows_close(out, attn_exact(q, k, v, keep=keep), what="full " + what)
        if step == 1:
            inds, counts = m._stored_indices(multiple_of, 192)
            if compress:
                counts = torch.minimum(counts, kl.view(-1, 1, 1))
                for b, L in enumerate(LENS):
                    listed = inds[b] * (torch.arange(inds.shape[-1], device=dev) < counts[b, ..., None])
                    assert int((listed >= L).sum()) == 0, f"{what}: an index row lists a key at or past k_lens[{b}] within its count"
            if compress:
                packed, shape = m._stored_mask()
                mask = ops.bitunpack(packed, shape)
                assert tuple(mask.shape) == (B, H, 2, N)
                for b, L in enumerate(LENS):
                    assert not mask[b, ..., L:].any(), f"{what}: the stored mask keeps a key at or past k_lens[{b}] = {L}"
                assert mask[1, :, :, :LENS[1]].any()
            else:
                tk = int(counts.flatten()[0])
                assert tk > 0 and (counts == tk).all()
                for b, L in enumerate(LENS):
                    assert int((inds[b, ..., :tk] >= L).sum()) == 0, f"{what}: a stored index at or past k_lens[{b}] = {L}"
            dense1 = attn_exact(q, k, v, keep=keep)
            state.update(inds=inds.clone(), counts=counts.clone(), base=dense1 - attn_exact(q, k, v, inds, counts))
        if step >= 2:
            ref = state["base"] + attn_exact(q, k, v, state["inds"], state["counts"])
            err = (out.double() - ref).abs()
            tol = 6e-3 + 2e-2 * ref.abs()
            print(f"sparse {what}: worst error / tolerance {float((err / tol).max()):.3f}")
            assert torch.isfinite(out.float()).all() and bool((err <= tol).all()), f"sparse {what}: {int((err > tol).sum())} elements off"
        return out

    _schedule(mod, dev, 1, call)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("compress", [True, False], ids=["packed_mask", "topk_rows"])
def test_without_lengths_the_layer_is_unchanged(fresh_config, compress, fused):
    _configure(fresh_config, compress, fused)
    dev = torch.device("cuda:0")
    a = _schedule(_module(dev, compress), dev, 2, lambda m, q, k, v, step: m(q, k, v, None))
    b = _schedule(_module(dev, compress), dev, 2, lambda m, q, k, v, step: m(q, k, v))
    for step, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"step {step}"


def test_disabled_layer_masks_the_padding_in_sdpa(fresh_config):
    """``attn.is_enabled`` off: torch's attention with the lengths as a key mask -- per sequence the call on the cropped K / V, at the
    project's tolerance for two bf16 attention results (atol = rtol = 2e-2)."""
    _configure(fresh_config, True, True)
    fresh_config["attn"]["is_enabled"] = False
    dev = torch.device("cuda:0")
    kl = torch.tensor(LENS, dtype=torch.int32, device=dev)
    q, k, v = _inputs(dev, 0)
    out = _module(dev, False)(q, k, v, kl)
    for b, L in enumerate(LENS):
        want = torch.nn.functional.scaled_dot_product_attention(q[b:b + 1], k[b:b + 1, :, :L], v[b:b + 1, :, :L])
        torch.testing.assert_close(out[b:b + 1].float(), want.float(), atol=2e-2, rtol=2e-2)
