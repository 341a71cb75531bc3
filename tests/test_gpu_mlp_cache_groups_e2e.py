"""``mlp.cache_layout: group`` through SparseDiffMlp / SparseDiffGatedMlp on the device ("Group-major cache").

Two modules built from the same seed see the same inputs, one with the key on ``"group"``, one on ``"column"``: a full step and three
sparse steps (the third reuses the second's selection), N = 293 (three groups, the last 37 rows: the column route runs on its pitched
cache), K = 128, F = 1024 (the fewest columns the modules' selection kernel takes).  The output of every step, and after every step the activation cache converted to the column layout with
torch permute / reshape, must be ``torch.equal``: the two routes run the same arithmetic on the same values, through different operators
(on the group route tanh-GELU with a bias takes ``csp_mlp_mm1_act`` / ``_fp8_act``, and an unfused tail ``csp_scatter_add_gm`` + GEMM2)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K, F = 293, 128, 1024      # (F: the modules' column selection, topk_indices, takes its quantile over 1024 columns and refuses fewer)
G = (N + 127) // 128
E4M3 = torch.float8_e4m3fn
OFFLOADED = {"global_disable_offloading": False, "mlp.sparse_act_T": True, "keep_resident_if_fits": False}


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    assert torch.cuda.is_available()
    ot.gpu_tensors.clear()
    saved = ot._resident_bytes, ot._kept_offloaded_bytes
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    ot.gpu_tensors.clear()
    ot._resident_bytes, ot._kept_offloaded_bytes = saved


def need_scaled_mm(dev):
    """torch's own fp8 GEMM, called as F8Linear calls it: its support varies with the ROCm build; nothing of the project runs here"""
    a, b = torch.zeros(16, K, device=dev).to(E4M3), torch.zeros(F, K, device=dev).to(E4M3)
    one = torch.ones((), device=dev)
    try:
        torch._scaled_mm(a, b.T, scale_a=one, scale_b=one, bias=torch.zeros(F, device=dev, dtype=torch.bfloat16), out_dtype=torch.bfloat16,
                         use_fast_accum=True)
    except (RuntimeError, NotImplementedError) as e:
        pytest.skip(f"torch._scaled_mm fp8 unavailable here: {e}")


def configure(cfg, layout, offload=False, fused_scatter=True, fp8_fc2=False):
    cfg["offloading"].update(OFFLOADED if offload else {"global_disable_offloading": True})
    cfg["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=10, block_mask_cache=2, first_n_dense_layers=0, counts_multiple_of=8,
                           cache_layout=layout, fused_scatter=fused_scatter, fp8_fc2=fp8_fc2))


def build(dev, kind, fp8_fc2):
    """one module of `kind` from a fixed seed: "bf16", "fp8 tensor", "fp8 row" (SparseDiffMlp), "glu", "glu fp8" (SparseDiffGatedMlp)"""
    from chipmunk_amd.modules import F8Linear, SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    torch.manual_seed(11)
    lin = lambda i, o: torch.nn.Linear(i, o, device=dev, dtype=torch.bfloat16)      # noqa: E731
    counter = LayerCounter(1, 1)
    counter.cur_inference_step = 10      # a full step, then 11 and 12 make a selection and 13 reuses it (the module reuses from step 10 on)
    fc2 = lin(F, K)
    if fp8_fc2:
        fc2 = F8Linear.from_linear(fc2, input_float8_dtype=E4M3)
    if kind.startswith("glu"):
        gate, up = lin(K, F), lin(K, F)
        if kind == "glu fp8":
            gate, up = (F8Linear.from_linear(m, input_float8_dtype=E4M3) for m in (gate, up))
        return SparseDiffGatedMlp(0, counter, gate, up, torch.nn.SiLU(), fc2, 6)
    fc1 = lin(K, F)
    if kind.startswith("fp8"):
        fc1 = F8Linear.from_linear(fc1, input_float8_dtype=E4M3, scaling=kind.split()[1])
    return SparseDiffMlp(0, counter, fc1, torch.nn.GELU(approximate="tanh"), fc2, 6)


def as_columns(stored, n):
    """the stored activation cache as [B, F, n], from either layout (plain torch)"""
    if stored.ndim == 4:
        b, g, f, _ = stored.shape
        return stored.permute(0, 2, 1, 3).reshape(b, f, g * 128)[..., :n].contiguous()
    return stored[..., :n].contiguous()


def run(dev, cfg, layout, kind, B, xs, offload=False, fused_scatter=True, fp8_fc2=False):
    """outputs of the four steps, the converted cache after each, the stored tensors after each"""
    configure(cfg, layout, offload, fused_scatter, fp8_fc2)
    mlp = build(dev, kind, fp8_fc2)
    outs, caches, stored = [], [], []
    with torch.no_grad():
        for x in xs:
            if offload and outs:
                mlp.storage.load_async()
                mlp.storage.load_async_wait()
            outs.append(mlp(x).clone())
            torch.cuda.synchronize()
            if offload:
                holder = mlp.storage.sparse_act_T
                assert not holder.is_resident(), "the activation cache was to live in pinned host memory"
                mlp.storage.load_async()
                mlp.storage.load_async_wait()
            s = mlp.storage.get_sparse_act_T()
            stored.append(s.clone())
            caches.append(as_columns(s, x.shape[1]))
    return outs, caches, stored, mlp


CONFIGS = [("bf16", 1, {}), ("bf16", 2, {}), ("fp8 tensor", 1, {}), ("fp8 row", 1, {}), ("glu", 1, {}), ("glu fp8", 1, {}),
           ("bf16", 2, dict(fused_scatter=False)), ("fp8 tensor", 1, dict(fused_scatter=False)), ("bf16", 1, dict(fp8_fc2=True)),
           ("bf16", 1, dict(offload=True)), ("glu", 2, dict(fused_scatter=False))]


@pytest.mark.parametrize("kind,B,extra", CONFIGS, ids=[f"{k}, B{b}" + "".join(f", {n}" for n in e) for k, b, e in CONFIGS])
def test_group_layout_equals_column_layout_step_by_step(dev, fresh_config, kind, B, extra):
    if "fp8" in kind or extra.get("fp8_fc2"):
        need_scaled_mm(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    xs = [torch.randn(B, N, K, device=dev, generator=g).to(torch.bfloat16)]
    for _ in range(3):
        xs.append((xs[-1].float() + 0.3 * torch.randn(B, N, K, device=dev, generator=g)).to(torch.bfloat16))
    col = run(dev, fresh_config, "column", kind, B, xs, **extra)
    grp = run(dev, fresh_config, "group", kind, B, xs, **extra)
    for s in col[2]:
        assert s.shape == (B, F, (N + 7) // 8 * 8)
    for step, s in enumerate(grp[2]):
        assert s.shape == (B, G, F, 128) and s.is_contiguous(), (step, s.shape)
        assert not s[:, -1, :, N % 128:].any(), f"step {step}: rows of the last group at or past N are not zero"
    for step in range(4):
        assert torch.equal(grp[0][step].view(torch.int16), col[0][step].view(torch.int16)), f"step {step}: outputs differ"
        assert torch.equal(grp[1][step].view(torch.int16), col[1][step].view(torch.int16)), f"step {step}: activation caches differ"
    # the steps did something: every sparse step moved the output and refreshed cache columns; the selection of the last one was reused
    for step in range(1, 4):
        assert not torch.equal(grp[0][step], grp[0][step - 1]) and not torch.equal(grp[1][step], grp[1][step - 1]), step
    counts = grp[3].storage.get_counts()
    assert counts.shape == (B, G) and int(counts.max()) > 0
    assert torch.equal(counts, col[3].storage.get_counts())


def test_changing_the_key_between_full_steps_cannot_mix_layouts(dev, fresh_config):
    """the sparse steps follow the stored tensor: a module whose full step stored groups keeps running on them with the key back on "column",
    and gives the outputs of the column route"""
    g = torch.Generator(device=dev).manual_seed(4)
    xs = [torch.randn(1, N, K, device=dev, generator=g).to(torch.bfloat16) for _ in range(3)]
    col = run(dev, fresh_config, "column", "bf16", 1, xs)
    configure(fresh_config, "group")
    mlp = build(dev, "bf16", False)
    with torch.no_grad():
        out0 = mlp(xs[0]).clone()
        fresh_config["mlp"]["cache_layout"] = "column"
        outs = [out0] + [mlp(x).clone() for x in xs[1:]]
    assert mlp.storage.get_sparse_act_T().shape == (1, G, F, 128)
    for step in range(3):
        assert torch.equal(outs[step].view(torch.int16), col[0][step].view(torch.int16)), step
