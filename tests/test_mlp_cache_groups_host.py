"""Group-major activation cache of the sparse MLP without a GPU ("Group-major cache"):

1. the config key ``mlp.cache_layout``: its default and the refusal of anything but ``"column"`` / ``"group"``;
2. the C ABI lists the seven entries, and each refuses bad arguments with code 1 and a message that names the rule (no launch happens);
3. a CPU full step of ``SparseDiffMlp`` / ``SparseDiffGatedMlp`` stores ``[B, G, F, 128]`` with zero padding, and the operators' view of the
   stored tensor follows its rank, not the key;
4. the fake kernels of the two new operators give the right shapes, and the GEMM1 fakes trace with a group-major cache."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("chipmunk_csp_mlp_mm1_act_gm", "chipmunk_csp_mlp_mm1_fp8_act_gm", "chipmunk_csp_mlp_mm1_fp8_act_rs_gm", "chipmunk_csp_mlp_mm1_glu_gm",
         "chipmunk_csp_mlp_mm1_glu_fp8_gm", "chipmunk_csp_scatter_add_gm", "chipmunk_transpose16_groups")


def to_groups(x):
    """[..., N, F] -> [..., ceil(N/128), F, 128] with zero tail rows, in plain torch"""
    n, f = x.shape[-2:]
    g = (n + 127) // 128
    return torch.nn.functional.pad(x, (0, 0, 0, g * 128 - n)).reshape(x.shape[:-2] + (g, 128, f)).transpose(-1, -2).contiguous()


# ------------------------------------------------------------------------------------------------ 1. the key
def test_the_key_defaults_to_column_and_refuses_unknown_values(fresh_config):
    from chipmunk_amd.modules.mlp import CACHE_LAYOUTS, activation_cache_of
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.cache_layout"] == "column" and cfg.BASE_CONFIG["mlp"]["cache_layout"] == "column"
    assert cfg.amd_key("mlp", "cache_layout") == "column" and CACHE_LAYOUTS == ("column", "group")
    del fresh_config["mlp"]["cache_layout"]             # (a section copied from the reference does not carry the key)
    assert cfg.amd_key("mlp", "cache_layout") == "column"
    act = torch.randn(1, 37, 64)
    assert activation_cache_of("test", act).shape == (1, 64, 40)
    fresh_config["mlp"]["cache_layout"] = "group"
    assert activation_cache_of("test", act).shape == (1, 1, 64, 128)
    for bad in ("Group", "row", "", None, 1):
        fresh_config["mlp"]["cache_layout"] = bad
        with pytest.raises(ValueError, match=r"test: mlp\.cache_layout must be one of column, group"):
            activation_cache_of("test", act)


# ------------------------------------------------------------------------------------------------ 2. the C ABI
def test_every_symbol_is_declared_exported_and_listed():
    from chipmunk_amd import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in _native.SYMBOLS and re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(_native.lib(), name), f"{name} is not exported"
    assert _native.lib().chipmunk_abi_version() == 1


def _gemm1_calls(lib, last_error):
    """name -> call(**overrides) for the five GEMM1 entries; every default is valid: M = 293 (G = 3), K = 128, F = 256, B = 2"""
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)

    def make(name, n_w, n_bias, n_scale):
        def call(a=p, w=p, c=p, bias=null, cache=p, inds=p, cnt=p, scale=p, M=293, K=128, F=256, act=0, upd=0, B=2, bs=None):
            bs = (M + 127) // 128 * F * 128 if bs is None else bs
            args = [a] + [w] * n_w + [c] + [bias] * n_bias + [cache, inds, cnt] + [scale] * n_scale
            rc = getattr(lib, name)(*args, M, K, F, act, upd, B, ctypes.c_int64(bs), null)
            return rc, last_error()
        return call
    return {"csp_mlp_mm1_act": make("chipmunk_csp_mlp_mm1_act_gm", 1, 1, 0), "csp_mlp_mm1_fp8_act": make("chipmunk_csp_mlp_mm1_fp8_act_gm", 1, 1, 2),
            "csp_mlp_mm1_fp8_act_rs": make("chipmunk_csp_mlp_mm1_fp8_act_rs_gm", 1, 1, 2), "csp_mlp_mm1_glu": make("chipmunk_csp_mlp_mm1_glu_gm", 2, 2, 0),
            "csp_mlp_mm1_glu_fp8": make("chipmunk_csp_mlp_mm1_glu_fp8_gm", 2, 2, 3)}


def test_gemm1_entries_refuse_bad_arguments_with_a_code_and_the_rule():
    from chipmunk_amd import _native
    null = ctypes.c_void_p(0)
    block = 3 * 256 * 128
    for who, call in _gemm1_calls(_native.lib(), _native.last_error).items():
        fp8 = "fp8" in who
        cases = [(dict(a=null), "null"), (dict(w=null), "null"), (dict(c=null), "null"), (dict(cache=null), "null"),
                 (dict(inds=null), "indices / counts"), (dict(cnt=null), "indices / counts"), (dict(M=0), "M must be positive"),
                 (dict(F=96), "multiple of 64"), (dict(act=3), "unknown activation 3"), (dict(upd=-1), "update_cache"),
                 (dict(upd=3), "update_cache"), (dict(K=0), "K must be"), (dict(K=192 if fp8 else 96), "multiple of 128" if fp8 else "multiple of 64"),
                 (dict(B=0), "batch size"), (dict(B=-1), "batch size"), (dict(B=65536), "65535"),
                 (dict(bs=block - 8), "G * F * 128"), (dict(bs=block + 4), "multiple of 8"), (dict(B=1, bs=block - 8), "batch stride"),
                 (dict(M=1 << 20, F=1 << 12, bs=1 << 40), "G * F * 128 too large for 32-bit offsets")]
        if fp8:
            cases.append((dict(scale=null), "null"))
        if who in ("csp_mlp_mm1_act", "csp_mlp_mm1_glu", "csp_mlp_mm1_glu_fp8"):
            cases.append((dict(upd=2), "update_cache must be 0 or 1"))
        for kw, text in cases:
            rc, msg = call(**kw)
            assert rc == 1 and text in msg, (who, kw, rc, msg)
        for kw in (dict(act=3), dict(upd=-1), dict(K=0)):      # the entry's own checks name its family
            assert call(**kw)[1].startswith(who.replace("_rs", "") + ":"), (who, kw, call(**kw)[1])


def test_scatter_add_and_transpose_entries_refuse_bad_arguments():
    from chipmunk_amd import _native
    lib, p, null = _native.lib(), ctypes.c_void_p(16), ctypes.c_void_p(0)
    block = 3 * 256 * 128

    def scatter(packed=p, cache=p, inds=p, cnt=p, M=293, F=256, B=2, bs=block):
        return lib.chipmunk_csp_scatter_add_gm(packed, cache, inds, cnt, M, F, B, ctypes.c_int64(bs), null), _native.last_error()
    for kw, text in ((dict(packed=null), "null"), (dict(cache=null), "null"), (dict(inds=null), "indices / counts"), (dict(cnt=null), "indices / counts"),
                     (dict(M=0), "M must be positive"), (dict(F=100), "multiple of 64"), (dict(B=0), "batch size"), (dict(B=65536), "65535"),
                     (dict(bs=block - 8), "G * F * 128"), (dict(bs=block + 2), "multiple of 8"), (dict(B=1, bs=0), "batch stride"),
                     (dict(M=1 << 20, F=1 << 12, bs=1 << 40), "too large for 32-bit offsets")):
        rc, msg = scatter(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)

    def transpose(src=p, dst=p, B=1, R=293, C=256):
        return lib.chipmunk_transpose16_groups(src, dst, B, R, C, null), _native.last_error()
    for kw, text in ((dict(src=null), "null"), (dict(dst=null), "null"), (dict(B=0), "must be positive"), (dict(R=0), "must be positive"),
                     (dict(C=-1), "must be positive"), (dict(B=65536), "65535"), (dict(R=128 * 32767 + 1), "32767"),
                     (dict(src=ctypes.c_void_p(8)), "16-byte aligned"), (dict(dst=ctypes.c_void_p(24)), "16-byte aligned")):
        rc, msg = transpose(**kw)
        assert rc == 1 and text in msg and msg.startswith("transpose16_groups:"), (kw, rc, msg)


# ------------------------------------------------------------------------------------------------ 3. the modules on the CPU
def _cfg(cfg, layout):
    cfg["offloading"]["global_disable_offloading"] = True
    cfg["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=4, first_n_dense_layers=0, cache_layout=layout))


@pytest.mark.parametrize("B,N", [(2, 203), (1, 128), (1, 37)])
def test_cpu_full_step_stores_groups_with_zero_padding(fresh_config, B, N):
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.modules.mlp import activation_cache_view
    from chipmunk_amd.util.layer_counter import LayerCounter
    _cfg(fresh_config, "group")
    torch.manual_seed(0)
    K, F, G = 16, 64, (N + 127) // 128
    fc1, fc2, act = torch.nn.Linear(K, F), torch.nn.Linear(F, K), torch.nn.GELU(approximate="tanh")
    mlp = SparseDiffMlp(0, LayerCounter(1, 1), fc1, act, fc2, 6)
    x = torch.randn(B, N, K)
    with torch.no_grad():
        out = mlp(x)
        a = act(fc1(x))
    stored = mlp.storage.get_sparse_act_T()
    assert stored.shape == (B, G, F, 128) and stored.is_contiguous()
    assert torch.equal(stored, to_groups(a))
    back = stored.permute(0, 1, 3, 2).reshape(B, G * 128, F)
    assert torch.equal(back[:, :N], a) and (back[:, N:] == 0).all()
    assert torch.equal(out, fc2(a)) and mlp.storage.get_out_cache().shape == (B, N, K)
    # the operators' view follows the stored tensor's rank, whatever the key says by then
    fresh_config["mlp"]["cache_layout"] = "column"
    view = activation_cache_view(stored, N, B > 1)
    assert view.shape == ((B, G, F, 128) if B > 1 else (G, F, 128)) and view.data_ptr() == stored.data_ptr()
    # ... as a column-major [B, F, ceil8(N)] gives its [F, N] view with the key on "group"
    fresh_config["mlp"]["cache_layout"] = "group"
    col = activation_cache_view(torch.zeros(B, F, (N + 7) // 8 * 8), N, B > 1)
    assert col.shape == ((B, F, N) if B > 1 else (F, N))


def test_cpu_full_step_of_the_gated_module_stores_groups(fresh_config):
    from chipmunk_amd.modules import SparseDiffGatedMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    _cfg(fresh_config, "group")
    torch.manual_seed(1)
    B, N, K, F = 2, 150, 16, 64
    gate, up, fc2, act = torch.nn.Linear(K, F), torch.nn.Linear(K, F), torch.nn.Linear(F, K), torch.nn.SiLU()
    mlp = SparseDiffGatedMlp(0, LayerCounter(1, 1), gate, up, act, fc2)
    x = torch.randn(B, N, K)
    with torch.no_grad():
        mlp(x)
        a = act(gate(x)) * up(x)
    stored = mlp.storage.get_sparse_act_T()
    assert stored.shape == (B, 2, F, 128) and torch.equal(stored, to_groups(a)) and (stored[:, 1, :, 150 - 128:] == 0).all()
    fresh_config["mlp"]["cache_layout"] = "rows"
    mlp2 = SparseDiffGatedMlp(0, LayerCounter(1, 1), gate, up, act, fc2)
    with torch.no_grad(), pytest.raises(ValueError, match=r"SparseDiffGatedMlp: mlp\.cache_layout must be one of column, group \(got 'rows'\)"):
        mlp2(x)


def test_the_wrappers_tell_the_layouts_apart_by_rank():
    import sys
    import chipmunk_amd.ops  # noqa: F401
    om = sys.modules["chipmunk_amd.ops.mlp"]
    x2, x3 = torch.empty(293, 128), torch.empty(2, 293, 128)
    assert om.group_major(x2, torch.empty(3, 256, 128)) and om.group_major(x3, torch.empty(2, 3, 256, 128))
    assert not om.group_major(x2, torch.empty(256, 296)[:, :293]) and not om.group_major(x3, torch.empty(2, 256, 296)[..., :293])
    assert not om.group_major(x2, torch.empty(1, 256, 293))                  # (the column-major cache with a leading 1, as ever)
    assert not om.group_major(torch.empty(128, 128), torch.empty(1, 256, 128))   # one whole group: the same elements either way
    assert om.group_major(torch.empty(2, 128, 128), torch.empty(2, 1, 256, 128))


# ------------------------------------------------------------------------------------------------ 4. fakes
def test_fake_kernels_give_the_right_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    E4M3, bf16 = torch.float8_e4m3fn, torch.bfloat16
    with FakeTensorMode():
        ops = torch.ops.chipmunk
        for shape, want in (((293, 256), (3, 256, 128)), ((2, 37, 64), (2, 1, 64, 128)), ((1, 128, 64), (1, 1, 64, 128)), ((2, 3, 129, 8), (2, 3, 2, 8, 128))):
            out = ops.transpose_to_groups(torch.empty(shape, dtype=bf16))
            assert out.shape == want and out.dtype == bf16
        with pytest.raises(RuntimeError, match="16-bit"):
            ops.transpose_to_groups(torch.empty(4, 4))
        packed, cache = torch.empty(2, 293, 256, dtype=bf16), torch.empty(2, 3, 256, 128, dtype=bf16)
        inds, counts, s = torch.empty(2, 3, 256, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32), torch.empty(1)
        assert ops.csp_scatter_add_gm(packed, cache, inds, counts) is None
        with pytest.raises(RuntimeError, match=r"unpacked_groups must be \[B, ceil\(M/128\), F, 128\]"):
            ops.csp_scatter_add_gm(packed, cache[:, :2], inds, counts)
        with pytest.raises(RuntimeError, match="sp_inds"):
            ops.csp_scatter_add_gm(packed, cache, inds[:, :2], counts)
        # the GEMM1 operators keep their schemas and trace with the group-major cache
        a, w, bias = torch.empty(2, 293, 128, dtype=bf16), torch.empty(256, 128, dtype=bf16), torch.empty(256, dtype=bf16)
        assert ops.csp_mlp_mm1_act(a, w, packed, bias, cache, inds, counts, "gelu_tanh", True) is None
        assert ops.csp_mlp_mm1_act(a[0], w, packed[0], None, cache[0], inds[0], counts[0], "silu", False) is None
        assert ops.csp_mlp_mm1_fp8_act(a.to(E4M3), w.to(E4M3), packed, bias, cache, inds, counts, s, s, "gelu", 2) is None
        assert ops.csp_mlp_mm1_glu(a, w, w, packed, None, None, cache, inds, counts, "silu", True) is None
