"""``mlp.top_p`` without a GPU: the rule's model (tests/mlp_top_p_model.py) against a brute-force statement, the CPU branch of
``ops.topk_indices_p`` against the model, the checker of the GPU tests against mutant selections, SparseDiffMlp with the key set on the
CPU mirror (tests/cpu_ops.py) against the fp64 method model and the selection model, and the op sequence with the key off."""
import pytest
import torch

import method_model as mm
import mlp_top_p_model as tp

CPU_N = 256
OFF = {"global_disable_offloading": True}


def _reset():
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)


# ------------------------------------------------------------------------------------------------------------------ 1. model vs brute force
def _eighths(seed, kind):
    """1024 values that are multiples of 1/8"""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.randint(0, 64, (1024,), generator=g).double() / 8
    if kind == "signed":            # the plain operator takes negative activations: no mass, but they are part of the sample
        return torch.randint(-32, 64, (1024,), generator=g).double() / 8
    if kind == "few_classes":       # long tie classes
        return torch.randint(0, 4, (1024,), generator=g).double() / 8
    if kind == "peaked":
        return torch.floor(64 * torch.rand(1024, generator=g, dtype=torch.float64) ** 6) / 8
    assert kind == "zeros"
    return torch.zeros(1024, dtype=torch.float64)


@pytest.mark.parametrize("kind", ["uniform", "signed", "few_classes", "peaked", "zeros"])
def test_model_is_the_brute_force_rule(kind):
    seen = set()
    for seed in range(3):
        v = _eighths(seed, kind)
        for sparsity in (0.0, 0.5, 0.75, 1.0):
            for top_p in (0.25, 0.5, 0.875, 1.0):
                for min_keys in (0.0, 0.125, 0.25):
                    if min_keys > 1 - sparsity:
                        continue
                    got = tp.kept_columns(v, sparsity, top_p, min_keys).tolist()
                    want = tp.brute_force_row(v.tolist(), sparsity, top_p, min_keys)
                    assert got == want, (kind, seed, sparsity, top_p, min_keys, len(got), len(want))
                    if 0 < sparsity < 1:
                        # a subset of what the top_keys rule keeps
                        thr_q = sorted(v.tolist())[int(1024 * sparsity)]
                        assert all(v[c] >= thr_q for c in got)
                        seen.add(tp.regime(tp.thresholds(v, sparsity, top_p, min_keys)))
    if kind == "zeros":
        assert tp.kept_columns(v, 0.5, 0.5, 0.25).numel() == 0        # an all-zero row keeps nothing, floor or not
    if kind in ("uniform", "peaked"):
        assert seen == {"cap", "top_p", "floor"}, seen


def test_exact_rows_cover_the_three_regimes():
    seen = tp.assert_exact_rows_cover_the_regimes()
    print("rows per regime over the GPU test's parameter set:", seen)
    for f in tp.EXACT_F:
        rows = tp.exact_rows(f)
        assert float(rows.max()) <= 255 and torch.equal(rows, rows.to(torch.bfloat16).float()) and float(rows.sum(-1).max()) < 2 ** 24 / 3


# ------------------------------------------------------------------------------------------------------------------ 2. CPU branch
def _general_rows(rows, f, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, f, generator=g).abs() * torch.exp(torch.randn(1, f, generator=g))).to(dtype)


@pytest.mark.parametrize("f", [1024, 1500])
@pytest.mark.parametrize("top_p,min_keys", tp.EXACT_PARAMS)
def test_cpu_branch_is_the_model(f, top_p, min_keys):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    for vals in (tp.exact_rows(f).to(torch.bfloat16), _general_rows(6, f, 3), _general_rows(4, f, 4, torch.float32) - 0.3):
        act = vals[None]
        inds = torch.full(act.shape, -1, dtype=torch.int32)
        counts = torch.full(act.shape[:2], -1, dtype=torch.int32)
        ops.topk_indices_p(act, inds, counts, 0.7, top_p, min_keys, 256, 0.0)
        tp.check_rows(inds[0], counts[0], vals, 0.7, top_p, min_keys, 256, "cpu branch")
        for r in range(vals.shape[0]):       # without random keys the padding is fixed too
            want, count = tp.selection(vals[r], 0.7, top_p, min_keys, 256)
            assert int(counts[0, r]) == count and torch.equal(inds[0, r], want)
        # random keys: the listed set contains the model's, the extras are not kept columns
        ops.topk_indices_p(act, inds, counts, 0.7, top_p, min_keys, 256, 0.05)
        for r in range(vals.shape[0]):
            kept = set(tp.kept_columns(vals[r], 0.7, top_p, min_keys).tolist())
            listed = inds[0, r, : int(counts[0, r])].tolist()
            assert kept <= set(listed) and len(set(listed)) == len(listed) and int(counts[0, r]) % 256 == 0


def test_cpu_branch_edges_and_argument_checks():
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    act = tp.exact_rows(1024)[None, :2].to(torch.bfloat16)
    inds, counts = torch.zeros(act.shape, dtype=torch.int32), torch.zeros(act.shape[:2], dtype=torch.int32)
    ops.topk_indices_p(act, inds, counts, 1.0, 0.5, 0.0, 256, 0.0)
    assert (counts == 0).all() and (inds == -1).all()                   # sparsity_amount 1 keeps nothing, as topk_indices
    ops.topk_indices_p(torch.zeros_like(act), inds, counts, 0.7, 0.5, 0.1, 256, 0.0)
    assert (counts == 0).all()                                          # an all-zero row: count 0
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(min_keys=-0.1), dict(min_keys=0.4)):
        args = dict(dict(top_p=0.5, min_keys=0.1), **bad)
        with pytest.raises(ValueError, match="topk_indices_p"):
            ops.topk_indices_p(act, inds, counts, 0.7, args["top_p"], args["min_keys"], 256, 0.0)
    ops.topk_indices_p(act, inds, counts, 1 - 0.1, 0.5, 0.1, 256, 0.0)  # min_keys == top_keys, with 1 - (1 - 0.1) < 0.1 in double


# ------------------------------------------------------------------------------------------------------------------ 3. checker vs mutants
def _mutant_cases():
    """(values, top_p, min_keys) at top_keys 0.3: the exact rows at 1500 columns and hand-made rows that single out a defect"""
    cases = [(row, top_p, min_keys) for top_p, min_keys in tp.EXACT_PARAMS for row in tp.exact_rows(1500)]
    exact_hit = torch.zeros(1024)
    # total 8, target 4: reached exactly by column 1 alone.  (The runner-up sits in FRONT of it: behind it, inside the same padded count, a
    # column kept in error is indistinguishable from a padding column, which may be any rejected column.)
    exact_hit[:4] = torch.tensor([2.0, 4.0, 1.0, 1.0])
    cases.append((exact_hit, 0.5, 0.0))
    one_hot = torch.zeros(1500)
    one_hot[700] = 3.0                                                  # floor threshold 0: the zero columns pass `v >= thr`
    cases.append((one_hot, 0.5, 0.1))
    return cases


@pytest.mark.parametrize("defect", tp.DEFECTS)
def test_checker_rejects_the_mutant(defect):
    rejected = 0
    cases = _mutant_cases()
    for v, top_p, min_keys in cases:
        kept = tp.kept_columns(v, 0.7, top_p, min_keys)
        good, count = tp.selection(v, 0.7, top_p, min_keys, 256)
        tp.check_row(good, count, kept, v.numel(), 256, "the model's own selection")
        bad, bad_count = tp.selection(v, 0.7, top_p, min_keys, 256, defect=defect)
        try:
            tp.check_row(bad, bad_count, kept, v.numel(), 256, defect)
        except AssertionError:
            rejected += 1
    print(f"{defect}: rejected on {rejected} of {len(cases)} rows")
    assert rejected >= (1 if defect in ("strict_target", "zero_mass_kept") else 6), f"{defect}: rejected on {rejected} rows only"


# ------------------------------------------------------------------------------------------------------------------ 4. modules on the CPU mirror
TOP_P, MIN_KEYS = 0.4, 0.05           # the GPU end-to-end test's setting (tests/test_gpu_mlp_top_p_e2e.py)


def _mirror_route(top_p, min_keys, set_keys=True, trace=None, floors=None, n=CPU_N):
    import cpu_ops
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    cpu_ops.register()
    _reset()
    if set_keys:
        GLOBAL_CONFIG["mlp"].update(top_p=top_p, top_p_min_keys=min_keys)
    else:
        del GLOBAL_CONFIG["mlp"]["top_p"], GLOBAL_CONFIG["mlp"]["top_p_min_keys"]      # a section that does not know the keys at all
    return mm.run_mlp_route("flux", n, torch.device("cpu"), cpu_ops.ExactLinear, cpu_ops.ExactGELU(approximate="tanh"),
                            offloading=OFF, floors=floors, eps=None, trace=trace)


def test_modules_with_top_p_on_the_cpu_mirror():
    """The state machine holds the fp64 method model's bounds (the floors pinned without top-p: the method, not the count, sets them),
    every stored selection is the model's, and the per-group count really is smaller than the top_keys rule's in most calls."""
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    try:
        trace = []
        chk = _mirror_route(TOP_P, MIN_KEYS, trace=trace, floors=mm.MLP_FLOORS)
        assert ("output", 3) in chk.worst
        made, smaller = tp.check_mlp_trace(trace, chk.modules, GLOBAL_CONFIG["mlp"])
        print(f"top_p {TOP_P}: {smaller} of {made} selection calls store fewer columns than top_keys alone in some group; worst figures",
              {k: round(v, 4) for k, v in sorted(chk.worst.items())})
        assert made >= 8 and 2 * smaller >= made
    finally:
        _reset()


@pytest.mark.parametrize("bad", [dict(top_p=1.2), dict(top_p=-0.1), dict(top_p=0.5, top_p_min_keys=0.35)])
def test_modules_refuse_bad_keys_at_the_call(bad):
    import cpu_ops
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    from chipmunk_amd.util.layer_counter import LayerCounter
    cpu_ops.register()
    _reset()
    try:
        mm.configure_mlp(GLOBAL_CONFIG, "flux")
        GLOBAL_CONFIG["mlp"].update(bad)
        GLOBAL_CONFIG["mlp"]["first_n_dense_layers"] = 0
        lin = lambda i, o: cpu_ops.ExactLinear(i, o).bfloat16()      # noqa: E731
        x = mm.mlp_input(0, 0, 0, 128, 64)
        with pytest.raises(ValueError, match="mlp.top_p"):
            SparseDiffMlp(0, LayerCounter(1, 1), lin(64, 1024), cpu_ops.ExactGELU(approximate="tanh"), lin(1024, 64))(x)
        with pytest.raises(ValueError, match="mlp.top_p"):
            SparseDiffGatedMlp(0, LayerCounter(1, 1), lin(64, 1024), lin(64, 1024), torch.nn.SiLU(), lin(1024, 64))(x)
    finally:
        _reset()


# ------------------------------------------------------------------------------------------------------------------ 5. top-p off
def test_top_p_off_is_todays_op_sequence(monkeypatch):
    import cpu_ops
    from chipmunk_amd import ops

    def boom(*a, **kw):
        raise AssertionError("a top-p operator was called with mlp.top_p = 0")

    monkeypatch.setattr(ops, "topk_indices_p", boom)
    monkeypatch.setattr(ops, "topk_delta_indices_p", boom)
    try:
        traces, outs = [], []
        for set_keys in (True, False):
            with cpu_ops.recording() as calls:
                chk = _mirror_route(0.0, 0.0, set_keys=set_keys)
                traces.append(list(calls))
            outs.append(chk.modules[-1].storage.get_out_cache().clone())
        assert traces[0] == traces[1] and len(traces[0]) > 20
        assert not any(name.endswith("_p") for name, _ in traces[0])
        assert "topk_indices" in {name for name, _ in traces[0]}
        assert torch.equal(outs[0], outs[1])
    finally:
        _reset()


def test_new_keys_are_extra_keys_with_the_feature_off():
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.top_p"] == 0.0 and cfg.AMD_EXTRA_KEYS["mlp.top_p_min_keys"] == 0.0
    assert cfg.BASE_CONFIG["mlp"]["top_p"] == 0.0 and cfg.BASE_CONFIG["mlp"]["top_p_min_keys"] == 0.0


def test_schemas_fake_kernels_and_aliases():
    import chipmunk  # noqa: F401
    import chipmunk_amd
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert chipmunk.ops.topk_indices_p is chipmunk_amd.ops.topk_indices_p
    assert chipmunk.ops.topk_delta_indices_p is chipmunk_amd.ops.topk_delta_indices_p
    plain = str(torch.ops.chipmunk.topk_indices_p.default._schema)
    fused = str(torch.ops.chipmunk.topk_delta_indices_p.default._schema)
    assert "Tensor(indices!) indices" in plain and "Tensor(counts!) counts" in plain
    assert "Tensor(cache!) cache" in fused and "Tensor(indices!) indices" in fused and "Tensor(counts!) counts" in fused
    with FakeTensorMode():
        act = torch.empty(1, 8, 1024, dtype=torch.bfloat16)
        inds, counts = torch.empty(1, 8, 1024, dtype=torch.int32), torch.empty(1, 8, dtype=torch.int32)
        assert torch.ops.chipmunk.topk_indices_p(act, inds, counts, 0.7, 0.5, 0.1, 256, 0.0) is None
        assert torch.ops.chipmunk.topk_delta_indices_p(act, act.clone(), inds, counts, 0.7, 0.5, 0.1, 256, 0.0) is None


def test_c_abi_argument_checks():
    import ctypes
    from chipmunk_amd import _native
    lib = _native.lib()
    p16, null, d = ctypes.c_void_p(16), ctypes.c_void_p(0), ctypes.c_double
    call = lambda cols, sp, top_p, mk: lib.chipmunk_topk_indices_p(p16, 0, p16, p16, 4, cols, d(sp), d(top_p), d(mk), 256, d(0.0), null)   # noqa: E731
    assert call(512, 0.7, 0.5, 0.1) == 1 and "1024" in _native.last_error()
    assert call(1024, 0.7, 0.0, 0.1) == 1 and "top_p" in _native.last_error()
    assert call(1024, 0.7, 1.1, 0.1) == 1 and "top_p" in _native.last_error()
    assert call(1024, 0.7, 0.5, 0.4) == 1 and "min_keys" in _native.last_error()
    assert call(1024, 0.7, 0.5, -0.1) == 1 and "min_keys" in _native.last_error()
    rc = lib.chipmunk_topk_delta_indices_p(p16, null, 0, p16, p16, 4, 1024, d(0.7), d(0.5), d(0.1), 256, d(0.0), null)
    assert rc == 1 and "cache" in _native.last_error()
