"""The sparse-delta state machine of ``SparseDiffMlp`` and ``SparseDiffGatedMlp`` as a recorded trace, without a GPU, and the table of the
column selection's route function.

``tests/golden/mlp_state_traces.json`` was recorded from the two modules as they stood when each had a ``forward`` of its own (run this
file as a script to record it again); the test replays the same schedules and compares, per case,

* the ordered list of operator calls (``ops.topk_indices[_p]``, ``ops.copy_indices``, ``ops.mlp`` / ``ops.mlp_glu`` / ``ops.mlp_glu_fp8``), of
  the ``offload_cur_value`` calls of the block-mean and activation-cache holders and of the storage setters, each with the shapes, dtypes
  and strides of its tensor arguments, its scalars, and which arguments were passed by keyword;
* after every call of the sparse layer the exact bits (SHA-256) of ``indices``, ``counts`` and the block-mean cache and, for the ungated
  layer, of the output.

The schedule is two layers with ``first_n_dense_layers`` 1, 13 steps, ``full_step_every`` 4 and ``block_mask_cache`` 2 (step 11
takes the selection of step 10).  ``topk_indices``, ``copy_indices`` and the ungated GEMMs run through the CPU oracle (``cpu_ops``); the gated
GEMMs have no CPU stand-in and are recorders that do nothing, as are the ungated GEMMs for a batch, the group-major cache or a token
count that is no multiple of 128 (which only the GPU operators take): the output digest of those cases is that of the unchanged output
cache.  With ``offload`` on the two holders
report ``is_resident() == False`` (nothing is moved: offloading itself needs a GPU) and the host copies the modules ask for are recorded.

The bits do not depend on the host: every operand is a small integer times a power of two, so every dot product and block mean is exact
in fp32 whatever the summation order, and is rounded to bf16 once; the dense paths of the ungated layer go through ``cpu_ops.ExactLinear``
/ ``ExactGELU`` (float64).  The recording gives the same file with one thread and with the default thread count.
"""
import hashlib
import itertools
import json
import os
import sys

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_state_traces.json")
K, F, C = 64, 1024, 64          # F: the selection takes rows of 1024 columns or more
STEPS, LAYERS = 13, 2
_SHORT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.int32: "i32", torch.float8_e4m3fn: "e4m3", torch.float64: "f64"}

OUTER = [(kind, b, n, r) for kind in ("ungated", "gated") for b in (1, 2) for n in (256, 200) for r in (1, 2)] + \
        [("gated_fp8", 1, 200, r) for r in (1, 2)]
INNER = list(itertools.product(("column", "group"), (0.0, 0.6), (False, True)))       # cache_layout, top_p, offload


def case_id(kind, b, n, r, layout, top_p, offload):
    return f"{kind}-B{b}-N{n}-r{r}-{layout}-{'top_p' if top_p else 'top_keys'}-{'offload' if offload else 'resident'}"


# ------------------------------------------------------------------------------------------------------------------ operands
def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _input(step, layer, b, n):
    """integers in [-10, 10] / 4: a fixed base of the layer plus a fresh perturbation of the step"""
    return ((_ints((b, n, K), -8, 8, 100 + layer) + _ints((b, n, K), -2, 2, 1000 + 10 * step + layer)) / 4).to(torch.bfloat16)


def _linear(fin, fout, seed, bias=True):
    import cpu_ops
    lin = cpu_ops.ExactLinear(fin, fout, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(_ints((fout, fin), -4, 4, seed) / 8)
        if bias:
            lin.bias.copy_(_ints((fout,), -4, 4, seed + 1) / 8)
    return lin.bfloat16()


class _E4m3Linear(torch.nn.Module):
    """What ``SparseDiffGatedMlp`` reads of an ``F8Linear``: e4m3 weights (here the exact image of the bf16 ones), scales of one, and a
    forward in float64 over the quantised input -- ``torch._scaled_mm`` is not a host-independent fixture."""
    input_float8_dtype = torch.float8_e4m3fn
    scaling = "tensor"

    def __init__(self, lin):
        super().__init__()
        self.weight = torch.nn.Parameter(lin.weight.data.to(torch.float8_e4m3fn), requires_grad=False)
        self.bias = None
        self.input_scale_reciprocal = torch.ones(())
        self.scale_reciprocal = torch.ones(())

    def quantize_input(self, x):
        return x.to(torch.float8_e4m3fn)

    def forward(self, x):
        return torch.nn.functional.linear(self.quantize_input(x).double(), self.weight.double()).to(x.dtype)


def _modules(kind, counter):
    import cpu_ops
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    mods = []
    for i in range(LAYERS):
        fc2 = _linear(F, C, 40 + 10 * i)
        if kind == "ungated":
            mods.append(SparseDiffMlp(i, counter, _linear(K, F, 20 + 10 * i), cpu_ops.ExactGELU(approximate="tanh"), fc2, 6))
            continue
        gate, up = _linear(K, F, 20 + 10 * i, bias=False), _linear(K, F, 30 + 10 * i, bias=False)
        if kind == "gated_fp8":
            gate, up = _E4m3Linear(gate), _E4m3Linear(up)
        mods.append(SparseDiffGatedMlp(i, counter, gate, up, torch.nn.SiLU(), fc2, 6))
    return mods


# ------------------------------------------------------------------------------------------------------------------ recording
def _digest(t):
    if t is None:
        return "-"
    t = t.detach().contiguous()
    raw = t.view(torch.uint8) if t.dtype != torch.uint8 else t
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(raw.numpy().tobytes())
    return h.hexdigest()[:20]


def _listed(indices, counts):
    """the listed entries of every group, in order (the rows of ``indices`` are uninitialised memory behind their count)"""
    if indices is None:
        return None
    rows, lens = indices.reshape(-1, indices.shape[-1]), counts.reshape(-1).tolist()
    return torch.cat([row[:k] for row, k in zip(rows, lens)])


def _desc(v):
    if isinstance(v, torch.Tensor):
        return f"{_SHORT.get(v.dtype, str(v.dtype))}{list(v.shape)}s{list(v.stride())}".replace(" ", "")
    if isinstance(v, float):
        return repr(round(v, 12))
    return repr(v)


def _call(name, args, kwargs):
    return f"{name}({', '.join([_desc(a) for a in args] + [f'{k}={_desc(v)}' for k, v in kwargs.items()])})"


class _Spies:
    """Puts the spies in place (``monkeypatch`` undoes them) and collects the calls of one case."""
    HOLDERS = ("mlp.blockmean_mid_cache", "mlp.sparse_act_T")
    SELECTION = ("topk_indices", "topk_indices_p", "copy_indices", "topk_delta_indices_p", "topk_group_delta_indices",
                 "topk_group_delta_indices_p")

    def __init__(self, monkeypatch):
        from chipmunk_amd import ops
        from chipmunk_amd.util.storage import MlpStorage
        from chipmunk_amd.util.storage.offloaded_tensor import MaybeOffloadedTensor
        self.calls, self.offload, self.run_gemms = [], False, False
        for name in self.SELECTION:
            monkeypatch.setattr(ops, name, self._through(name, getattr(ops, name)))
        monkeypatch.setattr(ops, "mlp", self._through("mlp", ops.mlp, lambda: self.run_gemms))
        monkeypatch.setattr(ops, "mlp_glu", self._through("mlp_glu", None))
        monkeypatch.setattr(ops, "mlp_glu_fp8", self._through("mlp_glu_fp8", None))
        for field in MlpStorage._fields:
            monkeypatch.setattr(MlpStorage, f"set_{field}", self._through(f"set_{field}", getattr(MlpStorage, f"set_{field}"), skip=1))
        spies, resident = self, MaybeOffloadedTensor.is_resident

        def is_resident(holder):
            return False if spies.offload and holder.name in spies.HOLDERS else resident(holder)

        def offload_cur_value(holder):
            spies.calls.append(f"offload_cur_value:{holder.name}")

        monkeypatch.setattr(MaybeOffloadedTensor, "is_resident", is_resident)
        monkeypatch.setattr(MaybeOffloadedTensor, "offload_cur_value", offload_cur_value)

    def _through(self, name, fn, when=lambda: True, skip=0):
        def spy(*args, **kwargs):
            self.calls.append(_call(name, args[skip:], kwargs))
            if fn is not None and when():
                return fn(*args, **kwargs)
        return spy


def run_case(spies, kind, b, n, r, layout, top_p, offload):
    """{"calls": [...], "state": [...]} of one case: see the module docstring"""
    import cpu_ops
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    from chipmunk_amd.util.layer_counter import LayerCounter
    cpu_ops.register()
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)
    try:
        conf = cfg.GLOBAL_CONFIG
        conf["steps"] = 50
        conf["num_model_invocations_per_inference_step"] = 1
        conf["offloading"]["global_disable_offloading"] = True
        conf["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=4, block_mask_cache=2, first_n_dense_layers=1,
                                counts_multiple_of=256, bm=128, mbm=128 // r, cache_layout=layout, top_p=top_p, top_p_min_keys=0.05))
        spies.calls, spies.offload = [], offload
        spies.run_gemms = b == 1 and layout == "column" and n % 128 == 0     # what the oracle's GEMMs take
        mods = _modules(kind, LayerCounter(LAYERS, 1))
        state = []
        with torch.no_grad():
            for step in range(STEPS):
                for layer, mod in enumerate(mods):
                    out = mod(_input(step, layer, b, n))
                    assert tuple(out.shape) == (b, n, C)
                    if layer < 1:
                        continue
                    st = mod.storage
                    digests = [_digest(_listed(st.get_indices(), st.get_counts())), _digest(st.get_counts()),
                               _digest(st.get_blockmean_mid_cache())]
                    if kind == "ungated":
                        digests.append(_digest(out))
                    state.append(" ".join(digests))
        return {"calls": list(spies.calls), "state": state}
    finally:
        cfg.reset_to_base()
        lc.singleton.__init__(0, 0)


def record(monkeypatch):
    """Every case, with the call records as numbers into one table of the distinct ones (the file stays small and diffs stay readable)."""
    spies, table, cases = _Spies(monkeypatch), {}, {}
    for outer in OUTER:
        for inner in INNER:
            got = run_case(spies, *outer, *inner)
            cases[case_id(*outer, *inner)] = {"calls": [table.setdefault(c, len(table)) for c in got["calls"]], "state": got["state"]}
    return {"records": list(table), "cases": cases}


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.mark.parametrize("kind,b,n,r", OUTER, ids=[f"{k}-B{b}-N{n}-r{r}" for k, b, n, r in OUTER])
def test_state_trace_is_the_recorded_one(monkeypatch, gold, kind, b, n, r):
    spies = _Spies(monkeypatch)
    for inner in INNER:
        cid = case_id(kind, b, n, r, *inner)
        want = gold["cases"][cid]
        got = run_case(spies, kind, b, n, r, *inner)
        assert got["calls"] == [gold["records"][i] for i in want["calls"]], cid
        assert got["state"] == want["state"], cid


def test_recorded_schedules_take_every_branch(gold):
    """what the fixture has to show for the comparison above to mean something"""
    for cid, case in gold["cases"].items():
        names = [gold["records"][i].split("(")[0] for i in case["calls"]]
        gemms = [n for n in names if n in ("mlp", "mlp_glu", "mlp_glu_fp8")]
        assert len(set(gemms)) == 1 and gemms[0] == {"ungated": "mlp", "gated": "mlp_glu", "gated_fp8": "mlp_glu_fp8"}[cid.split("-")[0]]
        assert names.count("set_sparse_act_T") == 4 and len(gemms) == 9                       # full steps 0, 4, 8, 12 of the sparse layer
        selections = names.count("topk_indices_p" if "top_p" in cid else "topk_indices")
        assert selections == names.count("copy_indices") == names.count("set_indices") == 8   # step 11 takes the selection of step 10
        assert not any(n.startswith("topk_") and "delta" in n for n in names)                 # CPU tensors: the chain
        offloads = [n for n in names if n.startswith("offload_cur_value")]
        assert len(offloads) == (8 + 9 if cid.endswith("-offload") else 0)
        assert len(case["state"]) == STEPS and len(set(case["state"])) > 7
    assert len(gold["cases"]) == len(OUTER) * len(INNER)


def test_select_route_table():
    """The route of the column selection is a function of (is_cuda, contiguous, R, the two keys) and nothing else: the single-row kernel
    for R == 1 and the group kernel for R > 1, each on contiguous GPU tensors with its key on; the chain everywhere else."""
    from chipmunk_amd.modules.mlp import select_route
    for cuda, contiguous, R, single_key, group_key in itertools.product((False, True), (False, True), (1, 2, 4), (False, True),
                                                                         (False, True)):
        if cuda and contiguous and R == 1 and single_key:
            want = "single"
        elif cuda and contiguous and R > 1 and group_key:
            want = "group"
        else:
            want = "chain"
        assert select_route(cuda, contiguous, R, single_key, group_key) == want, (cuda, contiguous, R, single_key, group_key)


if __name__ == "__main__":      # python tests/test_mlp_state_trace_host.py [FILE]: record the fixture
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle
    oracle.build()
    with pytest.MonkeyPatch.context() as mp:
        recorded = record(mp)
    lines = lambda items: "[\n" + ",\n".join(json.dumps(i) for i in items) + "\n]"      # noqa: E731
    cases = ",\n".join(f'{json.dumps(cid)}: {{"calls": {json.dumps(c["calls"])},\n"state": {lines(c["state"])}}}'
                       for cid, c in sorted(recorded["cases"].items()))
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLD, "w") as f:
        f.write(f'{{"records": {lines(recorded["records"])},\n"cases": {{\n{cases}\n}}}}\n')
