"""SparseDiffMlp / SparseDiffGatedMlp with an e4m3 F8Linear ``fc2`` (``mlp.fp8_fc2`` on) on the device against the fp64 model of the
sparse-delta method (tests/fp8_fc2_method_model.py): the sparse steps' GEMM2 gathers e4m3 rows of ``fc2.weight^T`` (``csp_mlp_mm2_w8``), dense
and full steps call ``fc2.forward`` (``torch._scaled_mm``).  The model takes the module's own quantised operands -- the dequantised ``fc2``
weight, at full steps the activation as ``fc2`` quantised it, the quantised ``x`` / ``fc1`` where ``fc1`` is fp8 -- so quantisation error is
not counted.

Routes: SparseDiffMlp over the `flux` (bf16 fc1) and `wan_fp8` (fp8 fc1, two model invocations) schedules of tests/method_model.py at
N = 1003, B = 1 (ragged last group, pitched cache) and N = 1024, B = 2; `flux` at N = 1003 again with the activation cache offloaded and not
resident; SparseDiffGatedMlp over two F8Linear projections (SiLU, N = 1003).  Bounds: MARGIN x MLP_FLOORS (GLU_FLOORS) and the selection
shortfall of the corresponding existing route.  `Fc2Emulation`, which runs no chipmunk operator, is held to the same bounds on the `flux`
schedule: the reference the floors would be taken from if the fp8 ``fc2`` moved them (it does not: docs/EXPERIMENTS_r13.md)."""
import pytest
import torch

import fp8_fc2_method_model as f2
import glu_fp8_method_model as gfp
import glu_method_model as gm
import method_model as mm

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    assert torch.cuda.is_available()
    why = f2.scaled_mm_available(torch.device("cuda:0"))
    if why is not None:
        pytest.skip(f"torch._scaled_mm fp8 unavailable here: {why}")
    ot.gpu_tensors.clear()
    saved = ot._resident_bytes, ot._kept_offloaded_bytes
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    ot.gpu_tensors.clear()
    ot._resident_bytes, ot._kept_offloaded_bytes = saved


def report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


def mlp_factory():
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    counter, gelu = LayerCounter(mm.MLP_LAYERS, 1), torch.nn.GELU(approximate="tanh")
    return lambda layer, fc1, fc2: SparseDiffMlp(layer, counter, fc1, gelu, fc2, 6)


def shortfall_of(route):
    return mm.MLP_SELECTION_SHORTFALL_FP8 if route == "wan_fp8" else mm.MLP_SELECTION_SHORTFALL


def assert_fp8_fc2(chk, first_sparse_layer):
    for m in chk.modules[first_sparse_layer:]:
        wT = m.fc2w_T if not isinstance(m.fc2w_T, list) else m.fc2w_T[0]
        assert m.fc2[0].weight.dtype == f2.F8 and wT.dtype == f2.F8, "the sparse steps ran GEMM2 on e4m3 rows"


MLP_CASES = [("flux", 1003, 1, "resident"), ("flux", 1024, 2, "resident"), ("wan_fp8", 1003, 1, "resident"), ("wan_fp8", 1024, 2, "resident"),
             ("flux", 1003, 1, "offloaded")]


@pytest.mark.parametrize("route,n,batch,res", MLP_CASES, ids=[f"{r} n{n} b{b} {res}" for r, n, b, res in MLP_CASES])
def test_mlp_modules_with_an_fp8_fc2_against_the_method_model(dev, route, n, batch, res):
    what = f"mlp fp8 fc2 {route}, n {n}, b {batch}, {res}"
    chk = f2.run_mlp_route(route, n, batch, dev, mlp_factory(), floors=mm.MLP_FLOORS, eps=2 * shortfall_of(route), what=what,
                           offloading=f2.OFFLOADED if res == "offloaded" else {"global_disable_offloading": True})
    report(what, chk)
    assert ("output", 3) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    assert_fp8_fc2(chk, mm.MLP_DENSE_LAYERS)
    assert (chk.modules[-1].fc1[0].weight.dtype == f2.F8) == (route == "wan_fp8")
    assert chk.modules[-1].storage.sparse_act_T.is_resident() == (res == "resident")


def test_gated_module_with_an_fp8_fc2_against_the_method_model(dev):
    from chipmunk_amd.modules import SparseDiffGatedMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    counter = LayerCounter(gfp.LAYERS, 1)

    def make(layer, projs, fc2, fused, act):
        assert fused is None
        return SparseDiffGatedMlp(layer, counter, projs[0], projs[1], gm.act_module(act), fc2, 6)
    what = "glu fp8 silu_n1003 with an fp8 fc2"
    chk = f2.run_glu_route("silu_n1003", dev, make, floors=gfp.GLU_FLOORS, eps=2 * gfp.GLU_SELECTION_SHORTFALL_FP8, what=what)
    report(what, chk)
    assert ("output", 9) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    assert all(m.fp8 for m in chk.modules)
    assert_fp8_fc2(chk, 0)


@pytest.mark.parametrize("n,batch", [(1003, 1), (1024, 2)], ids=["n1003 b1", "n1024 b2"])
def test_the_torch_emulation_holds_the_same_bounds(dev, fresh_config, n, batch):
    """no chipmunk operator runs: bf16 fc1 in torch, fc2's own forward with the torch quantisation chain, GEMM2 on the e4m3 weight in fp64"""
    fresh_config["mlp"]["fused_fp8_quantize"] = False
    what = f"emulation fp8 fc2 flux, n {n}, b {batch}"
    make = lambda layer, fc1, fc2: f2.Fc2Emulation(layer, fc1, fc2, fresh_config, mm.MLP_DENSE_LAYERS)      # noqa: E731
    chk = f2.run_mlp_route("flux", n, batch, dev, make, floors=mm.MLP_FLOORS, eps=2 * mm.MLP_SELECTION_SHORTFALL, what=what)
    report(what, chk)
    assert ("output", 3) in chk.worst
