"""SparseDiffMlp over a weight-only ``W8Linear`` ``fc1`` with ``mlp.w8_stream_rows`` set: the block-mean probe ``fc1(block_mean(x))`` runs the
streaming kernel (``ops.w8_linear``).  The `flux` schedule of tests/method_model.py at N = 1003 with B = 1 and B = 2, against the fp64 method
model on the widened weights with the bounds tests/test_gpu_mlp_w8_e2e.py uses (``MLP_FLOORS`` x 2, selection shortfall
2 x ``MLP_SELECTION_SHORTFALL``).  Index equality with the widened module is not required: the kernel's sums run in another order than the
vendor GEMM's, so near-ties of the selection may fall differently -- the selection bound is what holds.

With the key at 1024 every call of ``fc1`` of at most 1024 rows goes through the kernel; with the key at the probe's row count only the
probes of the selecting steps do; with the key at 0 nothing does and the outputs are the parent's ``F.linear`` over the widened weight, bit
for bit."""
import pytest
import torch

import method_model as mm
import test_gpu_mlp_w8_e2e as e2e

pytestmark = pytest.mark.gpu

N = 1003
dev = e2e.dev      # the same fixture: fresh config, cleared storage


def _reset():
    from chipmunk_amd.util import config as cfg
    from chipmunk_amd.util import layer_counter as lc
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    torch.cuda.synchronize()
    cfg.reset_to_base()
    lc.singleton.__init__(0, 0)
    ot.gpu_tensors.clear()
    ot._resident_bytes = ot._kept_offloaded_bytes = 0


def _spy(monkeypatch):
    import chipmunk_amd.ops
    real, calls = chipmunk_amd.ops.w8_linear, []

    def spy(x, *a, **kw):
        calls.append(x.numel() // x.shape[-1])
        return real(x, *a, **kw)
    monkeypatch.setattr(chipmunk_amd.ops, "w8_linear", spy)
    return calls


def _run(batch, device, key, what, outputs=None, monkeypatch=None):
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    _reset()
    GLOBAL_CONFIG["mlp"]["w8_stream_rows"] = key
    if outputs is not None:
        after = e2e.W8Checker.after

        def recording(self, step, inv, layer, module, args, out):
            outputs.append(out.clone())
            return after(self, step, inv, layer, module, args, out)
        monkeypatch.setattr(e2e.W8Checker, "after", recording)
    chk, sel = e2e.run_route(N, batch, device, True, floors=mm.MLP_FLOORS, eps=2 * mm.MLP_SELECTION_SHORTFALL, what=what)
    if outputs is not None:
        monkeypatch.setattr(e2e.W8Checker, "after", after)
    return chk, sel


def _selecting(sel):
    """the (step, layer) pairs of the sparse steps that make a selection (modules/mlp.py: a step >= 10 off the block_mask_cache grid reuses
    the stored one)"""
    cache = mm.MLP_ROUTES["flux"][3]
    return [(step, li) for step, li, _, _ in sel if not (step % cache != 0 and step >= 10)]


@pytest.mark.parametrize("batch", [1, 2])
def test_module_with_the_probe_through_the_kernel(dev, monkeypatch, batch):
    from chipmunk_amd.modules import W8Linear
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    calls = _spy(monkeypatch)
    what = f"mlp w8 fc1 flux, n {N}, b {batch}, w8_stream_rows 1024"
    chk, sel = _run(batch, dev, 1024, what)
    e2e.report(what, chk)
    assert ("output", 3) in chk.worst and ("refreshed", 1) in chk.worst and chk.shortfall > 0
    assert all(isinstance(m.fc1[0], W8Linear) for m in chk.modules[mm.MLP_DENSE_LAYERS:])
    probe_rows = batch * ((N + GLOBAL_CONFIG["mlp"]["mbm"] - 1) // GLOBAL_CONFIG["mlp"]["mbm"])
    selecting = _selecting(sel)
    assert 0 < len(selecting) < len(sel), "the schedule holds selecting steps and a step that reuses its selection"
    assert calls.count(probe_rows) == len(selecting), (calls, probe_rows, len(selecting))
    full_rows = batch * N
    assert (full_rows in calls) == (full_rows <= 1024), "full steps take the kernel exactly when their rows fit under the key"
    assert set(calls) <= {probe_rows, full_rows}
    # the key at the probe's row count: the probes of the selecting steps and nothing else
    calls.clear()
    what = f"mlp w8 fc1 flux, n {N}, b {batch}, w8_stream_rows {probe_rows}"
    chk, sel = _run(batch, dev, probe_rows, what)
    e2e.report(what, chk)
    assert calls == [probe_rows] * len(_selecting(sel)), calls


def test_key_off_gives_the_parents_bits(dev, monkeypatch):
    from chipmunk_amd.modules import W8Linear
    calls = _spy(monkeypatch)
    off, parent = [], []
    _run(1, dev, 0, "key 0", off, monkeypatch)
    assert calls == [] and off
    # the parent's forward, written out
    monkeypatch.setattr(W8Linear, "forward", lambda self, x: torch.nn.functional.linear(
        x, self.widened() if x.dtype == torch.bfloat16 else self.widened().to(x.dtype), self.bias))
    _run(1, dev, 0, "parent forward", parent, monkeypatch)
    assert len(off) == len(parent) and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(off, parent))
