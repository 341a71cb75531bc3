"""The row-wise norm metric without a GPU: the CPU paths of ``ops.qkv_split_norm``, ``split_heads_rownorm`` and ``residual_ln_modulate``
(the reference's op sequences) against the fp64 definitions of tests/rowwise_model.py over every input family -- the floors, pinned
tight -- and mutants, the exact result with one defect rounded where the operator rounds, that ``MARGIN * floor`` must reject while
the old guard (``assert_close(rtol=1.6e-2, atol=2e-2 | 1e-6)`` plus "more than 99 % of the elements equal", against the CPU path) is
evaluated beside it.  docs/TEST_SENSITIVITY.md, "Row-wise norm kernels", has the tables this file prints (``pytest -s -k table``)."""
import functools

import pytest
import torch

import rowwise_model as rm
from helpers import assert_rowwise_close, row_rel_err, seg_rel_err

OPS = ("head", "wide", "ln")


# ------------------------------------------------------------------------------------------------ cases (CPU sizes)
def _cases(op, mutants=False):
    """name -> arguments.  Floors: the small shapes of tests/test_gpu_rowwise_accuracy.py (the row-wide operator at n = 24: every step
    of the ladder and every special row).  mutants: shapes with three `every 128th` rows, so that the old guard's 99 % means something."""
    out = {}
    if op == "head":
        shapes = [(37, 3, 64), (300, 4, 0)] if mutants else rm.QKV_SHAPES[:3]
        for n, heads, extra in shapes:
            ropes = rm.rope_row_choices(n) if n < 1000 else [0, 1199]
            for weights in (True, False):
                for rope in ropes:
                    for fam in rm.ALL:
                        out[f"n{n} h{heads} +{extra} {'w' if weights else 'no w'} rope {rope} {fam}"] = dict(
                            n=n, heads=heads, extra=extra, weights=weights, rope=rope, family=fam, seed=len(out))
    elif op == "wide":
        sets = ([(1, 260, h, 3, "mixed") for h in (5, 12)] + [(1, 24, 3, p, w) for p in (1, 2, 3) for w in ("bf16", "fp32")] if mutants else
                [(1, 24, h, p, w) for h in rm.WIDE_HEADS for p in (1, 2, 3) for w in rm.WIDE_WEIGHTS] + [(3, 9, 5, 3, "mixed")])
        for B, n, heads, parts, kind in sets:
            rope = {1: n, 2: 0, 3: next(r for r in range(n - 1, 0, -1) if r % 4)}[parts]
            for fam in rm.ALL:
                out[f"B{B} n{n} h{heads} parts {parts} {kind} rope {rope} {fam}"] = dict(
                    B=B, n=n, heads=heads, parts=parts, kind=kind, rope=rope, family=fam, seed=len(out))
    else:
        shapes = [(300, 8), (300, 520), (260, 3072)] if mutants else [(rm.LN_ROWS, c) for c in rm.LN_COLS]
        for rows, cols in shapes:
            for residual in (True, False):
                for fam in ("iid", "ladder", "special"):
                    out[f"{rows}x{cols}{' residual' if residual else ''} {fam}"] = dict(rows=rows, cols=cols, residual=residual, family=fam, seed=len(out))
    return out


def _old_guard_accepts(got, ref, atol, want=None):
    """the assertion pair of tests/test_gpu_reorder.py / test_gpu_wan_glue.py; ``want``: what `assert_close` compares with (LayerNorm: the
    fp32 formula), ``ref``: the CPU path's bf16 for the equality count"""
    g = got.float()
    w = ref.float() if want is None else want
    close = bool(((g - w).abs() <= atol + 1.6e-2 * w.abs()).all())      # (a NaN fails the comparison, as in assert_close)
    return close and float((got.to(torch.bfloat16) == ref).float().mean()) > 0.99


def _run(op, c, defects=()):
    """One case: the CPU path against the exact reference -- per class the worst segment -- and per defect (worst error / bound, inert,
    old guard accepts).  Outputs that are copies must be bit copies."""
    from chipmunk_amd.ops import qkv as ops
    res = {"floor": {}, "mut": {}}
    if op == "ln":
        x, y, gate, shift, scale = rm.ln_inputs(c["family"], c["rows"], c["cols"], c["residual"], 500 + c["seed"])
        rx, rxm = ops.residual_ln_modulate(x, y, gate, shift, scale, rm.EPS)
        if y is not None:
            assert rm.nearest_bf16_violations(rx, rm.residual_exact(x, y, gate)) == 0
        exact, prod = rm.ln_modulate_exact(x, y, gate, shift, scale, x_out=rx if y is not None else None, with_prod=True)
        bound, few = rm.bound_ln(exact, prod)
        err = seg_rel_err(rxm, exact, rm.SEG_W)
        if (~few).any():
            res["floor"]["ln"] = float(err[~few].max())
        if few.any():
            res["few"] = float((err / bound)[few].max())
        assert_rowwise_close(rxm, exact, bound, "CPU path", width=rm.SEG_W)
        xf = rx.float()
        xn = ((xf - xf.mean(-1, keepdim=True)) * torch.rsqrt(xf.var(-1, unbiased=False, keepdim=True) + 1e-6)).to(torch.bfloat16).float()
        want = shift.float() + xn * (1 + scale).float()
        outs = lambda d: [rm.ln_modulate_exact(x, y, gate, shift, scale, x_out=rx if y is not None else None, rounded=True, defect=d)]      # noqa: E731
        judged = [(0, exact, bound, rxm, 2e-2, want, rm.SEG_W)]
    else:
        if op == "head":
            n, H = c["n"], c["heads"]
            x = rm.rms_inputs(c["family"], 1, n, H, 3, c["extra"], 100 + c["seed"], wide=False)[0]
            qw, kw = (rm.rms_weight(128, torch.bfloat16, 7 + c["seed"]), rm.rms_weight(128, torch.bfloat16, 8 + c["seed"])) if c["weights"] else (None, None)
            fc, fs = rm.rope_tables(c["rope"], 9 + c["seed"])
            cpu = ops.qkv_split_norm(x, qw, kw, H, rm.EPS, fc, fs)
            outs = lambda d: rm.rms_head_exact(x, qw, kw, H, rm.EPS, fc, fs, rounded=d is not None, defect=d)      # noqa: E731
            rot = rm.rotated_tokens(1, H, n, c["rope"])
            bound_of = [lambda e: rm.bound_head(rot, e)] * 2 + [None]
            classes = [("head", rot), ("head", rot), None]
        else:
            B, n, H, parts = c["B"], c["n"], c["heads"], c["parts"]
            x = rm.rms_inputs(c["family"], B, n, H, parts, 64 if H == 64 else 0, 300 + c["seed"], wide=True)
            norm, rope = rm.wide_flags(parts, c["rope"])
            ws = rm.wide_weights(c["kind"], norm, H * 128, 11 + c["seed"])
            fc, fs = rm.rope_tables(c["rope"], 12 + c["seed"])
            cpu = ops.split_heads_rownorm(x, H, ws, norm, rope, rm.EPS, fc, fs)
            outs = lambda d: rm.rms_row_exact(x, H, ws, norm, rope, rm.EPS, fc, fs, rounded=d is not None, defect=d)      # noqa: E731
            rots = [rm.rotated_tokens(B, H, n, c["rope"], rope[p]) for p in range(parts)]
            bound_of = [(lambda e, p=p: rm.bound_wide(rm.weight_kind(ws[p]), rots[p], e)) if norm[p] else None for p in range(parts)]
            classes = [(rm.weight_kind(ws[p]), rots[p]) if norm[p] else None for p in range(parts)]
        exact = outs(None)
        judged, bounds = [], []
        for p, e in enumerate(exact):
            bounds.append(None if bound_of[p] is None else bound_of[p](e)[0])
            if bound_of[p] is None:
                assert_rowwise_close(cpu[p], e, 0.0, "CPU path, copied part", copy_of=e.to(torch.bfloat16))
                continue
            b, few = bound_of[p](e)
            assert_rowwise_close(cpu[p], e, b, "CPU path")
            err = row_rel_err(cpu[p], e)
            if few.any():
                res["few"] = max(res.get("few", 0.0), float((err / b)[few].max()))
            for rotated in (False, True):
                sel = err[(classes[p][1] == rotated) & ~few]
                if sel.numel():
                    key = (classes[p][0], rotated)
                    res["floor"][key] = max(res["floor"].get(key, 0.0), float(sel.max()))
            judged.append((p, e, b, cpu[p], 2e-2 if c["rope"] else 1e-6, None, None))
        exact = None
    if defects:
        base = outs(rm.NO_DEFECT)
        for d in defects:
            m = outs(d)
            inert = all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num()) for a, b in zip(m, base))
            ratio, accepts = 0.0, True
            for p, e, b, ref, atol, want, width in judged:
                err = seg_rel_err(m[p], e, width) if width else row_rel_err(m[p], e)
                ratio = max(ratio, float((err / b).max()))
                accepts = accepts and _old_guard_accepts(m[p], ref, atol, want)
            if op != "ln":          # a copied part that is no copy any more: the bit equality catches it
                for p, b in enumerate(bounds):
                    if b is None and not torch.equal(m[p], base[p]):
                        ratio, accepts = float("inf"), False
            res["mut"][d] = (ratio, inert, accepts)
    return res


def _class_floor(op, key):
    return rm.FLOOR_LN if op == "ln" else rm.FLOOR_HEAD[key[1]] if op == "head" else rm.FLOOR_WIDE[key]


@functools.lru_cache(maxsize=None)
def _floors(op):
    """(class, family) -> (smallest, largest) worst segment over the cases"""
    table = {}
    for name, c in _cases(op).items():
        for key, v in _run(op, c)["floor"].items():
            lo, hi = table.get((key, c["family"]), (v, v))
            table[(key, c["family"])] = (min(lo, v), max(hi, v))
    return table


@functools.lru_cache(maxsize=None)
def _mutants(op):
    """case name -> (case, defect -> (worst error / bound, inert, old guard accepts))"""
    defects = rm.DEFECTS[op] + (rm.SCALE_101,) + ((rm.UNBIASED,) if op == "ln" else ()) + (rm.NO_DEFECT,)
    return {name: (c, _run(op, c, defects)["mut"]) for name, c in _cases(op, mutants=True).items()}


# ------------------------------------------------------------------------------------------------ the model's own arithmetic
def test_exact_references_are_the_definitions():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 3 * 256 + 8, generator=g).to(torch.bfloat16)
    w = rm.rms_weight(256, torch.float32, 3)
    fc, fs = rm.rope_tables(3, 4)
    assert torch.equal(fc[:, 0::2], fc[:, 1::2]) and torch.equal(fs[:, 0::2], fs[:, 1::2])
    assert float(fc[1, 0]) == 1.0 and float(fs[1, 0]) == 0.0 and abs(float(fc[2, 0])) < 1e-7 and float(fs[2, 0]) == 1.0
    q, k, v = rm.rms_row_exact(x, 2, [w, None, None], [True, True, False], [True, False, False], rm.EPS, fc, fs)
    xd = x.double()
    for b in range(2):
        for t in range(5):
            row = xd[b, t, :256]
            want = row / (row.pow(2).mean() + rm.EPS).sqrt() * w.double()
            if t < 3:
                z = torch.view_as_complex(want.reshape(128, 2).contiguous()) * torch.complex(fc[t, 0::2].double(), fs[t, 0::2].double()).repeat(2)
                want = torch.view_as_real(z).flatten()
            assert torch.allclose(q[b, :, t].flatten(), want, rtol=1e-13, atol=1e-15)
            row = xd[b, t, 256:512]
            assert torch.allclose(k[b, :, t].flatten(), row / (row.pow(2).mean() + rm.EPS).sqrt(), rtol=1e-13, atol=0)
    assert torch.equal(v, xd[:, :, 512:768].reshape(2, 5, 2, 128).permute(0, 2, 1, 3))
    qh = rm.rms_head_exact(x[0], None, None, 2, rm.EPS)[0]
    assert torch.allclose(qh[0, 1, 4], xd[0, 4, 128:256] / (xd[0, 4, 128:256].pow(2).mean() + rm.EPS).sqrt(), rtol=1e-13, atol=0)
    x2, y2, gate, shift, scale = rm.ln_inputs("iid", 4, 24, True, 5)
    xm = rm.ln_modulate_exact(x2, y2, gate, shift, scale)
    xr = (x2.double() + gate.double() * y2.double()).to(torch.bfloat16).double()
    want = shift.double() + (xr - xr.mean(-1, keepdim=True)) / (xr.var(-1, unbiased=False, keepdim=True) + rm.EPS).sqrt() * (1 + scale).double()
    assert torch.allclose(xm, want, rtol=1e-13, atol=1e-15)


def test_input_families_contain_what_they_promise():
    s = rm.ladder_scale(64)
    assert float(s.min()) == 2.0 ** -12 and float(s.max()) == 2.0 ** 8 and float((s[1:] / s[:-1]).log2().abs().min()) >= 5
    x = rm.rms_inputs("ladder", 1, 64, 12, 1, 0, 0, wide=True).double()
    ms = x.pow(2).mean(-1)[0]
    assert ((ms > rm.EPS / 4) & (ms < rm.EPS * 4)).any() and float(ms.min()) < rm.EPS / 4
    hs = rm.head_ladder_scale(8, 5)
    assert len({int(r.argmax()) for r in hs}) == 5 and float(hs.max() / hs.min()) >= 2.0 ** 9
    assert rm.special_rows(37, 3) == {5: 0, 6: 1, 7: 2, 36: 0, 35: 1, 34: 2}
    assert rm.special_rows(8209, 5, 8192)[8195] == 0 and rm.special_rows(8209, 5, 8192)[8208] == 0 and rm.special_rows(1, 3) == {0: 0}
    x = rm.rms_inputs("special", 1, 37, 3, 3, 64, 0, wide=True)[0, :, :3 * 384].reshape(37, 3, 384)
    assert not x[5].any() and not x[36].any() and x[6, :, 0].all() and not x[6, :, 1:].any() and x[7, :, 383].all() and not x[7, :, :383].any()
    assert abs(float(x[6, 0].double().pow(2).mean()) / rm.EPS - 1) < 0.02
    lx = rm.ln_inputs("special", 70, 520, True, 0)[0].double()
    assert not lx[5].any() and (lx[8] == 3.0).all() and abs(float(lx[9].mean()) - 100) < 1 and 3 < float(lx[9].std()) < 5
    assert abs(float(lx[6].var(unbiased=False)) / rm.EPS - 1) < 0.02
    assert rm.rope_row_choices(1) == [0, 1] and rm.rope_row_choices(37) == [0, 1, 35, 37] and rm.rope_row_choices(1200) == [0, 1, 1199, 1200]


def test_segment_helper_definition():
    e = torch.zeros(1, 2, 3, 128, dtype=torch.float64)
    e[0, 0] = 1.0
    got = e.clone()
    got[0, 0, 1, 5] = 1.0 + 0.01 * 128 ** 0.5
    assert abs(assert_rowwise_close(got, e, 0.011, "definition") - 0.01) < 1e-9
    with pytest.raises(AssertionError, match="segment error"):
        assert_rowwise_close(got, e, 0.009, "definition")
    bad = e.clone()
    bad[0, 1, 2, 7] = 1e-30
    with pytest.raises(AssertionError, match="exactly zero"):
        assert_rowwise_close(bad, e, 0.011, "definition")
    bad = e.clone()
    bad[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_rowwise_close(bad, e, 0.011, "definition")
    with pytest.raises(AssertionError, match="bit copy"):
        assert_rowwise_close(e.to(torch.bfloat16), e, 0.0, "definition", copy_of=got.to(torch.bfloat16))
    xm = torch.ones(2, 136, dtype=torch.float64)
    g2 = xm.clone()
    g2[1, 130] = 1.0 + 0.01 * 8 ** 0.5                            # the short last segment: 8 columns, not diluted over the row
    assert abs(assert_rowwise_close(g2, xm, 0.011, "definition", width=128) - 0.01) < 1e-9


# ------------------------------------------------------------------------------------------------ floors
@pytest.mark.parametrize("op", OPS)
def test_cpu_path_is_under_its_floor(op):
    """(`_run` also asserts, per case, the CPU path under MARGIN * floor, the zero rows exactly zero, the copied parts bit copies and the
    residual a nearest bf16 of the fp64 sum)"""
    for (key, fam), (_, hi) in _floors(op).items():
        assert hi <= _class_floor(op, key), (op, key, fam, hi)


def test_floor_constants_are_tight():
    """every pinned constant is the measured maximum over families and cases rounded up, not a generous guess"""
    for op in OPS:
        worst = {}
        for (key, _), (_, hi) in _floors(op).items():
            worst[key] = max(worst.get(key, 0.0), hi)
        for key, w in worst.items():
            assert w <= _class_floor(op, key) <= w + 1e-4, (op, key, w)
    assert set(k for (k, _) in _floors("wide")) == set(rm.FLOOR_WIDE) and set(k for (k, _) in _floors("head")) == {("head", False), ("head", True)}


def test_floor_table():
    print("\noperator | class | " + " | ".join(rm.ALL))
    for op in OPS:
        t = _floors(op)
        for key in sorted({k for (k, _) in t}, key=str):
            cells = [("" if (key, f) not in t else f"{t[(key, f)][0]:.4f} .. {t[(key, f)][1]:.4f}") for f in rm.ALL]
            print(f"{op} | {key} | " + " | ".join(cells) + f" | pinned {_class_floor(op, key)}")


# ------------------------------------------------------------------------------------------------ mutants
def _applies(op, d, c):
    """whether defect `d` can touch case `c` at all, by the reason stated beside each line"""
    rope = c.get("rope", 0)
    rows = c["rows"] if op == "ln" else c.get("B", 1) * c["n"]
    weighted = {"head": c.get("weights"), "wide": c.get("kind") != "none", "ln": False}[op]
    if d in (rm.EPS_X10, rm.EPS_OUTSIDE, rm.SCALE_102, rm.SCALE_101):
        return not (c["family"] == "special" and rows == 1)                  # the only row is all-zero: it stays zero
    if d == rm.STATS_ROW:
        return rows >= 2
    if d in (rm.STATS_HEAD, rm.HEAD_FOR_ROW, rm.ROW_FOR_HEAD):
        return c["heads"] >= 2                                               # one head: the row IS the head
    if d == rm.DIVISOR:
        return (c["cols"] % 512 != 0) if op == "ln" else (c["heads"] % 4 != 0)      # 512 * NV = C
    if d == rm.W_COL8:
        return bool(weighted)
    if d == rm.Q_ON_K:
        return bool(weighted) and (op == "head" or c["parts"] == 3)          # a second normalised part with a weight of its own
    if d == rm.ROT_BEFORE_WEIGHT:
        return bool(weighted) and rope > 0
    if d == rm.ROT_NEXT_TOKEN:
        return rope >= 2                                                     # a table of one row has no other row
    if d == rm.ROT_BOUNDARY:
        return rope > 0 and not (c["family"] == "special" and rope == c["n"])   # no row rope_rows, and row rope_rows - 1 is the all-zero last row
    if d in (rm.ROT_SIGN, rm.ROT_HALF):
        return rope > 0
    if d == rm.ROT_UNFLAGGED:
        return rope > 0 and (op == "head" or c["parts"] >= 2)                # a table, and a part without the flag
    if d in (rm.GATE_TWICE, rm.XM_BEFORE_RESIDUAL):
        return bool(c["residual"])
    return True


@pytest.mark.parametrize("op", OPS)
def test_every_counted_mutant_is_rejected(op):
    for name, (c, muts) in _mutants(op).items():
        for d in rm.DEFECTS[op]:
            ratio, inert, _ = muts[d]
            if c["family"] in rm.FAMILIES[d] and _applies(op, d, c):
                assert not inert, f"{op}, {name}: '{d}' touches nothing"
                assert ratio > 1.0, f"{op}, {name}: mutant '{d}' stays under the bound ({ratio:.3f} of it)"


@pytest.mark.parametrize("op", OPS)
def test_mutants_that_do_not_apply_are_inert_for_the_stated_reason(op):
    """where `_applies` says a defect cannot touch a case (one head, one row, no table, no weight, 512 * NV = C, no residual, ...) the mutant
    IS the undamaged result bit for bit; every counted defect applies to two cases or more of each family it is counted on"""
    seen = {}
    for name, (c, muts) in _mutants(op).items():
        for d in rm.DEFECTS[op]:
            if not _applies(op, d, c):
                assert muts[d][1], f"{op}, {name}: '{d}' was expected to touch nothing"
            elif c["family"] in rm.FAMILIES[d]:
                seen[(d, c["family"])] = seen.get((d, c["family"]), 0) + 1
    for d in rm.DEFECTS[op]:
        for fam in rm.FAMILIES[d]:
            if not (op == "ln" and fam == "head_ladder"):
                assert seen.get((d, fam), 0) >= 2, (op, d, fam)


def _weakest(op):
    """defect -> family -> (weakest ratio, strongest ratio, old guard accepts in some case, cases)"""
    table = {}
    for name, (c, muts) in _mutants(op).items():
        for d, (ratio, inert, accepts) in muts.items():
            if _applies(op, d, c) and not inert:
                lo, hi, acc, cnt = table.setdefault(d, {}).get(c["family"], (ratio, ratio, False, 0))
                table[d][c["family"]] = (min(lo, ratio), max(hi, ratio), acc or accepts, cnt + 1)
    return table


def test_mutant_table_and_separation():
    """prints the table of docs/TEST_SENSITIVITY.md.  MARGIN * floor <= weakest counted mutant / 2: every counted (defect, family) pair is
    at 2 x its bound or more in its weakest case.  The eps defects are what the old guard accepts on iid rows and the bound rejects on
    the ladder and the special rows."""
    for op in OPS:
        table = _weakest(op)
        print(f"\n{op}: mutant | " + " | ".join(f"{f}: error / bound, weakest .. strongest case (* = old guard accepts)" for f in rm.ALL))
        weakest = (float("inf"), None)
        for d in rm.DEFECTS[op] + (rm.SCALE_101,) + ((rm.UNBIASED,) if op == "ln" else ()):
            cells = []
            for f in rm.ALL:
                t = table.get(d, {}).get(f)
                counted = d in rm.DEFECTS[op] and f in rm.FAMILIES[d]
                cells.append("" if t is None else f"{'' if counted else '('}{t[0]:.3g} .. {t[1]:.3g}{' *' if t[2] else ''}{'' if counted else ')'}")
                if t is not None and counted:
                    weakest = min(weakest, (t[0], (d, f)))
            print(f"{'' if d in rm.DEFECTS[op] else 'recorded: '}{d} | " + " | ".join(cells))
        print(f"{op}: weakest counted: {weakest}")
        assert weakest[0] >= 2.0, (op, weakest)
        for d in rm.EPS_DEFECTS:
            assert table[d]["iid"][2], (op, d, "the old guard was expected to accept it on iid rows")
            for f in ("ladder", "special"):
                assert table[d][f][0] > 1.0, (op, d, f)
        for name, (c, muts) in _mutants(op).items():      # an exact result rounded where the operator rounds is under its bound
            assert muts[rm.NO_DEFECT][0] <= 1.0 and muts[rm.NO_DEFECT][2], (op, name, muts[rm.NO_DEFECT])
