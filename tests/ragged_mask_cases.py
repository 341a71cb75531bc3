"""Seeded masks for the mask -> ragged index rows tests (host and GPU): every mask mixes the row kinds whose handling differs."""
import torch

KINDS = ("all_false", "all_true", "one_true", "whole_multiple", "random")


def case_masks(shape, multiple_of, seed=0, density=0.06):
    """Bool CPU masks of ``shape`` whose rows cycle through KINDS -- nothing kept (a row of width 0, other rows behind it), everything
    kept (counts > n when n % multiple_of != 0: the padding columns run out), exactly one key, a kept count that is a multiple of
    ``multiple_of`` already (no padding), about ``density`` random -- as many masks as it takes for every kind to occur."""
    b, h, m, n = shape
    rows = b * h * m
    g = torch.Generator().manual_seed(seed + 1000 * n + multiple_of)
    out = []
    for j in range((len(KINDS) + rows - 1) // rows):
        mask = torch.zeros(rows, n, dtype=torch.bool)
        for r in range(rows):
            kind = KINDS[(j * rows + r) % len(KINDS)]
            if kind == "all_true":
                mask[r] = True
            elif kind == "one_true":
                mask[r, int(torch.randint(0, n, (1,), generator=g))] = True
            elif kind == "whole_multiple":
                keep = min(max(1, int(density * n) // multiple_of) * multiple_of, n // multiple_of * multiple_of)
                mask[r, torch.randperm(n, generator=g)[:keep]] = True
            elif kind == "random":
                mask[r] = torch.rand(n, generator=g) < density
        out.append(mask.view(b, h, m, n))
    return out


def expected_flat(inds, counts, offsets, n):
    """What the ragged rows must hold, from the padded rows ``inds [rows, pad_n]``: the first min(counts, n) entries of every row, zeros
    behind them up to the next offset (the padded tensor holds no defined value past min(counts, n))."""
    rows, pad_n = inds.shape
    total = int(offsets[-1])
    pos = torch.arange(total, device=inds.device)
    row = torch.searchsorted(offsets, pos, right=True) - 1
    j = pos - offsets[row]
    valid = j < counts.flatten().long().clamp(max=n)[row]
    return torch.where(valid, inds[row, j.clamp(max=pad_n - 1)], torch.zeros_like(inds[0, 0]))
