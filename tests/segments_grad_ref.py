"""Shared by tests/test_segments_grad.py and tests/test_gpu_segments_grad.py: the oracle's segments as torch dicts, the
cell behind a shortened walk's last face taken from the longer walk, holders by a plain loop, and the exact bisector
times of a fixed cell sequence."""
import numpy as np
import torch

NONE = 0xFFFFFFFF


def seg_to_torch(ref, device="cpu"):
    return {k: torch.from_numpy(np.ascontiguousarray(ref[k])).to(device) for k in ("offsets", "cells", "t_exit", "t_enter")}


def exit_cells_from_longer_walk(short, full):
    """uint32 [R]: for every ray of `short` whose last t_exit is finite, the cell the walk `full` (the same rays under
    settings that end later) lists at the next position; NONE elsewhere.  Asserts that `short` is a prefix of `full`."""
    counts, off_s, off_f = short["counts"], short["offsets"], full["offsets"]
    out = np.full(len(counts), NONE, dtype=np.uint32)
    for r in range(len(counts)):
        c = int(counts[r])
        assert c <= full["counts"][r]
        assert np.array_equal(short["cells"][off_s[r]:off_s[r] + c], full["cells"][off_f[r]:off_f[r] + c])
        if c and np.isfinite(short["t_exit"][off_s[r] + c - 1]):
            assert full["counts"][r] > c, "the longer walk ends where the shorter does"
            out[r] = full["cells"][off_f[r] + c]
    return out


def holders_by_loop(offsets, t_exit):
    """held_by [S] (int64): for every entry the index of the entry whose t_exit its t_enter is, -1 where t_enter is the
    constant 0.  The walk's own rule, ray by ray: t0 = max(t0, t1) with a strict '>'."""
    offsets, t_exit = np.asarray(offsets), np.asarray(t_exit)
    held_by = np.full(len(t_exit), -1, dtype=np.int64)
    for r in range(len(offsets) - 1):
        t0, holder = np.float32(0.0), -1
        for e in range(offsets[r], offsets[r + 1]):
            held_by[e] = holder
            if t_exit[e] > t0:
                t0, holder = t_exit[e], e
    return held_by


def next_cells(seg, exit_cells):
    """int64 [S]: the cell behind every entry's face (NONE: none)."""
    off = seg["offsets"].numpy()
    cells = seg["cells"].numpy().astype(np.int64)
    after = np.concatenate([cells[1:], [NONE]])
    last = off[1:][off[1:] > off[:-1]] - 1
    after[last] = np.asarray(exit_cells, dtype=np.int64)[off[1:] > off[:-1]]
    after[np.isinf(seg["t_exit"].numpy())] = NONE
    return after


def exact_times(points, rays, seg, after, held_by):
    """(t_enter, t_exit) float64 torch [S] of the FIXED cell sequence from the exact bisectors of `points` (float64
    torch [N, 3]): t_exit[j] = ((p_a + p_b) / 2 - O) . (p_b - p_a) / ((p_b - p_a) . d), inf without a next cell;
    t_enter[m] = t_exit[held_by[m]], 0 where held_by is -1."""
    off = seg["offsets"]
    counts = off[1:] - off[:-1]
    ray = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    r = torch.as_tensor(rays, dtype=torch.float64).reshape(-1, 6)
    origin, direction = r[ray, :3], (r[:, 3:] / r[:, 3:].norm(dim=1, keepdim=True))[ray]
    after = torch.as_tensor(after)
    has = after != NONE
    pa, pb = points[seg["cells"].to(torch.int64)], points[torch.where(has, after, torch.zeros_like(after))]
    t = (((pa + pb) / 2 - origin) * (pb - pa)).sum(-1) / ((pb - pa) * direction).sum(-1)
    t_exit = torch.where(has, t, torch.full_like(t, float("inf")))
    held = torch.as_tensor(held_by)
    t_enter = torch.where(held >= 0, t_exit[held.clamp_min(0)], torch.zeros_like(t))
    return t_enter, t_exit
