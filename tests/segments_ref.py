"""The CPU oracle's walk (oracle.trace_paths) in the CSR form Pipeline.trace_segments returns; shared by
tests/test_segments.py and tests/test_gpu_segments.py, computed once per case."""
import numpy as np

CAP = 512
C0 = 0.28209479177387814

_CASES = {}


def to_csr(cells, t1, n, max_intersections=1024):
    """Padded [R, cap] arrays of oracle.trace_paths -> dict of numpy arrays (offsets, cells, t_exit, t_enter, n).
    t_enter is the t0 the oracle's compositing used (t0 = 0, then t0 = max(t0, t_exit) after every cell): the float32
    running maximum of 0 and the earlier t_exit -- 0, not the exit, behind a first exit that is negative (a ray whose
    origin lies a rounding outside its start cell: tests/foam_zoo.py has such rays far from the world origin)."""
    r, cap = t1.shape
    counts = np.minimum(n.astype(np.int64), max_intersections)
    assert counts.max(initial=0) <= cap, "oracle cap too small for this case"
    keep = np.arange(cap)[None, :] < counts[:, None]
    t_enter = np.fmax.accumulate(np.concatenate([np.zeros((r, 1), np.float32), t1], axis=1), axis=1)[:, :-1]
    assert t_enter.dtype == np.float32
    return {"offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), "cells": cells[keep],
            "t_exit": t1[keep], "t_enter": t_enter[keep], "n": n.astype(np.uint32), "counts": counts}


def oracle_segments(fm, rays, starts, weight_threshold=None, max_intersections=None, attributes=None):
    """The oracle's segments of `rays` (any leading shape, flattened row-major) through foam dict `fm`."""
    from oracle import oracle as O

    attrs = fm["attributes"] if attributes is None else attributes
    cells, t1, n = O.trace_paths(fm["sh_degree"], fm["points"], attrs, fm["point_adjacency"],
                                 fm["point_adjacency_offsets"], rays, np.asarray(starts).reshape(-1), cap=CAP,
                                 weight_threshold=weight_threshold, max_intersections=max_intersections)
    return to_csr(cells, t1, n, 1024 if max_intersections is None else max_intersections)


def image_case(foam_factory, sh_degree=2, **settings):
    """foam_factory(3000, sh_degree, 21) under the 64x48 camera: (fm, rays [48,64,6], start, oracle segments)."""
    from tests import helpers

    key = (sh_degree,) + tuple(sorted(settings.items()))
    if key not in _CASES:
        fm = foam_factory(3000, sh_degree, 21)
        _, rays, start = helpers.camera_setup(fm, 64, 48)
        starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
        _CASES[key] = (fm, rays, starts, oracle_segments(fm, rays, starts, **settings))
    return _CASES[key]


def flat_colour(attributes):
    """The colour trace_forward gives a cell of an SH-degree-0 foam, in float64: max(0.5 + C0 coef, 0), and 0 for cells of
    density <= 1e-6."""
    a = attributes.astype(np.float64)
    return np.where(a[:, 3:4] > 1e-6, np.maximum(0.5 + C0 * a[:, :3], 0.0), 0.0)
