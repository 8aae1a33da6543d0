"""Time of the walk by cell (radfoam.cell_entries, reduce_entries, gather_cells; the kernels of rf_cell_reduce.hip)
against torch's own routes on the same device tensors, on the frame of scripts/gpu_quantiles_time.py (100,000 points,
960x540), at C = 1 and C = 16 channels:

    the index build                              cell_entries(seg, N), a cost per walk
    reduce_entries(index, values)                against  zeros(N, C).index_add_(0, cells, values) in float32
    gather_cells(index, table), fwd + bwd        against  table[cells], forward plus backward

HIP events around the Python calls, 3 warm-up calls each, then 10 repetitions that ALTERNATE the two sides in this one
process; median (min, max) of each.  The frame's longest and median cell list come with it.

    python scripts/gpu_cell_reduce_time.py              # prints one JSON line
    python scripts/gpu_cell_reduce_time.py --hip-only   # the kernels alone (comparing builds of the library)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd import _lib, foam

N, W, H, D = 100000, 960, 540, 2
HIP_ONLY = "--hip-only" in sys.argv
t = time.time()
fm = foam.make_synthetic_foam(N, D, 1)
print("foam", time.time() - t, flush=True)
dev = "cuda:0"
p, a = torch.from_numpy(fm["points"]).to(dev), torch.from_numpy(fm["attributes"]).to(dev)
adj, off = torch.from_numpy(fm["point_adjacency"]).to(dev), torch.from_numpy(fm["point_adjacency_offsets"]).to(dev)
cam = foam.default_camera(W, H)
rays = torch.from_numpy(foam.camera_rays(cam)).to(dev)
start = torch.full(rays.shape[:-1], foam.nearest_point(fm["points"], cam["position"]), dtype=torch.int64, device=dev).to(torch.uint32)
pipe = radfoam.create_pipeline(D)
pipe.record_trail = False
seg = pipe.trace_segments(p, a, adj, off, rays, start)
S = int(seg["cells"].numel())
index = radfoam.cell_entries(seg, N)
cells = index.cells
lengths = index.cell_offsets[1:] - index.cell_offsets[:-1]


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating(sides, reps=10):
    """{name: [median, min, max] ms} of the callables in ``sides``, taking turns."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            out[name].append(once(fn))
    return {name: [float(np.median(v)), float(min(v)), float(max(v))] for name, v in out.items()}


def lookup(table, index_it):
    leaf = table.clone().requires_grad_(True)

    def fn():
        leaf.grad = None
        index_it(leaf).backward(grad)
    return fn


res = {"points": N, "rays": W * H, "entries": S, "cells_with_entries": int((lengths > 0).sum()),
       "longest_list": int(lengths.max()), "median_list": int(lengths[lengths > 0].median()),
       "chunk": int(_lib.load().rf_reduce_entries_chunk())}
res["index_build_ms"] = alternating({"cell_entries": lambda: radfoam.cell_entries(seg, N)})["cell_entries"]
gen = torch.Generator().manual_seed(1)
for C in (1, 16):
    values = (torch.rand((S, C), generator=gen) * 2 - 1).to(dev)
    table = (torch.rand((N, C), generator=gen) * 2 - 1).to(dev)
    grad = values
    if HIP_ONLY:
        with torch.no_grad():
            res["C=%d" % C] = alternating({"reduce_entries": lambda: radfoam.reduce_entries(index, values)})
        continue
    with torch.no_grad():
        r = alternating({"reduce_entries": lambda: radfoam.reduce_entries(index, values),
                         "index_add_float32": lambda: torch.zeros((N, C), device=dev).index_add_(0, cells, values)})
    r.update(alternating({"gather_cells_fwd_bwd": lookup(table, lambda t: radfoam.gather_cells(index, t)),
                          "table_cells_fwd_bwd": lookup(table, lambda t: t[cells])}))
    with torch.no_grad():                                        # how far the routes are from the sum in float64
        want = radfoam.reduce_entries(index, values.double(), backend="torch")
        bound = 1e-7 + 2e-7 * want.abs()
        got = radfoam.reduce_entries(index, values)
        r["reduce_entries_error_over_test_bound"] = float(((got.double() - want).abs() / bound).max())
        plain = torch.zeros((N, C), device=dev).index_add_(0, cells, values)
        r["index_add_float32_error_over_test_bound"] = float(((plain.double() - want).abs() / bound).max())
        r["same_bits_twice"] = bool(torch.equal(got, radfoam.reduce_entries(index, values)))
    res["C=%d" % C] = r
print(json.dumps(res))
