"""Time of radfoam.sh_entries (the kernels of rf_sh_entries.hip) against the route the walk operators offered before it, on
the same device tensors, on the frame of scripts/gpu_cell_reduce_time.py (100,000 points, 960x540) at SH degree 3:

    sh_entries(seg, index, coeffs, directions)          forward; forward + backward to coeffs; forward + backward to
                                                        directions; and each backward alone
    the yardstick: gather_cells(index, coeffs) [S, 48], times the basis gathered by entry ray, summed over k and
    clamped; forward; forward + backward to coeffs; forward + backward to directions

HIP events around the Python calls, 3 warm-up calls each, then 10 repetitions that ALTERNATE the sides in this one
process; median (min, max) of each, and the peak of torch's allocator over one forward + backward of either route.

    python scripts/gpu_sh_entries_time.py                        # prints one JSON line
    python scripts/gpu_sh_entries_time.py --hip-only             # the kernels alone
    python scripts/gpu_sh_entries_time.py --variants a.so,b.so   # and the backward to coeffs of other builds of the
                                                                 # library (RF_SH_ENTRIES_GROUP), taking turns with this one
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import radfoam
from radfoam_amd import _lib, foam
from radfoam_amd.pipeline import _ptr, _stream_ptr
from radfoam_amd.sh_entries import _sh_basis

N, W, H, D = 100000, 960, 540, 3
HIP_ONLY = "--hip-only" in sys.argv
VARIANTS = sys.argv[sys.argv.index("--variants") + 1].split(",") if "--variants" in sys.argv else []
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
coeffs0 = a[:, :-1].contiguous()
dirs0 = rays[..., 3:6].reshape(-1, 3).contiguous()
entry_ray = torch.repeat_interleave(torch.arange(W * H, device=dev), seg["offsets"][1:] - seg["offsets"][:-1], output_size=S)
grad = torch.randn((S, 3), generator=torch.Generator().manual_seed(1)).to(dev)
print("walk", S, time.time() - t, flush=True)


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


def yardstick(coeffs, dirs):
    """The route of the parent commit: the rows of every entry's cell, [S, 48], times the basis of the entry's ray."""
    rows = radfoam.gather_cells(index, coeffs).reshape(S, -1, 3)
    unit = dirs / dirs.square().sum(dim=-1, keepdim=True).sqrt()
    pre = 0.5 + (_sh_basis(unit, D).index_select(0, entry_ray).unsqueeze(-1) * rows).sum(dim=1)
    return torch.where(pre > 0, pre, torch.zeros_like(pre))


def ours(coeffs, dirs):
    return radfoam.sh_entries(seg, index, coeffs, dirs)


def fwd_bwd(route, want_coeffs, want_dirs):
    coeffs, dirs = coeffs0.clone().requires_grad_(want_coeffs), dirs0.clone().requires_grad_(want_dirs)

    def fn():
        coeffs.grad = dirs.grad = None
        route(coeffs, dirs).backward(grad)
    return fn


def bwd_alone(want_coeffs, want_dirs):
    coeffs, dirs = coeffs0.clone().requires_grad_(want_coeffs), dirs0.clone().requires_grad_(want_dirs)
    rgb = ours(coeffs, dirs)
    leaf = coeffs if want_coeffs else dirs
    return lambda: torch.autograd.grad(rgb, leaf, grad, retain_graph=True)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 30


lib = _lib.load()
res = {"points": N, "rays": W * H, "entries": S, "degree": D, "group": int(lib.rf_sh_entries_group()),
       "chunk": int(lib.rf_reduce_entries_chunk())}
routes = {"sh_entries": ours} if HIP_ONLY else {"sh_entries": ours, "yardstick": yardstick}
with torch.no_grad():
    res["forward_ms"] = alternating({name: (lambda r=route: r(coeffs0, dirs0)) for name, route in routes.items()})
res["forward_backward_coeffs_ms"] = alternating({name: fwd_bwd(route, True, False) for name, route in routes.items()})
res["forward_backward_directions_ms"] = alternating({name: fwd_bwd(route, False, True) for name, route in routes.items()})
res["backward_alone_ms"] = alternating({"coeffs": bwd_alone(True, False), "directions": bwd_alone(False, True)})
res["peak_GiB"] = {name: peak(fwd_bwd(route, True, True)) for name, route in routes.items()}
if not HIP_ONLY:
    with torch.no_grad():
        got, want = ours(coeffs0, dirs0), yardstick(coeffs0.double(), dirs0.double())
        res["forward_largest_difference_from_float64"] = float((got.double() - want).abs().max())
        res["same_bits_twice"] = bool(torch.equal(got, ours(coeffs0, dirs0)))
        del want

if VARIANTS:                                                     # the backward to coeffs of other builds, by hand
    with torch.no_grad():
        rgb = ours(coeffs0, dirs0)
    rays32 = entry_ray.to(torch.int32)
    out = torch.empty((N, coeffs0.size(1)), device=dev)
    ws = torch.empty(int(lib.rf_sh_entries_workspace_bytes(S, D)) // 8, dtype=torch.float64, device=dev)
    sides, first = {}, None
    for path in [_lib.LIB_PATH] + VARIANTS:
        other = ctypes.CDLL(path)
        for name in ("rf_sh_entries_group", "rf_sh_entries_backward_coeffs", "rf_last_error"):
            getattr(other, name).restype, getattr(other, name).argtypes = _lib.SYMBOLS[name]

        def fn(other=other):
            rc = other.rf_sh_entries_backward_coeffs(D, N, S, W * H, _ptr(index.sorted_cells), _ptr(index.entries),
                                                     _ptr(rays32), _ptr(dirs0), _ptr(rgb), _ptr(grad), _ptr(out),
                                                     _ptr(ws), ws.numel() * 8, _stream_ptr(torch.device(dev)))
            if rc != 0:
                raise RuntimeError(other.rf_last_error().decode())
        fn()
        first = out.clone() if first is None else first
        assert torch.equal(first, out), "the builds disagree"
        sides["group %d" % other.rf_sh_entries_group()] = fn
    res["backward_coeffs_by_group_ms"] = alternating(sides)
print(json.dumps(res))
