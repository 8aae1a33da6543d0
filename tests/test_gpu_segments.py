"""Pipeline.trace_segments on the GPU against the CPU oracle's walk (oracle.trace_paths, cap 512), bit for bit: offsets,
cells, t_exit, t_enter (the float32 running maximum of the earlier t_exit, derived here) and num_intersections; then the
properties that do not need the oracle.  References are computed once per case (tests/segments_ref.py)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import segments_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _pipeline(d, dtype=torch.float32):
    import radfoam

    return radfoam.create_pipeline(d, dtype)


def _device_inputs(fm, rays, starts, attr_dtype=None):
    p, a, adj, off = H.to_torch_foam(fm, DEV, attr_dtype)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint32)).to(DEV)
    return p, a, adj, off, r, s


def _segments(pipe, inputs, **kw):
    seg = pipe.trace_segments(*inputs, **kw)
    torch.cuda.synchronize()
    return seg, {k: v.cpu().numpy() for k, v in seg.items()}


def _assert_bitwise(got, ref, batch):
    assert got["offsets"].dtype == np.int64 and got["cells"].dtype == np.uint32
    assert got["t_exit"].dtype == np.float32 and got["t_enter"].dtype == np.float32
    assert got["num_intersections"].dtype == np.uint32 and got["num_intersections"].shape == tuple(batch) + (1,)
    np.testing.assert_array_equal(got["num_intersections"].reshape(-1), ref["n"])
    np.testing.assert_array_equal(got["offsets"], ref["offsets"])
    np.testing.assert_array_equal(got["cells"], ref["cells"])
    np.testing.assert_array_equal(got["t_exit"].view(np.uint32), ref["t_exit"].view(np.uint32))
    np.testing.assert_array_equal(got["t_enter"].view(np.uint32), ref["t_enter"].view(np.uint32))


def _last_exit(seg):
    """t_exit of every ray's last entry (rays without entries left out)."""
    off = seg["offsets"]
    return seg["t_exit"][off[1:][off[1:] > off[:-1]] - 1]


def test_image_bit_exact(foam_factory):
    fm, rays, starts, ref = S.image_case(foam_factory)
    assert ref["counts"].max() == 35 and len(ref["cells"]) == 78222 and np.isinf(_last_exit(ref)).all()
    # a zero-length crossing is what makes t_enter differ from t_exit shifted by one entry
    assert (ref["t_exit"] <= ref["t_enter"]).any()
    _, got = _segments(_pipeline(2), _device_inputs(fm, rays, starts))
    _assert_bitwise(got, ref, (48, 64))
    first = got["offsets"][:-1]
    assert (got["cells"][first] == starts.reshape(-1)).all() and (got["t_enter"][first] == 0).all()


def test_threshold_termination_bit_exact(foam_factory):
    fm, rays, starts, ref = S.image_case(foam_factory, weight_threshold=0.5)
    last = _last_exit(ref)
    assert np.isfinite(last).any() and np.isinf(last).any()          # both kinds of ending
    _, got = _segments(_pipeline(2), _device_inputs(fm, rays, starts), weight_threshold=0.5)
    _assert_bitwise(got, ref, (48, 64))


def test_step_cap_bit_exact(foam_factory):
    fm, rays, starts, ref = S.image_case(foam_factory, max_intersections=20)
    assert (ref["n"] == 21).mean() > 0.5 and (ref["n"] < 20).any()
    _, got = _segments(_pipeline(2), _device_inputs(fm, rays, starts), max_intersections=20)
    counts = np.diff(got["offsets"])
    np.testing.assert_array_equal(counts, np.minimum(got["num_intersections"].reshape(-1).astype(np.int64), 20))
    _assert_bitwise(got, ref, (48, 64))


_FLAT = {}


def _flat_case(foam_factory):
    if not _FLAT:
        fm = foam_factory(6000, 0, 11)
        rays, starts = H.random_rays(fm, 3000, seed=3)
        _FLAT["case"] = (fm, rays, starts, S.oracle_segments(fm, rays, starts))
    return _FLAT["case"]


def test_flat_incoherent_rays_bit_exact(foam_factory):
    fm, rays, starts, ref = _flat_case(foam_factory)
    assert ref["counts"].min() >= 13 and ref["counts"].max() > 35
    pipe = _pipeline(0)
    _, got = _segments(pipe, _device_inputs(fm, rays, starts))
    _assert_bitwise(got, ref, (3000,))
    # a ray count that is no multiple of the wave or the block
    end = int(ref["offsets"][2999])
    part = {"n": ref["n"][:2999], "offsets": ref["offsets"][:3000], "cells": ref["cells"][:end],
            "t_exit": ref["t_exit"][:end], "t_enter": ref["t_enter"][:end]}
    _, got = _segments(pipe, _device_inputs(fm, rays[:2999], starts[:2999]))
    _assert_bitwise(got, part, (2999,))
    # any leading shape is flattened in row-major order
    _, got = _segments(pipe, _device_inputs(fm, rays.reshape(50, 60, 6), starts.reshape(50, 60)))
    _assert_bitwise(got, ref, (50, 60))


def test_fp16_pipeline_walks_as_fp32_on_widened_attributes(foam_factory):
    fm, rays, starts, _ = S.image_case(foam_factory)
    half = fm["attributes"].astype(np.float16)
    ref = S.oracle_segments(fm, rays, starts, attributes=half.astype(np.float32))
    inputs = _device_inputs(fm, rays, starts, torch.float16)
    assert inputs[1].dtype == torch.float16
    _, got = _segments(_pipeline(2, torch.float16), inputs)
    _assert_bitwise(got, ref, (48, 64))


def _forward_backward(pipe, inputs, g, between=None):
    fwd = pipe.trace_forward(*inputs)
    state = None
    if between is not None:
        state = between(pipe)
    bwd = pipe.trace_backward(*inputs, fwd["rgba"], g)
    torch.cuda.synchronize()
    return fwd, bwd, state


def test_agrees_with_trace_forward_and_leaves_trail_and_tile_orders_alone(foam_factory):
    """num_intersections equals trace_forward's on the same pipeline object, and a trace_segments call between a
    trace_forward and its trace_backward changes nothing for them: the trail object, its contents and the tile orders
    are the ones the forward left, the backward replays the trail, and the gradients are those of a run without the
    call.  "The same gradients": trace_backward sums with floating-point atomics, so two runs of it agree bit for bit
    only if the hardware happens to serve the atomics in the same order.  Two plain runs are therefore compared with each
    other first: if they are bitwise equal, so must the run with trace_segments be; otherwise it must agree with them
    the way they may differ from each other (helpers.grad_close at 1e-3 per element, 1e-5 relative L2: the bar
    tests/test_gpu_parity.py sets for two backward runs over the same trail)."""
    fm, rays, starts, ref = S.image_case(foam_factory)
    inputs = _device_inputs(fm, rays, starts)
    g = torch.from_numpy(np.random.default_rng(4).normal(size=rays.shape[:-1] + (4,)).astype(np.float32)).to(DEV)

    def between(pipe):
        trail, tiles, sets = pipe._trail, pipe._tiles, dict(pipe._tile_sets)
        assert trail is not None
        recorded = trail["trail"].clone()
        seg = pipe.trace_segments(*inputs)
        assert pipe._trail is trail and torch.equal(trail["trail"], recorded)
        assert pipe._tiles is tiles and list(pipe._tile_sets) == list(sets)
        assert all(pipe._tile_sets[k] is sets[k] for k in sets)
        return seg

    runs = []
    for hook in (None, None, between):
        pipe = _pipeline(2)
        pipe.record_trail = True
        runs.append(_forward_backward(pipe, inputs, g, hook))
        assert pipe.last_backward_replayed is True
    fwd, _, seg = runs[2]
    assert torch.equal(seg["num_intersections"].view(torch.int32), fwd["num_intersections"].view(torch.int32))
    np.testing.assert_array_equal(seg["num_intersections"].cpu().numpy().reshape(-1), ref["n"])
    for key in ("points_grad", "attr_grad"):
        a, b, c = (np.ascontiguousarray(r[1][key].cpu().numpy()) for r in runs)
        reproducible = np.array_equal(a.view(np.uint32), b.view(np.uint32))
        print(key, "two plain runs bitwise equal:", reproducible, "- with trace_segments in between:",
              np.array_equal(a.view(np.uint32), c.view(np.uint32)))
        if reproducible:
            np.testing.assert_array_equal(c.view(np.uint32), a.view(np.uint32))
        ok, rel, worst = H.grad_close(c, a)
        assert ok and rel < 1e-5, (key, rel, worst)


def test_voronoi_property(foam_factory):
    """Independent of the oracle: the midpoint O + d (t_enter + t_exit) / 2 of every entry with a finite t_exit and
    t_exit - t_enter > 1e-4 lies in the Voronoi cell the entry names, i.e. its nearest site (radfoam.nn, exact) is
    cells[k].

    Measured on the oracle's segments of this case on the CPU (78 222 entries, 75 150 with a finite exit): the length
    filter leaves out 35 entries, 0.045 % of all (the bar is 2 %).  Of the 75 115 entries tested, 9 name a cell that is
    NOT the nearest site of their midpoint -- by 1e-6 to 1.8e-5 in distance, at cell sizes of 0.1 (the flat case of
    this file: 4 of 82 422, up to 1.5e-5; on the GPU, where radfoam.nn searches in float32, one more: an exact tie).  That is the walk's face table, not an error of the walk: the bisector
    between a and b is placed with the offset b - a rounded to fp16 (the reference's half4 table), 2^-11 relative, so
    the planes the walk crosses sit up to 2^-11 (|b - a| + distance to a) away from the exact ones, and a midpoint that
    close to a face can fall on the other side of the exact plane.  So an entry whose cell is not the nearest site must
    at least be that near a tie: distance to its own site - distance to the nearest site <= 2^-10 (L + distance to its
    own site), L the longest offset of the cell's adjacency row (twice the displacement above: both sites' planes
    move).  For this case that is about 2e-4, against the 0.05 to 0.1 by which a wrong cell would miss."""
    import radfoam

    fm, rays, starts, _ = S.image_case(foam_factory)
    inputs = _device_inputs(fm, rays, starts)
    seg = _pipeline(2).trace_segments(*inputs)
    points = inputs[0]
    counts = seg["offsets"][1:] - seg["offsets"][:-1]
    total = seg["cells"].numel()
    ray = torch.repeat_interleave(torch.arange(counts.numel(), device=DEV), counts, output_size=total)
    t_enter, t_exit = seg["t_enter"].double(), seg["t_exit"].double()
    tested = torch.isfinite(t_exit) & (t_exit - t_enter > 1e-4)
    excluded = int((torch.isfinite(t_exit) & ~tested).sum())
    print("entries", total, "finite exit", int(torch.isfinite(t_exit).sum()), "left out by the length filter", excluded)
    assert excluded < 0.02 * total and int(tested.sum()) > 0.9 * total
    r = inputs[4].reshape(-1, 6).double()
    direction = r[:, 3:] / r[:, 3:].norm(dim=1, keepdim=True)
    mid = (r[ray, :3] + direction[ray] * ((t_enter + t_exit) / 2).unsqueeze(-1))[tested]
    cells = seg["cells"].to(torch.int64)[tested]
    nearest = radfoam.nn(points, None, mid.float()).to(torch.int64)
    other = nearest != cells
    print("tested", int(tested.sum()), "entries whose cell is not the nearest site of the midpoint:", int(other.sum()))
    if bool(other.any()):
        p64 = points.double()
        own = (mid[other] - p64[cells[other]]).norm(dim=1)
        best = torch.cdist(mid[other], p64).min(dim=1).values
        off = inputs[3].to(torch.int64)
        adj = inputs[2].to(torch.int64)
        longest = torch.stack([(p64[adj[off[c]:off[c + 1]]] - p64[c]).norm(dim=1).max() for c in cells[other].tolist()])
        print("distance to own site - distance to nearest:", (own - best).tolist())
        assert bool((own - best <= 2.0 ** -10 * (longest + own)).all())


def test_composite_segments_reproduces_trace_forward(foam_factory):
    """composite_segments in float64 over the GPU's segments of an SH-degree-0 foam, with trace_forward's colour model,
    against trace_forward's fp32 rgba: within 1e-4 absolute, the project's RGB bar (the same comparison between the
    oracle's segments and the oracle's rgba measures 1.4e-7 on the CPU)."""
    import radfoam

    fm = foam_factory(3000, 0, 21)
    _, rays, start = H.camera_setup(fm, 64, 48)
    inputs = _device_inputs(fm, rays, np.full(rays.shape[:-1], start, dtype=np.uint32))
    density = torch.from_numpy(fm["attributes"][:, 3].astype(np.float64)).to(DEV)
    rgb = torch.from_numpy(S.flat_colour(fm["attributes"])).to(DEV)
    pipe = _pipeline(0)
    for kw in ({}, {"weight_threshold": 0.5}):
        seg = pipe.trace_segments(*inputs, **kw)
        got = radfoam.composite_segments(seg, density, rgb)
        want = pipe.trace_forward(*inputs, **kw)["rgba"].reshape(-1, 4).double()
        assert got.dtype == torch.float64 and got.shape == want.shape
        worst = float((got - want).abs().max())
        print(kw, "largest |composite_segments - trace_forward|:", worst)
        assert float(want[:, 3].max()) > 0.5 and worst <= 1e-4


def test_empty_batch_and_validation(foam_factory):
    fm, rays, starts, _ = S.image_case(foam_factory)
    p, a, adj, off, r, s = _device_inputs(fm, rays, starts)
    pipe = _pipeline(2)
    seg = pipe.trace_segments(p, a, adj, off, r[:0].reshape(0, 6), s[:0].reshape(0))
    assert seg["offsets"].dtype == torch.int64 and seg["offsets"].tolist() == [0]
    assert seg["cells"].dtype == torch.uint32 and seg["cells"].shape == (0,)
    assert seg["t_exit"].dtype == torch.float32 and seg["t_exit"].shape == (0,) and seg["t_enter"].shape == (0,)
    assert seg["num_intersections"].dtype == torch.uint32 and seg["num_intersections"].shape == (0, 1)
    assert pipe._cache.workspace is None                      # nothing was packed, nothing launched
    messages = []
    for call in (pipe.trace_forward, pipe.trace_segments):
        with pytest.raises(RuntimeError) as err:
            call(p, a, adj, off, r, s.view(torch.int32))
        messages.append(str(err.value))
    assert messages[0] == messages[1] == "start_point must have uint32 dtype"
