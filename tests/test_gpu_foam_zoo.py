"""-m gpu: the tracer, its fp16 instances and the walk export on the foams of tests/foam_zoo.py -- scaled across the fp16
edge of the face table, a 2312-face hub, three decades of cell size, a thin sheet, a lattice, far from the origin,
an unbounded-scene cloud, near-duplicate sites -- against the CPU oracle's LITERAL reference scan.  tests/test_foam_zoo.py
holds the oracle's mirror of the kernels equal to that scan on the same inputs, so a failure here is the kernels
differing from their own mirror.

Bars (unchanged): fp32 forward outputs bit-identical; scatter outputs helpers.grad_close (1e-3 per
element) and relative L2 < 1e-5; fp16 as in tests/test_gpu_half.py; the walk export as in tests/test_gpu_segments*.py,
through their own comparison code.  Every scatter comparison prints `zoo <foam> <what> <output>: observed over bound`."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import foam_zoo as Z
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAIN = ("hub", "scaled_2p14", "sheet")          # every backward instance, and the gradients of the walk export


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pipeline(d, dtype=torch.float32):
    """The hop trail always recorded (see tests/test_gpu_parity.py::_pipeline), and the sorted ray order -- with it the
    256-slot groups mode 5's cell table is built for -- in use from 1024 rays on: the zoo's batches have 4096."""
    import radfoam

    pipe = radfoam.create_pipeline(d, dtype)
    pipe.record_trail = True
    pipe.reorder_min_rays = 1024
    return pipe


def _bits(x):
    x = np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def _scatter(name, what, key, got, ref):
    got = got.float().cpu().numpy() if torch.is_tensor(got) else got
    ok, rel, worst = H.grad_close(got, ref)
    print("zoo %s %s %s: worst element at %.3g of its bound, relative L2 %.3g of 1e-5" % (name, what, key, worst, rel / 1e-5))
    assert np.abs(ref).max() > 0, (name, what, key)
    assert ok and rel < 1e-5, (name, what, key, rel, worst)


def _forward_bits(name, what, got, ref, quantiles):
    keys = ("rgba", "num_intersections") + (("depth", "depth_indices") if quantiles else ())
    for key in keys:
        np.testing.assert_array_equal(_bits(got[key]), _bits(ref[key]), err_msg="%s %s %s" % (name, what, key))


@pytest.mark.parametrize("forward_mode", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", Z.NAMES)
def test_forward_flat(name, forward_mode):
    """4096 flat rays in the sorted order, two quantiles per ray and the contribution.  Mode 4 runs its persistent waves
    only without quantiles (LaunchForward): it is called a second time without them."""
    fm, (r, s), u, ref = Z.foam(name), Z.rays(name), Z.upstream(name), Z.flat(name)["fwd"]
    pipe = _pipeline(fm["sh_degree"])
    pipe.forward_mode = forward_mode
    foam, tr, ts = H.to_torch_foam(fm, DEV), _t(r), _t(s)
    got = pipe.trace_forward(*foam, tr, ts, depth_quantiles=_t(u["q"]), return_contribution=True)
    torch.cuda.synchronize()
    assert pipe._order is not None and int(pipe._order["order"].numel()) == Z.NUM_RAYS
    _forward_bits(name, forward_mode, got, ref, True)
    _scatter(name, "forward mode %d" % forward_mode, "contribution", got["contribution"], ref["contribution"])
    if forward_mode == 4:
        plain = pipe.trace_forward(*foam, tr, ts)
        torch.cuda.synchronize()
        _forward_bits(name, "4, no quantiles", plain, ref, False)


@pytest.mark.parametrize("forward_mode", [1, 5])
@pytest.mark.parametrize("name", Z.NAMES)
def test_forward_image(name, forward_mode):
    fm, (r, s), ref = Z.foam(name), Z.image(name), Z.frame(name)
    pipe = _pipeline(fm["sh_degree"])
    pipe.forward_mode = forward_mode
    got = pipe.trace_forward(*H.to_torch_foam(fm, DEV), _t(r), _t(s))
    torch.cuda.synchronize()
    assert got["rgba"].shape == (48, 64, 4)
    _forward_bits(name, "image, mode %d" % forward_mode, got, ref, False)


def _half_tensors(fm):
    foam = H.to_torch_foam(fm, DEV)
    assert foam[1].dtype == torch.float16
    return foam


@pytest.mark.parametrize("name", Z.NAMES)
def test_forward_half(name):
    """fp16 pipeline, default scheduling and mode 5: rgba as fp16 bit patterns, integers and depth equal; contribution
    within one fp16 step (its fp32 accumulator is not exposed)."""
    from tests import test_gpu_half as GH

    fm, ref = Z.half_forward(name)
    (r, s), u = Z.rays(name), Z.upstream(name)
    foam, tr, ts, tq = _half_tensors(fm), _t(r), _t(s), _t(u["q"])
    for forward_mode in (0, 5):
        pipe = _pipeline(fm["sh_degree"], torch.float16)
        pipe.forward_mode = forward_mode
        got = pipe.trace_forward(*foam, tr, ts, depth_quantiles=tq, return_contribution=True)
        torch.cuda.synchronize()
        GH._check_forward(got, ref, True, "%s mode %d" % (name, forward_mode))
        assert got["contribution"].dtype == torch.float16 and np.any(ref["contribution"] != 0)
        ok, msg = H.half_step_check(got["contribution"].cpu().numpy(), ref["contribution"])
        print("zoo %s fp16 forward mode %d contribution: %s" % (name, forward_mode, msg))
        assert ok, (name, forward_mode, msg)


def _trail_setup(pipe, trail):
    if trail == "rewalk":
        pipe.record_trail = False
    elif trail == "short":
        pipe.trail_steps = 5


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("trail", ["rewalk", "replay", "short"])
@pytest.mark.parametrize("name", Z.HALF_BACKWARD)
def test_backward_half(name, trail, mode):
    """tests/test_gpu_half.py::test_backward_parity_half on the hub and across the fp16 edge: points_grad and the fp32
    accumulator of attr_grad (flat_grad) at the fp32 bar against the oracle on the widened inputs, through that file's
    own checks."""
    from tests import test_gpu_half as GH

    c = Z.half(name)
    fm, quant = c["fm"], c["q"] is not None
    pipe = _pipeline(fm["sh_degree"], torch.float16)
    pipe.backward_mode = mode
    pipe.forward_mode = 1 + mode % 2
    _trail_setup(pipe, trail)
    foam, tr, ts, tq = _half_tensors(fm), _t(c["rays"]), _t(c["starts"]), _t(c["q"])
    if trail != "rewalk":
        f = pipe.trace_forward(*foam, tr, ts, depth_quantiles=tq)
        GH._check_forward(f, c["fwd"], quant, name)
    out = GH._backward(pipe, foam, c, tr, ts, tq)
    assert pipe.last_backward_replayed == (trail != "rewalk")
    n, A = fm["attributes"].shape
    pitch = GH.AUTO_PITCH[A]
    what = "fp16 backward mode %d %s" % (mode, trail)
    _scatter(name, what, "points_grad", out["points_grad"], c["bwd32"]["points_grad"])
    _scatter(name, what, "attr_grad accumulator", out["flat_grad"][-n * pitch:].view(n, pitch)[:, :A], c["bwd32"]["attr_grad"])
    GH._check_backward(out, c, pitch, (name, mode, trail))


def _backward_cases():
    cases = [(name, mode, trail) for name in MAIN for mode in (1, 2, 3, 4) for trail in ("rewalk", "replay", "short")]
    cases += [(name, mode, trail) for name in Z.NAMES if name not in MAIN for mode, trail in ((0, "replay"), (3, "short"))]
    return cases


@pytest.mark.parametrize("name,mode,trail", _backward_cases())
def test_backward(name, mode, trail):
    """tests/test_gpu_parity.py::test_backward_parity: ray_error -> point_error everywhere, depth-quantile gradients on
    the foams of foam_zoo.QUANTILE_GRADS (hub and clustered among them)."""
    fm, (r, s), u, ref = Z.foam(name), Z.rays(name), Z.upstream(name), Z.flat(name)
    quant = name in Z.QUANTILE_GRADS
    pipe = _pipeline(fm["sh_degree"])
    pipe.backward_mode = mode
    pipe.forward_mode = 1 + mode % 2 if mode else 0
    _trail_setup(pipe, trail)
    foam, tr, ts, tq = H.to_torch_foam(fm, DEV), _t(r), _t(s), _t(u["q"] if quant else None)
    if trail != "rewalk":
        f = pipe.trace_forward(*foam, tr, ts, depth_quantiles=tq)
        _forward_bits(name, "before the backward", f, ref["fwd"], quant)
        assert pipe._trail is not None
    out = pipe.trace_backward(*foam, tr, ts, _t(ref["fwd"]["rgba"]), _t(u["g"]), tq,
                              _t(ref["fwd"]["depth_indices"]) if quant else None, _t(u["dg"]) if quant else None,
                              _t(u["err"]))
    torch.cuda.synchronize()
    assert pipe.last_backward_replayed == (trail != "rewalk")
    assert out["points_grad"].shape == fm["points"].shape and out["attr_grad"].shape == fm["attributes"].shape
    for key in ("points_grad", "attr_grad", "point_error"):
        _scatter(name, "backward mode %d %s" % (mode, trail), key, out[key], ref["bwd"][key])


@pytest.mark.parametrize("name", Z.NAMES)
def test_trace_segments(name):
    """Offsets, cells, t_exit and t_enter bits and num_intersections: tests/test_gpu_segments.py::_assert_bitwise."""
    from tests import test_gpu_segments as GS

    fm, (r, s), ref = Z.foam(name), Z.rays(name), Z.segments(name)
    np.testing.assert_array_equal(ref["n"], Z.flat(name)["fwd"]["num_intersections"].reshape(-1))
    _, got = GS._segments(GS._pipeline(fm["sh_degree"]), GS._device_inputs(fm, r, s))
    GS._assert_bitwise(got, ref, (Z.NUM_RAYS,))


@pytest.mark.parametrize("name", MAIN)
def test_segment_gradients(name):
    """segment_points_grad and segment_rays_grad against their float64 restatements with random normal gradients on
    every entry, at the bars and through the comparison code of tests/test_gpu_segments_grad.py::
    test_kernel_against_float64_restatement and tests/test_gpu_segments_rays_grad.py::_check."""
    import radfoam
    from tests import test_gpu_segments_grad as SG
    from tests import test_gpu_segments_rays_grad as SR

    fm, (r, s) = Z.foam(name), Z.rays(name)
    inputs = SG._device_inputs(fm, r, s)
    seg = SG._pipeline(fm["sh_degree"]).trace_differentiable_segments(*inputs)
    total = seg["cells"].numel()
    assert total == len(Z.segments(name)["cells"])
    g_enter, g_exit = SR._random_grads(total)
    points, rays = inputs[0], inputs[4]
    got = radfoam.segment_points_grad(seg, seg["exit_cells"], points, rays, g_enter, g_exit)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == points.shape
    SG._assert_bars("zoo %s segment_points_grad" % name, got.cpu().numpy(), *SG._restatements(seg, points, rays, g_enter, g_exit))
    SR._check("zoo %s segment_rays_grad" % name, seg, seg["exit_cells"], points, rays, g_enter, g_exit)


def test_geometry_only_repack_across_the_fp16_edge():
    """scaled_2p13 traced, its points doubled in place and its density halved: adjacency and offsets are the same tensors,
    so only cells and face offsets are repacked (foam_prepared == 2, prepare_geometry_kernel), and the workspace must be
    that of a fresh pack of scaled_2p14 -- whose overflowed paddings are all-zero where scaled_2p13 had scaled copies --
    and back again."""
    small, big = Z.foam("scaled_2p13"), Z.foam("scaled_2p14")
    assert Z.overflowed_paddings(big) > Z.overflowed_paddings(small) > 0
    d = small["sh_degree"]
    pipe = _pipeline(d)
    p, a, adj, off = H.to_torch_foam(small, DEV)

    def trace(name, what, pipeline, foam):
        (r, s), u, ref = Z.rays(name), Z.upstream(name), Z.flat(name)["fwd"]
        got = pipeline.trace_forward(*foam, _t(r), _t(s), depth_quantiles=_t(u["q"]), return_contribution=True)
        torch.cuda.synchronize()
        _forward_bits(name, what, got, ref, True)
        _scatter(name, what, "contribution", got["contribution"], ref["contribution"])

    trace("scaled_2p13", "first pack", pipe, (p, a, adj, off))
    for name, factor in (("scaled_2p14", 2.0), ("scaled_2p13", 0.5)):
        with torch.no_grad():
            p.mul_(factor)
            a[:, -1].mul_(1.0 / factor)
        np.testing.assert_array_equal(_bits(p), _bits(Z.foam(name)["points"]))
        np.testing.assert_array_equal(_bits(a), _bits(Z.foam(name)["attributes"]))
        opts = pipe._launch_opts(p, a, adj, off, (Z.NUM_RAYS, 6))
        assert opts.foam_prepared == 2
        pipe._cache.invalidate_geometry()
        trace(name, "geometry-only repack", pipe, (p, a, adj, off))
        trace(name, "fresh pipeline", _pipeline(d), H.to_torch_foam(Z.foam(name), DEV))


@pytest.mark.parametrize("half", [False, True])
def test_benchmark_path_across_the_fp16_edge(half):
    """trace_benchmark on scaled_2p14 with the caller's half table (build_adjacent_diff: the reference's, where offsets
    beyond fp16 are inf and nothing is padded): RGBA8 words equal the oracle's."""
    name = "scaled_2p14"
    fm = dict(Z.foam(name))
    if half:
        fm["attributes"] = fm["attributes"].astype(np.float16)
    d, cam, start = fm["sh_degree"], Z.camera(name), int(Z.image(name)[1][0, 0])
    topo = (fm["point_adjacency"], fm["point_adjacency_offsets"])
    diff = O.build_adjacent_diff(fm["points"], *topo)
    ref = O.trace_benchmark(d, fm["points"], fm["attributes"], *topo, diff, cam, start)
    assert len(np.unique(ref)) > 100 and ((ref >> 24) == 255).all()
    pipe = _pipeline(d, torch.float16 if half else torch.float32)
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    table = pipe.build_adjacent_diff(p, adj, off)
    np.testing.assert_array_equal(_bits(table), diff)
    out = torch.zeros((cam["height"], cam["width"]), dtype=torch.uint32, device=DEV)
    camera = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    sp = torch.tensor([start], dtype=torch.int64).to(torch.uint32).to(DEV)
    for frame in (0, 1):                     # the second frame walks in the tile order the first one taught
        out.zero_()
        pipe.trace_benchmark(p, a, adj, off, table, camera, sp, out)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), ref, err_msg="frame %d" % frame)


@pytest.mark.parametrize("mode", [2, 3])
def test_site_at_the_world_origin(mode):
    """The lattice without its shift, 512 rays from the cell of the site at (0, 0, 0): the reference's phantom first-cell
    term is 0/0 there.  The kernels write what the oracle writes: non-finite exactly in that site's points_grad row,
    everything else at the scatter bar with that row taken out on both sides, attr_grad finite."""
    c = Z.origin_case()
    fm, ref = c["fm"], c["bwd"]
    pipe = _pipeline(fm["sh_degree"])
    pipe.reorder_min_rays = 16384            # 512 rays: the plain order
    pipe.backward_mode = mode
    pipe.forward_mode = 1 + mode % 2
    foam, tr, ts = H.to_torch_foam(fm, DEV), _t(c["rays"]), _t(c["starts"])
    f = pipe.trace_forward(*foam, tr, ts)
    _forward_bits("origin", "forward", f, c["fwd"], False)
    out = pipe.trace_backward(*foam, tr, ts, f["rgba"], _t(c["g"]))
    torch.cuda.synchronize()
    assert pipe.last_backward_replayed
    pg, ag = out["points_grad"].cpu().numpy(), out["attr_grad"].cpu().numpy()
    bad = ~np.isfinite(ref["points_grad"])
    assert bad[c["site"]].all() and bad.sum() == 3
    print("zoo origin mode %d: row of the site: kernel %s, oracle %s" % (mode, pg[c["site"]], ref["points_grad"][c["site"]]))
    np.testing.assert_array_equal(~np.isfinite(pg), bad)
    assert np.isfinite(ag).all()
    what = "backward mode %d" % mode
    _scatter("origin", what, "points_grad", np.delete(pg, c["site"], axis=0), np.delete(ref["points_grad"], c["site"], axis=0))
    _scatter("origin", what, "attr_grad", ag, ref["attr_grad"])
