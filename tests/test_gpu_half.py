"""-m gpu: the fp16 (`HALF`) instances of the tracer kernels against the CPU oracle, backward included.

Reference (tests/test_oracle.py::test_half_mode_is_the_fp32_mode_on_widened_inputs_rounded_once): the oracle in fp16
mode computes exactly what its fp32 mode computes on the same fp16 values widened to fp32, with rgba and the scatter
outputs rounded to fp16 once.  The pipeline accumulates fp16 gradients in fp32 too and exposes that buffer
(`flat_grad`), so the fp16 kernels are held to the fp32 bars of tests/test_gpu_parity.py:

  * rgba as fp16 bit patterns, depth / depth_indices / num_intersections: BIT-IDENTICAL to the oracle;
  * points_grad and the fp32 attr_grad accumulator: helpers.grad_close (1e-3 per element) and relative L2 < 1e-5
    against the fp32 mode on the widened inputs;
  * the fp16 attr_grad: that accumulator rounded once, bit for bit;
  * outputs whose accumulator is not exposed (point_error, contribution): within one fp16 step of the fp16 oracle
    (helpers.half_step_check).

No fp16 instance deliberately computes anything other than "widen, then the fp32 arithmetic" (DESIGN.md section 2).
"""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AUTO_PITCH = {4: 4, 13: 16, 28: 32, 49: 64}

_CASES = {}


def _case(foam_factory, *key, **kw):
    """helpers.half_backward_case, computed once per module run and never modified."""
    k = key + tuple(sorted(kw.items()))
    if k not in _CASES:
        c = H.half_backward_case(foam_factory, *key, **kw)
        # what the bars below rely on (asserted at 3000 points on the CPU too): nothing near the fp16 maximum, every
        # output populated, found and not-found quantiles
        for name in ("attr_grad", "point_error"):
            if name in c["bwd32"]:
                assert np.abs(c["bwd32"][name]).max() < 65504.0 and np.any(c["bwd32"][name] != 0), name
        assert np.any(c["bwd32"]["points_grad"] != 0) and float(c["fwd32"]["rgba"][..., 3].max()) > 0.5
        if c["q"] is not None:
            di = c["fwd"]["depth_indices"]
            assert (di == 0xFFFFFFFF).any() and (di != 0xFFFFFFFF).any()
        _CASES[k] = c
    return _CASES[k]


def _pipeline(d):
    """fp16 pipeline with the hop trail always recorded (see tests/test_gpu_parity.py::_pipeline)."""
    import radfoam

    pipe = radfoam.create_pipeline(d, torch.float16)
    pipe.record_trail = True
    return pipe


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _foam_tensors(fm):
    p, a, adj, off = H.to_torch_foam(fm, DEV)
    assert a.dtype == torch.float16
    return p, a, adj, off


def _bits16(x):
    return np.ascontiguousarray(x).view(np.uint16)


def _check_forward(f, fwd, quantiles, what=""):
    """trace_forward outputs of an fp16 pipeline against the fp16 oracle, bit for bit."""
    assert f["rgba"].dtype == torch.float16
    np.testing.assert_array_equal(_bits16(f["rgba"].cpu().numpy()), _bits16(fwd["rgba"]), err_msg=what)
    np.testing.assert_array_equal(f["num_intersections"].cpu().numpy().view(np.uint32), fwd["num_intersections"],
                                  err_msg=what)
    if quantiles:
        np.testing.assert_array_equal(f["depth"].cpu().numpy().view(np.uint32), fwd["depth"].view(np.uint32),
                                      err_msg=what)
        np.testing.assert_array_equal(f["depth_indices"].cpu().numpy().view(np.uint32), fwd["depth_indices"],
                                      err_msg=what)


def _check_backward(out, c, pitch, what=""):
    """trace_backward outputs of an fp16 pipeline: the fp32 bars on what is accumulated in fp32, one rounding after."""
    bwd, bwd32 = c["bwd"], c["bwd32"]
    n, A = c["fm"]["attributes"].shape
    assert out["points_grad"].dtype == torch.float32 and out["points_grad"].shape == (n, 3)
    ok, rel, worst = H.grad_close(out["points_grad"].cpu().numpy(), bwd32["points_grad"])
    assert ok and rel < 1e-5, (what, "points_grad", rel, worst)
    rows = out["flat_grad"][-n * pitch:].view(n, pitch)
    assert rows.dtype == torch.float32 and out["flat_grad"].numel() >= 3 * n + n * pitch
    if pitch != A:
        assert float(rows[:, A:].abs().max()) == 0.0, (what, "padding columns")
    acc = rows[:, :A]
    ok, rel, worst = H.grad_close(acc.cpu().numpy(), bwd32["attr_grad"])
    assert ok and rel < 1e-5, (what, "attr_grad accumulator", rel, worst)
    ag = out["attr_grad"]
    assert ag.dtype == torch.float16 and ag.shape == (n, A)
    np.testing.assert_array_equal(_bits16(ag.cpu().numpy()), _bits16(acc.to(torch.float16).cpu().numpy()),
                                  err_msg="%s: attr_grad is not its accumulator rounded once" % (what,))
    if c["err"] is not None:
        pe = out["point_error"]
        assert pe.dtype == torch.float16 and pe.shape == (n, 1)
        ok, msg = H.half_step_check(pe.cpu().numpy(), bwd["point_error"])
        assert ok, (what, "point_error", msg)
    else:
        assert "point_error" not in out
    assert out["ray_grad"].shape == c["rays"].shape and float(out["ray_grad"].abs().max()) == 0.0


def _backward(pipe, foam, c, tr, ts, tq, depth_indices=None):
    p, a, adj, off = foam
    out = pipe.trace_backward(p, a, adj, off, tr, ts, _t(c["fwd"]["rgba"]), _t(c["g"]), tq,
                              _t(c["fwd"].get("depth_indices")) if depth_indices is None else depth_indices,
                              _t(c["dg"]), _t(c["err"]))
    torch.cuda.synchronize()
    return out


# every degree with and without quantiles: LaunchBackward<DEG, true> picks its replay instances by (mode, nq != 0)
_BACKWARD_CASES = [
    (0, True, False, False), (0, False, True, True), (1, False, False, True), (1, True, True, False),
    (2, True, True, False), (2, False, False, True), (3, False, True, True), (3, True, False, False),
]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("trail", ["rewalk", "replay", "short"])
@pytest.mark.parametrize("d,image,quantiles,with_error", _BACKWARD_CASES)
def test_backward_parity_half(foam_factory, d, image, quantiles, with_error, mode, trail):
    """tests/test_gpu_parity.py::test_backward_parity for `LaunchBackward<DEG, true>`: backward_mode 1 / 2 (replay
    kernels <.,1> / <.,2>), 3 (cached, QUANT by the case) and 4 (direct, QUANT by the case); trail 'rewalk' = no forward
    on this pipeline, backward_kernel re-scans every cell; 'replay' = the trail trace_forward recorded; 'short' = the
    trail holds 5 hops per ray, backward_kernel re-scans the rest.  5000-point foam, 80x56 image or 4000 flat rays."""
    c = _case(foam_factory, d, 20 + d, image, quantiles, with_error)
    pipe = _pipeline(d)
    pipe.backward_mode = mode
    pipe.forward_mode = 1 + mode % 2    # the trail comes from either forward instance (both write the same one)
    foam = _foam_tensors(c["fm"])
    tr, ts, tq = _t(c["rays"]), _t(c["starts"]), _t(c["q"])
    if trail == "rewalk":
        pipe.record_trail = False
    else:
        if trail == "short":
            pipe.trail_steps = 5
        f = pipe.trace_forward(*foam, tr, ts, depth_quantiles=tq)
        _check_forward(f, c["fwd"], quantiles)
        assert pipe._trail is not None
    out = _backward(pipe, foam, c, tr, ts, tq)
    assert pipe.last_backward_replayed == (trail != "rewalk")
    _check_backward(out, c, AUTO_PITCH[c["fm"]["attributes"].shape[1]], (mode, trail))


def test_dividing_scan_instance_half(foam_factory):
    """The fp16 instances of the `kScanStrict` forward (forward_mode 3, Pipeline.strict_reference_scan) and of the
    backward under it -- replay of a trail recorded under it, short trail + re-walk, no trail: the bars of
    test_backward_parity_half (tests/test_gpu_parity.py::test_dividing_scan_instance is the fp32 loop)."""
    d = 2
    c = _case(foam_factory, d, 62, False, True, True, n_points=7000)
    foam = _foam_tensors(c["fm"])
    tr, ts, tq = _t(c["rays"]), _t(c["starts"]), _t(c["q"])
    for trail in ("replay", "short", "rewalk"):
        pipe = _pipeline(d)
        pipe.strict_reference_scan = True
        assert pipe.forward_mode == 3
        if trail == "rewalk":
            pipe.record_trail = False
        elif trail == "short":
            pipe.trail_steps = 5
        f = pipe.trace_forward(*foam, tr, ts, depth_quantiles=tq)
        _check_forward(f, c["fwd"], True, trail)
        out = _backward(pipe, foam, c, tr, ts, tq, depth_indices=f["depth_indices"])
        assert pipe.last_backward_replayed == (trail != "rewalk")
        _check_backward(out, c, AUTO_PITCH[28], trail)


def test_gradient_row_pitch_half(foam_factory):
    """Pipeline.gradient_row_pitch "auto" / "dense" / A + 3 on an fp16 pipeline: the returned fp16 attr_grad is a dense
    [N, A] rounding of the pitched fp32 rows, whose padding stays zero -- same gradients whichever."""
    d = 1
    c = _case(foam_factory, d, 21, True, False, True)
    foam = _foam_tensors(c["fm"])
    tr, ts = _t(c["rays"]), _t(c["starts"])
    A = c["fm"]["attributes"].shape[1]
    assert A == 13
    for pitch in ("auto", "dense", A + 3):
        pipe = _pipeline(d)
        pipe.gradient_row_pitch = pitch
        f = pipe.trace_forward(*foam, tr, ts)
        _check_forward(f, c["fwd"], False, str(pitch))
        out = _backward(pipe, foam, c, tr, ts, None)
        want_pitch = {"auto": AUTO_PITCH[A], "dense": A}.get(pitch, pitch)
        _check_backward(out, c, want_pitch, str(pitch))


@pytest.mark.parametrize("forward_mode", [1, 2, 5])
@pytest.mark.parametrize("d", [0, 2, 3])
def test_forward_flat_rays_quantiles_contribution_half(foam_factory, d, forward_mode):
    """fp16 twin of tests/test_gpu_parity.py::test_forward_flat_rays_quantiles_contribution: 6000 points, 5000 flat rays,
    two quantiles.  contribution's fp32 accumulator is not exposed: one fp16 step."""
    c = _case(foam_factory, d, 12, False, True, False, n_points=6000, n_rays=5000)
    assert c["rays"].shape == (5000, 6) and c["q"].shape == (5000, 2)
    pipe = _pipeline(d)
    pipe.forward_mode = forward_mode
    p, a, adj, off = _foam_tensors(c["fm"])
    f = pipe.trace_forward(p, a, adj, off, _t(c["rays"]), _t(c["starts"]), depth_quantiles=_t(c["q"]),
                           return_contribution=True)
    torch.cuda.synchronize()
    _check_forward(f, c["fwd"], True)
    assert f["contribution"].dtype == torch.float16 and f["contribution"].shape == (6000, 1)
    assert np.any(c["fwd"]["contribution"] != 0)
    ok, msg = H.half_step_check(f["contribution"].cpu().numpy(), c["fwd"]["contribution"])
    assert ok, ("contribution", msg)


@pytest.mark.parametrize("d", [1, 2])
def test_geometry_only_repack_after_an_optimiser_step_half(foam_factory, d):
    """fp16 twin of tests/test_gpu_parity.py::test_geometry_only_repack_after_an_optimiser_step: `prepare_impl(..., true)`
    reads the density through `load_attr_scalar<true>` and the colours are repacked at the fp16 SH row stride.  Points
    move in fp32, attributes in fp16, the density column stays: foam_prepared == 2, then forward and backward through
    the repacked workspace as from a fresh pack."""
    c0 = _case(foam_factory, d, 20 + d, True, False, True)
    fm = c0["fm"]
    rng = np.random.default_rng(3)
    dp = rng.normal(0, 2e-3, fm["points"].shape).astype(np.float32)
    da = rng.normal(0, 5e-2, fm["attributes"].shape).astype(np.float16)
    da[:, -1] = 0
    moved = dict(fm)
    moved["points"] = fm["points"] + dp
    moved["attributes"] = fm["attributes"] + da          # one fp16 addition per element, as `a += da` on the device
    np.testing.assert_array_equal(_bits16(moved["attributes"][:, -1]), _bits16(fm["attributes"][:, -1]))
    # same rays, entry cell and upstream gradients, on the updated foam
    c1 = H.half_reference(d, moved, c0["rays"], c0["starts"], None, None, c0["g"], c0["err"])
    p, a, adj, off = _foam_tensors(fm)
    tr, ts = _t(c0["rays"]), _t(c0["starts"])
    pipe = _pipeline(d)
    f0 = pipe.trace_forward(p, a, adj, off, tr, ts)
    _check_forward(f0, c0["fwd"], False, "before the step")
    with torch.no_grad():
        p += _t(dp)
        a += _t(da)
    np.testing.assert_array_equal(_bits16(a.cpu().numpy()), _bits16(moved["attributes"]))
    opts = pipe._launch_opts(p, a, adj, off, tr.shape)
    assert opts.foam_prepared == 2
    pipe._cache.invalidate_geometry()
    f1 = pipe.trace_forward(p, a, adj, off, tr, ts)
    _check_forward(f1, c1["fwd"], False, "after the step")
    assert not np.array_equal(_bits16(c1["fwd"]["rgba"]), _bits16(c0["fwd"]["rgba"]))
    out = _backward(pipe, (p, a, adj, off), c1, tr, ts, None)
    assert pipe.last_backward_replayed
    _check_backward(out, c1, AUTO_PITCH[fm["attributes"].shape[1]], "after the step")
