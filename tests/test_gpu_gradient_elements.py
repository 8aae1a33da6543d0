"""-m gpu: the HIP backward against the CPU oracle, every gradient element on its own scale.

tests/test_gpu_parity.py and tests/test_gpu_half.py hold the backward to helpers.grad_close and a relative L2 norm, both
scaled by the whole tensor; tests/test_gradient_criterion.py shows what that lets through.  Here every element i of
points_grad, attr_grad and point_error has to lie within

    k * 2^-24 * M[i] + 2^-22 * |ref[i]|,     M[i] = the sum of |addend| over everything the oracle adds into element i,

of the oracle's value and to be exactly 0 where the oracle adds nothing (helpers.grad_close_elements).  k is not tuned to
the kernels: per case it is helpers.element_k(k0) = 4 * max(k0, 4), with k0 the distance, in the same units, of the oracle
from itself when it takes the rays in reverse order; never above 256.  Every test asserts the forward rgba bit for bit
first, as the parity tests do, and prints the worst ratio |got - ref| / (2^-24 M) per tensor with the instance's name
(the table in DESIGN.md section 2 is a copy of that output).

All on 5000-point foams with an 80x56 image or 4000 flat rays (one 70x24 and one 48x40 frame): the seams are block, wave
and epoch boundaries, not size.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_MAX = 256.0
_CASES = {}


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _cached(key, make):
    """Cases are computed once per run, shared, and never modified."""
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _matrix_case(foam_factory, d, image, quantiles, with_error, seed=None):
    seed = 20 + d if seed is None else seed
    return _cached(("matrix", d, seed, image, quantiles, with_error),
                   lambda: H.backward_case(foam_factory, d, seed, image, quantiles, with_error))


def _custom_case(key, d, fm, rays, starts, seed, quantiles=False, with_error=False, **settings):
    """A case on a foam / rays of the test's own; the draws follow helpers.backward_case."""
    def make():
        rng = np.random.default_rng(seed)
        batch = rays.shape[:-1]
        q = dg = None
        if quantiles:
            q = np.sort(rng.uniform(0.02, 0.98, size=batch + (2,)).astype(np.float32), axis=-1)[..., ::-1].copy()
            dg = rng.normal(size=batch + (2,)).astype(np.float32)
        g = rng.normal(size=batch + (4,)).astype(np.float32)
        err = rng.uniform(0, 1, size=batch).astype(np.float32) if with_error else None
        fwd, ref, k0, k0s = H.oracle_backward_elements(d, fm, rays, starts, g, q, dg, err, **settings)
        return {"d": d, "fm": fm, "rays": rays, "starts": starts, "q": q, "dg": dg, "g": g, "err": err, "fwd": fwd,
                "ref": ref, "k0": k0, "k0_by_tensor": k0s, "settings": settings}
    return _cached(key, make)


def _pipeline(d, dtype=torch.float32):
    import radfoam

    pipe = radfoam.create_pipeline(d, dtype)
    pipe.record_trail = True       # see tests/test_gpu_parity.py::_pipeline
    return pipe


def _run(c, pipe, trail="replay"):
    """Forward (rgba bit for bit against the oracle) and backward of case c on `pipe`.  trail: 'replay' = the backward
    replays the trail the forward recorded; 'short' = the trail holds 5 hops per ray, the rest is re-scanned; 'rewalk' =
    no trail, the backward re-scans every cell."""
    p, a, adj, off = H.to_torch_foam(c["fm"], DEV)
    tr, ts, tq = _t(c["rays"]), _t(c["starts"]), _t(c["q"])
    if trail == "rewalk":
        pipe.record_trail = False
    elif trail == "short":
        pipe.trail_steps = 5
    f = pipe.trace_forward(p, a, adj, off, tr, ts, depth_quantiles=tq, **c["settings"])
    want = c["fwd"]["rgba"]
    view = np.uint16 if want.dtype == np.float16 else np.uint32
    np.testing.assert_array_equal(f["rgba"].cpu().numpy().view(view), want.view(view))
    out = pipe.trace_backward(p, a, adj, off, tr, ts, _t(want), _t(c["g"]), tq, _t(c["fwd"].get("depth_indices")),
                              _t(c["dg"]), _t(c["err"]), **c["settings"])
    torch.cuda.synchronize()
    assert pipe.last_backward_replayed == (trail != "rewalk")
    got = {k: out[k].cpu().numpy() for k in H.GRAD_TENSORS if k in out}
    if out["attr_grad"].dtype == torch.float16:
        # the fp32 accumulator the fp16 attr_grad is rounded from (tests/test_gpu_half.py::_check_backward)
        n, A = out["attr_grad"].shape
        pitch = {4: 4, 13: 16, 28: 32, 49: 64}[A]
        got["attr_grad_accumulator"] = out["flat_grad"][-n * pitch:].view(n, pitch)[:, :A].cpu().numpy()
    return pipe, got


def _locate(c, key, where):
    """What a finding needs: the element, its cell and column, and the rays whose walk visits that cell."""
    fm = c["fm"]
    cell = where[0]
    cells, t1, n = O.trace_paths(c["d"], fm["points"], fm["attributes"].astype(np.float32), fm["point_adjacency"],
                                 fm["point_adjacency_offsets"], c["rays"].reshape(-1, 6),
                                 np.broadcast_to(c["starts"], c["rays"].shape[:-1]).reshape(-1), cap=1024, **c["settings"])
    rays = np.flatnonzero((cells == cell).any(axis=1))
    return "%s element %s: cell %d, column %d, density %r, %d rays visit the cell: %s" % (
        key, where, cell, where[-1], float(fm["attributes"][cell, -1]), rays.size, rays[:32].tolist())


def _check(name, c, out, ref=None, half_outputs=(), finite_only=False):
    """Every gradient tensor of `out` against the oracle's by helpers.grad_close_elements; prints the worst ratios."""
    ref = c["ref"] if ref is None else ref
    k = H.element_k(c["k0"])
    assert k <= K_MAX, (name, c["k0_by_tensor"])
    failures = []
    for key in H.GRAD_TENSORS:
        if key not in ref:
            assert key not in out
            continue
        got, want, mag = out[key].astype(np.float64), ref[key].astype(np.float64), ref[key + "_mag"]
        assert got.shape == want.shape and np.abs(want[np.isfinite(want)]).max() > 0, (name, key)
        if finite_only:
            # the reference's own arithmetic yields inf / NaN here (tests/test_gpu_parity.py::
            # test_backward_with_zero_weight_threshold): they sit in (nearly) the same places, and every element finite in
            # both, with finite addends, obeys the bound
            fin_w, fin_g = np.isfinite(want) & np.isfinite(mag), np.isfinite(got)
            assert (fin_w != fin_g).mean() < 2e-3, (name, key, (fin_w != fin_g).mean())
            assert 0.5 < fin_w.mean() < 1.0, (name, key)
            both = fin_w & fin_g
            got, want, mag = np.where(both, got, 0.0), np.where(both, want, 0.0), np.where(both, mag, 0.0)
        once = key in half_outputs      # an fp32 sum rounded to half once: helpers.grad_close_elements
        ok, worst, where = H.grad_close_elements(got, want, mag, k, extra_rel=2.0 ** -11 if once else 0.0,
                                                 extra_abs=2.0 ** -25 if once else 0.0)
        print("ELEMENTS | %s | %s | worst ratio %.2f at %s | k0 %.2f | k %.1f | %s"
              % (name, key, worst, where, c["k0"], k, "ok" if ok else "OUTSIDE"))
        if not ok:
            failures.append((worst, _locate(c, key, where)))
    assert not failures, (name, failures)


# ---- the matrix of tests/test_gpu_parity.py::test_backward_parity -------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("trail", ["rewalk", "replay", "short"])
@pytest.mark.parametrize("d,image,quantiles,with_error", [
    (0, True, False, False), (1, False, True, True), (2, True, True, False), (2, False, False, True),
    (3, True, False, False), (3, False, True, True),
])
def test_backward_elements(foam_factory, d, image, quantiles, with_error, mode, trail):
    c = _matrix_case(foam_factory, d, image, quantiles, with_error)
    pipe = _pipeline(d)
    pipe.backward_mode = mode
    pipe.forward_mode = 1 + mode % 2
    _, out = _run(c, pipe, trail)
    _check("matrix d%d %s%s%s mode %d %s" % (d, "image" if image else "flat", " quantiles" if quantiles else "",
                                               " error" if with_error else "", mode, trail), c, out)


# ---- flat batches down the training path: sorted order, row-coalesced direct atomics ------------------------------------

def _spread_rays(fm, n_rays, seed, n_origins=64, clearance=0.05):
    """Rays from 64 origins inside the foam, each at least `clearance` from every site and at least 0.25 from the world
    origin, towards uniform targets; un-normalised like random_rays.  (The reference's phantom first-cell term, SURVEY.md
    Appendix A.4, differentiates a bisector between the start cell's site P and the world origin and divides by
    (P . direction)^2: a start site near the world origin makes it large for every ray, which these origins avoid; a
    direction nearly perpendicular to P makes it large for that ray, which 4000 random directions do not avoid.)"""
    from radfoam_amd import foam as foam_mod

    rng = np.random.default_rng(seed)
    pts = fm["points"].astype(np.float64)
    origins = []
    while len(origins) < n_origins:
        o = rng.uniform(-0.6, 0.6, size=3)
        if np.linalg.norm(o) < 0.25:
            continue
        for _ in range(8):      # step off the nearest site until none is closer than the clearance
            dist = np.linalg.norm(pts - o, axis=1)
            i = int(np.argmin(dist))
            if dist[i] >= clearance:
                break
            o = pts[i] + (o - pts[i]) * (clearance * 1.01 / max(dist[i], 1e-12))
        if np.linalg.norm(pts - o, axis=1).min() >= clearance:
            origins.append(o)
    origins = np.asarray(origins, dtype=np.float32)
    assert np.linalg.norm(pts[None] - origins[:, None].astype(np.float64), axis=2).min() >= clearance * 0.999
    starts = np.array([foam_mod.nearest_point(fm["points"], o) for o in origins], dtype=np.uint32)
    which = rng.integers(0, n_origins, size=n_rays)
    target = rng.uniform(-0.7, 0.7, size=(n_rays, 3)).astype(np.float32)
    d = (target - origins[which]) * rng.uniform(0.5, 2.0, size=(n_rays, 1)).astype(np.float32)
    return np.concatenate([origins[which], d.astype(np.float32)], axis=1).astype(np.float32), starts[which]


def _training_case(foam_factory, d, kind):
    seed = 80 + d
    if kind == "random_rays":       # four origins, two of them inside the foam: the heavy tail of the phantom term included
        fm = foam_factory(5000, d, seed)
        rays, starts = H.random_rays(fm, 4000, seed=seed + 1)
    elif kind == "spread":          # many start cells, none of them next to the world origin
        fm = foam_factory(5000, d, seed)
        rays, starts = _spread_rays(fm, 4000, seed + 2)
    else:                           # "lit": every density above 0 and above the 1e-6 of load_attributes, as training has it
        fm = dict(foam_factory(5000, d, seed))
        fm["attributes"] = fm["attributes"].copy()
        fm["attributes"][:, -1] = np.maximum(fm["attributes"][:, -1], np.float32(0.05))
        assert (fm["attributes"][:, -1] > 1e-6).all()
        rays, starts = H.random_rays(fm, 4000, seed=seed + 1)
    return _custom_case(("training", d, kind), d, fm, rays, starts, seed + 3, quantiles=True, with_error=True)


@pytest.mark.parametrize("kind", ["random_rays", "spread", "lit"])
@pytest.mark.parametrize("d", [1, 3])
def test_flat_batches_down_the_training_path(foam_factory, d, kind):
    """Pipeline defaults (backward_mode 0) with reorder_min_rays = 1: the batch is traced in the sorted order and the
    backward takes the path a training step takes."""
    c = _training_case(foam_factory, d, kind)
    if kind == "spread":
        assert np.unique(c["starts"]).size >= 48
    pipe = _pipeline(d)
    pipe.reorder_min_rays = 1
    pipe, out = _run(c, pipe)
    assert pipe._order is not None
    pg = np.abs(c["ref"]["points_grad"][c["ref"]["points_grad"] != 0])
    print("ELEMENTS | training d%d %s | points_grad max %.3g median %.3g" % (d, kind, pg.max(), np.median(pg)))
    _check("training d%d %s" % (d, kind), c, out)


# ---- image instances with a path of their own ---------------------------------------------------------------------------

def _shell_foam(foam_factory, d, seed):
    """Density exactly 0 outside r = 0.8 and in the shell 0.3 < r < 0.5 (tests/test_gpu_backward_empty_memo.py's pattern):
    long runs of empty cells before, between and after the lit ones."""
    fm = dict(foam_factory(5000, d, seed))
    r = np.linalg.norm(fm["points"].astype(np.float64), axis=1)
    fm["attributes"] = fm["attributes"].copy()
    fm["attributes"][(r > 0.8) | ((r > 0.3) & (r < 0.5)), -1] = 0.0
    return fm


def _image_case(foam_factory, what):
    d = 2
    if what == "empty cells":
        fm = _shell_foam(foam_factory, d, 91)
        cam, rays, start = H.camera_setup(fm, 80, 56)
        settings, quantiles = {}, True
    elif what == "weight_threshold 0":        # the case of tests/test_gpu_parity.py::test_backward_with_zero_weight_threshold
        d = 1
        fm = dict(foam_factory(5000, d, 26))
        fm["attributes"] = fm["attributes"].copy()
        fm["attributes"][:, -1] *= 60.0
        cam, rays, start = H.camera_setup(fm, 48, 40)
        settings, quantiles = {"weight_threshold": 0.0}, False
    elif what == "max_intersections 3":
        fm = foam_factory(5000, d, 92)
        cam, rays, start = H.camera_setup(fm, 80, 56)
        settings, quantiles = {"max_intersections": 3}, True
    else:                                       # "70x24": rows and columns that are no multiple of the 16x16 block
        fm = foam_factory(5000, d, 31)
        cam, rays, start = H.camera_setup(fm, 70, 24)
        settings, quantiles = {}, False
    starts = np.full(rays.shape[:-1], start, dtype=np.uint32)
    return _custom_case(("image", what), d, fm, rays, starts, 93, quantiles=quantiles, **settings)


def test_image_with_runs_of_empty_cells(foam_factory):
    """The default image instance on a foam most of whose cells are empty: the empty-run memo of the cached backward."""
    c = _image_case(foam_factory, "empty cells")
    share = float((c["fm"]["attributes"][:, -1] == 0).mean())
    print("ELEMENTS | image empty cells | share of cells with density 0: %.3f" % share)
    assert share >= 0.6
    assert float(c["fwd"]["rgba"][..., 3].max()) > 0.5
    _, out = _run(c, _pipeline(c["d"]))
    _check("image empty cells", c, out)


@pytest.mark.parametrize("mode", [2, 3])
def test_image_with_zero_weight_threshold(foam_factory, mode):
    c = _image_case(foam_factory, "weight_threshold 0")
    assert c["fwd"]["rgba"][..., 3].max() == 1.0          # saturated: T reached exactly 0 somewhere
    pipe = _pipeline(c["d"])
    pipe.backward_mode = mode
    _, out = _run(c, pipe)
    _check("image weight_threshold 0 mode %d" % mode, c, out, finite_only=True)


@pytest.mark.parametrize("trail", ["replay", "rewalk"])
def test_image_with_three_intersections(foam_factory, trail):
    c = _image_case(foam_factory, "max_intersections 3")
    assert int(c["fwd"]["num_intersections"].max()) <= 4
    _, out = _run(c, _pipeline(c["d"]), trail)
    _check("image max_intersections 3 %s" % trail, c, out)


@pytest.mark.parametrize("mode,trail", [(3, "replay"), (2, "rewalk")])
def test_ragged_image(foam_factory, mode, trail):
    c = _image_case(foam_factory, "70x24")
    pipe = _pipeline(c["d"])
    pipe.backward_mode = mode
    _, out = _run(c, pipe, trail)
    _check("image 70x24 mode %d %s" % (mode, trail), c, out)


# ---- row pitch of the attr_grad accumulator ------------------------------------------------------------------------------

@pytest.mark.parametrize("pitch", ["auto", "dense", "A+3"])
@pytest.mark.parametrize("d,image", [(1, True), (2, False)])
def test_row_pitch(foam_factory, d, image, pitch):
    """The cases of tests/test_gpu_parity.py::test_gradient_row_pitch_does_not_change_the_gradients."""
    c = _matrix_case(foam_factory, d, image, False, False, seed=70 + d)
    A = c["fm"]["attributes"].shape[1]
    pipe = _pipeline(d)
    pipe.gradient_row_pitch = A + 3 if pitch == "A+3" else pitch
    _, out = _run(c, pipe)
    _check("pitch %s d%d %s" % (pitch, d, "image" if image else "flat"), c, out)


# ---- fp16 pipelines ------------------------------------------------------------------------------------------------------

def _half_case(foam_factory, d, image, quantiles, with_error):
    """helpers.half_backward_case (the cases of tests/test_gpu_half.py) with the magnitudes.  The reference is the
    oracle's fp32 mode on the fp16 inputs widened (`bwd32`): what the kernels' fp32 accumulators hold before their one
    rounding to half."""
    def make():
        h = H.half_backward_case(foam_factory, d, 20 + d, image, quantiles, with_error, return_magnitude=True)
        wide = lambda x: None if x is None else x.astype(np.float32)
        fm32 = dict(h["fm"])
        fm32["attributes"] = wide(h["fm"]["attributes"])
        fwd = {"rgba": wide(h["fwd"]["rgba"]), "depth_indices": h["fwd"].get("depth_indices")}
        _, ref, k0, k0s = H.oracle_backward_elements(d, fm32, h["rays"], h["starts"], wide(h["g"]), h["q"], h["dg"],
                                                     wide(h["err"]), fwd=fwd)
        for key in ref:
            np.testing.assert_array_equal(ref[key], h["bwd32"][key], err_msg=key)
        return {"d": d, "fm": h["fm"], "rays": h["rays"], "starts": h["starts"], "q": h["q"], "dg": h["dg"],
                "g": h["g"], "err": h["err"], "fwd": h["fwd"], "ref": ref, "k0": k0, "k0_by_tensor": k0s, "settings": {}}
    return _cached(("half", d, image, quantiles, with_error), make)


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("d,image,quantiles,with_error", [(1, True, True, False), (3, False, True, True)])
def test_backward_elements_half(foam_factory, d, image, quantiles, with_error, mode):
    """Two rows of tests/test_gpu_half.py::_BACKWARD_CASES, replay.  points_grad is fp32; attr_grad and point_error are
    fp32 sums rounded to half once on the way out: extra_rel = 2^-11, and 2^-25 for the sums that land among the subnormal
    halves (the oracle's own fp16 output needs it: tests/test_gradient_criterion.py)."""
    c = _half_case(foam_factory, d, image, quantiles, with_error)
    pipe = _pipeline(d, torch.float16)
    pipe.backward_mode = mode
    pipe.forward_mode = 1 + mode % 2
    _, out = _run(c, pipe)
    assert out["attr_grad"].dtype == np.float16 and out["points_grad"].dtype == np.float32
    assert out["attr_grad_accumulator"].dtype == np.float32
    name = "half d%d %s mode %d" % (d, "image" if image else "flat", mode)
    _check(name, c, out, half_outputs=("attr_grad", "point_error"))
    # and the fp32 sums themselves, where the pipeline exposes them, with no allowance for a rounding to half
    acc = {"points_grad": out["points_grad"], "attr_grad": out["attr_grad_accumulator"]}
    _check(name + " accumulator", c, acc, ref={k: v for k, v in c["ref"].items() if not k.startswith("point_error")})
